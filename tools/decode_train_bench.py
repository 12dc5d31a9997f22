#!/usr/bin/env python3
"""Time one training decode step (forward + backward) of LinkPredictor on the fused route (LinkPredictor.decode_train:
eps_mlp_decode_train + eps_mlp_decode_backward) against the torch route (h[u], h[v] gathers + LinkPredictor.forward on
autograd); one JSON line per step.

Without --step the tool is a driver: every (shape, dropout) step runs as a child process under its own `timeout -k 10`,
chained with `&&` (a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it).

  ddi:    N = 4,267,   B = 262,144 edges, H = 256, L = 2      collab: N = 235,868, B = 65,536, H = 256, L = 3
  each with dropout 0.5 and 0.  A step = scores -> training's log loss -> backward into h and the decoder's parameters.
  dea_ddi / dea_collab: the same batches through DEA_GNN_JK's decoder (Linear, BatchNorm on batch statistics, ReLU, dropout,
  Linear; L = 2, logits, BCE with logits): DEA_GNN_JK.decode_train (eps_mlp_decode_bn_stats + eps_mlp_decode_train on the folded
  layer + eps_mlp_decode_bn_backward, the running statistics' update included) against the torch ops of DEA_GNN_JK.forward.
  HIP events, median of --reps after --warmup.  Also reported: per tensor, the largest difference of the two routes' gradients at
  dropout 0 (at 0.5 they draw different masks), and whether two fused steps under one seed return the same bits.

Run:  python tools/decode_train_bench.py [--reps 10 --warmup 3]
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"ddi": (4_267, 262_144, 256, 2), "collab": (235_868, 65_536, 256, 3)}
DEA_SHAPES = {"dea_ddi": (4_267, 262_144, 256, 2), "dea_collab": (235_868, 65_536, 256, 2)}
STEPS = [f"{s}:{p}" for s in SHAPES for p in ("0.5", "0")] + ["dea_ddi:0.5", "dea_ddi:0", "dea_collab:0"]
STEP_SECONDS = 240


def run_step(a, dev):
    import torch
    import torch.nn.functional as F
    from eps_amd import models
    shape, p = a.step.split(":")
    dea = shape in DEA_SHAPES
    n, B, H, L = (DEA_SHAPES if dea else SHAPES)[shape]
    torch.manual_seed(0)
    h = torch.randn(n, H, device=dev).requires_grad_(True)
    edges = torch.randint(0, n, (2, B), device=dev)
    if dea:
        # (only the decoder runs here: one node's embedding, the TAG layers idle)
        lp = models.DEA_GNN_JK(1, H, H, H, H, 3, H, H, 1, 2, float(p), True, True).to(dev).train()
        named = [(k, t) for k, t in lp.named_parameters() if k.startswith(("lins.", "mlp_bns."))]
        label = torch.cat([torch.ones(B // 2), torch.zeros(B - B // 2)]).to(dev)
    else:
        lp = models.LinkPredictor(H, H, 1, L, float(p)).to(dev).train()
        named = list(lp.named_parameters())
    params = [h] + [t for _, t in named]

    def dea_torch():                # DEA_GNN_JK.forward's decoder
        x = lp.mlp_bns[0](lp.lins[0](h[edges[0]] * h[edges[1]]))
        return lp.lins[1](F.dropout(F.relu(x), p=lp.dropout, training=True)).squeeze(1)

    def step(fused):
        for t in params:
            t.grad = None
        if dea:
            loss = lp.loss(lp.decode_train(h, edges) if fused else dea_torch(), label)
        else:
            out = lp.decode_train(h, edges) if fused else lp(h[edges[0]], h[edges[1]]).squeeze(1)
            loss = -torch.log(out[:B // 2] + 1e-8).mean() - torch.log(1 - out[B // 2:] + 1e-8).mean()
        loss.backward()
        return [t.grad for t in params]

    def timed(fused):
        for _ in range(a.warmup):
            step(fused)
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(fused)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(statistics.median(ts), 3), round(min(ts), 3)

    res = {"step": a.step, "nodes": n, "edges": B, "H": H, "L": L, "dropout": float(p)}
    res["torch_ms"], res["torch_min_ms"] = timed(False)
    res["fused_ms"], res["fused_min_ms"] = timed(True)
    res["fused_over_torch"] = round(res["fused_ms"] / res["torch_ms"], 3)
    flop = B * (3 * 2 * H * H * (L - 1) + 6 * H)          # forward + dA + dW per hidden layer (the fused route adds one forward;
                                                          # dea's adds four: statistics, dy, grad gamma, dz)
    res["model_gflop_per_step"] = round(flop / 1e9, 2)
    grads = []
    for _ in range(2):
        torch.manual_seed(5)
        grads.append([g.clone() for g in step(True)])
    res["fused_reproducible"] = all(torch.equal(x, y) for x, y in zip(*grads))
    if float(p) == 0:
        ref = step(False)
        names = ["h"] + [k for k, _ in named]
        # (dea's lins.0.bias sits in front of batch statistics: its true gradient is 0, the fused route writes 0, torch float noise)
        rel = {k: float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for k, x, y in zip(names, grads[0], ref)
               if not (dea and k == "lins.0.bias")}
        res["rel_grad_diff_vs_torch"] = {k: float(f"{v:.3g}") for k, v in rel.items()}     # per tensor, of that tensor's max|grad|
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.step is None:
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} --reps {a.reps} --warmup {a.warmup}" for s in STEPS)
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("decode_train_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    print("RESULT " + json.dumps(run_step(a, torch.device("cuda:0"))), flush=True)


if __name__ == "__main__":
    main()
