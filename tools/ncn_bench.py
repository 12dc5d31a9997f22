#!/usr/bin/env python3
"""Time the pieces of `--model ncn` (csrc/pair_cn_list.hip, models.cn_embed_sum, NCNLinkGNN) on the stand-ins; one JSON line per
step.

Without --step the tool is a driver: it runs its steps as child processes, each under its own `timeout -k 10`, chained with `&&`
(a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  lists_ddi / lists_collab: one training batch of the stand-in (EPS_SYNTH_SCALE = --scale; ddi: 65,536 positives in both
      directions and as many negatives, collab: 16,384), HIP events, median / min / max of --reps after --warmup:
        count, fill:  the list kernel's two launches, in GB/s against both rows of every pair read once (4 B per entry) plus
                      4 B per match written (fill) / 4 B per pair (count) and the pair headers;
        transpose:    eps_cn_list_transpose (ms, and matches per second);
        spmm_fwd / spmm_bwd: Z = C H and dH = C^T dZ at H = --hidden, in GB/s against 4 H B gathered per match.
  train_ddi / train_collab: one training step of --model ncn with the dataset's default configuration (forward, loss, backward,
      clipping, Adam) on such a batch, and the same step of --model gcn next to it.
  eval_ddi: evaluate.test (the five scoring loops) of --model ncn on the ddi stand-in, and of --model gcn next to it.

Run:  python tools/ncn_bench.py [--scale 1.0 --hidden 256 --reps 7 --warmup 2]
"""
import argparse
import json
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_helpers import default_args, rate, stand_in, timed, train_batch, train_step  # noqa: E402

STEP_SECONDS = {"lists_ddi": 300, "lists_collab": 300, "train_ddi": 420, "train_collab": 420, "eval_ddi": 420}


def step_lists(a, dev, dataset):
    import torch
    from eps_amd import ops
    split_edge, data = stand_in(dataset, a.scale, dev)
    g = data.adj_t
    pos_edge, neg_edge = train_batch(dataset, split_edge, data, default_args(dataset, "ncn").batch_size, dev)
    e = torch.cat([pos_edge, neg_edge], 1).to(torch.int32)
    u, v = e[0].contiguous(), e[1].contiguous()
    b, n, H = u.numel(), g.n_rows, a.hidden
    deg = g.rowptr[1:] - g.rowptr[:-1]
    row_bytes = 4 * int((deg[u.long()] + deg[v.long()]).sum().item())
    count = ops.pair_cn_list_count(g.rowptr, g.col, n, u, v)
    ptr, w = ops.pair_cn_list(g.rowptr, g.col, n, u, v, count=count)
    m = w.numel()
    out = {"step": f"lists_{dataset}", "scale": a.scale, "nodes": n, "entries": g.nnz(), "pairs": b, "matches": m, "hidden": H,
           "row_bytes": row_bytes}
    out["count"] = rate(timed(lambda: ops.pair_cn_list_count(g.rowptr, g.col, n, u, v, check=False), a.reps, a.warmup), row_bytes + 28 * b)
    out["fill"] = rate(timed(lambda: ops.pair_cn_list_fill(g.rowptr, g.col, n, u, v, ptr, w, check=False), a.reps, a.warmup),
                       row_bytes + 4 * m + 40 * b)
    out["transpose"] = timed(lambda: ops.cn_list_transpose(ptr, w, n, check=False), a.reps, a.warmup)
    out["transpose"]["matches_per_s"] = round(m / (out["transpose"]["median_ms"] * 1e-3), 1)
    tptr, tb = ops.cn_list_transpose(ptr, w, n, check=False)
    h = torch.randn(n, H, device=dev)
    dz = torch.randn(b, H, device=dev)
    out["spmm_fwd"] = rate(timed(lambda: ops.spmm_csr(ptr, w, None, h), a.reps, a.warmup), 4 * H * m)
    out["spmm_bwd"] = rate(timed(lambda: ops.spmm_csr(tptr, tb, None, dz), a.reps, a.warmup), 4 * H * m)
    return out


def step_train(a, dev, dataset):
    import torch
    from eps_amd import models
    split_edge, data = stand_in(dataset, a.scale, dev)
    out = {"step": f"train_{dataset}", "scale": a.scale, "nodes": data.num_nodes, "entries": data.adj_t.nnz(), "models": {}}
    for name in ("ncn", "gcn"):
        args = default_args(dataset, name)
        torch.manual_seed(1)
        model = models.build_model(args, data, dev)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
        pos_edge, neg_edge = train_batch(dataset, split_edge, data, args.batch_size, dev)
        rec = timed(lambda: train_step(model, data, pos_edge, neg_edge, opt), a.reps, a.warmup)
        rec.update(pairs=2 * pos_edge.size(1), hidden=args.hidden_channels, layers=args.num_layers,
                   loss=round(float(train_step(model, data, pos_edge, neg_edge, opt)), 4))
        out["models"][name] = rec
    return out


def step_eval(a, dev, dataset):
    import torch
    from eps_amd import evaluate, models
    split_edge, data = stand_in(dataset, a.scale, dev)
    out = {"step": f"eval_{dataset}", "scale": a.scale, "nodes": data.num_nodes, "entries": data.adj_t.nnz(),
           "pairs": sum(int(split_edge[k][f].size(0)) for k, f in (("eval_train", "edge"), ("valid", "edge"), ("valid", "edge_neg"),
                                                                    ("test", "edge"), ("test", "edge_neg"))), "models": {}}
    for name in ("ncn", "gcn"):
        args = default_args(dataset, name)
        torch.manual_seed(1)
        model = models.build_model(args, data, dev)
        run = lambda: evaluate.test(model, data, split_edge, evaluate.evaluators[dataset], args.batch_size, args, dev)  # noqa: E731
        out["models"][name] = timed(run, a.reps, a.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--steps", nargs="*", default=["lists_ddi", "lists_collab", "train_ddi", "train_collab", "eval_ddi"],
                    choices=sorted(STEP_SECONDS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.step is None:
        common = f"--scale {a.scale} --hidden {a.hidden} --reps {a.reps} --warmup {a.warmup}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in a.steps)
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ncn_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    kind, dataset = a.step.split("_")
    res = {"lists": step_lists, "train": step_train, "eval": step_eval}[kind](a, dev, dataset)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
