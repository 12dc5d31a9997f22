#!/usr/bin/env python3
"""Time the pieces of `--model gat` (csrc/gat_attend.hip, models.GATConv / GAT) on the stand-ins; one JSON line per step.

Without --step the tool is a driver: it runs its steps as child processes, each under its own `timeout -k 10`, chained with `&&`
(a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  agg_ddi / agg_collab / agg_ppa: the attention aggregate on the stand-in's graph (EPS_SYNTH_SCALE = --scale) at H = --hidden with
      --heads heads, N(0,1) features and the layer's own scores; HIP events, median / min / max of --reps after --warmup:
        forward:   eps_gat_aggregate with bias, ReLU and lse, in GB/s against the byte model: per entry (the self loops included)
                   one 4 H B row and 4 heads B of scores;
        backward:  eps_gat_aggregate_backward (both launches), against the model with two more such rows per entry;
        spmm:      eps_spmm_csr WITH values, bias and ReLU on the same graph and features (GCN's aggregate: the yardstick),
                   against 4 H + 4 B per stored entry;
        scores:    the two score tables as 2 heads extra output columns of the transform's GEMM (W att folded into the weight)
                   against the transform plus a second small product over z -- which is what GATConv runs.
  train_ddi / train_collab: one training step of --model gat with the dataset's default configuration (forward, loss, backward,
      clipping, Adam) on one batch of training.train, and the same step of --model gcn next to it.
  eval_ddi: evaluate.test (the five scoring loops) of --model gat on the ddi stand-in, and of --model gcn next to it.

Run:  python tools/gat_bench.py [--scale 1.0 --hidden 256 --heads 4 --reps 7 --warmup 2]
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

STEP_SECONDS = {"agg_ddi": 300, "agg_collab": 300, "agg_ppa": 420, "train_ddi": 420, "train_collab": 420, "eval_ddi": 420}


def step_agg(a, dev, dataset):
    import torch
    from eps_amd import models, ops
    _, data = stand_in(dataset, a.scale, dev)
    g = data.adj_t
    n, H, heads = g.n_rows, a.hidden, a.heads
    torch.manual_seed(1)
    conv = models.GATConv(H, H, heads).to(dev).eval()
    x = torch.randn(n, H, device=dev)
    gout = torch.randn(n, H, device=dev)
    bias = torch.randn(H, device=dev)
    w = conv.lin.weight.detach()
    att = conv._att_matrix(True).detach().contiguous()
    z = ops.gemm(x, w)
    s = ops.gemm(z, att)
    s_src, s_dst = s[:, :heads], s[:, heads:2 * heads]
    entries = g.nnz() + n                                  # every row attends to itself too
    row, sc = 4 * H, 4 * heads
    out = {"step": f"agg_{dataset}", "scale": a.scale, "nodes": n, "stored_entries": g.nnz(), "hidden": H, "heads": heads}
    fwd = lambda: ops.gat_aggregate(g.rowptr, g.col, z, s_src, s_dst, heads, bias=bias, relu=True, want_lse=True)  # noqa: E731
    out["forward"] = rate(timed(fwd, a.reps, a.warmup), entries * (row + sc))
    o, lse = ops.gat_aggregate(g.rowptr, g.col, z, s_src, s_dst, heads, want_lse=True)
    bwd = lambda: ops.gat_aggregate_backward(g.rowptr, g.col, z, s_src, s_dst, heads, lse, o, gout)  # noqa: E731
    out["backward"] = rate(timed(bwd, a.reps, a.warmup), entries * (3 * row + sc))
    gn = g.gcn_normalized()
    spmm = lambda: ops.spmm_csr(gn.rowptr, gn.col, gn.val, z, bias=bias, relu=True)  # noqa: E731
    out["spmm"] = rate(timed(spmm, a.reps, a.warmup), gn.nnz() * (row + 4))
    out["forward_over_spmm"] = round(out["forward"]["median_ms"] / out["spmm"]["median_ms"], 3)
    out["backward_over_spmm"] = round(out["backward"]["median_ms"] / out["spmm"]["median_ms"], 3)
    w_ext = torch.cat([w, att @ w], 0).contiguous()       # [H + 2 heads (+ pad), in]: the scores ride in the transform
    out["scores"] = {"one_gemm": timed(lambda: ops.gemm(x, w_ext), a.reps, a.warmup),
                     "two_gemms": timed(lambda: ops.gemm(ops.gemm(x, w), att), a.reps, a.warmup)}
    return out


def _gat_args(dataset, heads):
    args = default_args(dataset, "gat")
    args.gat_heads = heads
    return args


def step_train(a, dev, dataset):
    import torch
    from eps_amd import models
    split_edge, data = stand_in(dataset, a.scale, dev)
    out = {"step": f"train_{dataset}", "scale": a.scale, "nodes": data.num_nodes, "entries": data.adj_t.nnz(), "models": {}}
    for name in ("gat", "gcn"):
        args = _gat_args(dataset, a.heads) if name == "gat" else default_args(dataset, name)
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
    for name in ("gat", "gcn"):
        args = _gat_args(dataset, a.heads) if name == "gat" else default_args(dataset, name)
        torch.manual_seed(1)
        model = models.build_model(args, data, dev)
        run = lambda: evaluate.test(model, data, split_edge, evaluate.evaluators[dataset], args.batch_size, args, dev)  # noqa: E731
        out["models"][name] = timed(run, a.reps, a.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--steps", nargs="*", default=["agg_ddi", "agg_collab", "agg_ppa", "train_ddi", "train_collab", "eval_ddi"],
                    choices=sorted(STEP_SECONDS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.step is None:
        common = f"--scale {a.scale} --hidden {a.hidden} --heads {a.heads} --reps {a.reps} --warmup {a.warmup}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in a.steps)
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gat_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    kind, dataset = a.step.split("_")
    res = {"agg": step_agg, "train": step_train, "eval": step_eval}[kind](a, dev, dataset)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
