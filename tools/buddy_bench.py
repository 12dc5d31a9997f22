#!/usr/bin/env python3
"""Time the pieces of `--model buddy` (csrc/sketch.hip, CSRGraph.sketches, heuristics.sketch_features, BuddyLinkModel) on the
full-scale stand-ins; one JSON line per step.

Without --step the tool is a driver: it runs its steps as child processes, each under its own `timeout -k 10`, chained with `&&`
(a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  tables_ddi / tables_collab / tables_ppa: the table build, HIP events, median / min / max of --reps after --warmup:
        own:          eps_sketch_own of every node (768 B written per node);
        hop1, hop2:   eps_sketch_propagate, in GB/s against 768 B gathered per stored entry plus 768 B written per node (hop2
                      also reads the node's own row), and the share of the stored entries that sit in rows longer than the row
                      chunk (the rows reduced piecewise);
        card:         the cardinality table (the pair kernel on (v, v) and the estimator on torch).
  pairs_ddi / pairs_collab / pairs_ppa: eps_sketch_pair_stats at K = 2 on 2^22 uniformly drawn pairs and on a slice of the first
        filter block (its first 256 columns, column-major, so v's rows repeat; a slice because a whole block of the ppa-like
        graph is 2^31 paths, on the order of 10^9 candidates: 32 GB of statistics next to the pairs -- the filter itself scores a
        block tile by tile and never holds them all -- and the column-major order, which is what the slice is about, is the
        same): ms, pairs per second, and GB/s against 2 K 768 + 8 K^2 bytes per pair; and heuristics.sketch_features of the same uniform pairs (statistics + estimator).
  train_ddi / train_collab: one training step of --model buddy with the dataset's default configuration (forward, loss, backward,
        clipping, Adam) on one batch of training.train, and the same step of --model gcn and --model ncn next to it.
  eval_ddi: evaluate.test (the five scoring loops) of --model buddy on the ddi stand-in, and of gcn and ncn next to it.

Run:  python tools/buddy_bench.py [--scale 1.0 --reps 7 --warmup 2]
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

from bench_helpers import default_args, rate, stand_in, timed, train_batch, train_step  # noqa: E402  (the batches and timers of ncn_bench.py)

STEP_SECONDS = {"tables_ddi": 300, "tables_collab": 300, "tables_ppa": 420, "pairs_ddi": 300, "pairs_collab": 300, "pairs_ppa": 420,
                "train_ddi": 420, "train_collab": 420, "eval_ddi": 420}
ROW_BYTES = 768
COMPARE = ("buddy", "gcn", "ncn")


def _graph(dataset, scale, dev):
    if dataset == "ppa":
        from eps_amd import synth
        return synth.ppa_like(seed=3, device=dev)
    return stand_in(dataset, scale, dev)[1].adj_t


def step_tables(a, dev, dataset):
    import torch
    from eps_amd import heuristics, ops
    g = _graph(dataset, a.scale, dev)
    n, nnz = g.n_rows, g.nnz()
    rc, _ = ops.sketch_limits()
    deg = g.degree()
    out = {"step": f"tables_{dataset}", "scale": a.scale, "nodes": n, "entries": nnz, "max_degree": int(deg.max()), "row_chunk": rc,
           "chunked_rows": int((deg > rc).sum()), "chunked_entry_share": round(float(deg[deg > rc].sum()) / max(nnz, 1), 4)}
    own = ops.sketch_own(0, n, dev)
    h1 = ops.sketch_propagate(g.rowptr, g.col, n, own[0], own[1], keep_own=False)
    h2 = ops.sketch_propagate(g.rowptr, g.col, n, h1[0], h1[1], keep_own=True, check=False)
    out["own"] = rate(timed(lambda: ops.sketch_own(0, n, dev), a.reps, a.warmup), ROW_BYTES * n)
    out["hop1"] = rate(timed(lambda: ops.sketch_propagate(g.rowptr, g.col, n, own[0], own[1], keep_own=False, check=False, out=h1),
                             a.reps, a.warmup), ROW_BYTES * (nnz + n))
    out["hop2"] = rate(timed(lambda: ops.sketch_propagate(g.rowptr, g.col, n, h1[0], h1[1], keep_own=True, check=False, out=h2),
                             a.reps, a.warmup), ROW_BYTES * (nnz + 2 * n))
    hll, mh = torch.stack([h1[0], h2[0]]), torch.stack([h1[1], h2[1]])
    ids = torch.arange(n, dtype=torch.int32, device=dev)

    def card():
        s, z, _ = ops.sketch_pair_stats(hll, mh, n, ids, ids, check=False)
        return heuristics.sketch_cardinality(s, z)

    out["card"] = timed(card, a.reps, a.warmup)
    out["mean_C1_over_degree"] = round(float((card()[:, 0, 0][deg > 0] / deg[deg > 0]).mean()), 4)
    return out


def step_pairs(a, dev, dataset):
    import torch
    from eps_amd import candidates, heuristics, ops
    g = _graph(dataset, a.scale, dev)
    n, K = g.n_rows, 2
    hll, mh, _ = g.sketches(K)
    per_pair = 2 * K * ROW_BYTES + 8 * K * K
    out = {"step": f"pairs_{dataset}", "scale": a.scale, "nodes": n, "entries": g.nnz(), "K": K, "bytes_per_pair": per_pair}
    e = torch.randint(0, n, (2, 1 << 22), generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    lo, hi = next(iter(candidates.column_blocks(g)))
    block = candidates.expand_block(g, lo, min(hi, lo + 256))[0]
    for name, pairs in (("uniform", e), ("filter_block", block)):
        u, v = pairs[0].to(torch.int32).contiguous(), pairs[1].to(torch.int32).contiguous()
        b = u.numel()
        rec = rate(timed(lambda: ops.sketch_pair_stats(hll, mh, n, u, v, check=False), a.reps, a.warmup), per_pair * b)
        rec.update(pairs=b, pairs_per_s=round(b / (rec["median_ms"] * 1e-3), 1))
        out[name] = rec
    rec = timed(lambda: heuristics.sketch_features(g, e, K), a.reps, a.warmup)
    rec.update(pairs=e.shape[1], pairs_per_s=round(e.shape[1] / (rec["median_ms"] * 1e-3), 1))
    out["features_uniform"] = rec
    return out


def step_train(a, dev, dataset):
    import torch
    from eps_amd import models
    split_edge, data = stand_in(dataset, a.scale, dev)
    out = {"step": f"train_{dataset}", "scale": a.scale, "nodes": data.num_nodes, "entries": data.adj_t.nnz(), "models": {}}
    for name in COMPARE:
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
    for name in COMPARE:
        args = default_args(dataset, name)
        torch.manual_seed(1)
        model = models.build_model(args, data, dev)
        run = lambda: evaluate.test(model, data, split_edge, evaluate.evaluators[dataset], args.batch_size, args, dev)  # noqa: E731
        out["models"][name] = timed(run, a.reps, a.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--steps", nargs="*", default=list(STEP_SECONDS), choices=sorted(STEP_SECONDS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.step is None:
        common = f"--scale {a.scale} --reps {a.reps} --warmup {a.warmup}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in a.steps)
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("buddy_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    kind, dataset = a.step.split("_")
    res = {"tables": step_tables, "pairs": step_pairs, "train": step_train, "eval": step_eval}[kind](a, dev, dataset)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
