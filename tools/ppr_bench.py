#!/usr/bin/env python3
"""Time `--model ppr` (csrc/ppr_push.hip, heuristics.ppr / ppr_columns, filter_stage.ppr_blocks) on the full-scale stand-ins; one
JSON line per step.

Without --step the tool is a driver: it runs its steps as child processes, each under its own `timeout -k 10`, chained with `&&`
(a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  push_ddi / push_collab / push_ppa: eps_ppr_push from 2^16 seeded sources with 64 uniformly drawn query nodes each, at eps = 1e-4
        and 1e-5 (alpha = 0.15), HIP events, median / min / max of --reps after --warmup: ms, sources per second, traversed entries
        per second (the kernel's own `steps`: one 64-bit atomic add each), the mean rounds, pushes and steps of a source, and the share
        of the sources whose table left LDS; then the same input with table='global' (no LDS attempt).
  filter_ddi / filter_collab / filter_ppa: the scoring section (filter_stage.LAST_TIMING: host clock and HIP events) of
        filter.py --model ppr --keep_top K next to --model jaccard, second run of two (the first also pays the one-off set-up).
  eval_ddi / eval_collab: evaluate.test (the five scoring loops, the pair entry) on the stand-in's lists.

Run:  python tools/ppr_bench.py [--scale 1.0 --reps 5 --warmup 1 --keep 4000000]
"""
import argparse
import json
import os
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_helpers import default_args, stand_in, timed  # noqa: E402

STEP_SECONDS = {"push_ddi": 300, "push_collab": 300, "push_ppa": 420, "filter_ddi": 300, "filter_collab": 420, "filter_ppa": 900,
                "eval_ddi": 300, "eval_collab": 300}
N_SOURCES, N_QUERIES = 1 << 16, 64


def _graph(dataset, scale, dev):
    if dataset == "ppa":
        from eps_amd import synth
        return synth.ppa_like(seed=3, device=dev)
    return stand_in(dataset, scale, dev)[1].adj_t


def step_push(a, dev, dataset):
    import torch
    from eps_amd import heuristics, ops
    g = _graph(dataset, a.scale, dev)
    n = g.n_rows
    gen = torch.Generator(device=dev).manual_seed(9)
    sources = torch.randint(0, n, (N_SOURCES,), generator=gen, device=dev).to(torch.int32)
    qnode = torch.randint(0, n, (N_SOURCES * N_QUERIES,), generator=gen, device=dev).to(torch.int32)
    qptr = torch.arange(N_SOURCES + 1, dtype=torch.int64, device=dev) * N_QUERIES
    lds_nodes, big_row, per_cu, _ = ops.ppr_push_limits(0)
    out = {"step": f"push_{dataset}", "scale": a.scale, "nodes": n, "entries": g.nnz(), "max_degree": int(g.degree().max()),
           "sources": N_SOURCES, "queries_per_source": N_QUERIES, "lds_nodes": lds_nodes, "big_row": big_row, "groups_per_cu": per_cu,
           "runs": {}}
    for eps in (1e-4, 1e-5):
        a16, thr = heuristics.ppr_parameters(heuristics.PPR_ALPHA, eps)
        table_nodes = ops.ppr_touched_bound(n, a16, thr)
        for table in ("auto", "global"):
            st = {}
            run = lambda: ops.ppr_push(g.rowptr, g.col, n, sources, qptr, qnode, a16, thr, heuristics.PPR_MAX_ROUNDS, table=table,  # noqa: E731
                                       check=False, stats=st)
            _, rounds, pushes, steps, capped = run()
            left = st["global_sources"] / N_SOURCES
            rec = timed(run, a.reps, a.warmup)
            total = int(steps.sum())
            rec.update(sources_per_s=round(N_SOURCES / (rec["median_ms"] * 1e-3), 1), entries_per_s=round(total / (rec["median_ms"] * 1e-3), 1),
                       mean_rounds=round(float(rounds.double().mean()), 2), max_rounds=int(rounds.max()),
                       mean_pushes=round(float(pushes.double().mean()), 1), mean_steps=round(total / N_SOURCES, 1),
                       capped=int(capped.sum()), left_lds_share=round(left, 4), table_nodes=table_nodes,
                       workspace_bytes_per_group=ops.ppr_push_limits(table_nodes)[3])
            out["runs"][f"eps={eps:g} table={table}"] = rec
    return out


def step_filter(a, dev, dataset):
    import torch
    from eps_amd import filter_stage
    os.environ["EPS_SYNTH_SCALE"] = str(a.scale)
    out = {"step": f"filter_{dataset}", "scale": a.scale, "keep_top": a.keep, "models": {}}
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            for name in ("ppr", "jaccard"):
                for run in (0, 1):                               # (the first run also pays the one-off set-up: the second is quoted)
                    filter_stage.main(["--dataset", dataset, "--model", name, "--checkpoint", f"{dataset}_{name}||0|{run}.pt",
                                       "--synthetic", "--keep_top", str(a.keep)])
                    torch.cuda.synchronize()
                t = filter_stage.LAST_TIMING
                out["models"][name] = {"scored_s": round(t["scored_s"], 3), "gpu_ms": round(t["gpu_ms"], 1), "candidates": t["candidates"],
                                       "candidates_per_s": round(t["candidates"] / max(t["gpu_ms"] * 1e-3, 1e-9), 1)}
        finally:
            os.chdir(cwd)
    return out


def step_eval(a, dev, dataset):
    from eps_amd import evaluate, models
    split_edge, data = stand_in(dataset, a.scale, dev)
    args = default_args(dataset, "ppr")
    model = models.build_model(args, data, dev)
    pairs = sum(int(split_edge[k][f].size(0)) for k, f in (("eval_train", "edge"), ("valid", "edge"), ("valid", "edge_neg"),
                                                            ("test", "edge"), ("test", "edge_neg")))
    run = lambda: evaluate.test(model, data, split_edge, evaluate.evaluators[dataset], args.batch_size, args, dev)  # noqa: E731
    rec = timed(run, a.reps, a.warmup)
    rec.update(pairs=pairs, pairs_per_s=round(pairs / (rec["median_ms"] * 1e-3), 1))
    return {"step": f"eval_{dataset}", "scale": a.scale, "nodes": data.num_nodes, "entries": data.adj_t.nnz(), "test": rec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--steps", nargs="*", default=list(STEP_SECONDS), choices=sorted(STEP_SECONDS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--keep", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if a.step is None:
        common = f"--scale {a.scale} --keep {a.keep} --reps {a.reps} --warmup {a.warmup}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in a.steps)
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ppr_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    kind, dataset = a.step.split("_")
    res = {"push": step_push, "filter": step_filter, "eval": step_eval}[kind](a, dev, dataset)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
