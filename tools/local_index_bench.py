#!/usr/bin/env python3
"""Time the local-index filters (`filter.py --model jaccard | pa`, csrc/local_index.hip) on the full-scale stand-ins; one JSON
line per step.

Without --step the tool is a driver: it runs its steps as child processes, each under its own `timeout -k 10`, chained with `&&`
(a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  kernel_collab / kernel_ppa: the column kernel ALONE on the largest column block of the collab-like / ppa-like stand-in
      (EPS_SYNTH_SCALE = --scale) as the filter's block route lays it out (list + common-neighbour count; the expansion is outside
      the timed region), per index: HIP events, median / min / max of --reps after --warmup,
        score:     every slot's score written (ms, and GB/s against 4 B cand_u + 4 B count + 4 B score per candidate),
        survivors: the three launches against a bar (the block's own --keep-th best score), nothing written but the survivors
                   (GB/s against the 8 B per candidate that the count launch reads; the fill launch skips slices without one).
  filter_collab / filter_ppa: the scoring section (filter_stage.LAST_TIMING: host clock and HIP events) of
      `filter.py --dataset D --synthetic --model M --keep_top --keep`, second of two runs, with the survivor path and with every
      block scored in full (filter_stage.LOCAL_INDEX_CUT = False), and the column kernel's share of the section (the HIP events
      ops.py puts around its calls, summed, over the section's).

Run:  python tools/local_index_bench.py [--scale 1.0 --keep 4000000 --reps 7 --warmup 2 --models jaccard pa]
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = {"kernel_collab": 300, "kernel_ppa": 600, "filter_collab": 600, "filter_ppa": 900}
BYTES_SCORE, BYTES_SURVIVORS = 12, 8


def timed(fn, reps, warmup):
    import torch
    ts = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def _graph(dataset, scale, dev):
    import torch
    from eps_amd import datasets
    from eps_amd.graph import add_edges
    os.environ["EPS_SYNTH_SCALE"] = str(scale)
    ei, ew, _, data = datasets.get_data(argparse.Namespace(dataset=dataset, synthetic=True, use_feature=False))
    return add_edges(dataset, ei.to(dev), ew.to(dev), torch.zeros((2, 0), dtype=torch.long, device=dev), data.num_nodes)


def step_kernel(a, dev, dataset):
    import torch
    from eps_amd import candidates, filter_stage, ops
    g = _graph(dataset, a.scale, dev)
    paths = candidates.path_counts(g)
    blocks = list(candidates.column_blocks(g))
    lo, hi = max(blocks, key=lambda b: int(paths[b[0]:b[1]].sum().item()))
    out = {"step": f"kernel_{dataset}", "scale": a.scale, "nodes": g.n_rows, "entries": g.nnz(), "blocks": len(blocks),
           "columns": [lo, hi], "indices": {}}
    blk = filter_stage._counted_block(g, lo, hi, count_free=False)
    n = int(blk.cand_u.numel())
    out["candidates"], out["count_form"] = n, str(blk.cn.dtype).replace("torch.", "")
    score = torch.empty(n, dtype=torch.float32, device=dev)
    args = (g.rowptr, g.n_rows, lo, hi, blk.colptr, blk.cand_u, blk.cn)
    for name in a.models:
        rec = {}
        ops.local_index_columns(*args, name, out=score, check=False)
        keep = min(a.keep, n)
        bar = ops.kth_largest(score, keep) if n else torch.zeros(1, device=dev)
        st = {}
        ops.local_index_columns(*args, name, bar=bar, capacity=filter_stage.CUT_CAPACITY, check=False, stats=st)
        rec["bar"], rec["survivors"] = float(bar.item()), st["n_surv"]
        rec["score"] = timed(lambda: ops.local_index_columns(*args, name, out=score, check=False), a.reps, a.warmup)
        rec["survivors_run"] = timed(lambda: ops.local_index_columns(*args, name, bar=bar, capacity=filter_stage.CUT_CAPACITY, check=False),
                                     a.reps, a.warmup)
        rec["score"]["GB_per_s"] = round(n * BYTES_SCORE / (rec["score"]["median_ms"] * 1e-3) / 1e9, 1)
        rec["survivors_run"]["GB_per_s"] = round(n * BYTES_SURVIVORS / (rec["survivors_run"]["median_ms"] * 1e-3) / 1e9, 1)
        out["indices"][name] = rec
    return out


def step_filter(a, dev, dataset):
    import torch
    from eps_amd import filter_stage, ops
    os.environ["EPS_SYNTH_SCALE"] = str(a.scale)
    out = {"step": f"filter_{dataset}", "scale": a.scale, "keep_top": a.keep, "models": {}}
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            for name in a.models:
                rec = {}
                for label, cut in (("survivors", True), ("scored_in_full", False)):
                    filter_stage.LOCAL_INDEX_CUT = cut
                    for run in (0, 1):                               # (the first run also pays the one-off set-up: the second is quoted)
                        ops.KERNEL_EVENTS, ops.EVENT_NAMES = [], ("local_index_columns_kernel",)
                        try:
                            filter_stage.main(["--dataset", dataset, "--model", name, "--checkpoint", f"{dataset}_{name}||0|{run}.pt",
                                               "--synthetic", "--keep_top", str(a.keep)])
                            torch.cuda.synchronize()
                            kernel_ms = sum(e0.elapsed_time(e1) for k, e0, e1, _ in ops.KERNEL_EVENTS if k == "local_index_columns_kernel")
                        finally:
                            ops.KERNEL_EVENTS, ops.EVENT_NAMES = None, None
                    t = filter_stage.LAST_TIMING
                    cuts = [c[3] for c in filter_stage.LAST_LOCAL_INDEX_CUTS]
                    rec[label] = {"scored_s": round(t["scored_s"], 3), "gpu_ms": round(t["gpu_ms"], 1), "candidates": t["candidates"],
                                  "column_kernel_ms": round(kernel_ms, 1), "column_kernel_share": round(kernel_ms / max(t["gpu_ms"], 1e-9), 3),
                                  "blocks": len(cuts), "blocks_cut": cuts.count("cut")}
                out["models"][name] = rec
        finally:
            filter_stage.LOCAL_INDEX_CUT = True
            os.chdir(cwd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--steps", nargs="*", default=["kernel_collab", "filter_collab", "kernel_ppa", "filter_ppa"], choices=sorted(STEP_SECONDS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--keep", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", nargs="*", default=["jaccard", "pa"])
    a = ap.parse_args()
    if a.step is None:
        common = f"--scale {a.scale} --keep {a.keep} --reps {a.reps} --warmup {a.warmup} --models {' '.join(a.models)}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in a.steps)
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("local_index_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    kind, dataset = a.step.split("_")
    res = {"kernel": step_kernel, "filter": step_filter}[kind](a, dev, dataset)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
