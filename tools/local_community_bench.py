#!/usr/bin/env python3
"""Time the local-community indices (`filter.py --model car | cpa | caa | cra | cjc`, csrc/local_community.hip) on the full-scale
stand-ins; one JSON line per step.

Without --step the tool is a driver: it runs its steps as child processes, each under its own `timeout -k 10`, chained with `&&`
(a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  degrees_ddi / degrees_ppa: the degree kernel ALONE (eps_local_community_degrees; lists built outside the timed region) on the
      ddi-like / ppa-like stand-in (EPS_SYNTH_SCALE = --scale), HIP events, median / min / max of --reps after --warmup, on
        edges:  a training-size batch (--batch) of stored edges drawn with a seed -- long lists,
        block:  the candidates with two or more common neighbours of the heaviest filter block, as the block route compacts
                them, the first piece of the entry budget -- short lists.
      ms, and GB/s against the byte model: 4 B per list entry read + 4 B per gamma written + every visited row once (4 B per
      stored entry of row w, for every list entry w).  With them the share of list entries on each of the kernel's three
      regimes (short lists dealt over the lanes; rows streamed against the staged list; rows searched in place).
  filter_ddi / filter_ppa: the scoring section (filter_stage.LAST_TIMING: host clock and HIP events) of
      `filter.py --dataset D --synthetic --model M --keep_top --keep`, second of two runs, for --models (cra next to jaccard),
      with the share of the section spent in the degree kernel (the HIP events ops.py puts around its calls, summed).

Run:  python tools/local_community_bench.py [--scale 1.0 --keep 4000000 --reps 7 --warmup 2 --batch 65536 --models cra jaccard]
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

STEP_SECONDS = {"degrees_ddi": 300, "degrees_ppa": 600, "filter_ddi": 600, "filter_ppa": 1100}


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


def _measure(a, g, u, v, count):
    """The degree kernel on the lists of the pairs (u, v) with their counts: times, the byte model and the regime shares."""
    import torch
    from eps_amd import ops
    short, cap, ratio = ops.local_community_limits()
    ptr, w = ops.pair_cn_list(g.rowptr, g.col, g.n_rows, u, v, check=False, count=count)
    m = int(w.numel())
    rec = {"pairs": int(u.numel()), "entries": m, "mean_list": round(m / max(int(u.numel()), 1), 2), "longest_list": int(count.max().item())}
    if m == 0:
        return rec
    gamma = torch.empty(m, dtype=torch.int32, device=w.device)
    rec.update(timed(lambda: ops.local_community_degrees(g.rowptr, g.col, g.n_rows, ptr, w, check=False, out=gamma), a.reps, a.warmup))
    deg = (g.rowptr[1:] - g.rowptr[:-1])[w.long()]
    length = torch.repeat_interleave(count.to(torch.int64), count.to(torch.int64), output_size=m)
    in_short = length <= short
    in_place = ~in_short & (deg >= 64) & (deg >= ratio * length.clamp(max=cap))
    rows = int(deg.sum().item())
    rec["bytes_model"] = {"list_in": 4 * m, "gamma_out": 4 * m, "rows": 4 * rows}
    rec["GB_per_s"] = round((8 * m + 4 * rows) / (rec["median_ms"] * 1e-3) / 1e9, 1)
    rec["entries_per_s"] = round(m / (rec["median_ms"] * 1e-3), 1)
    rec["regime_share"] = {"short": round(float(in_short.float().mean()), 4), "in_place": round(float(in_place.float().mean()), 4),
                           "staged": round(float((~in_short & ~in_place).float().mean()), 4)}
    rec["gamma_sum"] = int(gamma.sum(dtype=torch.int64).item())
    return rec


def step_degrees(a, dev, dataset):
    import torch
    from eps_amd import candidates, filter_stage, heuristics, ops
    g = _graph(dataset, a.scale, dev)
    short, cap, ratio = ops.local_community_limits()
    out = {"step": f"degrees_{dataset}", "scale": a.scale, "nodes": g.n_rows, "stored_entries": g.nnz(),
           "limits": {"short": short, "cap": cap, "inplace_ratio": ratio}}
    # a training-size batch of stored edges
    row, col, _ = g.coo()
    pick = torch.randperm(g.nnz(), generator=torch.Generator().manual_seed(0))[:a.batch].to(dev)
    u, v = row[pick].to(torch.int32).contiguous(), col[pick].to(torch.int32).contiguous()
    count = ops.pair_cn_list_count(g.rowptr, g.col, g.n_rows, u, v, check=False)
    out["edges"] = _measure(a, g, u, v, count)
    # the heaviest filter block's candidates with two or more common neighbours, one piece of the entry budget
    paths = candidates.path_counts(g)
    blocks = list(candidates.column_blocks(g))
    lo, hi = max(blocks, key=lambda b: int(paths[b[0]:b[1]].sum().item()))
    blk = filter_stage._counted_block(g, lo, hi, count_free=False)
    n = int(blk.cand_u.numel())
    cols = torch.arange(lo, hi, dtype=torch.int32, device=dev)
    v_all = torch.repeat_interleave(cols, blk.colptr[1:] - blk.colptr[:-1], output_size=n)
    cn = blk.cn.to(torch.int32)
    pos = torch.nonzero(cn >= 2).squeeze(1)
    c_lo, c_hi = heuristics._budget_cuts(cn[pos], int(heuristics.LOCAL_COMMUNITY_BUDGET))[0]
    pos = pos[c_lo:c_hi]
    out["block"] = dict(columns=[lo, hi], blocks=len(blocks), candidates=n, listed_candidates=int((cn >= 2).sum().item()),
                        mean_cn=round(float(cn.float().mean()), 3), **_measure(a, g, blk.cand_u[pos].contiguous(), v_all[pos], cn[pos]))
    return out


def step_filter(a, dev, dataset):
    import torch
    from eps_amd import filter_stage, ops
    os.environ["EPS_SYNTH_SCALE"] = str(a.scale)
    out = {"step": f"filter_{dataset}", "scale": a.scale, "keep_top": a.keep, "models": {}}
    names = ("local_community_degrees_kernel", "local_community_scores_kernel", "pair_cn_list_kernel<fill>")
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            for name in a.models:
                for run in (0, 1):                               # (the first run also pays the one-off set-up: the second is quoted)
                    ops.KERNEL_EVENTS, ops.EVENT_NAMES = [], names
                    try:
                        filter_stage.main(["--dataset", dataset, "--model", name, "--checkpoint", f"{dataset}_{name}||0|{run}.pt",
                                           "--synthetic", "--keep_top", str(a.keep)])
                        torch.cuda.synchronize()
                        ms = {k: round(sum(e0.elapsed_time(e1) for kk, e0, e1, _ in ops.KERNEL_EVENTS if kk == k), 1) for k in names}
                    finally:
                        ops.KERNEL_EVENTS, ops.EVENT_NAMES = None, None
                t = filter_stage.LAST_TIMING
                out["models"][name] = {"scored_s": round(t["scored_s"], 3), "gpu_ms": round(t["gpu_ms"], 1), "candidates": t["candidates"],
                                       "kernel_ms": ms}
        finally:
            os.chdir(cwd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--steps", nargs="*", default=["degrees_ddi", "filter_ddi", "degrees_ppa", "filter_ppa"], choices=sorted(STEP_SECONDS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--keep", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64 * 1024)
    ap.add_argument("--models", nargs="*", default=["cra", "jaccard"])
    a = ap.parse_args()
    if a.step is None:
        common = f"--scale {a.scale} --keep {a.keep} --reps {a.reps} --warmup {a.warmup} --batch {a.batch} --models {' '.join(a.models)}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in a.steps)
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("local_community_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    kind, dataset = a.step.split("_")
    res = {"degrees": step_degrees, "filter": step_filter}[kind](a, dev, dataset)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
