#!/usr/bin/env python3
"""Measure the per-node cut (eps_segment_topk, filter.py --keep_per_node k); one JSON line per step.

Without --step the tool is a driver: it runs its two steps as child processes, each under its own `timeout -k 10`, chained with
`&&` (a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  kernel: on the ppa-like stand-in (EPS_SYNTH_SCALE = --scale), Adamic-Adar, k = --k, per column block of the filter stage and in
      total, HIP events, median of --reps after --warmup:
        (a) the fused expansion of the block (candidates + scores),
        (b) ops.segment_topk on the block (its tensor-op prologue -- lengths, prefix, hand-out order -- included; the
            library call alone is reported next to it),
        (c) the same selection with tensor ops on the same block: a stable descending sort by score, a stable sort by segment
            id, a rank-in-segment cut.  Its output is compared to the kernel's before anything is timed.
      Also (b) split by the kernel's work class (one call per class on the block's segments of that class alone), and the gate:
      on the largest block (b) must not be slower than (c).  --ref_blocks largest: (c) on the largest block only.
  filter: wall time of `filter.py --dataset ppa --synthetic --model adamic_ogb --keep_per_node k` (second of two runs).

Run:  python tools/per_node_bench.py [--scale 1.0 --k 8 --reps 10 --warmup 3 --ref_blocks all]
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = {"kernel": 900, "filter": 600}


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 3), round(min(ts), 3)


def tensor_op_cut(colptr, score, k):
    """(c): positions of the k best per segment by two library sorts and a rank-in-segment cut; ascending."""
    import torch
    n = score.numel()
    seg = torch.searchsorted(colptr[1:].contiguous(), torch.arange(n, device=score.device), right=True)
    by_score = torch.sort(score + 0.0, descending=True, stable=True).indices       # (+ 0.0: the two zeros tie, as under eps_ordered_bits)
    by_seg = torch.sort(seg[by_score], stable=True)
    pos = by_score[by_seg.indices]                                                 # segment by segment, each in the declared order
    rank = torch.arange(n, device=score.device) - colptr[by_seg.values]
    return torch.sort(pos[rank < k]).values


def _graph(scale, dev):
    import torch
    from eps_amd import datasets, ops
    from eps_amd.graph import add_edges
    from eps_amd.heuristics import node_weight_table
    os.environ["EPS_SYNTH_SCALE"] = str(scale)
    ei, ew, _, data = datasets.get_data(argparse.Namespace(dataset="ppa", synthetic=True, use_feature=False))
    g = add_edges("ppa", ei.to(dev), ew.to(dev), torch.zeros((2, 0), dtype=torch.long, device=dev), data.num_nodes)
    return g, node_weight_table(g, ops.W_AA)


def step_kernel(a, dev):
    import torch
    from eps_amd import candidates, ops
    g, w = _graph(a.scale, dev)
    blocks = list(candidates.column_blocks(g))
    out = {"step": "kernel", "scale": a.scale, "k": a.k, "nodes": g.n_rows, "blocks": []}
    held = None

    def reference(rec, blk, got):
        want = tensor_op_cut(blk.colptr, blk.score, a.k)
        rec["tensor_ops_equal"] = bool(torch.equal(want, got))
        if not rec["tensor_ops_equal"]:
            raise SystemExit("per_node_bench: the tensor-op formulation and the kernel disagree on block " + json.dumps(rec))
        del want
        rec["tensor_ops_ms"], _ = timed(lambda: tensor_op_cut(blk.colptr, blk.score, a.k), a.reps, a.warmup)

    def kernel_only(colptr, score, k):
        """the library call alone: the prologue's tensors made once, outside the timed region"""
        lens = colptr[1:] - colptr[:-1]
        outptr = torch.zeros(colptr.numel(), dtype=torch.int64, device=dev)
        torch.cumsum(torch.clamp(lens, max=k), 0, out=outptr[1:])
        order = torch.argsort(lens, descending=True, stable=True).to(torch.int32)
        res = torch.empty(int(outptr[-1].item()), dtype=torch.int64, device=dev)
        return lambda: ops._call("eps_segment_topk", dev, colptr, None, score, colptr.numel() - 1, k, outptr, order, res)

    for lo, hi in blocks:
        blk = candidates.expand_block_lazy(g, lo, hi, w, want_score=True)
        n = int(blk.cand_u.numel())
        lens = blk.colptr[1:] - blk.colptr[:-1]
        rec = {"columns": [lo, hi], "candidates": n, "longest_column": int(lens.max().item()) if lens.numel() else 0}
        rec["expand_ms"], _ = timed(lambda: candidates.expand_block_lazy(g, lo, hi, w, want_score=True), a.reps, a.warmup)
        got = ops.segment_topk(blk.colptr, blk.score, a.k)
        rec["kept"] = int(got.numel())
        rec["segment_topk_ms"], rec["segment_topk_min_ms"] = timed(lambda: ops.segment_topk(blk.colptr, blk.score, a.k), a.reps, a.warmup)
        rec["library_call_ms"], _ = timed(kernel_only(blk.colptr, blk.score, a.k), a.reps, a.warmup)
        # by work class: the block's segments of one class alone (their colptr / counts layout over the same score array)
        edges = (0, ops.SEGMENT_TOPK_WAVE_MAX, ops.SEGMENT_TOPK_LDS_MAX, 1 << 62)
        rec["classes"] = {}
        for name, lo_len, hi_len in (("wave", -1, edges[1]), ("lds", edges[1], edges[2]), ("stream", edges[2], edges[3])):
            m = (lens > lo_len) & (lens <= hi_len)
            starts, cnts = blk.colptr[:-1][m].contiguous(), lens[m].contiguous()
            sub = torch.cat([starts, starts[-1:] + cnts[-1:]]) if starts.numel() else torch.zeros(1, dtype=torch.int64, device=dev)
            entry = {"segments": int(starts.numel()), "candidates": int(cnts.sum().item())}
            if starts.numel():
                entry["ms"], _ = timed(lambda: ops.segment_topk(sub, blk.score, a.k, counts=cnts), a.reps, a.warmup)
            rec["classes"][name] = entry
        out["blocks"].append(rec)
        print("block " + json.dumps(rec), file=sys.stderr, flush=True)      # (progress: a full-scale run is minutes long)
        if a.ref_blocks == "all":
            reference(rec, blk, got)
        elif held is None or n > held[0]["candidates"]:
            held = (rec, blk, got)                                   # (the largest block so far stays resident for (c))
        del blk, got
    if held is not None:
        reference(*held)
    largest = max(out["blocks"], key=lambda r: r["candidates"])
    tot = lambda key: round(sum(r[key] for r in out["blocks"] if key in r), 3)      # noqa: E731
    out["total"] = {"candidates": sum(r["candidates"] for r in out["blocks"]), "kept": sum(r["kept"] for r in out["blocks"]),
                    "expand_ms": tot("expand_ms"), "segment_topk_ms": tot("segment_topk_ms"), "library_call_ms": tot("library_call_ms"),
                    "tensor_ops_ms": tot("tensor_ops_ms") if a.ref_blocks == "all" else None}
    out["largest_block"] = {"candidates": largest["candidates"], "segment_topk_ms": largest["segment_topk_ms"],
                            "tensor_ops_ms": largest["tensor_ops_ms"],
                            "ratio_tensor_ops_over_kernel": round(largest["tensor_ops_ms"] / largest["segment_topk_ms"], 2)}
    out["gate_kernel_not_slower"] = bool(largest["segment_topk_ms"] <= largest["tensor_ops_ms"])
    return out


def step_filter(a, dev):
    import torch
    from eps_amd import filter_stage
    os.environ["EPS_SYNTH_SCALE"] = str(a.scale)
    out = {"step": "filter", "scale": a.scale, "k": a.k}
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            for run in (0, 1):                                       # (the first run also pays the one-off set-up: the second is quoted)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                name = filter_stage.main(["--dataset", "ppa", "--model", "adamic_ogb", "--checkpoint", f"ppa_adamic_ogb||0|{run}.pt",
                                          "--synthetic", "--keep_per_node", str(a.k)])
                torch.cuda.synchronize()
                out["command_s"] = round(time.perf_counter() - t0, 3)
                out["scored_s"] = round(filter_stage.LAST_TIMING["scored_s"], 3)
                out["candidates"] = filter_stage.LAST_TIMING["candidates"]
            out["rows"] = int(torch.load(name).shape[0])
        finally:
            os.chdir(cwd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref_blocks", choices=["all", "largest"], default="all")
    a = ap.parse_args()
    if a.step is None:
        common = f"--scale {a.scale} --k {a.k} --reps {a.reps} --warmup {a.warmup} --ref_blocks {a.ref_blocks}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in ("kernel", "filter"))
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("per_node_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    res = {"kernel": step_kernel, "filter": step_filter}[a.step](a, dev)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
