#!/usr/bin/env python3
"""The job eps_rescore_runs gets in one step of the bench: the key list scan._device_tail passes to ops.rescore_runs on the
bench graph, cut the way rescore_runs_kernel cuts it -- 256-pair chunks, and inside a chunk one unit of work per run of equal
u (bitmap of N(u) set, pairs scored, bitmap cleared: three workgroup barriers a unit).

    python tools/rescore_job_shape.py [--keep_top K] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import eps_amd  # noqa: F401
from eps_amd import ops, scan, synth
from eps_amd.heuristics import node_weight_table

RS_CHUNK, RS_SHORT = 256, 512                      # csrc/rescore.hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep_top", type=int, default=4_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.ppa_like(seed=3, device=dev)
    w = node_weight_table(g, ops.W_AA)
    seen = []
    plain = ops.rescore_runs

    def recording(rowptr, col, fixw, n_nodes, keys):
        seen.append((rowptr, keys))
        return plain(rowptr, col, fixw, n_nodes, keys)

    scan.scan_topk(g, w, args.keep_top)            # (tables, code objects)
    ops.rescore_runs = recording
    try:
        scan.scan_topk(g, w, args.keep_top)
    finally:
        ops.rescore_runs = plain
    assert len(seen) == 1, f"{len(seen)} calls of ops.rescore_runs in one step"
    deg_all = np.diff(seen[0][0].cpu().numpy())
    keys = seen[0][1].cpu().numpy()
    n = keys.size
    u = keys >> 32
    idx = np.arange(n)
    start = np.ones(n, dtype=bool)
    start[1:] = (u[1:] != u[:-1]) | (idx[1:] % RS_CHUNK == 0)
    first = np.flatnonzero(start)
    pairs = np.diff(np.append(first, n))
    deg = deg_all[u[first]]
    long_ = deg > RS_SHORT
    runs = 1 + int((u[1:] != u[:-1]).sum())
    pct = lambda a: "/".join(f"{x:.0f}" for x in np.percentile(a, [10, 50, 90])) if a.size else "-"   # noqa: E731
    per_chunk = np.bincount(first[long_] // RS_CHUNK, minlength=(n + RS_CHUNK - 1) // RS_CHUNK)
    lines = [
        f"graph: ppa_like(seed=3), keep_top {args.keep_top}; keys of one step: {n} pairs, {np.unique(u).size} distinct u, {runs} runs of equal u",
        f"pairs with deg(u) <= {RS_SHORT} (rescore_short_kernel's): {int(pairs[~long_].sum())}",
        f"chunks of {RS_CHUNK} pairs: {per_chunk.size}",
        f"(run, chunk) units with deg(u) > {RS_SHORT}: {int(long_.sum())}   -- units per chunk p10/50/90: {pct(per_chunk)}, max {per_chunk.max()}",
        f"sum of deg(u) over those units: {int(deg[long_].sum())} entries ({deg[long_].sum() * 4 / 1e6:.1f} MB read to set the bitmap; the same again where it is cleared from the row)",
        f"deg(u) per unit p10/50/90: {pct(deg[long_])}",
        f"pairs per unit p10/50/90: {pct(pairs[long_])}, mean {pairs[long_].mean():.1f}",
        f"units per resident workgroup (2 x 256 CUs = 512): {long_.sum() / 512:.0f}",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
