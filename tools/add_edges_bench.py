#!/usr/bin/env python3
"""Time graph.add_edges on its two routes -- the rebuild from the concatenated edge list (no ``base``: two coalescing passes
over every stored entry) against the merge into a resident base graph (``base=``: CSRGraph.with_edges -> eps_csr_merge_count /
_fill) -- on the ddi-, collab- and ppa-like stand-ins; one JSON line per graph.

Without --step the tool is a driver: every graph runs as a child process under its own `timeout -k 10`, chained with `&&` (a
step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it).

  ddi, collab: 100,000 extra edges;  ppa: 4,000,000.  The extras are seeded random node pairs (mirrored by the routes
  themselves); the base graph is built once, outside the timed region, as rank.py does per invocation.
  HIP events around the whole call, each call followed by a synchronise; median of --reps after --warmup.
  Also reported: whether the two routes return equal arrays, the share of the merge route spent sorting the batch, and the byte
  model -- the merge has to read rowptr and col [+ val] and write the new col [+ val]: (rowptr + 2 col [+ 2 val]) bytes at the
  6.29 TB/s a float4 copy reaches on this chip -- as a fraction of the measured merge (library calls alone, and whole route).

Run:  python tools/add_edges_bench.py [--reps 10 --warmup 3]
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

EXTRAS = {"ddi": 100_000, "collab": 100_000, "ppa": 4_000_000}
STEPS = list(EXTRAS)
STEP_SECONDS = 300
HBM_COPY_BYTES_PER_S = 6.29e12


def run_step(a, dev):
    import torch
    from eps_amd import datasets, ops
    from eps_amd.graph import add_edges, merge_keys
    name = a.step
    raw = datasets.load_raw(name, synthetic=True, device=dev)
    n = int(raw["num_nodes"])
    ei = raw["edge_index"]
    ew = raw["edge_weight"] if raw["edge_weight"] is not None else torch.ones(ei.shape[1], device=dev)
    gen = torch.Generator(device=dev).manual_seed(17)
    extra = torch.randint(0, n, (2, EXTRAS[name]), generator=gen, device=dev)
    collab = name == "collab"
    base = add_edges(name, ei, ew, extra[:, :0], n)

    def timed(fn):
        for _ in range(a.warmup):
            out = fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(statistics.median(ts), 3), round(min(ts), 3), out

    res = {"step": name, "nodes": n, "base_nnz": base.nnz(), "extra_edges": EXTRAS[name], "values": collab}
    res["rebuild_ms"], res["rebuild_min_ms"], want = timed(lambda: add_edges(name, ei, ew, extra, n))
    res["merge_ms"], res["merge_min_ms"], got = timed(lambda: add_edges(name, ei, ew, extra, n, base=base))
    res["new_nnz"] = got.nnz()
    res["equal"] = bool(torch.equal(got.rowptr, want.rowptr) and torch.equal(got.col, want.col)
                        and (got.val is None) == (want.val is None) and (got.val is None or torch.equal(got.val, want.val)))
    res["merge_over_rebuild"] = round(res["merge_ms"] / res["rebuild_ms"], 4)
    # the parts of the merge route: the batch (mirror, pack, sort) and the two library calls with the prefix sum between them
    res["sort_ms"], _, xkeys = timed(lambda: merge_keys(extra))
    bval = base.val if collab else None
    res["library_ms"], _, _ = timed(lambda: ops.csr_merge(base.rowptr, base.col, bval, n, xkeys, collab))
    per_entry = 8 if collab else 4
    model_bytes = 8 * (n + 1) + (base.nnz() + got.nnz()) * per_entry          # read the base, write the result
    res["model_bytes"] = model_bytes
    res["model_ms"] = round(model_bytes / HBM_COPY_BYTES_PER_S * 1e3, 4)
    res["model_over_library"] = round(res["model_ms"] / res["library_ms"], 4)
    res["model_over_merge"] = round(res["model_ms"] / res["merge_ms"], 4)
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
        raise SystemExit("add_edges_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    print("RESULT " + json.dumps(run_step(a, torch.device("cuda:0"))), flush=True)


if __name__ == "__main__":
    main()
