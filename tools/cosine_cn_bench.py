#!/usr/bin/env python3
"""Time the cosine common-neighbour filters ('simplecos' / 'mlpcos') on the ppa-like and collab-like stand-ins; one JSON line.

  prologue: eps_cos_node_features and eps_edge_cosines (half entries + mirror writes) on the graph, median of --reps after
      --warmup, against the byte model of their gathers (one padded feature row per stored entry for the smoothing, one per
      UNDIRECTED entry for the cosines; x / xhat rows of 128-byte multiples).
  eval lists: heuristics.cosine_common_neighbors over the five evaluation lists of rank.py (cosine graph cached).
  filter: filter.py --model simplecos --keep_top K (HIP events around the scoring section, filter_stage.LAST_TIMING) through
      the fused signed expansion and through candidate lists + the pair kernel, both on the full-size graph (and, with
      --small_scale, both again on a scaled-down stand-in).  "candidates" counts what a route expanded: the fused route
      stops expanding once its bar has saturated at 1.0 (the blocks it scored / cut / skipped are listed).

Run:  python tools/cosine_cn_bench.py [--datasets ppa,collab --keep_top 4000000 --small_scale 0.1 --reps 10 --warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return statistics.median(ts)


def filter_ms(dataset, keep, fused, scale):
    from eps_amd import filter_stage
    if scale is None:
        os.environ.pop("EPS_SYNTH_SCALE", None)
    else:
        os.environ["EPS_SYNTH_SCALE"] = str(scale)
    filter_stage.COSINE_FUSED = fused
    try:
        with tempfile.TemporaryDirectory() as d:
            cwd = os.getcwd()
            os.chdir(d)
            try:
                filter_stage.main(["--dataset", dataset, "--model", "simplecos", "--checkpoint", f"{dataset}_simplecos||0|0.pt",
                                   "--synthetic", "--use_feature", "True", "--keep_top", str(keep)])
            finally:
                os.chdir(cwd)
    finally:
        filter_stage.COSINE_FUSED = True
    t = dict(filter_stage.LAST_TIMING)
    r = {"gpu_ms": round(t["gpu_ms"], 3), "wall_s": round(t["scored_s"], 3), "candidates": t["candidates"],
         "scale": scale or 1.0, "route": "fused" if fused else "list+pair"}
    if fused:
        kinds = [k for _, _, _, k in filter_stage.LAST_COSINE_CUTS]
        r["blocks"] = {k: kinds.count(k) for k in ("scored", "cut", "skipped")}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="ppa,collab")
    ap.add_argument("--keep_top", type=int, default=4_000_000)
    ap.add_argument("--small_scale", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_filter", action="store_true")
    a = ap.parse_args()
    os.environ.pop("EPS_SYNTH_SCALE", None)
    import torch
    import eps_amd  # noqa: F401
    from eps_amd import datasets, heuristics, ops, scan

    dev = torch.device("cuda:0")
    out = {}
    for name in a.datasets.split(","):
        os.environ.pop("EPS_SYNTH_SCALE", None)
        _, _, split_edge, data = datasets.get_data(argparse.Namespace(dataset=name, synthetic=True, use_feature=True))
        data = data.to(dev)
        g = data.adj_t
        f = data.x.shape[1]
        ld = (f + ops.COS_ROW_FLOATS - 1) // ops.COS_ROW_FLOATS * ops.COS_ROW_FLOATS
        x = torch.zeros((g.n_rows, ld), dtype=torch.float32, device=dev)
        x[:, :f] = data.x
        x = x[:, :f]
        rev = scan.reverse_positions(g)
        xhat = ops.cos_node_features(g.rowptr, g.col, g.val, x)
        t_node = timed(lambda: ops.cos_node_features(g.rowptr, g.col, g.val, x), a.reps, a.warmup)
        t_edge = timed(lambda: ops.edge_cosines(g.rowptr, g.col, xhat, rev), a.reps, a.warmup)
        t_edge_full = timed(lambda: ops.edge_cosines(g.rowptr, g.col, xhat, None), a.reps, a.warmup)
        nnz, row_b = g.nnz(), ld * 4
        b_node = nnz * (row_b + 4 + (4 if g.val is not None else 0)) + g.n_rows * 2 * row_b
        b_edge = nnz // 2 * (row_b + 4 + 8) + nnz * 8 + g.n_rows * row_b     # gathers + col / revpos reads + two writes
        r = {"nodes": g.n_rows, "nnz": nnz, "f": f, "row_bytes": row_b,
             "node_features_ms": round(t_node, 3), "node_features_model_gb": round(b_node / 1e9, 2),
             "node_features_tbs": round(b_node / t_node / 1e9, 2),
             "edge_cosines_ms": round(t_edge, 3), "edge_cosines_model_gb": round(b_edge / 1e9, 2),
             "edge_cosines_tbs": round(b_edge / t_edge / 1e9, 2), "edge_cosines_all_entries_ms": round(t_edge_full, 3)}
        lists = [split_edge["eval_train"]["edge"], split_edge["valid"]["edge"], split_edge["valid"]["edge_neg"],
                 split_edge["test"]["edge"], split_edge["test"]["edge_neg"]]
        lists = [e.t().to(dev) for e in lists]
        heuristics.cosine_common_neighbors(g, data.x, lists[0])
        r["eval_pairs"] = int(sum(e.shape[1] for e in lists))
        r["eval_lists_ms"] = round(timed(lambda: [heuristics.cosine_common_neighbors(g, data.x, e) for e in lists],
                                         a.reps, a.warmup), 3)
        del xhat, x, data, g
        torch.cuda.empty_cache()
        if not a.no_filter:
            r["filter_fused"] = filter_ms(name, a.keep_top, True, None)
            r["filter_list_pair"] = filter_ms(name, a.keep_top, False, None)
            if a.small_scale:
                r["filter_fused_small"] = filter_ms(name, a.keep_top, True, a.small_scale)
                r["filter_list_pair_small"] = filter_ms(name, a.keep_top, False, a.small_scale)
        out[name] = r
        print(name, json.dumps(r), flush=True)
    print(json.dumps({"cosine_cn_bench": out}))


if __name__ == "__main__":
    main()
