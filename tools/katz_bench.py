#!/usr/bin/env python3
"""Time rank.py --model katz's scoring on the full-scale stand-ins and print one JSON line.

  collab (N = 235,868, truncated series): the pair kernel over the valid + test lists (eps_katz_pair_scores; median of
      --reps launches after --warmup), the whole evaluate.test_katz call (five lists on two graphs, cold caches on fresh
      graph objects: transposes, two-path counts), the pair count and the two-hop entries walked from the cheaper side.
  ddi (N = 4,267, exact inverse): the whole evaluate.test_katz call (one dense float64 inverse + gathers).

Run:  python tools/katz_bench.py [--reps 20 --warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    os.environ.pop("EPS_SYNTH_SCALE", None)
    import torch
    import eps_amd  # noqa: F401
    from eps_amd import datasets, evaluate, heuristics, ops

    dev = torch.device("cuda:0")

    def data_for(name):
        _, _, split_edge, data = datasets.get_data(argparse.Namespace(dataset=name, synthetic=True, use_feature=False))
        return split_edge, data.to(dev)

    # ---- collab: the kernel alone, over the validation and test lists
    split_edge, data = data_for("collab")
    g = data.adj_t
    pairs = torch.cat([split_edge["valid"]["edge"], split_edge["valid"]["edge_neg"], split_edge["test"]["edge"],
                       split_edge["test"]["edge_neg"]])
    u = pairs[:, 0].to(dev, torch.int32).contiguous()
    v = pairs[:, 1].to(dev, torch.int32).contiguous()
    gt, p_out, p_in = heuristics._katz_transpose(g)
    coeffs = heuristics.katz_coefficients()
    deg = g.rowptr[1:] - g.rowptr[:-1]
    ul, vl = u.long(), v.long()
    walk = torch.where(p_out[ul] + deg[vl] <= p_in[vl] + deg[ul], p_out[ul], p_in[vl])

    def launch():
        return ops.katz_pair_scores(g.rowptr, g.col, g.val, gt.rowptr, gt.col, gt.val, p_out, p_in, g.n_rows, u, v, coeffs)

    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        launch()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))

    def whole(name):
        se, d = data_for(name)             # fresh graph objects: nothing cached from an earlier call
        args = argparse.Namespace(dataset=name, model="katz")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate.test_katz(None, d, se, evaluate.evaluators[name], 1 << 16, args, dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    whole("collab")                        # (first call: code objects, allocator)
    collab_ms = whole("collab")
    whole("ddi")
    ddi_ms = whole("ddi")
    print(json.dumps({
        "metric": "katz scoring on the stand-ins",
        "collab_kernel_ms": round(statistics.median(times), 4),
        "collab_kernel_ms_min": round(min(times), 4),
        "collab_pairs": int(u.numel()),
        "collab_two_hop_entries": int(walk.sum().item()),
        "collab_max_walk": int(walk.max().item()),
        "collab_test_katz_ms": round(collab_ms, 2),
        "ddi_exact_test_katz_ms": round(ddi_ms, 2),
        "device": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
