#!/usr/bin/env python3
"""What the light single-piece columns cost the filter step's main launch (csrc/scan_pieces.hip, csrc/scan_light.hip).

On the bench graph, after two steps (so the column pack exists), the live column list of the step's head table is split with torch
ops alone -- a column is LIGHT when it has exactly one plan record, of the packed kind, at most 64 rows and at most 2048 paths +
known edges -- and the main launch is timed under HIP events (20 launches after 3) over
  * the light columns alone, the remaining live columns alone and the whole live list, all through the piece kernel (a library
    whose eps_scan_screen has no light zone runs exactly this part: the upper bound of what a lean kernel for them can win);
  * where the library has the light kernel: the light columns alone through it, and the whole list split as the step splits it --
    with the line above, the bracket-free breakdown of the call's two launches.
The events enclose the whole ops.scan_screen call (argument checks, the status and ticket memsets, the launches): the figures of the
short lists hold that host and start-up time, differences between whole-list figures do not.
It also prints the class histogram of the one-piece columns of at most 64 rows.  Run it in two processes; nothing is written but stdout.

    python tools/scan_light_probe.py [--nodes N --edges E --keep_top K]
"""
import argparse
import inspect
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=576_289)
    ap.add_argument("--edges", type=int, default=21_231_931)
    ap.add_argument("--keep_top", type=int, default=4_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import eps_amd  # noqa: F401
    from eps_amd import ops, scan, synth
    from eps_amd.heuristics import node_weight_table

    dev = torch.device("cuda:0")
    g0 = synth.ppa_like(seed=3, device=dev, n_nodes=args.nodes, n_undirected=args.edges)
    w = node_weight_table(g0, ops.W_AA)
    scan.scan_graph(g0, build=True)           # (the hubs-first copy the step scans: built once per graph, as bench.py does)
    stats = {}
    for _ in range(2):
        scan.scan_topk(g0, w, args.keep_top, stats=stats)
    g, perm = scan.scan_graph(g0)
    screen = scan.screen_weights(g0, g, perm, w)
    ht = screen.head_cur
    assert ht is not None and stats["heads"] and stats["sketch"], "the step ran without heads or sketch pieces: no light zone to probe"
    pack = scan.column_pack(g, screen, ht)
    assert pack is not None and scan.variant_is_main(g, screen)
    bar = torch.tensor([float(stats["bar"])], dtype=torch.float32, device=dev)
    live = scan.live_columns(g, screen, ht, 0, 1)
    has_light = "light_from" in inspect.signature(ops.scan_screen).parameters

    # ---- the split, with torch ops
    c = live.long()
    pptr = ht.plan[0].to(torch.int64).bitwise_and(0xFFFFFFFF)
    first = pptr[c]
    rec = ht.plan[1][first.clamp(max=ht.plan[1].shape[0] - 1)].to(torch.int64).bitwise_and(0xFFFFFFFF)
    deg = g.rowptr[c + 1] - g.rowptr[c]
    paths = rec[:, 0] & 0x3FFFFFFF
    keys = paths + (rec[:, 2] >> 16) - (rec[:, 2] & 0xFFFF)
    one_piece = ((pptr[c + 1] - first) == 1) & ((rec[:, 0] >> 30) == 1) & (deg <= 64)
    light = one_piece & (keys <= 2048)
    hx = ht.heads[c, 0].to(torch.int64).bitwise_and(0xFFFFFFFF)
    walked_all = int((ht.wpaths.to(torch.int64).bitwise_and(0xFFFFFFFF)[c]).sum())
    print(f"live columns {c.numel()}, walked half paths of the live list {walked_all}")
    print("one-piece packed columns of <= 64 rows, by paths + known edges:")
    print("| paths + known edges | columns | share of live | walked paths held | mean walked rows |")
    for top in (1024, 2048, 4096, 8192):
        m = one_piece & (keys <= top)
        n = int(m.sum())
        held = int(paths[m].sum())
        rows = float((deg[m] - hx[m]).clamp(min=0).to(torch.float64).mean()) if n else 0.0
        print(f"| <= {top} | {n} | {100.0 * n / c.numel():.1f} % | {held} ({100.0 * held / max(1, walked_all):.1f} %) | {rows:.1f} |")

    bounds, cuts = scan.screen_tables(g)
    word = scan.screen_variant(g) | ops.SCAN_SKETCH | (ops.SCAN_WIDE if ht.wide else 0)
    cache = {}
    cap = min(int(scan.HEAD_LIST * scan._capacity(int(2 * scan.SAFETY * args.keep_top), scan._PIECE_SLACK)), ops.SURVIVOR_SLOTS_MAX)

    def timed(name, cols, light_from=None):
        cols = cols.contiguous()
        if not cols.numel():
            print(f"{name}: no columns")
            return
        main = cols if light_from is None else cols[:light_from]
        colrec = scan.column_records(g, screen, cols, ht.plan, ht.heads, cache, (name, cols.data_ptr()))
        bf = scan.batch_from(g, main)
        extra = {} if light_from is None else {"light_from": light_from}
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ts, slots = [], None
        for i in range(args.warmup + args.launches):
            walked = ops.Survivors(cap, bar, dev, prefill=False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.scan_screen(g.rowptr, g.col, scan.reverse_positions(g), screen.fx32, cuts, bounds, g.n_rows, cols, screen.shift, walked,
                            status, word, None, None, ht.wpaths, screen.ssum, screen.smax, ht.plan, ht.heads, bf, screen.rowrec, colrec,
                            pack, **extra)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(1e3 * e0.elapsed_time(e1))
            slots = walked.counts()[0]
        print(f"{name}: columns {cols.numel()}, mean {statistics.mean(ts):.1f} us (min {min(ts):.1f}, max {max(ts):.1f}), "
              f"slots handed out {slots}, status {int(status)}")

    lite, rest = live[light], live[~light]
    timed("piece kernel, light columns alone", lite)
    timed("piece kernel, remaining live columns alone", rest)
    timed("piece kernel, whole live list", live)
    if has_light:
        timed("light kernel, light columns alone", lite, 0)
        timed("both kernels, whole list as the step splits it", torch.cat([rest, lite]), rest.numel())

if __name__ == "__main__":
    main()
