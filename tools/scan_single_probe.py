#!/usr/bin/env python3
"""What the single-round columns cost the filter step's main launch (csrc/scan_pieces.hip: the LEAN body).

On the bench graph, after two steps (so the column pack exists), the live column list of the step's head table is cut with torch ops
alone into the three zones of eps_amd.scan.light_split -- GENERAL | LEAN | LIGHT; a column is lean when it is not light, has at most
256 rows, no two-word hash record and no piece beyond one range of the unit bitmap -- and per zone it prints the columns, the plan
records by kind, the walked half paths, and the time of the main launch (HIP events, 20 launches after 3) over
  * each zone alone and the whole list through the generic body (a library without a lean zone runs exactly this);
  * where the library has the lean body: the lean zone alone through it, and the whole list as the step splits it (the general zone
    alone against its share of the one launch is the cost of its drain as a launch of its own).
The events enclose the whole ops.scan_screen call (argument checks, memsets, launches): short lists hold that host time, differences
between whole-list figures do not.  Nothing is written but stdout.

    python tools/scan_single_probe.py [--nodes N --edges E --keep_top K]
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
    scan.scan_graph(g0, build=True)
    stats = {}
    for _ in range(2):
        scan.scan_topk(g0, w, args.keep_top, stats=stats)
    g, perm = scan.scan_graph(g0)
    screen = scan.screen_weights(g0, g, perm, w)
    ht = screen.head_cur
    assert ht is not None and stats["heads"] and stats["sketch"], "the step ran without heads or sketch pieces: no zones to probe"
    pack = scan.column_pack(g, screen, ht)
    assert pack is not None and scan.variant_is_main(g, screen)
    bar = torch.tensor([float(stats["bar"])], dtype=torch.float32, device=dev)
    live = scan.live_columns(g, screen, ht, 0, 1)
    has_lean = "lean_from" in inspect.signature(ops.scan_screen).parameters
    if has_lean:
        print(f"lean body: {ops._lib.load().eps_scan_lean_blocks_per_cu()} workgroups per CU by the runtime's occupancy figure")

    # ---- the zones, with torch ops
    c = live.long()
    n = g.n_rows
    pptr = ht.plan[0].to(torch.int64).bitwise_and(0xFFFFFFFF)
    recs = ht.plan[1].to(torch.int64).bitwise_and(0xFFFFFFFF)
    rows = g.rowptr[1:] - g.rowptr[:-1]
    first = pptr[c]
    rec1 = recs[first.clamp(max=recs.shape[0] - 1)]
    keys = (rec1[:, 0] & 0x3FFFFFFF) + (rec1[:, 2] >> 16) - (rec1[:, 2] & 0xFFFF)
    light = ((pptr[c + 1] - first) == 1) & ((rec1[:, 0] >> 30) == 1) & (rows[c] <= 64) & (keys <= 2048)
    owner = torch.repeat_interleave(torch.arange(n, device=dev), pptr[1:] - pptr[:-1])
    kind = recs[:, 0] >> 30
    paths = recs[:, 0] & 0x3FFFFFFF
    bad = (kind == 0) | (paths + 3 * rows[owner] > 4 * 8192)
    n_bad = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, owner, bad.to(torch.int64))
    lean = (rows[c] <= 256) & (n_bad[c] == 0) & ~light
    general = ~light & ~lean
    in_list = torch.zeros(n, dtype=torch.bool, device=dev)
    walked_all = int(ht.wpaths.to(torch.int64).bitwise_and(0xFFFFFFFF)[c].sum())
    print(f"live columns {c.numel()}, plan records {int((pptr[c + 1] - pptr[c]).sum())}, walked half paths {walked_all}")
    print("| zone | columns | share | records 00 / 01 / 10 / 11 | walked paths | share | columns of > 256 rows |")
    for name, m in (("general", general), ("lean", lean), ("light", light)):
        in_list.zero_()
        in_list[c[m]] = True
        sel = in_list[owner]
        by_kind = [int(((kind == k) & sel).sum()) for k in range(4)]
        held = int(paths[sel].sum())
        print(f"| {name} | {int(m.sum())} | {100.0 * int(m.sum()) / c.numel():.1f} % | {' / '.join(map(str, by_kind))} | {held} | "
              f"{100.0 * held / max(1, walked_all):.1f} % | {int((rows[c[m]] > 256).sum())} |")

    bounds, cuts = scan.screen_tables(g)
    word = scan.screen_variant(g) | ops.SCAN_SKETCH | (ops.SCAN_WIDE if ht.wide else 0)
    cache = {}
    cap = min(int(scan.HEAD_LIST * scan._capacity(int(2 * scan.SAFETY * args.keep_top), scan._PIECE_SLACK)), ops.SURVIVOR_SLOTS_MAX)

    def timed(name, cols, lean_from=None, light_from=None):
        cols = cols.contiguous()
        if not cols.numel():
            print(f"{name}: no columns")
            return
        light_at = cols.numel() if light_from is None else light_from
        lean_at = light_at if lean_from is None else lean_from
        main, lean_view = cols[:lean_at], cols[lean_at:light_at]
        colrec = scan.column_records(g, screen, cols, ht.plan, ht.heads, cache, (name, cols.data_ptr()))
        extra = {}
        if light_from is not None:
            extra["light_from"] = light_from
        if lean_from is not None:
            extra.update(lean_from=lean_from, lean_batch_from=scan.batch_from(g, lean_view))
        bf = scan.batch_from(g, main)
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

    gen, lea, lit = live[general], live[lean], live[light]
    timed("generic body, general zone alone", gen)
    timed("generic body, lean zone alone", lea)
    timed("generic body, general + lean zones (one launch)", torch.cat([gen, lea]))
    timed("generic body + light kernel, whole list (the step before the lean body)", torch.cat([gen, lea, lit]), None, gen.numel() + lea.numel())
    if has_lean:
        timed("lean body, lean zone alone", lea, 0)
        timed("three zones, whole list as the step splits it", torch.cat([gen, lea, lit]), gen.numel(), gen.numel() + lea.numel())


if __name__ == "__main__":
    main()
