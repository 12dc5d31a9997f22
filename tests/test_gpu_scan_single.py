"""The LEAN body of the main scan launch (csrc/scan_pieces.hip; eps_amd.scan.light_split: GENERAL | LEAN | LIGHT) on a hand-made graph.

The graph is the one of test_gpu_scan_light.py (65 536 ids scanned as labelled, 32 windows: one node tied to 2400 base nodes, 32 hubs,
a sparse random base on ids 64 .. 50 000, GADGET columns with rows of their own) with gadgets for the lean body's three piece kinds.
Pieces are planned greedily from id 0, so a gadget's targets decide its pieces: targets far apart in the base's upper half give ONE
packed record (a sketch piece); targets below id 16 384 give a 16-bit direct piece [0, ..) -- or a 32-bit one below id 8192 when the
column's row sum is too large for 15-bit fields (256 rows whose node weight is set to 0.5) --; both give direct followed by sketch.
A column v inside the base with targets below it gets the direct piece [0, v): its span is v, its last field v - 1 (16-bit fields
for 8192 < v <= 16 384; below that both kinds reach v and the planner keeps the exact 32-bit sums).

Every case compares the refined survivor list of scan._launch with the zones on -- all three, and lean without light, where the
small columns run in the lean body too -- against the same launch with the zones off: keys and sums equal as sorted lists,
n_candidates and the status word equal, after asserting from the split that the columns meant to be lean ARE lean.  The backstop
cases call ops.scan_screen with a lean zone made by hand.  scan_topk is held to SciPy on this graph and, on rmat_graph(15, 14, 7)
under hubs-first labels, zones on to zones off -- that graph runs no sketch launch for AA and RA (its fixed point is too fine for a
sketch slot never to wrap), so rmat_graph(17, 10, 3), which does, is held the same way with a lean zone asserted.

A lean column of more than nine pieces (cuts of pieces 1..8 from the pack, later ones from the row records) cannot be had in 65 536
ids: a direct piece spans 8192 ids whatever it holds.  It has a graph of its own, 2^20 ids wide: with windows wider than a 16-bit
direct piece and more than 4096 paths of the column in each, the planner makes one packed record per window."""
import numpy as np
import pytest
import torch

from test_gpu_scan_light import BASE_HI, BIG_DEG, HUB_DEG, N, N_HUB, TARGET_LO, _Builder, _host_rows

pytestmark = pytest.mark.gpu

SPAN16_V, SPAN32_V, LOW32_V = 9000, 7000, 6000
RESERVED = np.concatenate([np.arange(5990, 6010), np.arange(6990, 7040), np.arange(8990, 9040), np.arange(1000, 1002), np.arange(2000, 2002)])
SWITCHES = ("SMALL_SET", "HEAD_MIN_PATHS", "SKETCH_MIN_PATHS", "LIGHT_COLUMNS", "LEAN_COLUMNS", "SKETCH_SET", "LEAN_ROWS")


class _B(_Builder):
    lo, hi = TARGET_LO, BASE_HI

    def within(self, lo, hi):
        self.lo, self.hi = lo, hi
        return self

    def targets(self, m, avoid=()):
        pool = np.setdiff1d(np.arange(self.lo, self.hi), RESERVED)
        t = self.rng.choice(pool, size=m + len(avoid), replace=False)
        return t[~np.isin(t, avoid)][:m]


def _build():
    b = _B()
    rng = b.rng
    free = np.setdiff1d(np.arange(64, BASE_HI), RESERVED)
    b.edges(rng.choice(free, size=BIG_DEG, replace=False), 0)
    for h in range(1, N_HUB + 1):
        b.edges(rng.choice(free, size=HUB_DEG, replace=False), h)
    m = 3 * (BASE_HI - 64)
    b.edges(rng.choice(free, size=m), rng.choice(free, size=m))
    hot = iter(range(TARGET_LO + 7, TARGET_LO + 6000, 13))
    half = []                                                            # rows whose node weight is set to 0.5
    SPARSE, LOW16, LOW32 = (TARGET_LO, BASE_HI), (64, 16_000), (64, 5_990)
    for d in (1, 2, 255, 256, 257):
        b.within(*SPARSE).gadget(f"rows{d}", [8] * d, hot=[next(hot)])
    b.within(*SPARSE).gadget("sk", [30] * 100, hot=[next(hot)])
    # 16-bit direct: a survivor (1001) and a known edge every row reaches too (1000) share a table word
    b.within(*LOW16).gadget("d16", [40] * 200, hot=[1001, 1000], tie_v=[1000])
    half += list(b.within(*LOW32).gadget("d32", [20] * 256, hot=[2001])["rows"])
    g = b.within(*LOW16).gadget("mix", [30] * 150, hot=[3001])
    for w in g["rows"]:
        b.edges(b.within(*SPARSE).targets(10), w)
    b.within(64, 12_000).gadget("fat", [140] * 256)                    # 35 840 paths in one direct piece: more than 8192 units
    b.within(*LOW32).gadget("low32", [6] * 40, hot=[LOW32_V - 1], v=LOW32_V)      # (a span both kinds reach: 32-bit sums, small ones)
    for r in range(4):
        # (nine ids apart: no span column is another's last field)
        b.within(*LOW32).gadget(f"span16_{r}", [6] * 40, hot=[SPAN16_V + 9 * r - 1], v=SPAN16_V + 9 * r)
        half += list(b.within(*LOW32).gadget(f"span32_{r}", [6] * 256, hot=[SPAN32_V + 9 * r - 1], v=SPAN32_V + 9 * r)["rows"])
    for i in range(8):
        b.within(*SPARSE).gadget(f"seg{i}", [1 + (j + i) % 9 for j in range(27)], hot=[next(hot)])
    h = next(hot)
    b.within(*SPARSE).gadget("head_last", [1], hot=[h], hubs=2)
    b.edges([h, h], [1, 2])
    b.gadget("head_heavy", [6] * 3, hubs=7, hot=[next(hot)])
    b.gadget("two_hot", [10] * 30, hot=[next(hot), next(hot)])
    b.gadget("dead", [400])
    for i in range(12):
        b.gadget(f"plain{i}", [5 + i] * 20, hot=[next(hot)])
    import scipy.sparse as ssp
    r, c = np.concatenate(b.rows), np.concatenate(b.cols)
    keep = r != c
    r, c = r[keep], c[keep]
    A = ssp.coo_matrix((np.ones(2 * len(r), np.float32), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(N, N)).tocsr()
    A.data[:] = 1.0
    A.sort_indices()
    w = np.minimum(1.0 / np.log(np.maximum(np.diff(A.indptr), 2)), 0.5).astype(np.float32)
    w[np.asarray(half, np.int64)] = 0.5
    return A, b.gadgets, w


@pytest.fixture(scope="module")
def world(eps, dev):
    from eps_amd import scan
    A, gadgets, wt = _build()
    g = eps.CSRGraph.from_scipy(A, device=dev, keep_values=False)
    w = torch.from_numpy(wt).to(dev)
    saved = {k: getattr(scan, k) for k in SWITCHES}
    scan.SMALL_SET, scan.HEAD_MIN_PATHS, scan.SKETCH_MIN_PATHS, scan.SKETCH_SET = 0, 0, 0.0, 0
    scan.LIGHT_COLUMNS = scan.LEAN_COLUMNS = True
    try:
        gs, perm = scan.scan_graph(g)
        assert perm is None and gs is g
        K = 30                                                       # (a bar above all but the hot candidates: a row node's column reports few ids)
        scan.scan_topk(g, w, K)                                      # (a graph's first scan has no pack: no zones)
        st = {}
        rows = scan.scan_topk(g, w, K, stats=st)
        screen = scan.screen_weights(g, gs, perm, w)
        yield dict(A=A, gadgets=gadgets, g=g, w=w, wt=wt, screen=screen, K=K, st=st, rows=rows, cache={}, keep=[])
    finally:
        for k, v in saved.items():
            setattr(scan, k, v)


@pytest.fixture()
def switches(monkeypatch):
    from eps_amd import scan
    for k, v in (("SMALL_SET", 0), ("HEAD_MIN_PATHS", 0), ("SKETCH_MIN_PATHS", 0.0), ("SKETCH_SET", 0)):
        monkeypatch.setattr(scan, k, v)
    return monkeypatch


def _tables(world, bar):
    from eps_amd import scan
    g, screen = world["g"], world["screen"]
    units = int(bar * 2.0 ** screen.shift)
    assert units < 1 << 24
    return scan.head_tables(g, screen, scan.head_budget(units), wide=True), units


def _launch(world, ht, cols, units, lean, light, monkeypatch):
    """(keys ascending, sums as bits, status word, n_candidates, the split) of the refined list of one main launch."""
    from eps_amd import scan
    g, screen = world["g"], world["screen"]
    monkeypatch.setattr(scan, "LEAN_COLUMNS", lean)
    monkeypatch.setattr(scan, "LIGHT_COLUMNS", light)
    bar = torch.tensor([float(np.float32(units) * np.float32(2.0 ** -screen.shift))], dtype=torch.float32, device=g.device)
    cap = scan._capacity(1 << 20, scan._PIECE_SLACK)
    split = scan.light_split(g, screen, ht, cols, True)
    world["keep"] += [cols, split.columns]       # (column records are cached by the list's address: no list of this module is freed)
    res = scan._launch(g, None, cols, bar, cap, both=True, screen=screen, heads=ht, walked_capacity=2 * cap, sketch=True)
    assert res.zoned == (split.lean_from < cols.numel())
    slots = res.counts()[0]
    assert slots <= res.capacity and int(res.walked_slots) <= 2 * cap
    k, v = res.valid(slots)
    o = torch.argsort(k)
    k, v = k[o], v[o].view(torch.int32)
    assert torch.unique(k).numel() == k.numel(), "a candidate was reported twice"
    return k.cpu().numpy(), v.cpu().numpy(), int(res.status), res.counts()[1], split


def _both(world, ht, cols, units, monkeypatch):
    """The launch with all zones, with the lean zone alone and without zones; -> (all zones, lean alone), each equal to the last."""
    off = _launch(world, ht, cols, units, False, False, monkeypatch)
    assert off[4].lean_from == off[4].light_from == cols.numel()
    out = []
    for light in (True, False):
        on = _launch(world, ht, cols, units, True, light, monkeypatch)
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and on[2:4] == off[2:4], \
            (light, on[2:4], off[2:4], len(on[0]), len(off[0]))
        out.append(on)
    return out


def _zone(split, which):
    a, b = {"general": (0, split.lean_from), "lean": (split.lean_from, split.light_from), "light": (split.light_from, split.columns.numel())}[which]
    return set(split.columns[a:b].tolist())


def _cols(world, names):
    return [world["gadgets"][n]["v"] for n in names]


def _pairs_of(keys, v):
    return sorted(int(k & 0xFFFFFFFF) for k in keys if int(k >> 32) == v)


def _records(ht, v):
    pptr = ht.plan[0].cpu().numpy().view(np.uint32).astype(np.int64)
    rec = ht.plan[1].cpu().numpy().view(np.uint32).astype(np.int64)
    return rec[pptr[v]:pptr[v + 1]]


@pytest.fixture(scope="module")
def whole(world):
    """The whole live list at a bar of 2.5, all three ways (computed once, shared)."""
    from eps_amd import scan
    mp = pytest.MonkeyPatch()
    try:
        for k, v in (("SMALL_SET", 0), ("HEAD_MIN_PATHS", 0), ("SKETCH_MIN_PATHS", 0.0), ("SKETCH_SET", 0)):
            mp.setattr(scan, k, v)
        ht, units = _tables(world, 2.5)
        live = scan.live_columns(world["g"], world["screen"], ht, 0, 1)
        both, lean_only = _both(world, ht, live, units, mp)
        return dict(ht=ht, units=units, live=live, both=both, lean_only=lean_only)
    finally:
        mp.undo()


def test_the_lean_body_holds_the_runtimes_four_workgroups_per_cu(eps, dev):
    assert eps.ops._lib.load().eps_scan_lean_blocks_per_cu() == 4


def test_zones_and_piece_kinds_of_the_gadgets(world, whole, switches):
    """1, 2 rows: light (lean without a light zone; at a bar of their own -- under the list's they are dead); 255, 256 rows lean; 257
    rows and the piece of more than 8192 units general.  The plan gives the gadgets the piece kinds they were built for, and every
    launch equals the launch without zones (the fixture)."""
    gd, ht = world["gadgets"], whole["ht"]
    keys, vals, st, ncand, split = whole["both"]
    lean, light, general = _zone(split, "lean"), _zone(split, "light"), _zone(split, "general")
    assert st == 16 and 0 < split.lean_from < split.light_from < split.columns.numel()
    v_of = lambda n: gd[n]["v"]                                           # noqa: E731
    assert light and {v_of("rows255"), v_of("rows256")} <= lean and {v_of("rows257"), v_of("fat")} <= general
    assert light <= _zone(whole["lean_only"][4], "lean") and not _zone(whole["lean_only"][4], "light")
    small = torch.tensor(_cols(world, ["rows1", "rows2"]), dtype=torch.int32, device=world["g"].device)
    ht_small, units_small = _tables(world, 0.25)
    both, lean_only = _both(world, ht_small, small, units_small, switches)
    assert _zone(both[4], "light") == set(small.tolist()) == _zone(lean_only[4], "lean") and both[2] == 16
    for n in ("rows1", "rows2"):
        assert gd[n]["hot"][0] in _pairs_of(lean_only[0], v_of(n)), n
    kinds = lambda n: [int(x) for x in _records(ht, v_of(n))[:, 0] >> 30]      # noqa: E731
    assert kinds("sk") == [1] and set(kinds("d16")) == {3} and kinds("d32") == [2] == kinds("low32"), (kinds("sk"), kinds("d16"), kinds("d32"))
    assert kinds("mix")[0] in (2, 3) and kinds("mix")[-1] == 1 and len(kinds("mix")) >= 2, kinds("mix")
    assert set(kinds("fat")) == {3} and (_records(ht, v_of("fat"))[0, 0] & 0x3FFFFFFF) > 4 * 8192
    for n in ("sk", "d16", "d32", "mix", "rows255", "rows256"):
        assert v_of(n) in lean, n
    for n in ("sk", "d16", "d32", "mix", "rows255", "rows256", "rows257"):
        assert gd[n]["hot"][0] in _pairs_of(keys, v_of(n)), n
    # the flagged known edge next to the survivor in one 16-bit pair: 1001 is reported, 1000 (tied to v) is not
    assert 1000 not in _pairs_of(keys, v_of("d16")) and 1001 in _pairs_of(keys, v_of("d16"))


def test_direct_spans_through_every_residue_with_the_survivor_in_the_last_field(world, whole):
    """Columns inside the base whose one direct piece is [0, v): spans v = 9000 + 9 r (16-bit fields: the low and the high half of
    the last word) and 7000 + 9 r (32-bit), r = 0 .. 3 -- every residue mod 4 --, the survivor v - 1 in the last field."""
    gd, ht = world["gadgets"], whole["ht"]
    keys, split = whole["both"][0], whole["both"][4]
    for name, kind, v0 in (("span16", 3, SPAN16_V), ("span32", 2, SPAN32_V)):
        for r in range(4):
            v = gd[f"{name}_{r}"]["v"]
            rec = _records(ht, v)
            assert v == v0 + 9 * r and v % 4 == (v0 + r) % 4 and len(rec) == 1 and rec[0, 0] >> 30 == kind and rec[0, 3] == 0, (name, r, rec)
            assert v in _zone(split, "lean") and v - 1 in _pairs_of(keys, v), (name, r)


def test_segments_of_one_to_nine_entries_at_every_start_residue(world, whole):
    gd, g = world["gadgets"], world["g"]
    rp = g.rowptr.cpu().numpy()
    seen = set()
    for i in range(8):
        for w, m in zip(gd[f"seg{i}"]["rows"], gd[f"seg{i}"]["lens"]):
            assert rp[w + 1] - rp[w] == m + 1
            seen.add((m, int(rp[w]) & 3))
    assert seen == {(m, r) for m in range(1, 10) for r in range(4)}
    keys, split = whole["lean_only"][0], whole["lean_only"][4]
    for i in range(8):
        v = gd[f"seg{i}"]["v"]
        assert v in _zone(split, "lean") and gd[f"seg{i}"]["hot"][0] in _pairs_of(keys, v)


def test_heads_a_dead_column_in_a_ticket_and_the_bar_on_a_reported_sum(world, switches):
    gd, g, screen = world["gadgets"], world["g"], world["screen"]
    ht, units = _tables(world, 0.8)
    hd = ht.heads.cpu().numpy().view(np.uint32)
    v = gd["head_last"]["v"]
    assert hd[v, 0] == 2 and hd[gd["rows2"]["v"], 0] == 0 and hd[gd["dead"]["v"], 0] == 0
    ssum = screen.ssum.cpu().numpy().view(np.uint32)
    assert ssum[gd["dead"]["v"]] < units <= ssum[v]
    # nine small columns behind a general one: with the lean zone alone they are its last ticket's eight and one more
    names = ["plain0", "plain1", "head_last", "dead", "rows1", "rows2", "plain2", "plain3", "two_hot"]
    cols = torch.tensor(_cols(world, ["rows257"] + names), dtype=torch.int32, device=g.device)
    both, lean_only = _both(world, ht, cols, units, switches)
    assert _zone(lean_only[4], "lean") == set(_cols(world, names)) and lean_only[4].lean_from == 1 and lean_only[2] == 16
    assert not _pairs_of(lean_only[0], gd["dead"]["v"]) and _pairs_of(lean_only[0], v) == gd["head_last"]["hot"]
    # the bar on a reported sum stays, one unit above goes (a sketch column without a head, then a 32-bit direct one)
    ht, units = _tables(world, 2.5)
    in_units = lambda x: [int(round(float(f) * 2.0 ** screen.shift)) for f in np.asarray(x, np.int32).view(np.float32)]      # noqa: E731
    for name in ("two_hot", "low32"):
        v2 = gd[name]["v"]
        cols = torch.tensor(_cols(world, ["rows257", name, "plain4"]), dtype=torch.int32, device=g.device)
        keys, vals = _both(world, ht, cols, units, switches)[1][:2]
        est = min(in_units(vals[(keys >> 32) == v2]))
        assert hd[v2, 0] == 0 and units < est < (1 << 24) - 1
        for at, stays in ((est, True), (est + 1, False)):
            k2, x2, _, _, split = _both(world, ht, cols, at, switches)[1]
            assert v2 in _zone(split, "lean") and (est in in_units(x2[(k2 >> 32) == v2])) == stays, (name, at, est)
    # a head as heavy as the bar: the table of the higher bar under a lower one -- status bit 2, the column left out
    v7 = gd["head_heavy"]["v"]
    hy = int(ht.heads.cpu().numpy().view(np.uint32)[v7, 1])
    assert ht.heads.cpu().numpy().view(np.uint32)[v7, 0] == 7 and 0 < hy
    cols = torch.tensor(_cols(world, ["rows257", "head_heavy", "plain5"]), dtype=torch.int32, device=g.device)
    keys, _, st, _, split = _both(world, ht, cols, hy, switches)[1]
    assert v7 in _zone(split, "lean") and st & 4 and not _pairs_of(keys, v7)


@pytest.mark.parametrize("n_lean", [0, 1, 7, 8, 9])
def test_lean_zones_of_a_few_columns(world, switches, n_lean):
    gd, g = world["gadgets"], world["g"]
    ht, units = _tables(world, 2.5)
    names = [f"plain{i}" for i in range(n_lean)]
    cols = torch.tensor(_cols(world, ["rows257", "fat"] + names), dtype=torch.int32, device=g.device)
    keys, _, st, _, split = _both(world, ht, cols, units, switches)[1]
    assert (split.lean_from, split.light_from) == (2, 2 + n_lean) and _zone(split, "lean") == set(_cols(world, names))
    for n in ["rows257"] + names:
        assert gd[n]["hot"][0] in _pairs_of(keys, gd[n]["v"]), n


def _screen_by_hand(world, ht, cols, units, lean_from, plan=None):
    """ops.scan_screen over ``cols`` with columns[lean_from:] as the lean zone -> the status word."""
    from eps_amd import ops, scan
    g, screen = world["g"], world["screen"]
    plan = ht.plan if plan is None else plan
    bounds, cuts = scan.screen_tables(g)
    bar = torch.tensor([float(np.float32(units) * np.float32(2.0 ** -screen.shift))], dtype=torch.float32, device=g.device)
    walked = ops.Survivors(1 << 20, bar, g.device, prefill=False)
    status = torch.zeros(1, dtype=torch.int32, device=g.device)
    world["keep"] += [cols, plan]
    colrec = scan.column_records(g, screen, cols, plan, ht.heads, world["cache"], ("by hand", len(world["keep"])))
    ops.scan_screen(g.rowptr, g.col, scan.reverse_positions(g), screen.fx32, cuts, bounds, g.n_rows, cols, screen.shift, walked, status,
                    scan.screen_variant(g) | ops.SCAN_SKETCH | ops.SCAN_WIDE, None, None, ht.wpaths, screen.ssum, screen.smax, plan,
                    ht.heads, lean_from, screen.rowrec, colrec, scan.column_pack(g, screen, ht), None, lean_from, cols.numel() - lean_from)
    return int(status)


def test_the_lean_body_refuses_what_the_split_rules_out(world, switches):
    """A 257-row column, a two-word hash record (the kind bits of a packed record cleared in a copy of the plan) and a piece of more than
    8192 units in a lean zone made by hand: the backstop bit; the same zone without them: clean."""
    g = world["g"]
    ht, units = _tables(world, 2.5)
    ok = _cols(world, ["d16", "sk"])
    cols = lambda names: torch.tensor(_cols(world, ["rows257"]) + ok + _cols(world, names), dtype=torch.int32, device=g.device)      # noqa: E731
    assert _screen_by_hand(world, ht, cols([]), units, 1) & ~16 == 0
    assert _screen_by_hand(world, ht, cols(["rows257"]), units, 1) & 2
    assert _screen_by_hand(world, ht, cols(["fat"]), units, 1) & 2
    pptr = ht.plan[0].cpu().numpy().view(np.uint32).astype(np.int64)
    recs = ht.plan[1].clone()
    at = int(pptr[world["gadgets"]["sk"]["v"]])
    assert (int(recs[at, 0]) & 0xFFFFFFFF) >> 30 == 1
    recs[at, 0] = int(recs[at, 0]) & 0x3FFFFFFF
    assert _screen_by_hand(world, ht, cols([]), units, 1, plan=(ht.plan[0], recs)) & 2


def test_scan_topk_is_the_host_truth_and_a_wrong_split_falls_back(world, switches):
    """scan_topk with the zones against SciPy; then with a row bound of 1000 on the host, which sends the 257-row column to the lean
    body, and with a unit bound of 2^20, which sends the piece of more than 8192 units there: the backstop bit, the call repeats
    without zones, and the rows are still the truth.  (A two-word hash record in a lean zone needs a doctored plan: the direct
    launch above.)"""
    from eps_amd import scan
    g, w, K = world["g"], world["w"], world["K"]
    above, top = _host_rows(world["A"], world["wt"], K)
    assert world["st"]["heads"] and world["st"]["sketch"] and not world["st"]["zones_off"], world["st"]
    zoned = [s for ht in world["screen"].heads.values() for s in ht.light.values() if s.lean_from < s.light_from]
    assert zoned, "the second scan had no lean zone"
    switches.setattr(scan, "LIGHT_COLUMNS", True)
    switches.setattr(scan, "LEAN_COLUMNS", True)
    for rows_max, units_max in ((256, 8192), (1000, 8192), (256, 1 << 20)):
        switches.setattr(scan, "LEAN_ROWS", rows_max)
        switches.setattr(scan, "LEAN_UNITS", units_max)
        st = {}
        pairs, scores = world["rows"] if (rows_max, units_max) == (256, 8192) else scan.scan_topk(g, w, K, stats=st)
        if (rows_max, units_max) != (256, 8192):
            assert st["zones_off"], st
        p, s = pairs.cpu().numpy(), scores.cpu().numpy()
        assert np.array_equal(np.sort(s)[::-1], top)
        assert set(zip(p[0][s > top[-1]].tolist(), p[1][s > top[-1]].tolist())) == above


@pytest.fixture(scope="module")
def rmat(eps, dev):
    from eps_amd import synth
    return synth.rmat_graph(15, 14, 7, device=dev)


@pytest.mark.parametrize("kind", ["aa", "ra", "cn"])
def test_scan_topk_on_an_rmat_graph_with_and_without_zones(eps, rmat, kind, monkeypatch):
    """Hubs-first labels, K in {1, 5000, 200 001}: rows, scores and stats with the zones equal those without.  Common neighbours
    (Screen.exact) run without sketch pieces, hence without zones: asserted.  (Whether an AA or RA launch has zones depends on the
    screen's fixed point -- a slot of a sketch piece must not wrap --; on this graph it has none, so these two cases hold the host
    path with the switches on to the one with them off.)"""
    from eps_amd import ops, scan
    from eps_amd.heuristics import node_weight_table
    g = rmat
    w = (torch.ones(g.n_rows, dtype=torch.float32, device=g.device) if kind == "cn"
         else node_weight_table(g, {"aa": ops.W_AA, "ra": ops.W_RA}[kind]))
    for k, v in (("SMALL_SET", 0), ("RELABEL_MIN_NODES", 0), ("HEAD_MIN_PATHS", 0), ("SKETCH_MIN_PATHS", 0.0)):
        monkeypatch.setattr(scan, k, v)
    for K in (1, 5000, 200_001):
        got = {}
        for on in (False, True, True):                                   # (the second scan of a graph builds the pack)
            monkeypatch.setattr(scan, "LIGHT_COLUMNS", on)
            monkeypatch.setattr(scan, "LEAN_COLUMNS", on)
            st = {}
            p, s = scan.scan_topk(g, w, K, relabel=True, stats=st)
            got[on] = (p, s, {k: st[k] for k in ("survivors", "rescored", "touched", "candidates", "launches", "zones_off")})
        assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1]) and got[True][2] == got[False][2], \
            (K, got[True][2], got[False][2])
    if kind == "cn":
        gs, perm = scan.scan_graph(g)
        screen = scan.screen_weights(g, gs, perm, w)
        assert screen.exact and not [s for ht in screen.heads.values() for s in ht.light.values() if s.lean_from < s.columns.numel()]


# ---- a lean column of more than nine pieces: an id space of 2^20 ids, whose 32 windows are wider than any direct piece ------------
WIDE_N, WIDE_BASE_HI, WIDE_V, WIDE_ROW0, WIDE_HOT = 1 << 20, 900_000, 1_000_000, 950_000, 200_003


def _build_wide():
    """Node 0 tied to 2400 nodes (the row sum that brings the fixed point down to where sketch pieces are allowed), a uniform sparse
    base on ids 64 .. 900 000, and ONE column: v = 1 000 000 with 256 rows of its own (ids from 950 000), each tied to 250 ids of the
    base's lowest 300 000 and to the hot id.  64 256 half paths -- within what the 256-thread geometry takes without re-walking -- over
    a dozen windows of ~25 000 ids: ~5400 in each (over 450 000 ids they were ~4050, and two windows shared a record: nine records), so no two windows fit one packed record."""
    import scipy.sparse as ssp
    rng = np.random.default_rng(23)
    free = np.setdiff1d(np.arange(64, WIDE_BASE_HI), [WIDE_HOT])
    r = [rng.choice(free, size=2400, replace=False), rng.choice(free, size=200_000), ]
    c = [np.zeros(2400, np.int64), rng.choice(free, size=200_000)]
    rows = np.arange(WIDE_ROW0, WIDE_ROW0 + 256)
    low = free[free < 300_000]
    for w in rows:
        t = np.concatenate([[WIDE_HOT], rng.choice(low, size=250, replace=False)])
        r.append(t)
        c.append(np.full(t.shape, w, np.int64))
    r.append(rows)
    c.append(np.full(rows.shape, WIDE_V, np.int64))
    r, c = np.concatenate(r), np.concatenate(c)
    keep = r != c
    r, c = r[keep], c[keep]
    A = ssp.coo_matrix((np.ones(2 * len(r), np.float32), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(WIDE_N, WIDE_N)).tocsr()
    A.data[:] = 1.0
    A.sort_indices()
    return A, np.minimum(1.0 / np.log(np.maximum(np.diff(A.indptr), 2)), 0.5).astype(np.float32)


@pytest.fixture(scope="module")
def wide(eps, dev):
    from eps_amd import scan
    A, wt = _build_wide()
    g = eps.CSRGraph.from_scipy(A, device=dev, keep_values=False)
    w = torch.from_numpy(wt).to(dev)
    saved = {k: getattr(scan, k) for k in SWITCHES + ("RELABEL_MIN_NODES",)}
    scan.SMALL_SET, scan.HEAD_MIN_PATHS, scan.SKETCH_MIN_PATHS, scan.SKETCH_SET, scan.RELABEL_MIN_NODES = 0, 0, 0.0, 0, 1 << 30
    scan.LIGHT_COLUMNS = scan.LEAN_COLUMNS = True
    try:
        gs, perm = scan.scan_graph(g)
        assert perm is None and gs is g and scan.screen_variant(g) == 2
        for _ in range(2):                                           # (the second scan of a graph builds the pack)
            scan.scan_topk(g, w, 30)
        yield dict(g=g, w=w, screen=scan.screen_weights(g, gs, perm, w), cache={}, keep=[])
    finally:
        for k, v in saved.items():
            setattr(scan, k, v)


def test_a_lean_column_of_more_than_nine_pieces(wide, switches):
    """Ten or more plan records, all packed, in a column of 256 rows: lean by the split, its cuts from the pack up to piece 8 and from
    the row records after it; with the zones on and off the launch reports the same list, the hot candidate in it."""
    from eps_amd import scan
    switches.setattr(scan, "RELABEL_MIN_NODES", 1 << 30)
    g = wide["g"]
    ht, units = _tables(wide, 2.5)
    rec = _records(ht, WIDE_V)
    assert len(rec) >= 10 and set((rec[:, 0] >> 30).tolist()) == {1}, (len(rec), (rec[:, 0] >> 30).tolist())
    assert ((rec[:, 0] & 0x3FFFFFFF) + 3 * 256 <= 4 * 8192).all() and int(g.rowptr[WIDE_V + 1] - g.rowptr[WIDE_V]) == 256
    cols = torch.tensor([WIDE_ROW0, WIDE_V], dtype=torch.int32, device=g.device)      # (a row node's column has 251 rows and few paths)
    both, lean_only = _both(wide, ht, cols, units, switches)
    assert WIDE_V in _zone(both[4], "lean") and WIDE_V in _zone(lean_only[4], "lean") and both[2] == 16
    assert WIDE_HOT in _pairs_of(both[0], WIDE_V)


def test_scan_topk_on_a_larger_rmat_graph_with_a_lean_zone(eps, dev, monkeypatch):
    """rmat_graph(17, 10, 3), Adamic-Adar, hubs-first labels: at its fixed point (2^-18) launches under a bar are sketch launches, so the
    zones are real -- a lean zone is asserted (2218 of 3214 live columns at K = 2000) -- and rows, scores and stats with the zones equal those without."""
    from eps_amd import ops, scan, synth
    from eps_amd.heuristics import node_weight_table
    g = synth.rmat_graph(17, 10, 3, dev)
    w = node_weight_table(g, ops.W_AA)
    for k, v in (("SMALL_SET", 0), ("RELABEL_MIN_NODES", 0), ("HEAD_MIN_PATHS", 0), ("SKETCH_MIN_PATHS", 0.0)):
        monkeypatch.setattr(scan, k, v)
    for K in (2000, 150_000):
        got = {}
        for on in (False, True, True):
            monkeypatch.setattr(scan, "LIGHT_COLUMNS", on)
            monkeypatch.setattr(scan, "LEAN_COLUMNS", on)
            st = {}
            p, s = scan.scan_topk(g, w, K, relabel=True, stats=st)
            got[on] = (p, s, {k: st[k] for k in ("survivors", "rescored", "touched", "candidates", "launches", "zones_off")})
        assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1]) and got[True][2] == got[False][2], \
            (K, got[True][2], got[False][2])
    gs, perm = scan.scan_graph(g)
    screen = scan.screen_weights(g, gs, perm, w)
    zoned = [s for ht in screen.heads.values() for s in ht.light.values() if s.lean_from < s.light_from]
    assert zoned, (screen.shift, [(s.lean_from, s.light_from, s.columns.numel()) for ht in screen.heads.values() for s in ht.light.values()])
