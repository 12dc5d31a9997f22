"""The lean kernel of the main launch's LIGHT columns (csrc/scan_light.hip; eps_amd.scan.light_split) on a hand-made graph.

The graph (65 536 ids, scanned as labelled): one node tied to 2400 base nodes (its row sum is what brings the screening fixed point
down to where sketch pieces are allowed: 2048 of the heaviest weight), 32 hub ids tied to 300 base nodes each, a sparse random base
on ids 64 .. 50 000, and the node weights min(1 / ln(degree), 0.5) -- Adamic-Adar's, capped so that the heaviest weight is small next
to that row sum -- and GADGETS at the top of the id space -- a column v (ids from 60 000) whose rows are nodes of its own (ids from 50 000), each tied to
a chosen number of targets in the base's upper half (ids 20 000 .. 50 000: farther apart than a direct piece is wide, so the
column's walk is ONE packed piece, which a sketch launch runs as a sketch piece).  A gadget's paths are the sum of its rows'
targets, its known edges its rows: paths + known edges, rows, segment lengths and the hot candidates are all set by hand.

Every case compares (a) the refined survivor list of scan._launch with LIGHT_COLUMNS on against the same launch with it off -- keys
and sums equal as sorted lists -- after asserting from the cached split that the columns meant to be light ARE light (otherwise the
new kernel did not run), and the module's last test (b) scan_topk's rows against a truth worked out on the host with SciPy: the
exact 2^-40 fixed-point sums over the common neighbours of every two-hop non-edge, the K largest.

One case of the issue cannot exist for a WALKED row: "a row whose cut comes before its revpos".  A light column is ONE piece.  The
planner emits no piece of zero paths, so that piece may end at a window boundary below v -- but only when the windows between that
boundary and v hold no entry of any walked row (the plan counts the walked rows' paths); a walked row's cut (its entries below the
boundary) then equals its revpos (its entries below v), and otherwise the piece ends at or above v and the cut is the larger.  Only
a row of the skipped head, which the kernel does not read the segment of, can have cut < revpos.  The test asserts cut >= revpos
on the pack lines of every walked row (row index >= the head's rows) of every light column, and that rows whose revpos ends the
segment strictly before the cut occur (the lower of two columns over the same rows: all of its rows)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1 << 16
N_HUB, HUB_DEG = 32, 300          # hub ids 1 .. 32
BIG_DEG = 2400                      # id 0
BASE_HI = 50_000
TARGET_LO = 20_000
ROW0, COL0 = 50_000, 60_000


class _Builder:
    def __init__(self):
        self.rng = np.random.default_rng(17)
        self.rows, self.cols = [], []
        self.next_row, self.next_col = ROW0, COL0
        self.gadgets = {}

    def edges(self, r, c):
        self.rows.append(np.asarray(r, np.int64).reshape(-1))
        self.cols.append(np.broadcast_to(np.asarray(c, np.int64), np.asarray(r).reshape(-1).shape).copy())

    def targets(self, m, avoid=()):
        t = self.rng.choice(np.arange(TARGET_LO, BASE_HI), size=m + len(avoid), replace=False)
        return t[~np.isin(t, avoid)][:m]

    def gadget(self, name, lens, hot=(), hubs=0, tie_v=(), v=None, rows=None):
        """Column ``v`` with one row of its own per entry of ``lens`` (row i: lens[i] targets, the ``hot`` ids among them), ``hubs``
        hub rows in front, and the ids ``tie_v`` tied to v directly (known edges that are also reached through the rows if hot)."""
        if v is None:
            v = self.next_col
            self.next_col += 1
        if rows is None:
            rows = np.arange(self.next_row, self.next_row + len(lens))
            self.next_row += len(lens)
            for w, m in zip(rows, lens):
                t = np.concatenate([np.asarray(hot, np.int64), self.targets(m - len(hot), hot)]) if m >= len(hot) else self.targets(m)
                self.edges(t, w)
        self.edges(rows, v)
        if hubs:
            self.edges(np.arange(1, hubs + 1), v)
        if len(tie_v):
            self.edges(np.asarray(tie_v), v)
        self.gadgets[name] = dict(v=int(v), rows=np.asarray(rows), lens=list(lens), hot=list(hot), hubs=hubs)
        return self.gadgets[name]


def _even(total, d):
    return [total // d + (1 if i < total % d else 0) for i in range(d)]


def _build():
    b = _Builder()
    rng = b.rng
    b.edges(rng.choice(np.arange(64, BASE_HI), size=BIG_DEG, replace=False), 0)
    for h in range(1, N_HUB + 1):
        b.edges(rng.choice(np.arange(64, BASE_HI), size=HUB_DEG, replace=False), h)
    m = 3 * (BASE_HI - 64)
    b.edges(rng.integers(64, BASE_HI, m), rng.integers(64, BASE_HI, m))
    hot = iter(range(TARGET_LO + 7, TARGET_LO + 4000, 13))                     # (hot candidates: ids nobody else picks twice by design)
    # rows: 1, 2, 63, 64 are light, 65 is not; each row 8 targets, one of them a candidate every row reaches
    for d in (1, 2, 63, 64, 65):
        b.gadget(f"rows{d}", [8] * d, hot=[next(hot)])
    # paths + known edges on both sides of the table-size edge (1024 / 1025) and the eligibility edge (2048 / 2049): through paths
    # (3 or 4 rows, each longer than a single-round column: as columns of their own they are no sketch pieces, which at scan_topk's
    # bar -- two paths of a base node's weight -- would report more ids than the dedupe set holds) and through known edges (64 rows)
    for pk in (1024, 1025, 2048, 2049):
        d = 3 if pk < 2048 else 4
        b.gadget(f"pk{pk}_paths", _even(pk - d, d), hot=[next(hot)])
        b.gadget(f"pk{pk}_edges", _even(pk - 64, 64), hot=[next(hot)])
    # row segments of 1 .. 9 entries (their starts in col[] run through the residues mod 4: asserted)
    for i in range(8):
        b.gadget(f"seg{i}", [1 + (j + i) % 9 for j in range(27)], hot=[next(hot)])
    # two columns over the SAME rows and the same hot id: for the lower one every row has an entry above it (revpos < cut)
    h = next(hot)
    a = b.gadget("share_a", [12] * 24, hot=[h])
    b.gadget("share_b", [12] * 24, hot=[h], rows=a["rows"])
    # heads: two hub rows in front of one row of the column's own (the head skips all rows but the last at a low bar); seven hub rows
    # (a head as heavy as a bar below the one its table was built for)
    h = next(hot)
    b.gadget("head_last", [1], hot=[h], hubs=2)
    b.edges([h, h], [1, 2])                                              # (its one candidate shares the skipped rows too: it clears the bar)
    b.gadget("head_heavy", [6] * 3, hubs=7, hot=[next(hot)])
    # a hot slot whose only id is a neighbour of v: u0 is tied to v and to every row
    u0 = next(hot)
    b.gadget("known_hot", [4] * 30, hot=[u0], tie_v=[u0])
    # two hot candidates in one column (a dedupe set of one slot fills up)
    b.gadget("two_hot", [10] * 30, hot=[next(hot), next(hot)])
    # a column whose rows weigh less than any bar used here (dead inside a ticket)
    b.gadget("dead", [400])
    # plain light columns for the ticket edges
    for i in range(12):
        b.gadget(f"plain{i}", [5 + i] * 20, hot=[next(hot)])
    import scipy.sparse as ssp
    r, c = np.concatenate(b.rows), np.concatenate(b.cols)
    keep = r != c
    r, c = r[keep], c[keep]
    A = ssp.coo_matrix((np.ones(2 * len(r), np.float32), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(N, N)).tocsr()
    A.data[:] = 1.0
    A.sort_indices()
    return A, b.gadgets


def _node_weights(A):
    return np.minimum(1.0 / np.log(np.maximum(np.diff(A.indptr), 2)), 0.5).astype(np.float32)


@pytest.fixture(scope="module")
def world(eps, dev):
    """The graph on the device, scanned TWICE by scan_topk under the patched switches (the second scan builds the pack), and what
    the first scan's split looked like."""
    from eps_amd import scan
    A, gadgets = _build()
    g = eps.CSRGraph.from_scipy(A, device=dev, keep_values=False)
    w = torch.from_numpy(_node_weights(A)).to(dev)
    saved = {k: getattr(scan, k) for k in ("SMALL_SET", "HEAD_MIN_PATHS", "SKETCH_MIN_PATHS", "LIGHT_COLUMNS", "SKETCH_SET")}
    scan.SMALL_SET, scan.HEAD_MIN_PATHS, scan.SKETCH_MIN_PATHS, scan.LIGHT_COLUMNS, scan.SKETCH_SET = 0, 0, 0.0, True, 0
    try:
        gs, perm = scan.scan_graph(g)
        assert perm is None and gs is g                              # (scanned as labelled: the ids above are the kernel's)
        K = 700                                                      # (a bar above two paths of the heaviest weight: few reports a column)
        st1 = {}
        rows1 = scan.scan_topk(g, w, K, stats=st1)
        screen = scan.screen_weights(g, gs, perm, w)
        first = [(s.light_from, s.columns.numel()) for ht in screen.heads.values() for s in ht.light.values()]
        no_pack = all(scan.column_pack(g, screen, ht) is None for ht in screen.heads.values())
        st2 = {}
        rows2 = scan.scan_topk(g, w, K, stats=st2)
        yield dict(A=A, gadgets=gadgets, g=g, w=w, screen=screen, K=K, st1=st1, st2=st2, rows1=rows1, rows2=rows2, first_splits=first, first_no_pack=no_pack)
    finally:
        for k, v in saved.items():
            setattr(scan, k, v)


@pytest.fixture()
def switches(monkeypatch):
    from eps_amd import scan
    monkeypatch.setattr(scan, "SMALL_SET", 0)
    monkeypatch.setattr(scan, "HEAD_MIN_PATHS", 0)
    monkeypatch.setattr(scan, "SKETCH_MIN_PATHS", 0.0)
    monkeypatch.setattr(scan, "SKETCH_SET", 0)
    return monkeypatch


def _tables(world, bar):
    """The head tables (plan for sketch launches) of a bar in score units, and the bar as the launch takes it."""
    from eps_amd import scan
    g, screen = world["g"], world["screen"]
    units = int(bar * 2.0 ** screen.shift)
    assert units < 1 << 24                                           # (a float32 bar sits exactly on a whole number of table units)
    ht = scan.head_tables(g, screen, scan.head_budget(units), wide=True)
    return ht, units


def _launch(world, ht, cols, units, on, monkeypatch):
    """(keys ascending, sums as bits, status word, the split) of the refined list of one main launch over ``cols`` at ``units``."""
    from eps_amd import scan
    g, screen = world["g"], world["screen"]
    monkeypatch.setattr(scan, "LIGHT_COLUMNS", on)
    bar = torch.tensor([float(np.float32(units) * np.float32(2.0 ** -screen.shift))], dtype=torch.float32, device=g.device)
    cap = scan._capacity(1 << 20, scan._PIECE_SLACK)
    split = scan.light_split(g, screen, ht, cols, True)
    res = scan._launch(g, None, cols, bar, cap, both=True, screen=screen, heads=ht, walked_capacity=2 * cap, sketch=True)
    slots = res.counts()[0]
    assert slots <= res.capacity and int(res.walked_slots) <= 2 * cap
    k, v = res.valid(slots)
    o = torch.argsort(k)
    k, v = k[o], v[o].view(torch.int32)
    assert torch.unique(k).numel() == k.numel(), "a candidate was reported twice"
    return k.cpu().numpy(), v.cpu().numpy(), int(res.status), split


def _both(world, ht, cols, units, monkeypatch):
    on = _launch(world, ht, cols, units, True, monkeypatch)
    off = _launch(world, ht, cols, units, False, monkeypatch)
    assert off[3].light_from == cols.numel()
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and on[2] == off[2], (on[2], off[2], len(on[0]), len(off[0]))
    return on


def _light_set(split):
    return set(split.columns[split.light_from:].tolist())


def _cols(world, names):
    return [world["gadgets"][n]["v"] for n in names]


def _pairs_of(keys, v):
    return sorted(int(k & 0xFFFFFFFF) for k in keys if int(k >> 32) == v)


def test_first_scan_has_no_light_zone_and_the_second_has(world):
    """A graph's first scan has no pack: the split is off and the call runs the piece kernel alone; the second scan splits."""
    from eps_amd import scan
    assert world["st1"]["heads"] and world["first_no_pack"] and world["first_splits"], world["st1"]
    assert all(lf == n for lf, n in world["first_splits"]), world["first_splits"]
    brief = lambda st: {k: (float(st[k]) if k == "bar" else st[k]) for k in ("bar", "launches", "sketch", "sketch_void", "head_budget")}
    assert world["st2"]["heads"] and world["st2"]["sketch"], (brief(world["st1"]), brief(world["st2"]))
    screen = world["screen"]
    later = [s for ht in screen.heads.values() for s in ht.light.values() if s.light_from < s.columns.numel()]
    assert later, "the second scan did not split its column list"
    assert torch.equal(world["rows1"][0], world["rows2"][0]) and torch.equal(world["rows1"][1], world["rows2"][1])


def test_rows_and_key_bounds_decide_lightness(world, switches):
    """1, 2, 63 and 64 rows are light, 65 is not; 1024 / 1025 and 2048 paths + known edges are light, 2049 is not -- reached through
    paths (three or four long rows) and through known edges (64 rows) -- and each launch equals the piece kernel's; so does the launch over
    the whole live list.  Every group runs at a bar under which its columns report fewer ids than the dedupe set holds: a table at
    load 1/2 puts several paths into most slots, so the bar of the three- and four-row columns lies just under their hot candidate's
    three or four paths, where one id in 14 resp. 150 collides its way up to it.  (The first group has no column for the piece kernel: that launch is skipped.)"""
    from eps_amd import scan
    g, screen, gd = world["g"], world["screen"], world["gadgets"]
    wt = _node_weights(world["A"]).astype(np.float64)
    groups = ((0.25, ["rows1", "rows2"]), (0.45, ["pk1024_paths", "pk1025_paths"]), (0.58, ["pk2048_paths", "pk2049_paths"]),
              (2.5, ["rows63", "rows64", "rows65"] + [f"pk{pk}_edges" for pk in (1024, 1025, 2048, 2049)]))
    for bar, names in groups:
        cols = torch.tensor(_cols(world, names), dtype=torch.int32, device=g.device)
        ht, units = _tables(world, bar)
        keys, vals, st, split = _both(world, ht, cols, units, switches)
        assert st == 16
        light = _light_set(split)
        pptr = ht.plan[0].cpu().numpy().view(np.uint32).astype(np.int64)
        rec = ht.plan[1].cpu().numpy().view(np.uint32).astype(np.int64)
        for n in names:
            v = gd[n]["v"]
            assert pptr[v + 1] - pptr[v] == 1 and rec[pptr[v], 0] >> 30 == 1, (n, "is not one packed piece")
            pk = (rec[pptr[v], 0] & 0x3FFFFFFF) + (rec[pptr[v], 2] >> 16) - (rec[pptr[v], 2] & 0xFFFF)
            if n.startswith("pk"):
                assert pk == int(n[2:6]), (n, pk)
            assert (v in light) == (n != "rows65" and not n.startswith("pk2049")), (n, pk, bar)
            # the candidate every row reaches is reported (once: _launch checks) where its sum of row weights clears the bar
            assert float(wt[gd[n]["rows"]].sum()) > 1.05 * bar or n == "rows65", (n, bar)
            if float(wt[gd[n]["rows"]].sum()) > 1.05 * bar:
                assert gd[n]["hot"][0] in _pairs_of(keys, v), (n, bar)
    live = scan.live_columns(g, screen, ht, 0, 1)
    keys, vals, st, split = _both(world, ht, live, units, switches)
    assert st == 16 and 0 < split.light_from < live.numel() and len(keys) > 100


def test_segments_revpos_and_shared_rows(world, switches):
    """Row segments of 1 .. 9 entries starting at every residue mod 4 of col[]; rows whose revpos ends the segment before the piece's
    cut (the lower of two columns over the same rows; the cut never comes first in a one-piece column: asserted); the two columns
    that share rows and a hot id each report it."""
    from eps_amd import scan
    g, screen, gd = world["g"], world["screen"], world["gadgets"]
    ht, units = _tables(world, 2.5)
    live = scan.live_columns(g, screen, ht, 0, 1)
    keys, vals, st, split = _both(world, ht, live, units, switches)
    light = _light_set(split)
    names = [f"seg{i}" for i in range(8)] + ["share_a", "share_b"]
    assert all(gd[n]["v"] in light for n in names)
    rp = g.rowptr.cpu().numpy()
    seen = set()
    for i in range(8):
        for w, m in zip(gd[f"seg{i}"]["rows"], gd[f"seg{i}"]["lens"]):
            assert rp[w + 1] - rp[w] == m + 1                        # (its targets, all below v, and v)
            seen.add((m, int(rp[w]) & 3))
    assert seen == {(m, r) for m in range(1, 10) for r in range(4)}, sorted({(m, r) for m in range(1, 10) for r in range(4)} - seen)
    pack = scan.column_pack(g, screen, ht).cpu().numpy().view(np.uint32).reshape(-1, 8)
    xv = ht.heads.cpu().numpy().view(np.uint32)[:, 0].astype(np.int64)
    for v in sorted(light):
        w3 = pack[rp[v] + xv[v]:rp[v + 1], 3]                        # (the walked rows: those past the skipped head)
        assert ((w3 >> 16) >= (w3 & 0xFFFF)).all(), "a walked row's cut ends below its revpos"
    a = gd["share_a"]["v"]
    w3 = pack[rp[a]:rp[a + 1], 3]
    assert ((w3 & 0xFFFF) < (w3 >> 16)).all()
    h = gd["share_a"]["hot"][0]
    assert h in _pairs_of(keys, a) and h in _pairs_of(keys, gd["share_b"]["v"])
    assert a in _pairs_of(keys, gd["share_b"]["v"])                  # (the lower column is itself a candidate of the upper one)
    for i in range(8):
        assert gd[f"seg{i}"]["hot"][0] in _pairs_of(keys, gd[f"seg{i}"]["v"])
    # the two columns side by side in the light zone, in the middle of one ticket: no id of one column's set or table reaches the other
    names = ["plain0", "plain1", "share_a", "share_b", "plain2"]
    cols = torch.tensor(_cols(world, ["rows65"] + names), dtype=torch.int32, device=g.device)
    keys, vals, st, split = _both(world, ht, cols, units, switches)
    assert split.light_from == 1 and st == 16
    assert split.columns.tolist()[3:5] == [a, gd["share_b"]["v"]]
    assert _pairs_of(keys, a) == [h] and _pairs_of(keys, gd["share_b"]["v"]) == sorted([h, a])


def test_heads_dead_columns_known_neighbours_and_the_bar_on_an_estimate(world, switches):
    from eps_amd import scan
    g, screen, gd = world["g"], world["screen"], world["gadgets"]
    # a head that skips all rows but the last, heads of no rows, a dead column inside a ticket
    ht, units = _tables(world, 0.8)
    hd = ht.heads.cpu().numpy().view(np.uint32)
    v = gd["head_last"]["v"]
    assert hd[v, 0] == 2 and hd[gd["rows2"]["v"], 0] == 0 and hd[gd["dead"]["v"], 0] == 0, hd[v]
    ssum = screen.ssum.cpu().numpy().view(np.uint32)
    assert ssum[gd["dead"]["v"]] < units <= ssum[gd["head_last"]["v"]]
    names = ["plain0", "plain1", "head_last", "dead", "rows1", "rows2", "known_hot", "plain2", "plain3", "two_hot"]
    cols = torch.tensor(_cols(world, ["rows65"] + names), dtype=torch.int32, device=g.device)
    keys, vals, st, split = _both(world, ht, cols, units, switches)
    assert split.light_from == 1 and _light_set(split) == set(_cols(world, names)) and st == 16
    assert not _pairs_of(keys, gd["dead"]["v"])
    assert _pairs_of(keys, v) == gd["head_last"]["hot"]              # (the one target of the one walked row; the skipped rows complete it)
    # a hot slot whose only id is a neighbour of v: nothing of the column is reported at a bar only that id reaches
    ht, units = _tables(world, 2.5)
    cols = torch.tensor(_cols(world, ["rows65", "known_hot", "two_hot", "plain4"]), dtype=torch.int32, device=g.device)
    keys, vals, st, split = _both(world, ht, cols, units, switches)
    assert split.light_from == 1 and st == 16
    assert not _pairs_of(keys, gd["known_hot"]["v"]) and _pairs_of(keys, gd["two_hot"]["v"]) == sorted(gd["two_hot"]["hot"])
    # a bar exactly on an estimate stays, one unit above goes: the estimate is the reported walked sum of a column without a head
    v2 = gd["two_hot"]["v"]
    # (a refined sum is float(units) x 2^-shift, exact below 2^24 units)
    in_units = lambda x: [int(round(float(f) * 2.0 ** screen.shift)) for f in np.asarray(x, np.int32).view(np.float32)]
    est = min(in_units(vals[(keys >> 32) == v2]))
    assert hd[v2, 0] == 0 and units < est < (1 << 24) - 1
    for at, stays in ((est, True), (est + 1, False)):
        k2, x2, st, split = _both(world, ht, cols, at, switches)
        assert split.light_from == 1 and (est in in_units(x2[(k2 >> 32) == v2])) == stays, (at, est)
    # a dedupe set of ONE slot (the launch word): the light column with two hot candidates fills it -- status bit 3 from the light
    # kernel itself (the column of the piece kernel in this list reports one id); which of the two ids got the slot is a race, so
    # the lists of a void launch are not compared
    switches.setattr(scan, "SKETCH_SET", 1)
    cols = torch.tensor(_cols(world, ["rows65", "two_hot"]), dtype=torch.int32, device=g.device)
    for on in (True, False):
        k1, x1, st, split = _launch(world, ht, cols, units, on, switches)
        assert st & 8 and st & ~(16 | 8) == 0, (on, st)
        assert (split.light_from == 1 and _light_set(split) == {v2}) if on else split.light_from == 2
        assert _pairs_of(k1, gd["rows65"]["v"]) == gd["rows65"]["hot"] and len(_pairs_of(k1, v2)) == 1
    switches.setattr(scan, "SKETCH_SET", 0)
    # a head as heavy as the bar: the table of the higher bar under a lower one -- status bit 2, the column left out
    v7 = gd["head_heavy"]["v"]
    hy = int(ht.heads.cpu().numpy().view(np.uint32)[v7, 1])
    assert ht.heads.cpu().numpy().view(np.uint32)[v7, 0] == 7 and 0 < hy
    cols = torch.tensor(_cols(world, ["rows65", "head_heavy", "plain5"]), dtype=torch.int32, device=g.device)
    keys, vals, st, split = _both(world, ht, cols, hy, switches)
    assert split.light_from == 1 and st & 4 and not _pairs_of(keys, v7)


@pytest.mark.parametrize("n_light", [0, 1, 7, 8, 9])
def test_ticket_edges(world, switches, n_light):
    """Light zones of 1, 7, 8 and 9 columns behind two columns of the piece kernel, and an empty one."""
    gd, g = world["gadgets"], world["g"]
    ht, units = _tables(world, 2.5)
    names = [f"plain{i}" for i in range(n_light)]
    cols = torch.tensor(_cols(world, ["rows65", "pk2049_edges"] + names), dtype=torch.int32, device=g.device)
    keys, vals, st, split = _both(world, ht, cols, units, switches)
    assert split.light_from == 2 and split.columns.numel() == 2 + n_light and _light_set(split) == set(_cols(world, names))
    for n in ["rows65", "pk2049_edges"] + names:
        assert gd[n]["hot"][0] in _pairs_of(keys, gd[n]["v"]), n


def _host_rows(A, w, k):
    """(directed pairs above the k-th score as a set, the k largest scores descending) of every two-hop non-edge: float32 of the exact
    sum of round(w 2^40) over the common neighbours, times 2^-40."""
    import scipy.sparse as ssp
    fixw = np.rint(w.astype(np.float64) * 2.0 ** 40).astype(np.int64)
    Ai = ssp.csr_matrix((np.ones(A.nnz, np.int64), A.indices, A.indptr), shape=A.shape)
    S = (Ai @ ssp.diags(fixw) @ Ai).tocoo()
    m = S.row != S.col
    r, c, s = S.row[m].astype(np.int64), S.col[m].astype(np.int64), S.data[m]
    n = A.shape[0]
    ekey = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * n + A.indices
    m = ~np.isin(r * n + c, ekey)
    r, c, s = r[m], c[m], s[m]
    score = (s.astype(np.float64) * 2.0 ** -40).astype(np.float32)
    top = np.sort(score)[::-1][:k]
    above = score > top[-1]
    return set(zip(r[above].tolist(), c[above].tolist())), top


def test_scan_topk_rows_are_the_host_truth_and_a_full_set_falls_back(world, switches):
    """scan_topk with the light zone against the host's rows; then with a dedupe set of ONE slot, which the column with two hot
    candidates fills: status bit 3, the call repeats without sketch pieces and the rows are still the truth."""
    from eps_amd import scan
    g, w, K = world["g"], world["w"], world["K"]
    above, top = _host_rows(world["A"], w.cpu().numpy(), K)
    switches.setattr(scan, "LIGHT_COLUMNS", True)
    for sketch_set in (0, 1):
        switches.setattr(scan, "SKETCH_SET", sketch_set)
        st = {}
        pairs, scores = world["rows2"] if sketch_set == 0 else scan.scan_topk(g, w, K, stats=st)
        if sketch_set:
            assert st["sketch_void"] >= 1, st
        p, s = pairs.cpu().numpy(), scores.cpu().numpy()
        assert np.array_equal(np.sort(s)[::-1], top)
        got = set(zip(p[0][s > top[-1]].tolist(), p[1][s > top[-1]].tolist()))
        assert got == above
    # (the hot candidates of the gadget columns are among the rows: the light zone's reports reached the selection)
    gd = world["gadgets"]["two_hot"]
    assert all((u, gd["v"]) in above for u in gd["hot"])
