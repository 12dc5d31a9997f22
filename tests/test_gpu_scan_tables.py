"""GPU parity of the one-pass scan's per-graph tables and plan records (csrc/scan_tables.hip; sp_plan_kernel and
eps_scan_plan_rewalk in csrc/scan_pieces.hip) with the integer definitions of include/eps_abi.h as tests/scan_table_truth.py
states them in numpy (tests/test_scan_tables_host.py holds those to brute force on the CPU, and pins the piece kinds the
graphs below are cut into).  Every comparison is exact integer equality, int32 / int16 bits read as unsigned.

Graphs (N / stored entries): rmat14_hubs_first 16384 / 329808, rmat15_hubs_last 32768 / 680348, rmat17_as_labelled
131072 / 999388 (generated on the CPU from eps_amd.synth and uploaded, so the host pin speaks about the same arrays), two stars
of 65535 leaves (cuts of 0xFFFF), and the degenerate ones: no edges, one node, one edge, 20 nodes (fewer than windows), rows of
exactly 63 / 64 / 65 / 129 entries (the lane stride of the wave-per-row kernels)."""
import numpy as np
import pytest
import torch

import scan_table_truth as T

pytestmark = pytest.mark.gpu

M = T.M
SMALL = ("star_hub_first", "star_hub_last", "no_edges", "one_node", "one_edge", "n20", "lane_rows")
ALL = T.PIN_GRAPHS + SMALL
_WORLD = {}


def _graph(name):
    if name in T.PIN_GRAPHS:
        from eps_amd import synth
        return T.pin_graph(synth, name)
    if name.startswith("star"):
        return T.star(65535, name == "star_hub_first")
    if name == "no_edges":
        return np.zeros(51, np.int64), np.zeros(0, np.int64)
    if name == "one_node":
        return np.zeros(2, np.int64), np.zeros(0, np.int64)
    if name == "one_edge":
        return T.csr_from_edges(2, [0], [1])
    if name == "n20":
        return T.small_random(20, 60, 5)
    return T.lane_stride_graph()


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint32).view(np.int32))).to(dev)


def _i16(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint16).view(np.int16))).to(dev)


def _u(t):
    return T.unsigned(t.cpu().numpy())


class World:
    """One graph: the truth's tables (``t``) and the same arrays on the device -- what a kernel under test is fed, so that each
    comparison holds ONE kernel to its definition."""

    def __init__(self, eps, dev, name):
        self.t = t = T.Tables(*_graph(name))
        self.n, self.dev = t.n, dev
        self.rowptr = torch.from_numpy(t.rowptr).to(dev)
        self.col = _i32(t.col, dev)
        self.revpos = _i32(t.revpos, dev)
        self.bounds, self.cuts, self.wpaths = _i32(t.bounds, dev), _i16(t.cuts, dev), _i32(t.wpaths, dev)
        self.fx32, self.ssum, self.smax = _i32(t.fx32, dev), _i32(t.ssum, dev), _i32(t.smax, dev)
        self.graph = eps.CSRGraph(self.rowptr, self.col, None, t.n, t.n)
        self._heads = {}

    def heads(self, n_hub, budget):
        key = (int(n_hub), int(budget))
        if key not in self._heads:
            h, wp = self.t.head_tables(n_hub, budget)
            self._heads[key] = (_i32(h, self.dev), _i32(wp, self.dev))
        return self._heads[key]

    def plan_inputs(self, mode, variant):
        """The device side of T.plan_inputs: (wpaths, ssum, smax, heads, variant word)."""
        wp, ssum, smax, hd, word = T.plan_inputs(self.t, mode, variant)
        d_wp, d_hd = (self.wpaths, None) if hd is None else self.heads(self.n, self.t.mid_budget())[::-1]
        return d_wp, (None if ssum is None else self.ssum), (None if smax is None else self.smax), d_hd, word


@pytest.fixture
def world(eps, dev):
    def get(name):
        if name not in _WORLD:
            _WORLD[name] = World(eps, dev, name)
        return _WORLD[name]
    return get


# ------------------------------------------------------------------------------------------------- bounds, cuts
@pytest.mark.parametrize("name", ALL)
def test_bounds_and_cuts(eps, world, name):
    w = world(name)
    got = _u(eps.ops.scan_bounds(w.rowptr, w.n))
    assert np.array_equal(got, w.t.bounds)
    assert got[0] == 0 and got[M] == w.n and (np.diff(got) >= 0).all()
    if w.n < M or w.t.nnz == 0:
        assert (np.diff(got) == 0).any()                               # (empty windows repeat a boundary)
    cuts = _u(eps.ops.scan_cuts(w.rowptr, w.col, w.bounds))
    assert cuts.shape == (w.n, M) and np.array_equal(cuts, w.t.cuts)
    assert np.array_equal(cuts[:, M - 1], np.diff(w.t.rowptr))
    if name.startswith("star"):
        assert cuts.max() == 0xFFFF and w.t.revpos.max() == 0xFFFE


def test_a_row_of_65536_entries_is_refused(eps, dev):
    from eps_amd import scan
    rp, col = T.star(65536, True)
    g = eps.CSRGraph(torch.from_numpy(rp).to(dev), _i32(col, dev), None, len(rp) - 1, len(rp) - 1)
    with pytest.raises(eps.EpsError):
        scan.screen_tables(g)
    assert scan.screen_variant(g) is None


# ------------------------------------------------------------------------------------------------- window paths
@pytest.mark.parametrize("name", ALL)
def test_window_paths(eps, world, name):
    from eps_amd import scan
    w = world(name)
    got = _u(eps.ops.scan_window_paths(w.rowptr, w.col, w.revpos, w.cuts))
    assert np.array_equal(got, w.t.wpaths)
    if w.t.nnz:
        assert np.array_equal(_u(scan.reverse_positions(w.graph)), w.t.revpos)
        assert np.array_equal(got.sum(1), scan.half_paths(w.graph).cpu().numpy())
    assert np.array_equal(got.sum(1), T.half_paths(w.t.rowptr, w.t.col))
    # three head tables: nothing skipped, a few rows skipped, whole rows swallowed
    budgets = (w.t.mid_budget(),) if name == "rmat17_as_labelled" else (0, w.t.mid_budget(), (1 << 31) - 1)
    for budget in budgets:
        h, wp = w.heads(w.n, budget)
        assert np.array_equal(_u(eps.ops.scan_heads(w.rowptr, w.col, w.fx32, w.n, budget)), _u(h))
        assert np.array_equal(_u(eps.ops.scan_window_paths(w.rowptr, w.col, w.revpos, w.cuts, h)), _u(wp)), budget
        if w.t.nnz and budget == 0:
            assert not _u(h).any() and np.array_equal(_u(wp), w.t.wpaths)
        if w.t.nnz and budget == (1 << 31) - 1 and w.t.ssum.max() < budget:       # (every row fits the budget whole)
            assert np.array_equal(_u(h)[:, 0], np.diff(w.t.rowptr)) and not _u(wp).any()
        if name in T.PIN_GRAPHS and budget == w.t.mid_budget():
            assert 0 < _u(wp).sum() < w.t.wpaths.sum()


@pytest.mark.parametrize("name", ("rmat14_hubs_first", "lane_rows", "star_hub_last", "n20"))
def test_window_paths_of_listed_columns(eps, dev, world, name):
    w = world(name)
    rng = np.random.default_rng(7)
    some = np.unique(np.concatenate([rng.integers(0, w.n, max(3, w.n // 50)), [0, w.n - 1, w.n - 2]]))
    some = some[rng.permutation(len(some))]
    columns = _i32(some, dev)
    fill = 0x5A5A5A5A
    out = torch.full((w.n, M), fill, dtype=torch.int32, device=dev)
    eps.ops._call("eps_scan_window_paths_columns", dev, w.rowptr, w.col, w.revpos, w.cuts, w.n, columns, columns.numel(), out)
    got = _u(out)
    assert np.array_equal(got[some], w.t.wpaths[some])
    rest = np.setdiff1d(np.arange(w.n), some)
    assert (got[rest] == fill).all()
    got = _u(eps.ops.scan_window_paths(w.rowptr, w.col, w.revpos, w.cuts, columns=columns))
    assert np.array_equal(got[some], w.t.wpaths[some])


# ------------------------------------------------------------------------------------------------- screening weights
@pytest.mark.parametrize("shift", (0, 1, 12, 31, 40))
def test_screen_weights(eps, dev, shift):
    fixw, beyond = T.weight_edge_cases(shift)
    rng = np.random.default_rng(shift)
    fixw = np.concatenate([fixw, rng.integers(0, 1 << min(62, 71 - shift), 3000)])      # (quotients below 2^32)
    fx, bad = eps.ops.scan_screen_weights(torch.from_numpy(fixw).to(dev), shift)
    want, flag = T.screen_weights(fixw, shift)
    assert flag == 0 and int(bad) == 0 and np.array_equal(_u(fx), want)
    assert (want.max() == 0xFFFFFFFF) == (shift >= 10)
    down = 40 - shift
    assert ((want << down) >= fixw).all() and (((want - 1) << down) < np.maximum(fixw, 1)).all(), "not the round-up"
    if beyond is not None:
        over = np.append(fixw, beyond)
        fx, bad = eps.ops.scan_screen_weights(torch.from_numpy(over).to(dev), shift)
        want, flag = T.screen_weights(over, shift)
        assert flag == 2 and int(bad) == 2 and np.array_equal(_u(fx), want)
    neg = fixw.copy()
    neg[5] = -3
    d_neg = torch.from_numpy(neg).to(dev)
    fx, bad = eps.ops.scan_screen_weights(d_neg, shift)
    want, flag = T.screen_weights(neg, shift)
    assert flag == 1 and int(bad) == 1 and np.array_equal(_u(fx), want) and want[5] == 1
    # the flag word is cleared by the call: the same word, after a call that set it
    out = torch.empty(len(neg), dtype=torch.int32, device=dev)
    eps.ops._call("eps_scan_screen_weights", dev, d_neg, len(neg), shift, out, bad)
    assert int(bad) == 1
    eps.ops._call("eps_scan_screen_weights", dev, torch.from_numpy(fixw).to(dev), len(fixw), shift, out, bad)
    assert int(bad) == 0
    bad.fill_(-1)
    eps.ops._call("eps_scan_screen_weights", dev, None, 0, shift, None, bad)
    assert int(bad) == 0
    fx, bad = eps.ops.scan_screen_weights(torch.empty(0, dtype=torch.int64, device=dev), shift)
    assert fx.numel() == 0 and int(bad) == 0


# ------------------------------------------------------------------------------------------------- row sums, row records
def _row_sums(eps, w, fx):
    ssum, smax, min_fx = eps.ops.scan_row_sums(w.rowptr, w.col, _i32(fx, w.dev), w.bounds, w.n)
    want = T.row_sums(w.t.rowptr, w.t.col, fx, w.t.bounds)
    assert np.array_equal(_u(ssum), want[0])
    assert np.array_equal(_u(smax), want[1]) and _u(smax)[M] == 0
    assert int(_u(min_fx)[0]) == want[2]
    return want


@pytest.mark.parametrize("name", ALL)
def test_row_sums(eps, world, name):
    w = world(name)
    ssum, smax, min_fx = _row_sums(eps, w, w.t.fx32)
    assert np.array_equal(ssum, w.t.ssum) and (np.diff(smax) <= 0).all()
    if name in ("no_edges", "one_node", "one_edge"):
        assert min_fx == 0xFFFFFFFF                                    # (no node with two neighbours)
    if name in ("n20", "no_edges"):
        assert (np.diff(w.t.bounds) == 0).any()                        # (the window search meets empty windows)
    if name in ("lane_rows", "n20", "rmat14_hubs_first"):
        ids = np.arange(w.n)
        # weights of 2^31 and more on a third of the nodes: the sums are unsigned, rows beyond 2^31 - 1 are clamped ...
        ssum, _, min_fx = _row_sums(eps, w, np.where((ids % 3 == 0) & (ids != w.n - 1), 0x80000005 + ids, 1000 + ids))
        assert (ssum == 2 ** 31 - 1).any() and (ssum < 2 ** 31 - 1).any() and min_fx < 2 ** 31
        # ... and on every node: the smallest of them is found by an UNSIGNED comparison
        ssum, smax, min_fx = _row_sums(eps, w, 0x80000001 + (ids * 7919) % 1000)
        assert min_fx >= 2 ** 31 and smax[0] == 2 ** 31 - 1
    deg = np.diff(w.t.rowptr)
    if (deg == 1).any() and (deg >= 2).any():
        # the lightest node of all has ONE neighbour: it is no common neighbour of anything and must not set min_fx
        fx = 5000 + np.arange(w.n)
        fx[np.flatnonzero(deg == 1)[0]] = 7
        assert _row_sums(eps, w, fx)[2] >= 5000


@pytest.mark.parametrize("name", ALL)
def test_row_records(eps, world, name):
    w = world(name)
    rr = eps.ops.scan_row_records(w.cuts, w.rowptr, w.fx32)
    assert rr.shape == (w.n, 32) and rr.data_ptr() % 128 == 0
    got = _u(rr)
    assert np.array_equal(got, w.t.rowrec)
    assert not got[:, 18:].any() and np.array_equal(got[:, 17], w.t.fx32) and np.array_equal(got[:, 16], w.t.rowptr[:-1] & T.U32)


# ------------------------------------------------------------------------------------------------- the plan
PLAN_CASES = [(name, variant, mode) for name in T.PIN_GRAPHS for variant in (0, 1, 2) for mode in T.PLAN_MODES] + \
             [(name, 2, mode) for name in SMALL for mode in ("plain", "nosum", "heads_wide")]


@pytest.mark.parametrize("name,variant,mode", PLAN_CASES)
def test_plan(eps, dev, world, name, variant, mode):
    w = world(name)
    t = w.t
    wp, ssum, smax, hd, word = w.plan_inputs(mode, variant)
    h_wp, h_ssum, h_smax, h_hd, _ = T.plan_inputs(t, mode, variant)
    pptr, recs, d_word = eps.ops.scan_plan(w.rowptr, w.cuts, wp, ssum, smax, w.bounds, w.n, t.shift, word, with_d=True, heads=hd)
    want_pptr, want_recs, want_d = T.plan(t.rowptr, t.bounds, t.cuts, h_wp, h_ssum, h_smax, h_hd, t.shift, word)
    got_pptr = _u(pptr)
    n_rec = int(got_pptr[-1])
    got_recs = _u(recs)[:n_rec]
    assert np.array_equal(got_pptr, want_pptr)
    assert np.array_equal(got_recs, want_recs)
    assert int(_u(d_word)[0]) == want_d
    # the invariants, from the device's records and the truth's tables
    T.check_plan(got_pptr, got_recs, int(_u(d_word)[0]), t.rowptr, t.bounds, t.cuts, h_wp, h_ssum, h_smax, h_hd, t.shift, word)
    assert eps.ops.scan_plan_rewalk((pptr, recs), variant) == T.rewalk(got_recs, variant)
    # the counting call
    counts = torch.full((w.n,), -1, dtype=torch.int32, device=dev)
    eps.ops._call("eps_scan_plan", dev, w.rowptr, w.cuts, wp, ssum, smax, hd, w.bounds, w.n, t.shift, word, counts, None, None, None)
    assert np.array_equal(_u(counts), np.diff(want_pptr))
    if mode == "nosum":
        assert np.isin(T.fields(got_recs)["kind"], (0, 2)).all()


def test_plan_clears_d_used(eps, dev, world):
    """The word a plan with packed pieces set is cleared by a plan without."""
    w = world("rmat15_hubs_last")
    tables = (w.rowptr, w.cuts, w.wpaths)
    pptr, recs, d_word = eps.ops.scan_plan(*tables, w.ssum, w.smax, w.bounds, w.n, w.t.shift, 2, with_d=True)
    assert int(d_word) > 0
    p0, r0 = eps.ops.scan_plan(*tables, None, None, w.bounds, w.n, w.t.shift, 2)
    eps.ops._call("eps_scan_plan", dev, *tables, None, None, None, w.bounds, w.n, w.t.shift, 2, None, p0, r0, d_word)
    assert int(d_word) == 0


# ------------------------------------------------------------------------------------------------- the column pack
@pytest.mark.parametrize("name", ALL)
def test_column_pack(eps, world, name):
    w = world(name)
    t = w.t
    rr = eps.ops.scan_row_records(w.cuts, w.rowptr, w.fx32)
    seen = set()
    for mode in ("plain", "heads", "nosum"):
        wp, ssum, smax, hd, word = w.plan_inputs(mode, 2)
        plan = eps.ops.scan_plan(w.rowptr, w.cuts, wp, ssum, smax, w.bounds, w.n, t.shift, word, heads=hd)
        pack = eps.ops.scan_column_pack(w.rowptr, w.col, w.revpos, rr, plan)
        assert pack.shape == (max(t.nnz, 1), 8)
        pptr, recs = _u(plan[0]), _u(plan[1])
        want = T.column_pack(t.rowptr, t.col, t.revpos, t.rowrec, pptr, recs)
        assert np.array_equal(_u(pack)[:t.nnz], want), mode
        seen |= set(np.diff(pptr)[np.diff(t.rowptr) > 0].tolist())
    if name == "rmat17_as_labelled":
        assert 0 in seen and 9 in seen and max(seen) > 9 and set(range(1, 9)) <= seen
    if name.startswith("star"):
        assert (_u(pack)[:, 3] & 0xFFFF).max() == 0xFFFE


# ------------------------------------------------------------------------------------------------- Python consumers
def _weights(eps, g, kind):
    from eps_amd.heuristics import node_weight_table
    if kind == "cn":
        return torch.ones(g.n_rows, dtype=torch.float32, device=g.device)
    return node_weight_table(g, {"aa": eps.ops.W_AA, "ra": eps.ops.W_RA}[kind])


_SCREENS = {}


def _screen(eps, world, kind):
    """The Screen of rmat14_hubs_first under AA / RA / CN weights (the graph is scanned as it is: it IS hubs-first)."""
    from eps_amd import scan
    if kind not in _SCREENS:
        g = world("rmat14_hubs_first").graph
        wt = _weights(eps, g, kind)
        _SCREENS[kind] = (g, wt, scan.screen_weights(g, g, None, wt))
    return _SCREENS[kind]


@pytest.mark.parametrize("kind", ("aa", "ra", "cn"))
def test_screen_object_matches_the_truths(eps, world, kind):
    """scan.screen_weights: fx32 / ssum / smax are the truths of the weight table it was given, w_min is one unit below the
    smallest weight of a node with two neighbours, and d_used -- once the plan is built -- is the plan's."""
    from eps_amd import scan
    g, wt, sc = _screen(eps, world, kind)
    t = world("rmat14_hubs_first").t
    assert sc.usable and sc.ssum is not None
    fixw = sc.fixw.cpu().numpy()
    fx, flag = T.screen_weights(fixw, sc.shift)
    assert flag == 0 and np.array_equal(_u(sc.fx32), fx)
    ssum, smax, min_fx = T.row_sums(t.rowptr, t.col, fx, t.bounds)
    assert np.array_equal(_u(sc.ssum), ssum) and np.array_equal(_u(sc.smax), smax)
    assert sc.w_min == max(0, min_fx - 1) * 2.0 ** -sc.shift and sc.w_min > 0
    assert np.array_equal(_u(sc.rowrec), T.row_records(t.cuts, t.rowptr, fx))
    pptr, recs = sc.plan
    want = T.plan(t.rowptr, t.bounds, t.cuts, t.wpaths, ssum, smax, None, sc.shift, sc.vword)
    assert np.array_equal(_u(pptr), want[0]) and np.array_equal(_u(recs)[:int(want[0][-1])], want[1])
    assert sc.d_used == want[2]
    T.check_plan(_u(pptr), _u(recs), sc.d_used, t.rowptr, t.bounds, t.cuts, t.wpaths, ssum, smax, None, sc.shift, sc.vword)


def test_column_records_and_live_columns(eps, dev, world):
    from eps_amd import scan
    g, wt, sc = _screen(eps, world, "aa")
    t = world("rmat14_hubs_first").t
    ssum = _u(sc.ssum)
    ht = scan.head_tables(g, sc, int(0.58 * np.median(ssum[ssum > 0])))
    heads, pptr = _u(ht.heads), _u(ht.plan[0])
    order = scan.column_order(g)
    live = scan.live_columns(g, sc, ht, 0, 1)
    floor = int(ht.budget / scan.HEAD_KEEP[1])
    h_order, h_live = order.cpu().numpy().astype(np.int64), live.cpu().numpy().astype(np.int64)
    kept = ssum[h_order] >= floor
    assert 0 < kept.sum() < len(h_order)
    assert np.array_equal(h_live, h_order[kept])                       # (kept: at or above the floor; dropped: below; order preserved)
    assert (ssum[h_live] >= floor).all() and (ssum[np.setdiff1d(h_order, h_live)] < floor).all()
    for columns, hd in ((live, ht.heads), (order[::37].contiguous(), None)):
        rec = scan.column_records(g, sc, columns, ht.plan, hd, {}, "k")
        got = _u(rec)
        assert got.shape == (columns.numel(), 8)
        for i, v in enumerate(columns.cpu().numpy().tolist()):
            hx, hy = (int(heads[v, 0]), int(heads[v, 1])) if hd is not None else (0, 0)
            assert got[i].tolist() == [v, int(t.rowptr[v]), int(t.rowptr[v + 1] - t.rowptr[v]), hx, hy, int(ssum[v]), int(pptr[v]),
                                       int(pptr[v + 1] - pptr[v])]
    assert scan.column_records(g, sc, order, None, None, {}, "k") is None


# ------------------------------------------------------------------------------------------------- the bound the bar rests on
@pytest.mark.parametrize("kind", ("aa", "ra", "cn"))
def test_lower_bound_holds_for_every_survivor(eps, dev, world, kind):
    """Every candidate of the graph, from one launch without a bar: its screening score s, the exact score (int64 sums of sc.fixw
    over the common neighbours, on the host, x 2^-40) and Screen.lower_bound(s) satisfy
        lower_bound(s) (1 - 2^-22) <= exact <= s (1 + 2^-23)
    in float64 -- 2^-23 covers the float32 rounding of s (half an ulp, 2^-24, relative), 2^-22 that rounding plus the two float32
    operations of the bound's own arithmetic.  A w_min that is too large, a d_used that is too small or a weight that was
    rounded down breaks one side."""
    import scipy.sparse as ssp
    from eps_amd import scan
    g, wt, sc = _screen(eps, world, kind)
    t = world("rmat14_hubs_first").t
    bounds, cuts = scan.screen_tables(g)
    res = eps.ops.Survivors(scan._capacity(2 * scan.total_half_paths(g), scan._PIECE_SLACK), float("-inf"), dev, prefill=False)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    eps.ops.scan_screen(g.rowptr, g.col, scan.reverse_positions(g), sc.fx32, cuts, bounds, g.n_rows, scan.column_order(g), sc.shift, res,
                        status, sc.vword if sc.vword is not None else scan.screen_variant(g), wpaths=scan.window_paths(g), ssum=sc.ssum,
                        smax=sc.smax, plan=sc.plan)
    assert int(status) == 0
    slots, n_cand = res.counts()
    keys, s32 = res.valid(slots)
    low = sc.lower_bound(s32, scan.max_degree(g)).double().cpu().numpy()
    keys, s = keys.cpu().numpy(), s32.double().cpu().numpy()
    assert n_cand >= len(keys) > 10 ** 6 and len(np.unique(keys)) == len(keys)
    # exact scores on the host: (A diag(fixw) A)[v, u]; float64 holds the sums exactly (< 2^41 per term, < 2^12 terms)
    fixw = sc.fixw.cpu().numpy()
    assert fixw.max() < 1 << 41 and np.diff(t.rowptr).max() < 1 << 12
    n = t.n
    A = ssp.csr_matrix((np.ones(t.nnz), t.col, t.rowptr), shape=(n, n))
    AW = ssp.csr_matrix((fixw[t.col].astype(np.float64), t.col, t.rowptr), shape=(n, n))
    P = ssp.tril(AW @ A, -1).tocoo()
    pk = (P.row.astype(np.int64) << 32) | P.col.astype(np.int64)
    o = np.argsort(pk)
    pk, pv = pk[o], P.data[o]
    at = np.searchsorted(pk, keys)
    assert (at < len(pk)).all() and np.array_equal(pk[at], keys), "a survivor without a two-hop path"
    exact = pv[at] * 2.0 ** -40
    up = exact <= s * (1 + 2.0 ** -23)
    down = low * (1 - 2.0 ** -22) <= exact
    print(kind, "shift", sc.shift, "d_used", sc.d_used, "w_min", sc.w_min, "survivors", len(keys),
          "max exact/s", float((exact / s).max()), "min exact/low", float((exact / np.maximum(low, 1e-300)).min()))
    assert up.all(), ("a screening score below the exact one", int((~up).sum()))
    assert down.all(), ("lower_bound above the exact score", int((~down).sum()))
