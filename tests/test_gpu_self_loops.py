"""GPU: the filter step on graphs WITH stored self loops (tests/loop_graphs.py) against the oracle -- the per-graph tables of the
scan, the candidate lists of every expansion path, every scan launch, scan_topk in all its configurations, the command line, and
the other block scorers.  A stored loop is an entry like any other: it counts in degrees and column sums (so in AA / RA weights),
it is its own mirror in the reverse-position table, and it never makes a candidate (filter.py:96-109: A @ A minus the diagonal
minus the known edges).  tests/test_loop_graphs_host.py pins, from the oracle alone, that these graphs can tell a kernel that
ignores, double-counts or misplaces the diagonal from a correct one."""
import numpy as np
import pytest
import torch

import loop_graphs as lg
import scan_table_truth as T
from conftest import rel_err
from test_gpu_scan import _scan_all, _screen_all

pytestmark = pytest.mark.gpu

MAIN = ("rmat_loops", "collab_like_loops")
LISTS = MAIN + lg.STRUCTURED
SCREENS = ((2, False, False), (2, True, False), (2, True, True), (2, False, True), (0, False, False), (0, True, True), (1, True, True))
_G = {}


def _graph(eps, dev, name, twin=False):
    """(LoopGraph, the CSRGraph on the device): one object per graph, so its cached tables are built once."""
    if (name, twin) not in _G:
        g = lg.graph(name)
        _G[name, twin] = eps.CSRGraph.from_scipy(g.twin if twin else g.A, device=dev, keep_values=g.weighted)
    return lg.graph(name), _G[name, twin]


def _fresh(eps, g):
    """The same arrays in a graph object without cached tables (a relabelled copy, once cached, would be scanned from then on)."""
    return eps.CSRGraph(g.rowptr, g.col, g.val, g.n_rows, g.n_cols)


def _weights(eps, g, kind):
    from eps_amd.heuristics import node_weight_table
    if kind == "cn":
        return torch.ones(g.n_rows, dtype=torch.float32, device=g.device)
    return node_weight_table(g, {"aa": eps.ops.W_AA, "ra": eps.ops.W_RA}[kind])


def _u(t):
    return T.unsigned(t.cpu().numpy())


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint32).view(np.int32))).to(dev)


def _i16(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint16).view(np.int16))).to(dev)


# ------------------------------------------------------------------------------------------------- a. per-graph tables
def _check_tables(eps, g, rp, col):
    """Every per-graph table of the graph ``g`` (device) whose pattern is (rp, col) on the host, against the numpy truths."""
    from eps_amd import scan
    dev, n = g.device, g.n_rows
    t = T.Tables(rp, col)
    assert np.array_equal(g.rowptr.cpu().numpy(), rp) and np.array_equal(g.col.cpu().numpy(), col)
    row = T.row_of(rp)
    diag = np.flatnonzero(row == col)
    assert len(diag), "the graph has no stored loop"
    # a diagonal entry is its own mirror: its reverse position is its place in its own row
    assert np.array_equal(t.revpos[diag], diag - rp[row[diag]])
    hp = T.half_paths(rp, col)
    deg = np.diff(rp)
    rev, hps, info = eps.ops.reverse_positions_symmetric(g.rowptr, g.col)
    flag, max_deg, max_half, total = info.tolist()
    assert flag & 0xFFFFFFFF == 0, "the symmetric pass calls a looped symmetric pattern asymmetric"
    assert np.array_equal(_u(rev), t.revpos) and np.array_equal(hps.cpu().numpy(), hp)
    assert (max_deg, max_half, total) == (int(deg.max()), int(hp.max()), int(hp.sum()))
    rev, hps, flag = eps.ops.reverse_positions(g.rowptr, g.col, with_stats=True)
    assert int(flag) == 0 and np.array_equal(_u(rev), t.revpos) and np.array_equal(hps.cpu().numpy(), hp)
    assert scan.is_symmetric(g) and scan.scan_available(g)
    assert np.array_equal(_u(scan.reverse_positions(g)), t.revpos) and np.array_equal(scan.half_paths(g).cpu().numpy(), hp)
    assert scan.max_degree(g) == int(deg.max()) and scan.max_half_paths(g) == int(hp.max()) and scan.total_half_paths(g) == int(hp.sum())
    order = scan.column_order(g).cpu().numpy()
    assert np.array_equal(order, np.argsort(-hp, kind="stable"))
    # two-hop paths out of every node (the loop's own row counts among them)
    two = np.zeros(n, np.int64)
    np.add.at(two, row, deg[col])
    assert np.array_equal(eps.ops.two_path_counts(g.rowptr, g.col).cpu().numpy(), two)
    assert eps.ops.max_column_paths(g.rowptr, g.col, 0, n) == int(two.max())
    lo, hi = n // 3, 2 * n // 3 + 1
    assert eps.ops.max_column_paths(g.rowptr, g.col, lo, hi) == int(two[lo:hi].max())
    # id windows of the two-pass scan: this graph takes one; the split table for three windows of n / 3 ids
    assert eps.ops.filter_scan_windows(n)[1] == 1 and scan.window_splits(g) is None
    win = -(-n // 3)
    if win * 2 < n:
        splits = eps.ops.row_window_splits(g.rowptr, g.col, win, 3).cpu().numpy().reshape(2, n)
        keys = row * (n + 1) + col
        for k in range(2):
            below = np.searchsorted(keys, np.arange(n) * (n + 1) + (k + 1) * win) - rp[:-1]
            assert np.array_equal(splits[k], below), k
    # the one-pass scan's tables
    bounds, cuts = scan.screen_tables(g)
    assert np.array_equal(_u(bounds), t.bounds) and np.array_equal(_u(cuts), t.cuts)
    assert np.array_equal(_u(scan.window_paths(g)), t.wpaths) and np.array_equal(t.wpaths.sum(1), hp)
    d_fx, d_ssum, d_smax = _i32(t.fx32, dev), _i32(t.ssum, dev), _i32(t.smax, dev)
    ssum, smax, min_fx = eps.ops.scan_row_sums(g.rowptr, g.col, d_fx, bounds, n)
    assert np.array_equal(_u(ssum), t.ssum) and np.array_equal(_u(smax), t.smax) and int(_u(min_fx)[0]) == t.min_fx
    rr = eps.ops.scan_row_records(cuts, g.rowptr, d_fx)
    assert np.array_equal(_u(rr), t.rowrec)
    for budget in (0, t.mid_budget(), (1 << 31) - 1):
        h, wp = t.head_tables(n, budget)
        d_h = eps.ops.scan_heads(g.rowptr, g.col, d_fx, n, budget)
        assert np.array_equal(_u(d_h), h), budget
        assert np.array_equal(_u(eps.ops.scan_window_paths(g.rowptr, g.col, scan.reverse_positions(g), cuts, d_h)), wp), budget
    for variant in (0, 1, 2):
        for mode in ("plain", "nosum", "heads", "heads_wide"):
            h_wp, h_ssum, h_smax, h_hd, word = T.plan_inputs(t, mode, variant)
            d_hd = None if h_hd is None else _i32(h_hd, dev)
            pptr, recs, d_word = eps.ops.scan_plan(g.rowptr, cuts, _i32(h_wp, dev), None if h_ssum is None else d_ssum,
                                                   None if h_smax is None else d_smax, bounds, n, t.shift, word, with_d=True, heads=d_hd)
            want_pptr, want_recs, want_d = T.plan(t.rowptr, t.bounds, t.cuts, h_wp, h_ssum, h_smax, h_hd, t.shift, word)
            got_pptr = _u(pptr)
            got_recs = _u(recs)[:int(got_pptr[-1])]
            assert np.array_equal(got_pptr, want_pptr) and np.array_equal(got_recs, want_recs), (variant, mode)
            assert int(_u(d_word)[0]) == want_d
            T.check_plan(got_pptr, got_recs, want_d, t.rowptr, t.bounds, t.cuts, h_wp, h_ssum, h_smax, h_hd, t.shift, word)
            if variant == 2 and mode in ("plain", "heads"):
                pack = eps.ops.scan_column_pack(g.rowptr, g.col, scan.reverse_positions(g), rr, (pptr, recs))
                assert np.array_equal(_u(pack)[:t.nnz], T.column_pack(t.rowptr, t.col, t.revpos, t.rowrec, got_pptr, _u(recs))), mode
    # the Screen object scan_topk works with (unit values: its tables are the truths of the weight table it was given)
    if g.val is None:
        sc = scan.screen_weights(g, g, None, _weights(eps, g, "aa"))
        assert sc.usable and scan.one_pass_available(g) and sc.ssum is not None and sc.has_plan
        fx, bad = T.screen_weights(sc.fixw.cpu().numpy(), sc.shift)
        assert bad == 0 and np.array_equal(_u(sc.fx32), fx)
        ssum, smax, _ = T.row_sums(rp, col, fx, t.bounds)
        assert np.array_equal(_u(sc.ssum), ssum) and np.array_equal(_u(sc.smax), smax)
        assert np.array_equal(_u(sc.rowrec), T.row_records(t.cuts, rp, fx))
        pptr, recs = sc.plan
        want = T.plan(rp, t.bounds, t.cuts, t.wpaths, ssum, smax, None, sc.shift, sc.vword)
        assert np.array_equal(_u(pptr), want[0]) and np.array_equal(_u(recs)[:int(want[0][-1])], want[1]) and sc.d_used == want[2]
        columns = scan.column_order(g)[::3].contiguous()
        got = _u(scan.column_records(g, sc, columns, sc.plan, None, {}, "k"))
        v = columns.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, np.stack([v, rp[v], deg[v], 0 * v, 0 * v, ssum[v], want[0][v], np.diff(want[0])[v]], 1))


@pytest.mark.parametrize("name", LISTS)
def test_tables_as_labelled_and_hubs_first(eps, dev, name):
    g0, g = _graph(eps, dev, name)
    rp, col, val = lg.arrays(g0.A, g0.weighted)
    assert (g.val is not None) == g0.weighted
    _check_tables(eps, _fresh(eps, g), rp, col.astype(np.int64))
    gs, perm, inv = _fresh(eps, g).degree_ordered()
    order = lg.hubs_first_order(g0.A)
    assert np.array_equal(perm.cpu().numpy(), order) and np.array_equal(inv.cpu().numpy()[order], np.arange(g.n_rows))
    rp2, col2 = T.hubs_first(rp, col, keep_loops=True)
    assert rp2[-1] == rp[-1], "the relabelled truth lost entries"
    _check_tables(eps, gs, rp2, col2)
    if g0.weighted:                                                  # the values travel with their entries (the loop's included)
        B = g0.A.tocsr()[order][:, order]
        B.sort_indices()
        assert np.array_equal(gs.val.cpu().numpy(), B.data)


# ------------------------------------------------------------------------------------------------- b. full candidate lists
def _expansion(eps, g, wt, **kw):
    return eps.ops.expand_candidates(g.rowptr, g.col, g.val, wt, g.n_rows, kw.pop("lo", 0), kw.pop("hi", g.n_rows), **kw)


@pytest.mark.parametrize("name", LISTS)
def test_candidate_lists(eps, oracle, dev, name):
    from eps_amd import candidates, scan
    g0, g = _graph(eps, dev, name)
    n = g.n_rows
    t = lg.truth(oracle, name, "aa")
    wt = _weights(eps, g, "aa")
    full = _expansion(eps, g, wt)
    colptr, cu, cv, cn, sc = full
    assert np.array_equal(np.stack([cu.cpu().numpy(), cv.cpu().numpy()], 1), t.pairs), "not the oracle's column-major candidate list"
    assert np.array_equal(cn.cpu().numpy(), t.count)
    assert rel_err(sc.cpu().numpy(), t.f64.astype(np.float32)) <= 1e-6
    assert np.array_equal(np.diff(colptr.cpu().numpy()), np.bincount(t.pairs[:, 1], minlength=n))
    ones = _weights(eps, g, "cn")
    cn_t = lg.truth(oracle, name, "cn")
    by_ones = _expansion(eps, g, ones, want_cn=False)
    assert np.array_equal(by_ones[4].cpu().numpy(), cn_t.cn)                        # (unit weights: the reference's CN value, exactly)
    # a column sub-range, the tiled variant, a score cut
    lo, hi = n // 3, 2 * n // 3 + 1
    sel = (t.pairs[:, 1] >= lo) & (t.pairs[:, 1] < hi)
    at = torch.from_numpy(np.flatnonzero(sel)).to(dev)
    part = _expansion(eps, g, wt, lo=lo, hi=hi)
    for i in range(1, 5):
        assert torch.equal(part[i], full[i][at]), i
    assert np.array_equal(np.diff(part[0].cpu().numpy()), np.bincount(t.pairs[sel, 1] - lo, minlength=hi - lo))
    tiled = _expansion(eps, g, wt, tile_ranks=512)
    for i in range(5):
        assert torch.equal(tiled[i], full[i]), i
    if sc.numel():
        thr = float(sc.median())
        cut = _expansion(eps, g, wt, cut=(thr, sc.numel()))
        pos = torch.nonzero(sc > thr).squeeze(1)
        assert torch.equal(cut.survivors[0], pos) and torch.equal(cut.survivors[1], sc[pos])
        for i in range(5):
            assert torch.equal(cut[i], full[i]), i
    # the pair list in tensor operations
    assert np.array_equal(candidates.two_hop_block(g, 0, n).cpu().numpy().T, t.pairs)
    assert np.array_equal(candidates.two_hop_block(g, lo, hi).cpu().numpy().T, t.pairs[sel])
    if g.val is not None:
        return
    # the unit list kernels: count + fill (whole list and the u < v half), and the one-pass list -- the expansion's bits
    md, splits = scan.max_degree(g), scan.window_splits(g)
    unit = eps.ops.expand_unit(g.rowptr, g.col, wt, n, 0, n, md, splits)
    assert torch.equal(unit[0], full[0]) and torch.equal(unit[1], cu) and torch.equal(unit[2], cv) and torch.equal(unit[4], sc)
    sub = eps.ops.expand_unit(g.rowptr, g.col, wt, n, lo, hi, md, splits)
    assert torch.equal(sub[1], cu[at]) and torch.equal(sub[2], cv[at]) and torch.equal(sub[4], sc[at])
    half = eps.ops.expand_unit(g.rowptr, g.col, wt, n, 0, n, md, splits, revpos=scan.reverse_positions(g))
    lower = cu < cv
    assert torch.equal(half[1], cu[lower]) and torch.equal(half[2], cv[lower]) and torch.equal(half[4], sc[lower])
    assert int(half[0][-1]) * 2 == len(t.pairs)
    ub, _ = candidates.segment_bounds(g)
    once = eps.ops.expand_unit(g.rowptr, g.col, wt, n, 0, n, md, splits, want_v=False, colptr_ub=ub, total_ub=int(ub[-1]))
    assert int(once.status) == 0 and torch.equal(once.counts, colptr[1:] - colptr[:-1])
    slot = (ub[:-1].repeat_interleave(once.counts) + torch.arange(cu.numel(), device=dev) - colptr[:-1].repeat_interleave(once.counts))
    assert torch.equal(once[1][slot], cu) and torch.equal(once[4][slot], sc)
    # the dense path: the adjacency holds the diagonal, the product counts paths through a loop, the masked read drops both
    a = eps.ops.dense_adjacency(g.rowptr, g.col, n)
    assert np.array_equal(a[:n, :n].cpu().numpy(), g0.A.toarray()) and not bool(a[n:].any()) and not bool(a[:, n:].any())
    keys, vals = eps.ops.dense_cn_candidates(g.rowptr, g.col, n)
    lower_t = cn_t.pairs[:, 0] < cn_t.pairs[:, 1]
    assert np.array_equal(keys.cpu().numpy(), (cn_t.pairs[lower_t, 1] << 32) | cn_t.pairs[lower_t, 0])
    assert np.array_equal(vals.cpu().numpy(), cn_t.cn[lower_t])
    keys, vals = eps.ops.dense_cn_candidates(g.rowptr, g.col, n, directed=True, check_symmetric=True)
    assert np.array_equal(keys.cpu().numpy(), (cn_t.pairs[:, 1] << 32) | cn_t.pairs[:, 0]) and np.array_equal(vals.cpu().numpy(), cn_t.cn)


# ------------------------------------------------------------------------------------------------- c. scan launches
@pytest.mark.parametrize("name", LISTS)
def test_scan_launches(eps, oracle, dev, name):
    """Every launch flavour, without a bar and with the median score as the bar: exactly the u < v half of the expansion's list
    with its score bits, and the oracle's number of candidates.  (collab_like_loops: stored values -- eps_scan_screen_weighted.)"""
    from eps_amd import scan
    g0, g = _graph(eps, dev, name)
    t = lg.truth(oracle, name, "aa")
    wt = _weights(eps, g, "aa")
    _, cu, cv, _, sc = _expansion(eps, g, wt, want_cn=False)
    half = cu < cv
    full = {(int(u), int(v)): float(s) for u, v, s in zip(cu[half].tolist(), cv[half].tolist(), sc[half].tolist())}
    n_half = int((t.pairs[:, 0] < t.pairs[:, 1]).sum())
    assert len(full) == n_half and 2 * n_half == len(t.pairs)
    bar = sorted(full.values())[len(full) // 2] if full else 0.0
    above = {k: x for k, x in full.items() if x > bar}
    assert name not in MAIN or 0 < len(above) < len(full)             # (a star's candidates all tie: its bar keeps none)
    assert scan.scan_available(g)
    if g.val is None:
        got, n_cand = _scan_all(eps, g, wt)
        assert n_cand == n_half and got == full
        got, n_cand = _scan_all(eps, g, wt, thr=bar)
        assert n_cand == n_half and got == above
    gs = g if g.val is None else scan.scan_graph(g)[0]
    assert scan.one_pass_available(gs)
    if g.val is not None:                       # stored values are scanned under hubs-first labels: the same pairs, renamed
        perm = scan.scan_graph(g)[1].cpu().numpy()
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        ren = lambda d: {(min(inv[u], inv[v]), max(inv[u], inv[v])): x for (u, v), x in d.items()}      # noqa: E731
        full, above, wt = ren(full), ren(above), wt[scan.scan_graph(g)[1]].contiguous()
    for variant, packed, table in SCREENS:
        got, n_cand = _screen_all(eps, gs, wt, variant=variant, packed=packed, table=table)
        assert n_cand == n_half and got == full, (variant, packed, table)
        got, n_cand = _screen_all(eps, gs, wt, thr=bar, variant=variant, packed=packed, table=table)
        assert n_cand == n_half and got == above, (variant, packed, table)


# ------------------------------------------------------------------------------------------------- d. scan_topk
def _check_rows(pairs, scores, t, k, gate, what):
    """Rows of scan_topk against a Truth: candidates, sorted, scores within ``gate`` of the float64 truth, nothing better left out,
    ties in candidate order; and exactly the truth's rows wherever the truth is not within 2 x gate of its own K-th score."""
    n = int(t.pairs.max()) + 1 if len(t.pairs) else 1
    p, s = pairs.cpu().numpy(), scores.cpu().numpy()
    kk = min(k, len(t.pairs))
    assert p.shape == (2, kk) and s.shape == (kk,) and bool((s[:-1] >= s[1:]).all()), what
    key = t.pairs[:, 1] * n + t.pairs[:, 0]
    pos = np.searchsorted(key, p[1] * n + p[0])
    assert (pos < len(key)).all() and np.array_equal(key[pos], p[1] * n + p[0]), f"{what}: a row is no 2-hop non-edge"
    assert len(np.unique(pos)) == kk, f"{what}: a row twice"
    assert rel_err(s, t.f64[pos].astype(np.float32)) <= gate, what
    kth = np.sort(t.f64)[-kk]
    assert s.min() >= np.float32(kth) * (1 - 1e-6), f"{what}: a better candidate was left out"
    same = s[:-1] == s[1:]
    assert bool((pos[:-1][same] < pos[1:][same]).all()), f"{what}: tied rows out of candidate order"
    sure, maybe = np.flatnonzero(t.f64 > kth * (1 + 2 * gate)), np.flatnonzero(t.f64 >= kth * (1 - 2 * gate))
    assert set(sure.tolist()) <= set(pos.tolist()) <= set(maybe.tolist()), f"{what}: not the truth's first rows"


@pytest.mark.parametrize("name,kind", [("rmat_loops", "aa"), ("rmat_loops", "ra"), ("rmat_loops", "cn"),
                                       ("collab_like_loops", "aa"), ("collab_like_loops", "cn")])
def test_scan_topk_every_configuration(eps, oracle, dev, monkeypatch, name, kind):
    from eps_amd import scan
    g0, g = _graph(eps, dev, name)
    t = lg.truth(oracle, name, kind)
    gate = 1e-5 if g0.weighted else 1e-6
    wt = _weights(eps, g, kind)
    _, cu, cv, _, sc = _expansion(eps, g, wt, want_cn=False)
    order = torch.sort(sc, descending=True, stable=True).indices
    assert sc.numel() == len(t.pairs)
    defaults = dict(HEAD_MIN_PATHS=scan.HEAD_MIN_PATHS, SMALL_SET=scan.SMALL_SET)
    monkeypatch.setattr(scan, "RELABEL_MIN_NODES", 0)
    monkeypatch.setattr(scan, "SAMPLE_STRIDE", 7)                       # (a bar sample of a 2000-column graph: every 7th column)
    graphs = {False: _fresh(eps, g), True: _fresh(eps, g)}
    ran_heads = ran_bar = 0
    for k in (1, lg.K_INSIDE[name], sc.numel() + 5):
        kk = min(k, sc.numel())
        want_pairs, want_sc = torch.stack([cu[order[:kk]], cv[order[:kk]]]).long(), sc[order[:kk]]
        _check_rows(want_pairs, want_sc, t, k, gate, f"{name} {kind} K = {k}: the expansion's first rows")
        for relabel in (False, True):
            gr = graphs[relabel]
            w = _weights(eps, gr, kind)
            for head_min in (0, defaults["HEAD_MIN_PATHS"]):
                for small in (0, defaults["SMALL_SET"]):
                    for tail in (None, "library", "radix"):
                        monkeypatch.setattr(scan, "HEAD_MIN_PATHS", head_min)
                        monkeypatch.setattr(scan, "SMALL_SET", small)
                        monkeypatch.setattr(scan, "TAIL_DEVICE", tail is not None)
                        monkeypatch.setattr(scan, "TAIL_SORT", tail or "library")
                        what = (name, kind, k, relabel, head_min, small, tail)
                        st = {}
                        pairs, scores = scan.scan_topk(gr, w, k, relabel=relabel, stats=st)
                        assert torch.equal(pairs, want_pairs), what
                        assert torch.equal(scores, want_sc), what
                        assert st["candidates"] == len(t.pairs), what
                        if gr.val is None:
                            assert (scan.scan_graph(gr)[1] is not None) == relabel, what
                        ran_heads += int(bool(st["heads"]))
                        ran_bar += int(st["bar"] is not None)
    assert ran_bar, "no configuration scanned under an estimated bar"
    if g.val is None:
        assert ran_heads, f"{name} {kind}: no configuration ran with skipped heads -- the heads path was not exercised"
    else:
        assert not ran_heads                    # (stored values: scan_topk never skips heads -- its own condition)


def test_scan_topk_on_the_wide_graph_runs_in_windows(eps, oracle, dev, monkeypatch):
    """An id space the two-pass scan takes in two id windows: scan_topk through eps_filter_scan (windowed) and through the one-pass
    kernel gives the same rows, and they are the first K rows over the oracle's candidates (built in column slices)."""
    from eps_amd import scan
    g0, g = _graph(eps, dev, "wide_loops")
    n = g.n_rows
    win_ids, n_win = eps.ops.filter_scan_windows(n)
    assert n_win >= 2 and win_ids < n and scan.window_splits(g) is not None
    assert eps.ops.filter_scan_windows(n - 10_176)[1] == 1, "a smaller graph would not do: this is the threshold"
    step = 50_000
    parts = [oracle.candidates_scipy_columns(g0.A, lo, min(n, lo + step))[0] for lo in range(0, n, step)]
    t = lg.score_pairs(oracle, g0.A, False, "aa", np.concatenate(parts))
    wt = _weights(eps, g, "aa")
    k = 5000
    out = {}
    for one_pass in (False, True):
        monkeypatch.setattr(scan, "ONE_PASS", one_pass)
        gr = _fresh(eps, g)
        st = {}
        out[one_pass] = scan.scan_topk(gr, _weights(eps, gr, "aa"), k, stats=st)
        assert scan.one_pass_available(gr) == one_pass and scan.scan_graph(gr)[1] is None
        assert st["candidates"] == len(t.pairs)
        _check_rows(*out[one_pass], t, k, 1e-6, f"wide_loops one_pass = {one_pass}")
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])
    u, v = out[False][0].cpu().numpy()
    assert (np.minimum(u, v) < win_ids).any() and (np.maximum(u, v) >= win_ids).any()


# ------------------------------------------------------------------------------------------------- e. loops must be visible
@pytest.mark.parametrize("name,kind", [(n, k) for n in MAIN for k in ("aa", "ra")])
def test_the_rows_follow_the_loops(eps, oracle, dev, name, kind):
    """scan_topk on the looped graph and on its loop-free twin: the truths' first K rows differ (the loop is in the column sums),
    so the returned rows must differ too -- each following its own truth."""
    from eps_amd import scan
    k = lg.K_INSIDE[name]
    gate = 1e-5 if lg.graph(name).weighted else 1e-6
    got, tr = {}, {}
    for twin in (False, True):
        _, g = _graph(eps, dev, name, twin)
        tr[twin] = lg.truth(oracle, name, kind, twin=twin)
        got[twin] = scan.scan_topk(g, _weights(eps, g, kind), k)
        _check_rows(*got[twin], tr[twin], k, gate, f"{name} {kind} twin = {twin}")
    rows = {tw: tr[tw].pairs[lg.first_rows(tr[tw], k)] for tw in got}
    assert (rows[False] != rows[True]).any(), "the truth of the looped graph is the twin's: the loop is not in its column sums"
    assert not torch.equal(got[False][0], got[True][0]), "the looped graph's rows are its twin's: the scan does not see the loops"
    # the weight table itself: the oracle's, loop included
    _, g = _graph(eps, dev, name)
    assert rel_err(_weights(eps, g, kind).cpu().numpy(), tr[False].weights) <= 1e-6
    assert not np.array_equal(tr[False].weights, tr[True].weights)


# ------------------------------------------------------------------------------------------------- f. the command line, once
def test_filter_command_on_a_training_list_with_loops(eps, oracle, dev, tmp_path, monkeypatch):
    """filter.py --model adamic_ogb --keep_top K on the collab stand-in with (u, u) rows in its training edge list: the graph is
    oracle.add_edges_scipy's (the symmetrisation doubles a diagonal value), the file its candidates scored and ordered."""
    from eps_amd import datasets, filter_stage
    from test_gpu_katz_filter import _graph as stand_in_graph, _stand_in
    real = datasets.load_raw

    def looped(name, synthetic=False, device="cpu"):
        raw = real(name, synthetic, device)
        n = int(raw["num_nodes"])
        deg = torch.bincount(raw["edge_index"][0].cpu(), minlength=n)
        rng = np.random.default_rng(31)
        nodes = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < 1 / 3), torch.argsort(deg, descending=True)[:3].numpy(), [0, n - 1]]))
        loops = torch.from_numpy(np.stack([nodes, nodes])).to(raw["edge_index"])
        raw["edge_index"] = torch.cat([raw["edge_index"], loops], 1)
        raw["edge_weight"] = torch.cat([raw["edge_weight"], torch.from_numpy(rng.integers(1, 4, len(nodes))).to(raw["edge_weight"])])
        return raw
    monkeypatch.setattr(datasets, "load_raw", looped)
    k = 1000
    with _stand_in("collab", tmp_path):
        rows = torch.load(filter_stage.main(["--dataset", "collab", "--model", "adamic_ogb", "--checkpoint", "collab_adamic_ogb||0|0.pt",
                                             "--synthetic", "--keep_top", str(k)]))
        A = stand_in_graph(oracle, "collab").astype(np.float32)
    diag = A.diagonal()
    assert 0.3 * A.shape[0] < (diag != 0).sum() and set(np.unique(diag[diag != 0])) <= {2.0, 4.0, 6.0}, "the stand-in's loops are not doubled"
    assert (abs(A - A.T)).nnz == 0
    rows = rows.numpy()
    assert rows.dtype == np.float32 and rows.shape == (k, 3)
    u, v, s = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64), rows[:, 2]
    A = lg._csr(A)
    t = lg.score_pairs(oracle, A, True, "aa", oracle.candidates_scipy(A)[0])
    _check_rows(torch.from_numpy(np.stack([u, v])), torch.from_numpy(s), t, k, 1e-5, "filter.py on a looped training list")
    # score descending, then v ascending, then u ascending -- by the file's own scores
    assert np.array_equal(np.lexsort((u, v, -s.astype(np.float64))), np.arange(len(s))), "rows out of the declared order"


# ------------------------------------------------------------------------------------------------- g. the other block scorers
def _probe_pairs(g0, t, k=3000):
    """Pairs that put the loops in front of a scorer: candidates (every looped special node's among them), stored edges, the
    looped nodes with themselves and with each other."""
    rng = np.random.default_rng(41)
    n = g0.A.shape[0]
    special = np.concatenate([g0.hubs, g0.loop_alone, g0.loop_plus_one, [0, n - 1]])
    touch = np.flatnonzero(np.isin(t.pairs[:, 0], special) | np.isin(t.pairs[:, 1], special))
    cand = t.pairs[np.unique(np.concatenate([rng.choice(len(t.pairs), k, replace=False), touch[:k]]))]
    P = g0.A.tocoo()
    edges = np.stack([P.row, P.col], 1)[rng.choice(P.nnz, k, replace=False)]
    loops = lg.looped_nodes(g0.A)
    both = np.stack([np.concatenate([special, loops[:200]]), np.concatenate([special[::-1], loops[200:0:-1]])], 1)
    return np.concatenate([cand, edges, np.stack([special, special], 1), both]).astype(np.int64)


@pytest.mark.parametrize("scorer", ["local_index", "ppr", "sketch", "cn_list", "cosine"])
def test_other_block_scorers_on_rmat_loops(eps, oracle, dev, scorer):
    """Each scorer's own truth module on the looped graph, at the tolerance of that scorer's own GPU test."""
    from eps_amd import filter_stage, heuristics, ops
    g0, g = _graph(eps, dev, "rmat_loops")
    A, n = g0.A, g.n_rows
    t = lg.truth(oracle, "rmat_loops", "cn")
    rp, col, _ = lg.arrays(A, False)
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)      # noqa: E731
    if scorer == "local_index":
        import local_index_truth as lit
        cu, cv, cc = lit.two_hop_candidates(A)
        assert np.array_equal(np.stack([cu, cv], 1), t.pairs) and np.array_equal(cc, t.count)      # (this truth and the oracle agree)
        deg = lit.degrees(A)
        assert np.array_equal(deg, np.diff(rp))                                                    # (a loop counts in the degree)
        blk = filter_stage._counted_block(g, 0, n, False)
        assert np.array_equal(blk.cand_u.cpu().numpy(), cu) and np.array_equal(blk.cn.cpu().numpy().astype(np.int64), cc)
        for index in lit.INDICES:
            got = ops.local_index_columns(g.rowptr, n, 0, n, blk.colptr, blk.cand_u, blk.cn, index).cpu().numpy()
            lit.assert_within_one_ulp(got, lit.index_scores(index, cc, deg[cu], deg[cv]), f"rmat_loops {index}")
            pr = _probe_pairs(g0, t, 500)
            cnt = ops.pair_scores(g.rowptr, g.col, None, None, n, i32(pr[:, 0]), i32(pr[:, 1]))[0]
            got = ops.local_index_pairs(g.rowptr, n, i32(pr[:, 0]), i32(pr[:, 1]), cnt, index).cpu().numpy()
            lit.assert_within_one_ulp(got, lit.truth(A, pr[:, 0], pr[:, 1], index), f"rmat_loops {index} pairs")
    elif scorer == "ppr":
        import ppr_truth as pt
        sources = np.concatenate([g0.hubs, g0.loop_alone[:2], g0.loop_plus_one[:2], [0, n - 1], [int(np.flatnonzero(A.diagonal() == 0)[0])]])
        qptr = np.arange(len(sources) + 1, dtype=np.int64) * n
        qnode = np.tile(np.arange(n, dtype=np.int32), len(sources))
        for alpha, e in ((0.15, 1e-4), (0.5, 1e-6)):
            a16, thr = pt.parameters(alpha, e)
            want = pt.push_queries(rp, col, sources, qptr, qnode, a16, thr, 1024)
            assert want[1].max() >= 2
            for table in ("auto", "global"):
                got = ops.ppr_push(g.rowptr, g.col, n, i32(sources), torch.from_numpy(qptr).to(dev), i32(qnode), a16, thr, 1024, table=table)
                for what, a, b in zip(("mass", "rounds", "pushes", "steps", "capped"), got, want):
                    assert np.array_equal(a.cpu().numpy(), b), (alpha, e, table, what)
    elif scorer == "sketch":
        import sketch_truth as st
        hll, mh = st.tables(A, 2)
        own = ops.sketch_own(0, n, dev)
        h1 = ops.sketch_propagate(g.rowptr, g.col, n, own[0], own[1], keep_own=False)
        h2 = ops.sketch_propagate(g.rowptr, g.col, n, h1[0], h1[1], keep_own=True)
        as_np = lambda x: x.cpu().view(torch.int32).numpy().view(np.uint32) if x.dtype == torch.uint32 else x.cpu().numpy()      # noqa: E731
        for k, got in enumerate((h1, h2)):
            assert np.array_equal(as_np(got[0]), hll[k]) and np.array_equal(as_np(got[1]), mh[k]), f"hop {k + 1}"
        # a node whose row is its loop alone keeps its own sketch at hop 1; without the loop it would hold nothing
        own_h = as_np(own[0])
        assert all(np.array_equal(hll[0][v], own_h[v]) for v in g0.loop_alone) and own_h[g0.loop_alone].any()
        pr = _probe_pairs(g0, t, 500)
        tabs = (torch.stack([h1[0], h2[0]]), torch.stack([h1[1].view(torch.int32), h2[1].view(torch.int32)]).view(torch.uint32))
        S, Z, M = ops.sketch_pair_stats(tabs[0], tabs[1], n, i32(pr[:, 0]), i32(pr[:, 1]))
        wS, wZ, wM = st.pair_stats(hll, mh, pr[:, 0], pr[:, 1])
        assert np.array_equal(S.cpu().numpy(), wS) and np.array_equal(Z.cpu().numpy(), wZ) and np.array_equal(M.cpu().numpy(), wM)
    elif scorer == "cn_list":
        import cn_list_truth as ct
        pr = _probe_pairs(g0, t)
        ptr, w = ct.cn_lists(A, pr[:, 0], pr[:, 1])
        du, dv = i32(pr[:, 0]), i32(pr[:, 1])
        count = ops.pair_cn_list_count(g.rowptr, g.col, n, du, dv)
        assert np.array_equal(count.cpu().numpy(), np.diff(ptr))
        d_ptr = torch.from_numpy(ptr).to(dev)
        out = ops.pair_cn_list_fill(g.rowptr, g.col, n, du, dv, d_ptr, torch.full((len(w),), -1, dtype=torch.int32, device=dev))
        assert np.array_equal(out.cpu().numpy(), w)
        p2, w2 = ops.pair_cn_list(g.rowptr, g.col, n, dv, du)
        assert np.array_equal(p2.cpu().numpy(), ptr) and np.array_equal(w2.cpu().numpy(), w)
        # a looped node paired with itself lists its whole row, the loop included; with a neighbour, both ends of the edge
        looped = int(g0.hubs[0])
        at = int(np.flatnonzero((pr[:, 0] == looped) & (pr[:, 1] == looped))[0])
        assert np.array_equal(w[ptr[at]:ptr[at + 1]], col[rp[looped]:rp[looped + 1]]) and looped in w[ptr[at]:ptr[at + 1]]
        # candidates: the counts are the oracle's (no loop is ever a common neighbour of a non-edge)
        cand = t.pairs[::7]
        got = ops.pair_cn_list_count(g.rowptr, g.col, n, i32(cand[:, 0]), i32(cand[:, 1])).cpu().numpy()
        assert np.array_equal(got, t.count[::7])
    else:
        from test_cosine_cn_host import scores_truth, score_tolerance
        from test_gpu_cosine_cn import check_prologue, features
        x_dev, x_np = features(n, 58, seed=n)
        check_prologue(eps, A, x_dev, x_np, use_revpos=True)
        pr = _probe_pairs(g0, t, 1500).T
        got = heuristics.cosine_common_neighbors(g, x_dev, torch.from_numpy(pr).long()).cpu().numpy()
        truth, mag = scores_truth(A.astype(np.float64), x_np.astype(np.float64), pr)
        assert np.all(np.abs(got - truth) <= score_tolerance(mag, 58))
