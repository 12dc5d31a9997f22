"""The piece kernel's table sweeps, candidate counts and sketch hashes (csrc/scan_pieces.hip) against truths worked out on the host
with SciPy / numpy -- never with the library:

* ``n_candidates`` of a launch is the number of unordered two-hop non-edges its columns reach, on plans that hold every piece kind
  (32-bit direct, 16-bit direct, packed, two-word hash, hash-partitioned windows; stored values), and -- with skipped heads -- the
  number the walked rows reach;
* the survivors of every piece and their reported sums equal the host's sums of the rounded-up (and, per piece, coarsened) weights:
  table spans of every residue mod 4 and odd 16-bit spans, survivors in a table's first and last field, a known edge in the last
  field and next to a survivor in the same word, a sum at the bar and one unit below, candidates inside one wave's share of the
  table, a piece without a candidate;
* sketch pieces index inside their half tables for ids far above 2^16 / 2^20 and on plans whose sketch pieces take the smallest and
  the largest table size: the launch gives the same refined, exactly re-scored list as the hashed launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KIND_HASH, KIND_PACKED, KIND_DIRECT32, KIND_DIRECT16 = 0, 1, 2, 3


def _weights(eps, g, kind="aa"):
    from eps_amd.heuristics import node_weight_table
    if kind == "cn":
        return torch.ones(g.n_rows, dtype=torch.float32, device=g.device)
    return node_weight_table(g, eps.ops.W_AA)


def _sym(n, rows, cols):
    import scipy.sparse as ssp
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    m = rows != cols
    A = ssp.coo_matrix((np.ones(int(m.sum()) * 2, np.float32), (np.concatenate([rows[m], cols[m]]), np.concatenate([cols[m], rows[m]]))),
                       shape=(n, n)).tocsr()
    A.data[:] = 1.0
    A.sort_indices()
    return A


def _two_hop_non_edges(A):
    """Unordered pairs {u, v}, u != v, with a common neighbour and no edge: pattern of A.A minus A minus the diagonal, halved."""
    P = (A @ A).tocsr()
    P.data[:] = 1.0
    P.setdiag(0)
    P.eliminate_zeros()
    both = P.multiply(A)
    n2 = int(P.nnz) - int(both.nnz)
    assert n2 % 2 == 0
    return n2 // 2


def _plan_records(plan, bounds, n):
    """Per piece: column, kind, paths, lo, hi, dropped bits, known edges (host arrays) from the plan table's records."""
    pptr = plan[0].cpu().numpy().view(np.uint32).astype(np.int64)
    rec = plan[1].cpu().numpy().view(np.uint32).astype(np.int64)[:pptr[-1]]
    b = bounds.cpu().numpy().astype(np.int64)
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(pptr))
    k1 = (rec[:, 1] >> 8) & 0xFF
    kind = rec[:, 0] >> 30
    quant = (kind == KIND_PACKED) | (kind == KIND_DIRECT16)
    return {"v": col, "kind": kind, "paths": rec[:, 0] & 0x3FFFFFFF, "lo": rec[:, 3], "hi": np.minimum(b[k1], col),
            "d": np.where(quant, (rec[:, 1] >> 16) & 0xFF, 0), "edges": (rec[:, 2] >> 16) - (rec[:, 2] & 0xFFFF)}


def _is_edge(A, v, u):
    """A[v, u] != 0 for arrays of positions (the CSR entries are sorted: one search over row * n + column)."""
    n = A.shape[0]
    ekey = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * n + A.indices
    k = v * n + u
    at = np.minimum(np.searchsorted(ekey, k), len(ekey) - 1)
    return ekey[at] == k


def _host_survivors(A, fx, pieces, thr_units, scale, cols=None):
    """(keys v << 32 | u ascending, float32 reported sums, candidate count) of a launch without heads over the columns ``cols`` (all)
    at a bar of ``thr_units`` table units: per piece the sums of ceil(fx / 2^d) over the common neighbours -- d = the low weight bits
    the piece drops --, kept when they reach max(thr >> d, 1) and reported as sum << d; every reached non-edge u < v is a candidate."""
    import scipy.sparse as ssp
    rows = np.arange(A.shape[0], dtype=np.int64) if cols is None else np.sort(np.asarray(cols, np.int64))
    Asub = A[rows]
    order = np.lexsort((pieces["hi"], pieces["v"]))
    pkey = pieces["v"][order] * (1 << 32) + pieces["hi"][order]
    keys, vals, n_cand = [], [], None
    for d in np.unique(pieces["d"]):
        q = (fx + (1 << d) - 1) >> d
        S = (Asub @ ssp.diags(q.astype(np.float64)) @ A).tocoo()
        v, u, s = rows[S.row], S.col.astype(np.int64), np.rint(S.data).astype(np.int64)
        m = u < v
        v, u, s = v[m], u[m], s[m]
        m = ~_is_edge(A, v, u)
        v, u, s = v[m], u[m], s[m]
        if n_cand is None:
            n_cand = len(v)
        at = np.searchsorted(pkey, v * (1 << 32) + u, side="right")   # the column's first piece that ends above u
        assert (at < len(pkey)).all() and (pkey[at] >> 32 == v).all(), "a reached candidate lies in no piece of its column"
        pc = order[at]
        assert (pieces["lo"][pc] <= u).all()
        keep = (pieces["d"][pc] == d) & (s >= max(thr_units >> d, 1))
        keys.append(v[keep] * (1 << 32) + u[keep])
        vals.append((s[keep] << d).astype(np.float32) * np.float32(scale))
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    o = np.argsort(keys)
    return keys[o], vals[o], n_cand


def _as_dict(keys, vals):
    return {(int(k & 0xFFFFFFFF), int(k >> 32)): float(x) for k, x in zip(keys, vals)}


# A bar of T table units is handed to the launch as the float T x 2^-shift.  The kernel keeps a sum that reaches the smallest
# fixed-point value whose float32 EXCEEDS the bar, floored to table units: that is T itself as long as half an ulp of the float
# stays below one unit, i.e. T < 2^24 (float32's 24-bit mantissa).
BAR_UNITS_MAX = 1 << 24


def _launch(eps, g, sc, plan, thr, variant, heads=None, wpaths=None, ssum=True, cols=None):
    from eps_amd import scan
    bounds, cuts = scan.screen_tables(g)
    res = eps.ops.Survivors(scan._capacity(2 * scan.total_half_paths(g), scan._PIECE_SLACK), thr, g.device, prefill=False)
    status = torch.zeros(1, dtype=torch.int32, device=g.device)
    columns = scan.column_order(g) if cols is None else cols
    eps.ops.scan_screen(g.rowptr, g.col, scan.reverse_positions(g), sc.fx32, cuts, bounds, g.n_rows, columns, sc.shift, res,
                        status, variant, wpaths=scan.window_paths(g) if wpaths is None else wpaths, ssum=sc.ssum if ssum else None,
                        smax=sc.smax if ssum else None, plan=plan, heads=heads)
    return res, int(status)


def _reported(res):
    """(keys v << 32 | u ascending, reported float32 sums, the launch's candidate count)"""
    slots, n_cand = res.counts()
    assert slots <= res.capacity
    keys, vals = res.valid(slots)
    keys, vals = keys.cpu().numpy(), vals.cpu().numpy()
    assert len(np.unique(keys)) == len(keys), "a candidate was reported twice"
    o = np.argsort(keys)
    return keys[o], vals[o], n_cand


def _plan(eps, g, sc, variant, ssum=True, heads=None, wpaths=None):
    from eps_amd import scan
    bounds, cuts = scan.screen_tables(g)
    return eps.ops.scan_plan(g.rowptr, cuts, scan.window_paths(g) if wpaths is None else wpaths, sc.ssum if ssum else None,
                             sc.smax if ssum else None, bounds, g.n_rows, sc.shift, variant, heads=heads)


def _block_and_tail_graph():
    """A dense block of 512 hub ids that holds nearly all stored entries -- so the LAST id window spans the whole sparse tail, wider
    than any direct piece -- and a column (the last id) whose 300 hub neighbours reach 3000 tail ids: more paths in one window than
    a hash piece holds, i.e. hash-partitioned passes when the plan has no sum bounds."""
    rng = np.random.default_rng(5)
    n, nb = 20000, 512
    r, c = np.triu_indices(nb, 1)
    keep = rng.random(len(r)) < 0.9
    rows, cols = [r[keep]], [c[keep]]
    hubs = np.arange(300)
    rows.append(np.repeat(hubs, 10))
    cols.append(rng.integers(600, n - 1, 3000))
    rows.append(hubs)
    cols.append(np.full(300, n - 1))
    return _sym(n, np.concatenate(rows), np.concatenate(cols))


@pytest.fixture(scope="module")
def rmat16(eps, dev):
    """(graph under hubs-first labels, its adjacency on the host, the number of unordered two-hop non-edges)"""
    from eps_amd import synth
    g0 = synth.rmat_graph(16, 8, 11, dev)
    g = g0.degree_ordered()[0]
    A = g.to_scipy()
    A.data[:] = 1.0
    return g, A, _two_hop_non_edges(A)


def test_counts_are_exact_for_every_piece_kind(eps, dev, rmat16):
    from eps_amd import scan
    g, A, want = rmat16
    sc = scan.screen_weights(g, g, None, _weights(eps, g))
    assert sc.usable and sc.ssum is not None
    variant = scan.screen_variant(g)
    bounds, _ = scan.screen_tables(g)
    inf = float("inf")
    # with sum bounds: 32-bit direct, 16-bit direct and packed pieces
    plan = _plan(eps, g, sc, variant)
    kinds = _plan_records(plan, bounds, g.n_rows)["kind"]
    assert {KIND_DIRECT32, KIND_DIRECT16, KIND_PACKED} <= set(kinds.tolist()), np.bincount(kinds, minlength=4)
    res, st = _launch(eps, g, sc, plan, inf, variant)
    got, _, n_cand = _reported(res)
    assert st == 0 and not len(got) and n_cand == want
    # without: two-word hash pieces next to the 32-bit direct ones; the launch that plans itself counts the same
    plan = _plan(eps, g, sc, variant, ssum=False)
    kinds = _plan_records(plan, bounds, g.n_rows)["kind"]
    assert {KIND_DIRECT32, KIND_HASH} <= set(kinds.tolist()) and KIND_PACKED not in kinds and KIND_DIRECT16 not in kinds
    for pl in (plan, None):
        res, st = _launch(eps, g, sc, pl, inf, variant, ssum=False)
        got, _, n_cand = _reported(res)
        assert st == 0 and not len(got) and n_cand == want


def test_counts_are_exact_in_partitioned_windows_and_with_stored_values(eps, dev):
    import scipy.sparse as ssp
    from eps_amd import scan, synth
    A = _block_and_tail_graph()
    g = eps.CSRGraph.from_scipy(A, device=dev, keep_values=False)
    sc = scan.screen_weights(g, g, None, _weights(eps, g))
    variant = scan.screen_variant(g)
    bounds, _ = scan.screen_tables(g)
    plan = _plan(eps, g, sc, variant, ssum=False)
    pr = _plan_records(plan, bounds, g.n_rows)
    piece_paths = (1 << {0: 13, 1: 14, 2: 12}[variant & 0xFF]) // 2
    parted = (pr["kind"] == KIND_HASH) & (pr["paths"] + pr["edges"] > piece_paths)
    assert parted.any(), "no hash-partitioned window in this plan"
    want = _two_hop_non_edges(A)
    res, st = _launch(eps, g, sc, plan, float("inf"), variant, ssum=False)
    got, _, n_cand = _reported(res)
    assert st == 0 and not len(got) and n_cand == want
    # stored values: the weighted flavour of the kernel (32-bit direct and two-word hash pieces, planned inside the launch)
    ei = synth.rmat_edges(13, 10 << 13, 8, dev)
    ei = ei[:, ei[0] != ei[1]]
    val = torch.randint(1, 6, (ei.shape[1],), generator=torch.Generator(device=dev).manual_seed(2), device=dev).to(torch.float32)
    gw = eps.CSRGraph.from_edge_index(ei, val, sparse_sizes=(1 << 13, 1 << 13)).to_symmetric().degree_ordered()[0]
    assert gw.val is not None
    Aw = gw.to_scipy()
    Aw = ssp.csr_matrix((np.ones_like(Aw.data), Aw.indices, Aw.indptr), shape=Aw.shape)
    scw = scan.screen_weights(gw, gw, None, _weights(eps, gw))
    assert scw.usable and scw.val is not None
    bw, cw = scan.screen_tables(gw)
    res = eps.ops.Survivors(scan._capacity(2 * scan.total_half_paths(gw), scan._PIECE_SLACK), float("inf"), dev, prefill=False)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    eps.ops.scan_screen(gw.rowptr, gw.col, scan.reverse_positions(gw), scw.fx32, cw, bw, gw.n_rows, scan.column_order(gw), scw.shift, res,
                        status, scan.screen_variant(gw), scw.val, scw.node_w, wpaths=scan.window_paths(gw))
    got, _, n_cand = _reported(res)
    assert int(status) == 0 and not len(got) and n_cand == _two_hop_non_edges(Aw)


def test_count_with_skipped_heads_is_the_walked_rows_count(eps, dev, rmat16):
    """With heads (and no sketch pieces) a column v walks N(v)[heads[v].x:] only: the launch counts the ids below v those rows
    reach, minus v's neighbours, over the columns that are neither dead (row sum below the bar) nor void."""
    import scipy.sparse as ssp
    from eps_amd import scan
    g, A, _ = rmat16
    sc = scan.screen_weights(g, g, None, _weights(eps, g))
    variant = scan.screen_variant(g)
    bounds, cuts = scan.screen_tables(g)
    fx = sc.fx32.cpu().numpy().view(np.uint32).astype(np.int64)
    thr_units = int(fx.max()) * 6                          # (a bar of six of the heaviest weights)
    assert thr_units < BAR_UNITS_MAX
    bar = float(np.float32(thr_units) * np.float32(2.0 ** -sc.shift))
    hub = min(4096, g.n_rows)
    heads = eps.ops.scan_heads(g.rowptr, g.col, sc.fx32, hub, thr_units // 2)
    wp = eps.ops.scan_window_paths(g.rowptr, g.col, scan.reverse_positions(g), cuts, heads)
    plan = _plan(eps, g, sc, variant, heads=heads, wpaths=wp)
    res, st = _launch(eps, g, sc, plan, bar, variant, heads=heads, wpaths=wp)
    assert st == 0
    _, n_cand = res.counts()
    hd = heads.cpu().numpy().view(np.uint32).astype(np.int64)
    ssum = sc.ssum.cpu().numpy().view(np.uint32).astype(np.int64)
    assert hd[:, 0].max() > 0, "no head was skipped"
    live = (ssum >= thr_units) & (hd[:, 1] < thr_units)
    assert 0 < live.sum() < g.n_rows, "the bar kills no column or all of them"
    rp = A.indptr
    pos = np.arange(A.nnz) - np.repeat(rp[:-1], np.diff(rp))
    row = np.repeat(np.arange(g.n_rows), np.diff(rp))
    keep = (pos >= hd[row, 0]) & live[row]
    B = ssp.csr_matrix((np.ones(int(keep.sum())), (row[keep], A.indices[keep])), shape=A.shape)
    P = (B @ A).tocoo()
    m = P.col < P.row
    v, u = P.row[m], P.col[m]
    want = int((~_is_edge(A, v.astype(np.int64), u.astype(np.int64))).sum())
    assert n_cand == want


def _sweep_graph(n, seed, deg):
    """Random sparse graph + a path i -- i + 1 (the LAST table field of a column holds a known edge) + node 0 tied to every 16th node
    (candidates in the FIRST field) + OPEN columns, every v = 3 mod 7: no edge v - 1 -- v, and five common neighbours of v - 1 and v,
    so the last field of their table -- every span residue mod 4, even and odd -- is a survivor + three hand-made corners at the top ids:
      a = n - 1: one neighbour b whose other neighbours are ids 3, 5, 9 -- all candidates of the column in the first wave's share;
      t = n - 3: a triangle t, t - 1 (path), x with x -- t - 1: every path of that column ends on a known edge or above it."""
    rng = np.random.default_rng(seed)
    m = n * deg // 2
    r, c = rng.integers(0, n - 8, m), rng.integers(0, n - 8, m)
    opened = np.arange(45, n - 8, 7)                                 # (45 = 3 mod 7)
    is_open = np.zeros(n, bool)
    is_open[opened] = True
    keep = ~((np.abs(r - c) == 1) & is_open[np.maximum(r, c)])      # (no chance edge v - 1 -- v either)
    rows, cols = [r[keep]], [c[keep]]
    path = np.arange(n - 9)
    path = path[~is_open[path + 1]]
    rows.append(path)
    cols.append(path + 1)
    for j in range(5):                                               # (common neighbours below both, off the ids tied to node 0)
        w = rng.integers(1, opened - 3)
        w = np.where(w % 16 == 0, w + 1, w)
        rows += [w, w]
        cols += [opened, opened - 1]
    rows.append(np.zeros(len(range(16, n - 8, 16)), np.int64))
    cols.append(np.arange(16, n - 8, 16))
    a, b = n - 1, n - 2
    rows.append(np.array([a, b, b, b]))
    cols.append(np.array([b, 3, 5, 9]))
    t, x = n - 3, n - 5
    rows.append(np.array([t, t, x]))
    cols.append(np.array([n - 4, x, n - 4]))
    return _sym(n, np.concatenate(rows), np.concatenate(cols))


@pytest.mark.parametrize("n, kind", [(4099, KIND_DIRECT32), (12003, KIND_DIRECT16)])
def test_sweep_edges_against_host_sums(eps, dev, n, kind):
    """Every column of a small graph is ONE direct piece [0, v) -- 32-bit below 2 x the table's slots, 16-bit fields above -- so the
    spans run through every residue; the launch's survivors and reported sums at a bar are the host's, as is its count; the bar is
    moved onto a reported sum (it stays) and one unit above (it goes)."""
    from eps_amd import scan
    A = _sweep_graph(n, n, 10)
    g = eps.CSRGraph.from_scipy(A, device=dev, keep_values=False)
    sc = scan.screen_weights(g, g, None, _weights(eps, g))
    assert sc.usable and sc.ssum is not None
    variant = scan.screen_variant(g)
    assert variant & 0xFF == 2                                   # (4096 slots: 32-bit direct pieces span <= 8192 ids)
    bounds, _ = scan.screen_tables(g)
    plan = _plan(eps, g, sc, variant)
    pr = _plan_records(plan, bounds, g.n_rows)
    whole = (pr["kind"] == kind) & (pr["lo"] == 0) & (pr["hi"] == pr["v"])
    spans = pr["hi"][whole]
    assert {int(s) & 3 for s in spans} == {0, 1, 2, 3} and len(spans) > n // 4, np.bincount(pr["kind"], minlength=4)
    for corner in (n - 1, n - 3):
        assert whole[pr["v"] == corner].all() and (pr["v"] == corner).sum() == 1
    fx = sc.fx32.cpu().numpy().view(np.uint32).astype(np.int64)
    scale = 2.0 ** -sc.shift
    thr_units = int(np.sort(fx)[len(fx) // 2]) * 2               # (two median weights: a few per cent of the candidates pass)
    assert thr_units < BAR_UNITS_MAX
    want_k, want_v, want_cand = _host_survivors(A, fx, pr, thr_units, scale)
    res, st = _launch(eps, g, sc, plan, float(np.float32(thr_units) * np.float32(scale)), variant)
    got_k, got_v, n_cand = _reported(res)
    assert st == 0 and n_cand == want_cand == _two_hop_non_edges(A)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v)
    want = _as_dict(want_k, want_v)
    every = _as_dict(*_host_survivors(A, fx, pr, 1, scale)[:2])    # (a bar of one unit: every candidate)
    # what the truth holds: survivors in a table's last and first field, next to a flagged known edge in the same word, the corners
    one_piece = set(pr["v"][whole].tolist())
    last = [(u, v) for (u, v) in want if u == v - 2 and v in one_piece and A[v, v - 1]]  # (v - 1 is the path's known edge: the last field)
    assert last and any((v - 2) // (4 if kind == KIND_DIRECT32 else 2) == (v - 1) // (4 if kind == KIND_DIRECT32 else 2) for _, v in last)
    assert any(u == 0 for u, _ in want)
    # ... and a survivor IN the last field, id v - 1 = span - 1, with the host's sum (got == want above): the open columns, whose spans
    # run through every residue mod 4 -- even spans end on the high half of a 16-bit word, odd ones on the low half
    tail = [v for (u, v) in want if u == v - 1 and v in one_piece]
    assert {v & 3 for v in tail} == {0, 1, 2, 3} and len(tail) > n // 40, len(tail)
    assert not any(A[v, v - 1] for v in tail)
    assert A[n - 1, n - 2] and [3, 5, 9] == sorted(u for (u, v) in every if v == n - 1)      # (one wave's share of the table)
    assert not [1 for (u, v) in every if v == n - 3]                                           # (a piece without a candidate)
    # the bar on a reported sum, and one unit above it
    d_of = {int(v): int(d) for v, d in zip(pr["v"], pr["d"])}         # (one piece per column here)
    fits = {k: x for k, x in want.items() if int(round(x / scale)) + (1 << d_of[k[1]]) < BAR_UNITS_MAX}
    (u0, v0), s0 = max(fits.items(), key=lambda kv: kv[1])          # (the largest reported sum that a float32 bar can sit on)
    d0 = d_of[v0]
    at = int(round(s0 / scale))
    assert at % (1 << d0) == 0 and at > thr_units
    for units, stays in ((at, True), (at + (1 << d0), False)):
        res, st = _launch(eps, g, sc, plan, float(np.float32(units) * np.float32(scale)), variant)
        got_k, got_v, n_cand = _reported(res)
        assert st == 0 and n_cand == want_cand and ((v0 << 32 | u0) in got_k.tolist()) == stays
        hk, hv, _ = _host_survivors(A, fx, pr, units, scale)
        assert np.array_equal(got_k, hk) and np.array_equal(got_v, hv)


def test_sweeps_of_all_piece_kinds_against_host_sums(eps, dev, rmat16):
    """The same comparison on the R-MAT graph under hubs-first labels, whose plan mixes 32-bit direct, 16-bit direct and packed
    pieces (and, without sum bounds, two-word hash pieces): survivors and sums piece by piece."""
    from eps_amd import scan
    g, A, n2 = rmat16
    sc = scan.screen_weights(g, g, None, _weights(eps, g))
    variant = scan.screen_variant(g)
    bounds, _ = scan.screen_tables(g)
    fx = sc.fx32.cpu().numpy().view(np.uint32).astype(np.int64)
    scale = 2.0 ** -sc.shift
    thr_units = int(fx.max()) * 3
    assert thr_units < BAR_UNITS_MAX
    cols = scan.column_order(g)[::16].contiguous()              # (every 16th column of the heaviest-first order: the host's share of the work)
    for with_sums in (True, False):
        plan = _plan(eps, g, sc, variant, ssum=with_sums)
        pr = _plan_records(plan, bounds, g.n_rows)
        mine = np.isin(pr["v"], cols.cpu().numpy())
        kinds = {KIND_DIRECT32, KIND_DIRECT16, KIND_PACKED} if with_sums else {KIND_DIRECT32, KIND_HASH}
        assert kinds <= set(pr["kind"][mine].tolist())
        want_k, want_v, want_cand = _host_survivors(A, fx, pr, thr_units, scale, cols.cpu().numpy())
        res, st = _launch(eps, g, sc, plan, float(np.float32(thr_units) * np.float32(scale)), variant, ssum=with_sums, cols=cols)
        got_k, got_v, n_cand = _reported(res)
        assert st == 0 and n_cand == want_cand and len(want_k) > 1000
        assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v)


def _exact(g, sc, res, bar):
    from eps_amd import scan
    slots, _ = res.counts()
    assert slots <= res.capacity
    keys, _ = res.valid(slots)
    assert torch.unique(keys).numel() == keys.numel(), "a candidate was reported twice"
    k2, v2 = scan.rescore_exact(g, sc, keys, torch.tensor([bar], device=g.device))
    m = k2 >= 0
    o = torch.argsort(k2[m])
    return k2[m][o], v2[m][o]


def _piece_bits(pr, deg, table_bits, live):
    """Table bits of the plan's packed pieces of single-round columns -- the pieces a sketch launch runs as sketch pieces where the
    column is live -- by the kernel's sizing rule RESTATED here (the smallest table with load <= 1/2, between 10 bits and table bits
    + 1): a statement about the plan the launch was given and the columns it does not leave out (``live``), not a read-out of
    what the launch did."""
    m = (pr["kind"] == KIND_PACKED) & (deg[pr["v"]] <= 256) & live[pr["v"]]
    keys = np.maximum(pr["paths"][m] + pr["edges"][m], 2)
    want = np.ceil(np.log2(keys)).astype(np.int64) + 1
    return np.clip(want, 10, table_bits + 1)


@pytest.mark.parametrize("space", ["dense", "sparse"])
def test_sketch_indices_stay_inside_the_table(eps, dev, space):
    """Sketch launches against hashed launches with ids on both sides of 2^16 (``dense``: R-MAT 17 under hubs-first labels; its
    sketch pieces take the smallest tables, 10 bits) and with bits above 2^20 set (``sparse``: a small graph relabelled
    i -> 512 i + 7, whose sketch pieces reach the largest table, table bits + 1).  A slot index outside its half table
    would land in the other half, the row descriptors or the unit bitmap behind them: the refined, exactly re-scored lists are
    equal at bars of which at least two run sketch pieces.  The table sizes are read off the plan by the kernel's sizing rule
    restated here (``_piece_bits``), over the columns the launch does not leave out."""
    from eps_amd import scan, synth
    if space == "dense":
        g = synth.rmat_graph(17, 10, 3, dev).degree_ordered()[0]
    else:
        A0 = synth.rmat_graph(12, 12, 9, dev).degree_ordered()[0].to_scipy().tocoo()
        g = eps.CSRGraph.from_scipy(_sym(4096 * 512, A0.row.astype(np.int64) * 512 + 7, A0.col.astype(np.int64) * 512 + 7), device=dev,
                                    keep_values=False)
        assert int(g.col.max()) >= 1 << 20
    w = _weights(eps, g)
    sc = scan.screen_weights(g, g, None, w)
    assert sc.usable and sc.ssum is not None
    variant = scan.screen_variant(g)
    bounds, cuts = scan.screen_tables(g)
    hub = eps.ops.scan_hub_rows(g.rowptr, g.col, min(4096, g.n_rows))
    deg = g.degree().cpu().numpy()
    fx = sc.fx32.cpu().numpy().view(np.uint32).astype(np.int64)
    table_bits = {0: 13, 1: 14, 2: 12}[variant & 0xFF]
    seen_bits, compared = set(), []
    for paths_at_bar in (8.0, 5.0, 3.0):                      # (bars of eight, five and three of the heaviest weights)
        units = int(fx.max() * paths_at_bar)
        bar = units * 2.0 ** -sc.shift
        heads = eps.ops.scan_heads(g.rowptr, g.col, sc.fx32, hub.shape[0], units // 2)
        wp = eps.ops.scan_window_paths(g.rowptr, g.col, scan.reverse_positions(g), cuts, heads)
        lists = []
        # (the hashed launch reads the plain plan; the sketch launch the plan whose packed pieces of single-round columns hold up to
        #  2^(table bits + 1) paths, as the filter step's main launch does: its sketch pieces take every table size)
        for word in (variant, variant | eps.ops.SCAN_SKETCH | eps.ops.SCAN_WIDE):
            plan = _plan(eps, g, sc, variant | (word & eps.ops.SCAN_WIDE), heads=heads, wpaths=wp)
            walked, st = _launch(eps, g, sc, plan, bar, word, heads=heads, wpaths=wp)
            if word & eps.ops.SCAN_SKETCH and st & 8:         # (a piece had more ids to report than its set holds: the launch is void)
                continue
            assert st & ~16 == 0 and (word & eps.ops.SCAN_SKETCH or not st & 16), (hex(word), st)
            res = eps.ops.Survivors(walked.capacity, bar, dev, prefill=False)
            eps.ops.scan_refine(walked, heads, hub, sc.fx32, g.rowptr, g.col, g.n_rows, sc.shift, res)
            lists.append(_exact(g, sc, res, bar))
            if st & 16:
                compared.append(paths_at_bar)
                # (a column runs unless its row sum lies below the bar or its head weighs as much as the bar)
                hd = heads.cpu().numpy().view(np.uint32).astype(np.int64)
                live = (sc.ssum.cpu().numpy().view(np.uint32).astype(np.int64) >= units) & (hd[:, 1] < units)
                seen_bits |= set(_piece_bits(_plan_records(plan, bounds, g.n_rows), deg, table_bits, live).tolist())
        assert lists[0][0].numel() > 100
        for got in lists[1:]:
            assert torch.equal(got[0], lists[0][0]) and torch.equal(got[1], lists[0][1]), (space, paths_at_bar)
    assert len(compared) >= 2, "sketch pieces ran (and were not voided) at fewer than two bars"
    # (the small graph spread over a wide id space is where pieces fill up: the sketch pieces of its live columns reach the largest
    #  table, 2^(table bits + 1) words; the R-MAT graph's stay at the small end, 2^10, and bring the ids around 2^16)
    assert (table_bits + 1 if space == "sparse" else 10) in seen_bits, seen_bits
    assert space == "sparse" or (g.n_rows > 1 << 16 and int(g.degree()[1 << 16:].sum()) > 0)
