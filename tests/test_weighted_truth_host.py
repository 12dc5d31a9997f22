"""tests/weighted_truth.py (the numpy truth of the stored-value scoring path) against a triple Python loop over numpy.float32
scalars and Python ints, on graphs of at most 12 nodes, for every value family and weight table; the ties of the fixed-point
conversion; and the table of (graph, family, table) cases the GPU tests run: every kept case has what scan.scan_usable asks
for that the host can check, every removed one fails for the reason the helper states."""
import numpy as np
import pytest

import weighted_truth as W


def _small(seed, n, p):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    pick = rng.random(len(iu)) < p
    return n, iu[pick].astype(np.int64), ju[pick].astype(np.int64)


SMALL = {"n12": _small(1, 12, 0.4), "n11_dense": _small(2, 11, 0.7), "n9_sparse": _small(3, 9, 0.25)}


def _dense(g):
    A = np.zeros((g.n, g.n), np.float32)
    A[g.row_index(), g.col] = g.val
    return A


def _brute(A, w, u, v):
    """(int sum of the 2^-40 terms, float64 real sum, common neighbours) of one pair, by the definition."""
    total, real, count = 0, 0.0, 0
    for x in range(len(A)):
        if A[u, x] != 0 and A[v, x] != 0:
            t = np.float32(np.float32(A[u, x] * A[v, x]) * w[x])
            assert type(t) is np.float32
            total += int(round(float(t) * 2.0 ** 40))          # (Python's round: half to even; the scaling by 2^40 is exact)
            real += float(A[u, x]) * float(A[v, x]) * float(w[x])
            count += 1
    return total, real, count


@pytest.mark.parametrize("table", W.TABLES)
@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("name", sorted(SMALL))
def test_exact_scores_match_the_triple_loop(oracle, name, family, table):
    n, lo, hi = SMALL[name]
    g = W.Graph(n, lo, hi, W.draw_values(family, np.random.default_rng([7, W.FAMILIES.index(family)]), n, lo, hi))
    assert g.val.dtype == np.float32 and (g.val > 0).all()
    A = _dense(g)
    assert np.array_equal(A, A.T) and not A.diagonal().any()
    w = W.node_table(oracle, g, table)
    assert w.dtype == np.float32 and (table != "aa_zeroed" or not w[::W.ZERO_EVERY].any())
    if family == "wide":
        w = w * np.float32(2.0 ** -14)        # (a power of two: the same roundings, and sums of values up to 2^22 stay below 2^53 units)
    # the paths: the brute-force set
    pu, pw, pv, eu, ev = W.paths(g.rowptr, g.col)
    want = {(u, x, v) for v in range(n) for u in range(v) if A[u, v] == 0 for x in range(n) if A[u, x] != 0 and A[v, x] != 0}
    assert len(pu) == len(want) and set(zip(pu.tolist(), pw.tolist(), pv.tolist())) == want
    row = g.row_index()
    assert np.array_equal(row[eu], pw) and np.array_equal(row[ev], pw) and np.array_equal(g.col[eu], pu) and np.array_equal(g.col[ev], pv)
    # the scores
    keys, sums, scores, counts = W.exact_scores(g.rowptr, g.col, g.val, w)
    real = W.real_scores(g.rowptr, g.col, g.val, w)
    assert scores.dtype == np.float32 and sums.dtype == np.int64 and (np.diff(keys) > 0).all()
    cand = sorted({(v, u) for (u, _, v) in want})
    assert keys.tolist() == [(v << 32) | u for v, u in cand] and len(cand) > 3
    for i, (v, u) in enumerate(cand):
        total, r, c = _brute(A, w, u, v)
        assert int(sums[i]) == total and int(counts[i]) == c
        assert scores[i] == np.float32(total * 2.0 ** -40)
        assert abs(real[i] - r) <= 1e-14 * abs(r)
    # any pair at all (edges, u == v, no common neighbour), both ways round
    for u in range(n):
        for v in range(n):
            total = _brute(A, w, u, v)[0]
            assert W.pair_exact(g.rowptr, g.col, g.val, w, u, v) == np.float32(total * 2.0 ** -40)
    if family != "ints":
        t64 = g.val[eu].astype(np.float64) * g.val[ev].astype(np.float64)
        assert (t64 != (g.val[eu] * g.val[ev]).astype(np.float64)).mean() > 0.5, "the products of this family do not round"


def test_ties_go_to_even():
    one = np.float32(1.0)
    f = lambda x: int(W.fixed_term(one, np.float32(x), one))
    assert f(2.0 ** -41) == 0 and f(3 * 2.0 ** -41) == 2 and f(5 * 2.0 ** -41) == 2 and f(7 * 2.0 ** -41) == 4
    assert f(2.0 ** -41 * (1 + 2.0 ** -23)) == 1 and f(2.0 ** -41 * (1 - 2.0 ** -24)) == 0 and f(2.0 ** -40) == 1
    assert int(W.fixed_term(np.float32(3.0), np.float32(2.0 ** -41), one)) == 2
    # two multiplies, each rounded: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 before the weight is applied
    a = np.float32(1 + 2.0 ** -12)
    assert int(W.fixed_term(a, a, np.float32(2.0 ** -16))) == round((1 + 2.0 ** -11) * 2.0 ** 24)


@pytest.fixture(scope="module")
def world():
    from eps_amd import synth
    import scan_table_truth as T
    G = W.graphs(synth)
    P = {name: W.paths(G[(name, "ints")].rowptr, G[(name, "ints")].col) for name in W.GRAPHS}
    return G, P, T


def test_the_graphs_are_what_the_gpu_tests_need(world):
    G, P, T = world
    for name in W.GRAPHS:
        g = G[(name, "ints")]
        deg = g.degree()
        for family in W.FAMILIES:
            h = G[(name, family)]
            assert np.array_equal(h.rowptr, g.rowptr) and np.array_equal(h.col, g.col) and h.val.dtype == np.float32 and (h.val > 0).all()
            mirror = h.rowptr[h.col] + T.revpos(h.rowptr, h.col)
            assert np.array_equal(h.val[mirror], h.val) and np.array_equal(h.col[mirror], h.row_index())
        assert (g.col != g.row_index()).all()
        # the one-pass scan takes a graph as it is when no column holds more half paths than its windows of two-word hash pieces
        assert T.half_paths(g.rowptr, g.col).max() <= 2048 * T.M
        if name == "rmat11":
            assert g.n == 1 << 11 and (deg > 64).sum() >= 20 and deg.max() > 512 and (deg == 0).any()
        else:
            assert g.n == 300 and 16 < deg.max() < 64
        # two rows of equal length with a common neighbour, two hub rows: the pairs test_gpu_weighted_values picks exist
        assert len(P[name][0]) > 30000


@pytest.mark.parametrize("name,family,table", [(g, f, t) for g in W.GRAPHS for f in W.FAMILIES for t in W.TABLES])
def test_case_table(oracle, world, name, family, table):
    G, P, _ = world
    g = G[(name, family)]
    w = W.node_table(oracle, g, table)
    bound = W.bound_formula(g, w)
    why = W.REMOVED.get((name, family, table))
    if why == W.NEGATIVE_AA:
        assert (w < 0).any()
        return
    if why == W.BEYOND_RANGE:
        assert bound >= W.FUSED_SCORE_LIMIT
        return
    if why == W.BEYOND_EXACT:
        with pytest.raises(AssertionError):
            W.exact_scores(g.rowptr, g.col, g.val, w, P[name])
        return
    assert why is None and (name, family, table) in W.cases()
    assert (w >= 0).all() and np.isfinite(w).all() and bound * (1 + 2.0 ** -19) < W.FUSED_SCORE_LIMIT
    t = W.Truth(g, w, P[name])                                  # (asserts every sum below 2^53)
    assert len(t.keys) > 20000 and (t.sums >= 0).all() and t.real.max() <= bound
    assert (t.exact64 <= t.real * (1 + 2.0 ** -22) + 2.0 ** -41 * t.counts).all()
    if table == "aa_zeroed":
        assert (t.sums == 0).sum() > 1000
    if family == "big_scores":
        # the best score within a factor of 4 of the bound, the bound beyond 2: the scan's shift is then set by the bound, and
        # the best screening sums use the top three bits of the 31-bit word
        assert bound >= 2.0 and t.real.max() >= bound / 4
