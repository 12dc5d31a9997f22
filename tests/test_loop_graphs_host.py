"""The looped graphs of tests/loop_graphs.py, from the oracle alone (no GPU): the conditions that keep the GPU tests of
tests/test_gpu_self_loops.py from passing vacuously -- a loop changes no candidate, it does change the AA / RA order inside the
K the GPU tests ask for, the placements that reach particular code exist, and a looped hub lies among the rows a head skips."""
import numpy as np
import pytest

import loop_graphs as lg

MAIN = ("rmat_loops", "collab_like_loops")


@pytest.mark.parametrize("name", MAIN + lg.STRUCTURED + ("wide_loops",))
def test_graphs_are_symmetric_sorted_and_differ_from_their_twins_by_the_diagonal_alone(name):
    g = lg.graph(name)
    A, T = g.A, g.twin
    assert A.shape == T.shape and A.shape[0] == A.shape[1]
    assert A.has_sorted_indices and (abs(A - A.T)).nnz == 0 and (A.data > 0).all()
    loops = lg.looped_nodes(A)
    assert len(loops) and T.diagonal().sum() == 0 and (abs(lg.without_loops(A) - T)).nnz == 0
    assert A.nnz == T.nnz + len(loops)
    assert g.weighted == bool((A.data != 1).any())
    if name in MAIN + ("wide_loops",):
        n = A.shape[0]
        assert 0.3 * n <= len(loops) <= 0.37 * n and loops[0] == 0 and loops[-1] == n - 1


@pytest.mark.parametrize("name", MAIN)
def test_the_loop_placements_exist(name):
    g = lg.graph(name)
    A = g.A
    deg, diag = np.diff(A.indptr), A.diagonal()
    assert len(g.loop_alone) >= 5 and (deg[g.loop_alone] == 1).all() and (diag[g.loop_alone] != 0).all()
    assert len(g.loop_plus_one) >= 5 and (deg[g.loop_plus_one] == 2).all() and (diag[g.loop_plus_one] != 0).all()
    # the three highest-degree nodes -- of the twin AND of the looped graph -- carry a loop
    assert len(g.hubs) == lg.HUBS and (diag[g.hubs] != 0).all()
    assert (diag[lg.hubs_first_order(A)[:lg.HUBS]] != 0).all()
    assert diag[0] != 0 and diag[-1] != 0
    if name == "rmat_loops":
        assert 1900 <= A.shape[0] <= 2100 and (np.sort(deg)[-lg.HUBS:] >= A.shape[0] // 6).all() and (A.data == 1).all()
    else:
        assert A.shape[0] == 512 and set(np.unique(diag[diag != 0])) <= {2.0, 3.0, 4.0, 5.0, 6.0} and len(np.unique(diag)) > 3


@pytest.mark.parametrize("name", MAIN + lg.STRUCTURED)
def test_a_loop_makes_and_removes_no_candidate(oracle, name):
    a, b = lg.truth(oracle, name, "cn"), lg.truth(oracle, name, "cn", twin=True)
    assert np.array_equal(a.pairs, b.pairs)
    assert (a.pairs[:, 0] != a.pairs[:, 1]).all()
    if not lg.graph(name).weighted:
        assert np.array_equal(a.count, b.count) and np.array_equal(a.cn, b.cn)       # (the A @ A counts on the pattern too)
    assert (len(a.pairs) == 0) == (name == "complete")
    if name in MAIN:
        assert len(a.pairs) > 20 * lg.K_INSIDE[name]


def test_a_loop_makes_no_candidate_on_the_wide_graph_either(oracle):
    g = lg.graph("wide_loops")
    n = g.A.shape[0]
    for lo, hi in ((0, 3000), (n // 2 - 1500, n // 2 + 1500), (n - 3000, n)):
        a, b = oracle.candidates_scipy_columns(g.A, lo, hi), oracle.candidates_scipy_columns(g.twin, lo, hi)
        assert len(a[0]) > 1000 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name,kind", [(n, k) for n in MAIN for k in ("aa", "ra")])
def test_a_loop_changes_the_first_k_rows(oracle, name, kind):
    """What 3e of the GPU tests rests on: the truth's first K rows on the looped graph are not the twin's."""
    k = lg.K_INSIDE[name]
    a, b = lg.truth(oracle, name, kind), lg.truth(oracle, name, kind, twin=True)
    rows_a, rows_b = a.pairs[lg.first_rows(a, k)], b.pairs[lg.first_rows(b, k)]
    differ = int((rows_a != rows_b).any(1).sum())
    print(name, kind, "rows that differ among the first", k, ":", differ)
    assert differ >= 1
    assert not np.array_equal(a.weights, b.weights)
    # ... and not through ties alone: the SETS of rows differ, or the scores of the same rows do
    same_set = set(map(tuple, rows_a)) == set(map(tuple, rows_b))
    assert not same_set or not np.array_equal(a.f64[lg.first_rows(a, k)], b.f64[lg.first_rows(b, k)])


@pytest.mark.parametrize("name", MAIN)
def test_a_looped_hub_lies_in_the_head_of_a_column_with_candidates(oracle, name):
    """Hubs-first labels: a column's head is the front of its (sorted) row -- its hub neighbours.  Some column that has candidates
    starts with a looped hub, and some looped HUB column has candidates below itself."""
    g = lg.graph(name)
    A = g.A
    n = A.shape[0]
    order = lg.hubs_first_order(A)
    new = np.empty(n, np.int64)
    new[order] = np.arange(n)
    P = A.tocoo()
    B = lg._csr(lg.ssp.coo_matrix((P.data, (new[P.row], new[P.col])), shape=(n, n)))
    pairs = lg.truth(oracle, name, "cn").pairs
    has_cand = np.zeros(n, bool)
    has_cand[new[pairs[:, 1]][new[pairs[:, 0]] < new[pairs[:, 1]]]] = True     # columns with candidates u < v under the new labels
    diag = B.diagonal() != 0
    assert diag[:lg.HUBS].all()
    firsts = [B.indices[B.indptr[v]:B.indptr[v + 1]][:4] for v in range(n)]
    assert any(has_cand[v] and len(f) and f[0] < lg.HUBS and v >= lg.HUBS for v, f in enumerate(firsts)), "no column starts with a looped hub"
    # (a hub's own loop follows its entries u < v, all of them hubs: it lies in the stretch of ITS row a head may take)
    assert any(has_cand[v] and diag[v] for v in range(lg.HUBS, 64)), "no looped hub column with candidates"


@pytest.mark.parametrize("name", ("two_cliques", "path"))
def test_the_scan_table_truths_hold_on_a_looped_graph(name):
    """tests/scan_table_truth.py against brute-force loops on a graph WITH diagonal entries: the reverse positions (a loop is its
    own mirror), the half paths (v - v - u counts), the cuts and the window paths; and its relabelling keeps the loops."""
    import scan_table_truth as T
    A = lg.graph(name).A
    rp, col = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    n = len(rp) - 1
    rows = [col[rp[v]:rp[v + 1]].tolist() for v in range(n)]
    rev, b, ct = T.revpos(rp, col), T.bounds(rp), None
    ct = T.cuts(rp, col, b)
    wp = T.window_paths(rp, col, b)
    hp = T.half_paths(rp, col)
    for v in range(n):
        want_wp = np.zeros(T.M, np.int64)
        for j, w in enumerate(rows[v]):
            assert rev[rp[v] + j] == rows[w].index(v) == sum(1 for x in rows[w] if x < v)
            for u in rows[w]:
                if u < v:
                    want_wp[np.searchsorted(b, u, side="right") - 1] += 1
        assert np.array_equal(wp[v], want_wp) and hp[v] == want_wp.sum()
        assert np.array_equal(ct[v], [sum(1 for x in rows[v] if x < b[k + 1]) for k in range(T.M)])
    order = lg.hubs_first_order(A)
    new = np.empty(n, np.int64)
    new[order] = np.arange(n)
    rp2, col2 = T.hubs_first(rp, col, keep_loops=True)
    B = A.tocsr()[order][:, order]
    B.sort_indices()
    assert np.array_equal(rp2, B.indptr) and np.array_equal(col2, B.indices)
    assert T.hubs_first(rp, col)[0][-1] == rp[-1] - len(lg.looped_nodes(A))          # (the default still drops them)
