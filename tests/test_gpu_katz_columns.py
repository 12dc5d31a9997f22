"""GPU: the Katz column kernel (csrc/katz_columns.hip) against the float64 truth of the pair kernel's tests
(test_katz_host.truncated_truth), to one float32 ulp: golden graphs with every column's full 2-hop list plus a stored edge, the
diagonal and an unreachable node; an asymmetric weighted matrix; hubs beyond the LDS table and the work-unit size; bitwise
equality across launches and across any split into blocks; the edge cases.  No existing kernel serves as an oracle here."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

from conftest import golden_pair_files
from test_gpu_katz import assert_within_one_ulp, directed_weighted, hub_graph
from test_katz_host import truncated_truth

pytestmark = pytest.mark.gpu

COEFFS = (0.05, 0.005, 0.000125)


def device_graph(eps, A, unit=False):
    """The SciPy matrix on the device; ``unit``: without stored values (the kernel's integer-count table build)."""
    return eps.CSRGraph.from_scipy(ssp.csr_matrix(A, dtype=np.float32), device="cuda:0", keep_values=not unit)


def column_scores(g, v_lo, v_hi, u, v, device_out=False):
    """Scores of the column-major list (u, v) (v ascending, all in [v_lo, v_hi)) -> float32 numpy."""
    from eps_amd import heuristics
    assert np.all(v[1:] >= v[:-1]) and (len(v) == 0 or (v[0] >= v_lo and v[-1] < v_hi))
    colptr = np.searchsorted(v, np.arange(v_lo, v_hi + 1)).astype(np.int64)
    out = heuristics.truncated_katz_columns(g, v_lo, v_hi, torch.from_numpy(colptr), torch.from_numpy(u.astype(np.int32)),
                                            beta=0.05, iterations=2, device_out=device_out)
    return out if device_out else out.numpy()


def two_hop_lists(A, cols):
    """(u, v) of the 2-hop non-edges (A^2)[u,v] != 0, u != v, A[u,v] == 0 of the columns ``cols`` (ascending), column-major;
    and the number of nodes in each column's two-hop in-support."""
    cols = np.asarray(cols)
    Ac = A.tocsc()
    A2 = (A.tocsr() @ Ac[:, cols]).tocsc()
    A2.eliminate_zeros()
    A2.sort_indices()
    us, vs, support = [], [], []
    for j, v in enumerate(cols):
        su = A2.indices[A2.indptr[j]:A2.indptr[j + 1]]
        support.append(len(su))
        known = Ac.indices[Ac.indptr[v]:Ac.indptr[v + 1]]
        cu = su[(su != v) & ~np.isin(su, known)]
        us.append(cu)
        vs.append(np.full(len(cu), v))
    return np.concatenate(us).astype(np.int64), np.concatenate(vs).astype(np.int64), np.array(support)


# ------------------------------------------------------------------------------------------------------- golden graphs
def _golden_case(path):
    """Every column's full 2-hop non-edge list, then one stored edge, the diagonal and one node without a walk of length <= 3
    (where there is one) appended to the column; the truth of all of them.  Dense float64 products: the entries are integers
    far below 2^53 on these graphs, so they are exact and c1*a1 + c2*a2 + c3*a3 is truncated_truth's expression bit for bit
    (checked on a seeded sample below) -- truncated_truth itself takes minutes on the 2.8 M candidates of rmat12."""
    d = np.load(path)
    n = d["rowptr"].size - 1
    A = ssp.csr_matrix((d["val"].astype(np.float64), d["col"], d["rowptr"]), shape=(n, n))
    Ad = A.toarray()
    A2 = Ad @ Ad
    A3 = A2 @ Ad
    cand = (A2 != 0) & (Ad == 0)
    np.fill_diagonal(cand, False)
    cv, cu = np.nonzero(cand.T)                                  # column-major: v ascending, then u
    reach = (Ad != 0) | (A2 != 0) | (A3 != 0)
    xu, xv, n_unreach = [], [], 0
    for v in range(n):
        stored = np.flatnonzero(Ad[:, v])
        far = np.flatnonzero(~reach[:, v])
        far = far[far != v]
        extra = list(stored[:1]) + [v] + list(far[:1])
        n_unreach += len(far[:1])
        xu += extra
        xv += [v] * len(extra)
    u = np.concatenate([cu, np.array(xu, np.int64)])
    v = np.concatenate([cv, np.array(xv, np.int64)])
    order = np.argsort(v, kind="stable")                          # (the extras end their column's list: not sorted by u)
    u, v = u[order], v[order]
    truth = COEFFS[0] * Ad[u, v] + COEFFS[1] * A2[u, v] + COEFFS[2] * A3[u, v]
    sample = np.random.default_rng(17).choice(len(u), min(len(u), 2000), replace=False)
    assert np.array_equal(truth[sample], truncated_truth(A, np.stack([u[sample], v[sample]], 1), COEFFS))
    unreachable = ~reach[u, v] & (u != v)
    return A, u, v, truth, unreachable, n_unreach


@pytest.mark.parametrize("path", golden_pair_files(), ids=lambda p: os.path.basename(p)[6:-4])
def test_kernel_matches_fp64_on_golden_graphs(eps, dev, path):
    A, u, v, truth, unreachable, n_unreach = _golden_case(path)
    n = A.shape[0]
    name = os.path.basename(path)
    got = column_scores(device_graph(eps, A), 0, n, u, v)
    assert_within_one_ulp(got, truth, name)
    assert unreachable.sum() >= n_unreach and np.all(got[unreachable] == 0.0) and np.all(truth[unreachable] == 0.0)
    if np.all(A.data == 1.0):        # the same graph without stored values: counted, not summed -- and not a bit different
        assert column_scores(device_graph(eps, A, unit=True), 0, n, u, v).tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------------- asymmetric graph
def test_kernel_on_a_directed_weighted_matrix(eps, dev):
    """A is not symmetric: (u, v) and (v, u) are both listed and must come out as A's, not A^T's (a side swap shows here)."""
    A = directed_weighted()
    n = A.shape[0]
    assert n == 400 and (A != A.T).nnz > 0
    rng = np.random.default_rng(1)
    coo = A.tocoo()
    stored = np.stack([coo.row, coo.col], 1)[:300]
    rand = rng.integers(0, n, (3000, 2))
    pairs = np.concatenate([stored, stored[:, ::-1], rand, rand[:, ::-1], np.stack([np.arange(n), np.arange(n)], 1)])
    pairs = pairs[np.argsort(pairs[:, 1], kind="stable")]
    truth = truncated_truth(A, pairs, COEFFS)
    assert_within_one_ulp(column_scores(device_graph(eps, A), 0, n, pairs[:, 0], pairs[:, 1]), truth, "directed")
    assert not np.allclose(truth, truncated_truth(A.T, pairs, COEFFS))         # the transpose would be a different answer


# ---------------------------------------------------------------------------------------------------------------- hubs
@functools.lru_cache(maxsize=None)
def _hub_case(weighted):
    """hub_graph, columns 0 and 1 and 200 seeded others with their full 2-hop lists, and the truth (computed once, read only)."""
    A = hub_graph(weighted)
    n = A.shape[0]
    others = np.random.default_rng(3).choice(np.arange(2, n), 200, replace=False)
    cols = np.concatenate([[0, 1], np.sort(others)])
    u, v, support = two_hop_lists(A, cols)
    return A, cols, u, v, support, truncated_truth(A, np.stack([u, v], 1), COEFFS)


@pytest.mark.parametrize("weighted", [False, True])
def test_kernel_on_hubs_beyond_the_lds_table_and_one_chunk(eps, dev, weighted):
    """Column 0's two-hop in-support does not fit the LDS table (the table in the workspace ran) and its candidates are more
    than one work unit (the split ran); hub_graph's n = 6000 reaches both limits as they are."""
    A, cols, u, v, support, truth = _hub_case(weighted)
    assert A.shape[0] == 6000
    cap, chunk = eps.ops.katz_columns_limits()
    assert support[0] > cap, (support[0], cap)
    assert int((v == 0).sum()) > chunk, (int((v == 0).sum()), chunk)
    got = column_scores(device_graph(eps, A, unit=not weighted), 0, A.shape[0], u, v)
    assert_within_one_ulp(got, truth, "hubs")
    assert np.all(got > 0)


# ----------------------------------------------------------------------------------------------------- reproducibility
def test_scores_do_not_depend_on_the_launch_or_the_blocks(eps, dev):
    """Two launches are bitwise equal; so are one block, two blocks cut at a seeded column, and one block per column."""
    A, cols, u, v, _, truth = _hub_case(True)
    n = A.shape[0]
    g = device_graph(eps, A)
    one = column_scores(g, 0, n, u, v)
    assert_within_one_ulp(one, truth, "hubs")
    assert column_scores(g, 0, n, u, v).tobytes() == one.tobytes()
    cut = int(np.random.default_rng(23).integers(2, n - 1))
    lo = v < cut
    assert lo.any() and (~lo).any()
    two = np.concatenate([column_scores(g, 0, cut, u[lo], v[lo]), column_scores(g, cut, n, u[~lo], v[~lo])])
    assert two.tobytes() == one.tobytes()
    # another work-unit size splits other columns, at other places: 100 (every column here has more), 1000, one unit for all
    from eps_amd import heuristics
    gt, _, p_in = heuristics._katz_transpose(g)
    colptr = torch.from_numpy(np.searchsorted(v, np.arange(0, n + 1)).astype(np.int64)).cuda()
    cand_u = torch.from_numpy(u.astype(np.int32)).cuda()
    for chunk in (100, 1000, 1 << 20):
        got = eps.ops.katz_column_scores(g.rowptr, g.col, g.val, gt.rowptr, gt.col, gt.val, p_in, n, 0, n, colptr, cand_u, COEFFS,
                                         chunk=chunk)
        assert got.cpu().numpy().tobytes() == one.tobytes(), chunk
    # one block per column moves every column's place in the work units
    each = torch.cat([column_scores(g, int(c), int(c) + 1, u[v == c], v[v == c], device_out=True) for c in cols]).cpu().numpy()
    assert each.tobytes() == one.tobytes()


# ---------------------------------------------------------------------------------------------------------- edge cases
def test_kernel_edge_cases(eps, dev):
    """Isolated nodes, u == v, pairs with no walk of length <= 3 (exactly 0.0), columns without candidates, an empty list."""
    # a path 0-1-2-3-4-5-6, a triangle 7-8-9, isolated 10, 11 (the graph of test_gpu_katz.test_kernel_edge_cases)
    e = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (7, 8), (8, 9), (7, 9)]
    r, c = zip(*e)
    A = ssp.coo_matrix((np.ones(len(e)), (r, c)), shape=(12, 12)).tocsr()
    A = (A + A.T).tocsr()
    pairs = np.array([[10, 11], [10, 10], [0, 10], [0, 4], [0, 6], [0, 7], [0, 3], [0, 0], [7, 7], [2, 2], [8, 9], [3, 0]])
    order = np.argsort(pairs[:, 1], kind="stable")
    truth = truncated_truth(A, pairs, COEFFS)
    for unit in (False, True):
        g = device_graph(eps, A, unit=unit)
        got = np.empty(len(pairs), np.float32)
        got[order] = column_scores(g, 0, 12, pairs[order, 0], pairs[order, 1])
        assert_within_one_ulp(got, truth, "edge cases")
        assert np.all(got[:6] == 0.0) and np.all(got[6:] > 0)
        # every node against every column, the isolated ones included
        uu, vv = np.tile(np.arange(12), 12), np.repeat(np.arange(12), 12)
        full = column_scores(g, 0, 12, uu, vv)
        assert_within_one_ulp(full, truncated_truth(A, np.stack([uu, vv], 1), COEFFS), "all pairs")
        assert np.all(full[vv >= 10] == 0.0) and np.all(full[uu >= 10] == 0.0)
        # a block whose columns all have zero candidates, and an empty candidate array on the whole graph
        none = np.zeros(0, np.int64)
        assert column_scores(g, 3, 9, none, none).shape == (0,)
        assert column_scores(g, 0, 12, none, none).shape == (0,)
        assert column_scores(g, 5, 5, none, none).shape == (0,)
        # columns without candidates between columns that have some
        sparse_cols = np.isin(vv, [1, 8])
        assert column_scores(g, 0, 12, uu[sparse_cols], vv[sparse_cols]).tobytes() == full[sparse_cols].tobytes()
    with pytest.raises(eps.EpsError, match="node ids"):
        column_scores(g, 0, 12, np.array([12]), np.array([3]))
    with pytest.raises(eps.EpsError, match="node ids"):
        column_scores(g, 0, 12, np.array([-1]), np.array([3]))
