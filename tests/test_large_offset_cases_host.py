"""CPU: the builders of tests/large_offset_cases.py at SMALL marks (4 KiB and 8 KiB) on CPU tensors -- the same code the GPU
tests run at 2^31 and 2^32.  Checked here: the mark rows and entries straddle the marks as promised, for pitches that do and do
not divide them; the built operands hold what the host data says, everywhere; the truths computed from the kept rows alone (on
the compacted twin) equal a dense float64 computation over the whole small case, for every operation the GPU tests hold."""
import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import large_offset_cases as lo
import layer_truth as lt
import pair_score_truth as pt
import weighted_truth as wt

MARKS = (1 << 12, 1 << 13)
U64 = 2.0 ** -53


def _close(got, ref, scale, terms):
    """Two float64 evaluations of the same sums of at most ``terms`` terms: within gamma64(terms + 2) of the sums of absolute terms."""
    bound = pt.gamma64(terms + 2) * np.asarray(scale, np.float64) + 1e-300
    return bool((np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) <= bound).all())


# ---------------------------------------------------------------------------------------------------------- tall tables
@pytest.mark.parametrize("ld,width", [(8, 8), (7, 7), (64, 64), (65, 64), (12, 9)])
def test_tall_rows_straddle_and_table_content(ld, width):
    c = lo.TallCase(MARKS, ld, width, n_extra=60, ballast_rows=37)
    view, buf = c.build("cpu")
    c.check_straddle(view)
    p = c.pitch
    for m in MARKS:
        exact = m % p == 0
        assert exact == (ld in (8, 64))
        b, a = c.roles[("below", m)], c.roles[("at", m)]
        assert ((b + 1) * p == m and a * p == m) if exact else ((b + 1) * p < m and a * p < m < (a + 1) * p)
    # the smallest row count whose last row starts beyond the highest mark + margin
    assert (c.n_rows - 1) * p > max(MARKS) + 160 * p >= (c.n_rows - 2) * p
    # content: ballast by the formula everywhere, the kept rows' values over it, NaN pads
    want = lo.ballast_values(np.arange(c.n_rows) % 37, ld)
    want[:, width:] = np.nan
    want[c.rows, :width] = c.values
    assert np.array_equal(buf.numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(c.values[c.is_ballast], lo.ballast_values(c.rows[c.is_ballast] % 37, width))
    assert len(c.live) > 20 and c.is_ballast.sum() > 5
    assert np.array_equal(c.twin_ids(c.rows), np.arange(len(c.rows))) and np.array_equal(c.offsets(c.rows), c.rows * p)
    assert len(np.intersect1d(c.samples(), c.rows)) == 0
    # the ballast is exact in bfloat16
    assert torch.equal(torch.from_numpy(want[:, :width][~np.isin(np.arange(c.n_rows), c.rows)]).to(torch.bfloat16).float(),
                       torch.from_numpy(want[:, :width][~np.isin(np.arange(c.n_rows), c.rows)]))


def _dense_graph(c, g):
    rowptr, col, val = lo.tall_graph_device(c, g, "cpu")
    return ssp.csr_matrix((val.numpy().astype(np.float64), col.numpy(), rowptr.numpy()), shape=(c.n_rows, c.n_rows))


@pytest.mark.parametrize("ld,width", [(8, 8), (65, 64)])
def test_tall_truths_from_the_kept_rows_equal_dense_float64(ld, width):
    c = lo.TallCase(MARKS, ld, width, n_extra=150, ballast_rows=37)
    view, _ = c.build("cpu")
    x = view.numpy().astype(np.float64)
    g = lo.tall_graph(c)
    B, T = _dense_graph(c, g), lo.tall_graph_twin(c, g)
    assert set(c.mark_rows) <= set(g["rows"]) and set(c.mark_rows) <= set(g["col"]) and set(g["col"]) <= set(c.rows)
    assert sorted(set(np.diff(g["indptr"]))) == sorted(set(min(r, len(c.rows)) for r in lo.ROW_LENGTHS))
    assert np.array_equal(np.diff(T.indptr)[c.twin_ids(g["rows"])], np.diff(g["indptr"])) and T.nnz == B.nnz
    bias = np.random.default_rng(3).standard_normal(width)
    kept = np.isin(np.arange(c.n_rows), c.rows)
    Bd = B.toarray()
    for mean, with_bias, relu in ((False, False, False), (True, False, False), (False, True, True)):
        dense = Bd @ x if not mean else ((Bd != 0) @ x) / np.maximum((Bd != 0).sum(1), 1)[:, None]
        if with_bias:
            dense = dense + bias
        if relu:
            dense = np.maximum(dense, 0)
        twin = lt.spmm(T, c.values, bias if with_bias else None, relu, mean)
        scale = lt.spmm(abs(T), np.abs(c.values), np.abs(bias) if with_bias else None, False, mean)
        assert _close(twin, dense[c.rows], scale, 130)
        rest = dense[~kept]                                                # rows without entries: 0 (+ bias, ReLU)
        assert np.array_equal(rest, np.broadcast_to(np.maximum(bias, 0) if relu else bias if with_bias else 0.0, rest.shape))
    # gemm and decode read rows one by one: the twin's rows give the table's results
    rng = np.random.default_rng(4)
    b = rng.standard_normal((5, width))
    assert _close(lt.gemm(c.values, b), (x @ b.T)[c.rows], np.abs(c.values.astype(np.float64)) @ np.abs(b).T, width)
    ws = [rng.standard_normal((width, width)) / np.sqrt(width), rng.standard_normal((1, width))]
    bs = [rng.standard_normal(width) * 0.1, rng.standard_normal(1)]
    u, v = rng.choice(c.rows, 40), rng.choice(c.rows, 40)
    full, twin = lt.decode(x, u, v, ws, bs)[0], lt.decode(c.values, c.twin_ids(u), c.twin_ids(v), ws, bs)[0]
    assert np.allclose(full, twin, rtol=1e-12, atol=1e-12)


def test_out_buffer_guards():
    view, buf = lo.out_buffer(50, 12, 4, 5, "cpu")
    assert not lo.guards_intact(buf, view)                                 # nothing written yet: the view still holds the sentinel
    view.fill_(1.0)
    assert lo.guards_intact(buf, view)
    for r, cc in ((1, 5), (52, 5), (10, 3), (10, 9)):
        b2 = buf.clone()
        b2[r, cc] = 0.0
        assert not lo.guards_intact(b2, b2[2:52, 4:9])


# ---------------------------------------------------------------------------------------------------------- long entry arrays
LENS, B_ROW, L = [1, 2, 5, 17, 33, 40, 3], 3, 64


def _full(c, weighted=True):
    rowptr, col, val = c.build("cpu", weighted)
    data = val.numpy() if weighted else np.ones(c.nnz, np.float32)
    A = ssp.csr_matrix((data, col.numpy(), rowptr.numpy()), shape=(c.n, c.n))
    assert A.has_sorted_indices
    return A, rowptr, col, val


@pytest.mark.parametrize("entry_bytes", [4, 8])
@pytest.mark.parametrize("phase", [0, 1])
def test_long_csr_entries_straddle(phase, entry_bytes):
    c = lo.LongCSR(MARKS, LENS, L, B_ROW, phase=phase, entry_bytes=entry_bytes)
    col = torch.empty(c.nnz, dtype=torch.int32 if entry_bytes == 4 else torch.int64)
    c.check_straddle(col)
    assert tuple(c.kinds) == [("edge", "span"), ("span", "edge")][phase] and c.positions == [m // entry_bytes for m in MARKS]
    rp = c.rowptr
    for i, (p, kind) in enumerate(zip(c.positions, c.kinds)):
        r = c.set_rows[i][B_ROW]
        if kind == "edge":                                                 # one row ends exactly at the mark, the next starts at it
            assert rp[r + 1] * entry_bytes == MARKS[i] == rp[r + 1 + 0] * entry_bytes and (r + 1) in c.live_rows
        else:
            assert rp[r] * entry_bytes < MARKS[i] < rp[r + 1] * entry_bytes
    assert np.array_equal(np.diff(rp)[c.set_rows[0]], LENS) and len(c.set_rows) == 3
    deg = np.diff(rp)
    assert (deg[c.full_ballast_rows] == L).all() and len(c.full_ballast_rows) > 8
    assert (deg[c.ballast_rows] <= L).all() and (deg[c.ballast_rows] > 0).all() and (deg[c.n_used:] == 0).all()
    assert c.set_rows[-1][-1] == c.n_used - 1


@pytest.mark.parametrize("phase", [0, 1])
def test_long_csr_arrays_hold_the_host_data(phase):
    c = lo.LongCSR(MARKS, LENS, L, B_ROW, phase=phase)
    A, rowptr, col, val = _full(c)
    c.check_straddle(col)
    row, cc, vv = c.entry(np.arange(c.nnz))
    assert np.array_equal(cc, col.numpy()) and np.array_equal(vv, val.numpy())
    assert np.array_equal(row, np.repeat(np.arange(c.n), np.diff(c.rowptr)))
    for r in c.ballast_rows:
        ids, vals = c.row(int(r))
        assert np.array_equal(ids, np.arange(len(ids))) and np.array_equal(A[r].indices, ids) and np.array_equal(A[r].data, vals)
    T, keep = c.twin()
    assert set(c.live_rows) <= set(keep) and len(np.intersect1d(keep, c.full_ballast_rows)) >= 2
    assert (abs(T[keep] - A[keep])).nnz == 0 and T.nnz == A[keep].nnz and T.nnz < A.nnz // 3
    # unit build: the same pattern, no values
    _, _, col1, none = _full(c, weighted=False)
    assert none is None and torch.equal(col1, col)
    # the whole-array truths
    assert _close(c.row_sums(), np.asarray(A.astype(np.float64).sum(1)).ravel(), np.asarray(A.astype(np.float64).sum(1)).ravel(), L)
    assert np.array_equal(c.row_sums(False), np.diff(c.rowptr))
    s, a, k = c.col_sums()
    assert np.array_equal(k, np.bincount(col.numpy(), minlength=c.n))
    ref = np.asarray(A.astype(np.float64).sum(0)).ravel()
    assert _close(s, ref, ref, int(k.max())) and (a <= s).all()
    assert np.array_equal(c.col_sums(False)[0], k)
    for weighted in (True, False):
        ks = np.arange(c.nnz)
        truth, bound = lo.gcn_norm_at(c, ks, weighted)
        v = val.numpy() if weighted else None
        ref = lt.gcn_norm(rowptr.numpy(), col.numpy(), v)
        assert np.allclose(truth, ref, rtol=1e-13, atol=0) and np.allclose(bound, lt.gcn_norm_bound(rowptr.numpy(), col.numpy(), ref), rtol=1e-12)
        assert (truth[c.sample_entries()] != 0).sum() > 10
    se = c.sample_entries()
    assert all(p in se and p - 1 in se for p in c.positions) and 0 in se and c.nnz - 1 in se


@pytest.mark.parametrize("phase", [0, 1])
def test_long_csr_pair_truths_on_the_twin_equal_the_whole_graph(phase):
    c = lo.LongCSR(MARKS, LENS, L, B_ROW, phase=phase)
    A, rowptr, col, val = _full(c)
    T, keep = c.twin()
    u, v = lo.pair_lists(c)
    assert (np.diff(v) >= 0).all() and set(c.live_rows) <= set(u) and set(c.live_rows) <= set(v) and set(c.pair_ballast()) <= set(u) & set(v)
    assert set(c.pair_ballast()) <= set(c.kept_ballast()) and len(c.pair_ballast()) == 4
    assert set(u) | set(v) <= set(keep)
    w = np.random.default_rng(5).uniform(0.05, 1.0, c.n)
    for X, Y in ((A, T), (pt.unit(A), pt.unit(T))):
        full, twin = pt.scores(X, w, u, v), pt.scores(Y, w, u, v)
        mine = lo.pair_truth(c, X is A, w, u, v)
        for key in full:
            assert np.array_equal(full[key], twin[key]), key
            assert np.array_equal(mine[key], full[key]) if key == "count" else _close(mine[key], full[key], full["abs" if key in ("ws", "abs") else "abs_cn"], 1), key
        D = X.toarray().astype(np.float64)
        dense = np.einsum("ij,ij,j->i", D[u], D[v], w)
        assert _close(full["ws"], dense, full["abs"], int(full["count"].max()))
        assert np.array_equal(full["count"], ((D[u] != 0) & (D[v] != 0)).sum(1))
    assert full["count"].max() >= 30 and (full["count"] == 0).any()
    w32 = w.astype(np.float32)
    tr, tc, tv = T.indptr.astype(np.int64), T.indices, T.data
    for a, b in list(zip(u, v))[::7]:
        e = wt.pair_exact(tr, tc, tv, w32, a, b)
        assert e.view(np.int32) == wt.pair_exact(rowptr.numpy(), col.numpy(), val.numpy(), w32, a, b).view(np.int32)
    # SpMM with a narrow x: the twin's rows give the whole graph's rows
    x = np.random.default_rng(6).standard_normal((c.n, 4))
    assert _close((T.astype(np.float64) @ x)[keep], (A.astype(np.float64) @ x)[keep], (abs(T).astype(np.float64) @ np.abs(x))[keep], L)


def test_cn_lists_of_ballast_pairs_are_prefixes_of_the_other_row():
    """What test_gpu_large_offsets.py expects of ops.pair_cn_list for a pair with a ballast row -- the other row's ids below the
    ramp's length -- is what cn_list_truth.cn_lists gives on the whole graph."""
    import cn_list_truth as cl
    c = lo.LongCSR(MARKS, LENS, L, B_ROW)
    A, _, _, _ = _full(c)
    u, v = lo.pair_lists(c)
    ptr, w = cl.cn_lists(A, u, v)
    for i in np.flatnonzero(~(np.isin(u, c.live_rows) & np.isin(v, c.live_rows))):
        (ca, _), (cb, _) = c.row(int(u[i])), c.row(int(v[i]))
        a_ramp, b_ramp = u[i] not in c.live_rows, v[i] not in c.live_rows
        want = np.arange(min(len(ca), len(cb))) if a_ramp and b_ramp else cb[cb < len(ca)] if a_ramp else ca[ca < len(cb)]
        assert np.array_equal(w[ptr[i]:ptr[i + 1]], want)


@pytest.mark.parametrize("phase", [0, 1])
def test_gammas_from_the_host_data_equal_the_whole_graph(phase):
    """lo.gammas_truth (rows restated from the host data) is local_community_truth.gammas on the whole graph, for the lists of
    lo.pair_lists -- lists that hold live rows, ballast rows and rows without entries."""
    import cn_list_truth as cl
    import local_community_truth as lct
    c = lo.LongCSR(MARKS, LENS, L, B_ROW, phase=phase)
    A, _, _, _ = _full(c)
    u, v = lo.pair_lists(c)
    ptr, w = cl.cn_lists(A, u, v)
    want = lct.gammas(A, ptr, w)
    assert np.array_equal(lo.gammas_truth(c, ptr, w), want) and np.array_equal(want, lct.gammas_by_pair(A, ptr, w))
    assert want.max() > 3 and np.isin(w, c.live_rows).any() and np.isin(w, c.ballast_rows).any() and (w >= c.n_used).any()
    assert (want[np.isin(w, c.live_rows)] > 0).any()


def test_tall_case_with_a_second_pitch():
    """``more_pitches``: the mark rows of an ``out`` with another leading dimension are kept rows too, and the table reaches
    beyond the marks at either pitch."""
    c = lo.TallCase(MARKS, 8, more_pitches=(36,), n_extra=40, ballast_rows=37)
    view, _ = c.build("cpu")
    c.check_straddle(view)
    out, obuf = lo.out_buffer(c.n_rows, 9, 1, 8, "cpu")
    assert out.stride(0) * 4 == 36
    c.check_straddle(out)
    for p in (32, 36):
        for m in MARKS:
            assert {m // p - 1, m // p, m // p + 1} <= set(c.live) and (c.n_rows - 1) * p > max(MARKS)
