"""CPU: tests/layer_truth.py itself -- each float64 truth against a triple loop or a dense statement on tiny inputs, and each
case builder against what it promises (exact row lengths, the operand flavours' strides and address remainders, the guard
bands, the conditions on the decode cases), so that the GPU tests compare the kernels with something that was checked."""
import math

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import layer_truth as lt


# ---------------------------------------------------------------------------------------------------------- truths
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_acc", [False, True])
def test_gemm_truth_is_the_triple_loop(relu, with_bias, with_acc):
    rng = np.random.default_rng(1)
    m, n, k = 3, 4, 5
    a, b = rng.standard_normal((m, k)).astype(np.float32), rng.standard_normal((n, k)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32) if with_bias else None
    acc = rng.standard_normal((m, n)).astype(np.float32) if with_acc else None
    want = np.zeros((m, n))
    bound = np.zeros((m, n))
    for i in range(m):
        for j in range(n):
            s = t = 0.0
            for q in range(k):
                s += float(a[i, q]) * float(b[j, q])
                t += abs(float(a[i, q])) * abs(float(b[j, q]))
            if with_bias:
                s += float(bias[j]); t += abs(float(bias[j]))
            if with_acc:
                s += float(acc[i, j]); t += abs(float(acc[i, j]))
            want[i, j] = max(s, 0.0) if relu else s
            bound[i, j] = (k + 2 + with_acc) * 2.0 ** -24 * t
    np.testing.assert_allclose(lt.gemm(a, b, bias, relu, acc), want, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(lt.gemm_bound(a, b, bias, acc), bound, rtol=1e-14)


def _tiny_csr(rng, n=7, explicit_zero=True):
    D = (rng.random((n, n)) < 0.4) * rng.uniform(0.1, 2.0, (n, n)).astype(np.float32)
    D[2] = 0.0                                                    # an empty row
    B = ssp.csr_matrix(D)
    if explicit_zero:
        B.data[0] = 0.0                                           # a stored zero: counts for the mean, adds nothing to the sum
    return B


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_spmm_truth_is_the_triple_loop(mean, relu):
    rng = np.random.default_rng(2)
    B = _tiny_csr(rng)
    n, f = B.shape[0], 3
    x = rng.standard_normal((n, f)).astype(np.float32)
    bias = rng.standard_normal(f).astype(np.float32)
    want, bound = np.zeros((n, f)), np.zeros((n, f))
    for r in range(n):
        lo, hi = B.indptr[r], B.indptr[r + 1]
        for c in range(f):
            s = t = 0.0
            for e in range(lo, hi):
                w = 1.0 if mean else float(B.data[e])
                s += w * float(x[B.indices[e], c]); t += abs(w) * abs(float(x[B.indices[e], c]))
            if mean:
                s /= max(hi - lo, 1); t /= max(hi - lo, 1)
            s += float(bias[c]); t += abs(float(bias[c]))
            want[r, c] = max(s, 0.0) if relu else s
            bound[r, c] = lt.gamma(hi - lo + 1) * t
    np.testing.assert_allclose(lt.spmm(B, x, bias, relu, mean), want, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(lt.spmm_bound(B, x, bias, mean, extra=1), bound, rtol=1e-13)
    assert np.array_equal(lt.spmm(B, x, None, False, mean)[2], np.zeros(f))          # the empty row
    if mean:                                                      # the values play no part: a unit-valued copy gives the same bits
        ones = ssp.csr_matrix((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)
        assert np.array_equal(lt.spmm(B, x, bias, relu, True), lt.spmm(ones, x, bias, relu, True))


@pytest.mark.parametrize("unit", [False, True])
def test_gcn_norm_truth_is_the_dense_statement(unit):
    rng = np.random.default_rng(3)
    n = 9
    D = (rng.random((n, n)) < 0.5) * rng.uniform(0.05, 3.0, (n, n)).astype(np.float32)
    D = np.maximum(D, D.T)
    D[4] = 0.0                                                    # row 4 is empty; its column entries stay: they must come out 0
    B = ssp.csr_matrix(D)
    B.data[B.indptr[1]:B.indptr[1 + 1]] = 0.0                     # row 1: stored entries that sum to zero
    val = None if unit else B.data.astype(np.float32)
    got = lt.gcn_norm(B.indptr, B.indices, val)
    Dv = ssp.csr_matrix((np.ones(B.nnz) if unit else B.data.astype(np.float64), B.indices, B.indptr), shape=B.shape).toarray()
    s = Dv.sum(1)
    with np.errstate(divide="ignore"):
        dis = np.where(s > 0, 1.0 / np.sqrt(s), 0.0)
    want = dis[:, None] * Dv * dis[None, :]
    k = 0
    for r in range(n):
        for e in range(B.indptr[r], B.indptr[r + 1]):
            assert got[e] == pytest.approx(want[r, B.indices[e]], rel=1e-14, abs=0.0), (r, e)
            k += 1
    assert k == B.nnz and np.isfinite(got).all()
    if not unit:
        assert np.array_equal(got[B.indptr[1]:B.indptr[2]], np.zeros(B.indptr[2] - B.indptr[1]))
    assert (got[B.indices == 4] == 0.0).all() and (B.indices == 4).any()
    # the bound: deg counts ENTRIES (not values), averaged over the entry's row and column
    deg = np.diff(B.indptr)
    row = np.repeat(np.arange(n), deg)
    np.testing.assert_allclose(lt.gcn_norm_bound(B.indptr, B.indices, got),
                               ((deg[row] + deg[B.indices]) / 2 * 2.0 ** -24 + 1e-6) * np.abs(got), rtol=1e-14)


def test_decode_truth_is_the_loop():
    rng = np.random.default_rng(4)
    nn, hd = 6, 4
    h = rng.standard_normal((nn, hd)).astype(np.float32)
    ws = [rng.standard_normal((hd, hd)).astype(np.float32), rng.standard_normal((hd, hd)).astype(np.float32),
          rng.standard_normal((1, hd)).astype(np.float32)]
    bs = [rng.standard_normal(hd).astype(np.float32), rng.standard_normal(hd).astype(np.float32), rng.standard_normal(1).astype(np.float32)]
    u, v = rng.integers(0, nn, (2, 10)).astype(np.int32)
    logit, prob = lt.decode(h, u, v, ws, bs)
    for p in range(10):
        z = [float(h[u[p], c]) * float(h[v[p], c]) for c in range(hd)]
        for w, b in zip(ws[:-1], bs[:-1]):
            z = [max(sum(float(w[o, c]) * z[c] for c in range(hd)) + float(b[o]), 0.0) for o in range(hd)]
        s = sum(float(ws[-1][0, c]) * z[c] for c in range(hd)) + float(bs[-1][0])
        assert logit[p] == pytest.approx(s, rel=1e-13, abs=1e-15)
        assert prob[p] == pytest.approx(1.0 / (1.0 + math.exp(-s)), rel=1e-13)
    one = lt.decode(h, u, v, ws[-1:], bs[-1:])[0]                 # a single layer is the dot product alone
    np.testing.assert_allclose(one, (h[u].astype(np.float64) * h[v]) @ ws[-1][0].astype(np.float64) + float(bs[-1][0]), rtol=1e-13)


# ---------------------------------------------------------------------------------------------------------- graphs
def test_layer_graph_has_the_promised_rows_and_values():
    A = lt.layer_graph()
    assert A.shape == (lt.LAYER_NODES, lt.LAYER_NODES)
    assert np.diff(A.indptr)[:len(lt.LAYER_ROWS)].tolist() == lt.LAYER_ROWS == [0, 1, 31, 32, 33, 63, 64, 65, 129, 2049]
    assert abs(A - A.T).max() == 0.0                              # symmetric in pattern and values
    assert 0.05 < A.data.min() and A.data.max() < 3.0
    assert np.array_equal(A.data, A.data.astype(np.float32).astype(np.float64))      # what the device holds is what the truth reads
    assert np.mean(A.data != np.round(A.data)) > 0.99             # fractional: products and sums round
    Z = lt.layer_graph(zero_row=True)
    lo, hi = Z.indptr[lt.ZERO_ROW], Z.indptr[lt.ZERO_ROW + 1]
    assert hi - lo == 33 and (Z.data[lo:hi] == 0.0).all() and np.array_equal(Z.indptr, A.indptr)   # stored, and summing to zero
    assert np.array_equal(np.delete(Z.data, np.arange(lo, hi)), np.delete(A.data, np.arange(lo, hi)))
    t = lt.gcn_norm(Z.indptr, Z.indices, Z.data.astype(np.float32))
    assert (t[lo:hi] == 0.0).all() and (t[Z.indices == lt.ZERO_ROW] == 0.0).all() and np.isfinite(t).all()


def test_rows_graph_is_the_training_tests_graph():
    """The builder moved here from tests/test_gpu_training.py: same draws in the same order, integer weights 1..4."""
    A = lt.rows_graph(np.random.default_rng(17), [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2049, 4200], 4500)
    assert np.diff(A.indptr)[:13].tolist() == [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2049, 4200]
    assert abs(A - A.T).max() == 0.0 and set(np.unique(A.data)) == {1.0, 2.0, 3.0, 4.0}


# ---------------------------------------------------------------------------------------------------------- GEMM operands
@pytest.mark.parametrize("k", lt.GEMM_K + [130, 132])
@pytest.mark.parametrize("r", [1, 5])
def test_input_flavours_have_the_promised_storage(k, r):
    vals = torch.arange(r * k, dtype=torch.float32).reshape(r, k) + 1
    seen = {}
    for fl in lt.IN_FLAVOURS:
        view, buf = lt.operand(vals, fl)
        assert torch.equal(view, vals) and view.stride(1) == 1 and view.shape == (r, k)
        ld, rem = view.stride(0) if r > 1 else buf.stride(0), view.data_ptr() % 16
        seen[fl] = (ld % 4, rem)
        if fl == "contig":
            assert view.is_contiguous() and buf is view and rem == 0
            continue
        assert buf.data_ptr() % 16 == 0 and buf.shape[0] == r + 2 * lt.GUARD_ROWS
        # everything around the view is NaN: the guard rows and the columns beside it
        mask = torch.ones_like(buf, dtype=torch.bool)
        c0 = (view.data_ptr() - buf.data_ptr()) // 4 % buf.stride(0)
        mask[lt.GUARD_ROWS:lt.GUARD_ROWS + r, c0:c0 + k] = False
        assert bool(torch.isnan(buf[mask]).all()) and int(mask.sum()) == buf.numel() - r * k
        assert not bool(torch.isnan(buf[~mask]).any())
    assert seen["ld_odd"][0] != 0 and seen["slice_ld_odd"][0] != 0
    assert seen["slice_ld4"] == (0, 0) and seen["base_off1"] == (0, 4)
    if k % 4:                                                      # "contiguous with ld % 4 != 0": no pad column at all
        view, buf = lt.operand(vals, "ld_odd")
        assert buf.stride(0) == k
    # the slices have NaN columns on BOTH sides
    for fl in ("slice_ld4", "slice_ld_odd", "base_off1"):
        view, buf = lt.operand(vals, fl)
        c0 = (view.data_ptr() - buf.data_ptr()) // 4 % buf.stride(0)
        assert c0 >= 1 and buf.stride(0) - (c0 + k) >= 4
    if r > 1:
        assert [lt.is_fast(lt.operand(vals, fl)[0]) for fl in lt.IN_FLAVOURS] == [k % 4 == 0, False, True, False, False]


@pytest.mark.parametrize("n", lt.GEMM_N)
def test_out_flavours_have_the_promised_storage(n):
    m = 5
    init = torch.arange(m * n, dtype=torch.float32).reshape(m, n)
    for fl in lt.OUT_FLAVOURS:
        view, buf = lt.out_operand(m, n, fl)
        if fl in ("fresh", "bias_off1"):
            assert view is None and buf is None
            t, _ = lt.out_operand(m, n, fl, init=init)
            assert torch.equal(t, init) and t.is_contiguous() and t.data_ptr() != init.data_ptr()
            continue
        assert view.shape == (m, n) and bool((buf.view(torch.int32) == lt.SENTINEL).all()) and lt.guard_intact(buf, view)
        if fl == "slice_ld_odd":                                   # (rows at every remainder: the base's own does not matter)
            assert view.stride(0) % 4 == 1
        else:
            assert (view.stride(0) % 4, view.data_ptr() % 16) == {"slice_ld4": (0, 0), "base_off1": (0, 4)}[fl]
        view, buf = lt.out_operand(m, n, fl, init=init)
        assert torch.equal(view, init) and lt.guard_intact(buf, view)
        # one word written anywhere outside the view -- beside it, in a guard row, the last word of all -- is noticed
        for rr, cc in ((lt.GUARD_ROWS, 0), (lt.GUARD_ROWS + m - 1, buf.shape[1] - 1), (lt.GUARD_ROWS - 1, 4), (buf.shape[0] - 1, buf.shape[1] - 1),
                       (lt.GUARD_ROWS + m, (view.data_ptr() - buf.data_ptr()) // 4 % buf.stride(0))):
            v2, b2 = lt.out_operand(m, n, fl, init=init)
            b2[rr, cc] = 1.0
            assert not lt.guard_intact(b2, v2), (fl, rr, cc)
    b = lt.bias_operand(torch.arange(n, dtype=torch.float32), True)
    assert b.data_ptr() % 16 == 4 and b.is_contiguous() and torch.equal(b, torch.arange(n, dtype=torch.float32))
    assert lt.bias_operand(torch.arange(n, dtype=torch.float32), False).data_ptr() % 16 == 0


def test_gemm_path_restates_the_dispatch():
    """Over the whole grid of the GPU test: every flavour pair lands on the tile_load4 forms the issue names, both templates and
    both epilogues occur, and B takes the straddle form (the one no earlier test reached)."""
    seen = set()
    for k in lt.GEMM_K:
        a_vals, b_vals = torch.zeros(5, k), torch.zeros(4, k)
        for fa in lt.IN_FLAVOURS:
            for fb in lt.IN_FLAVOURS:
                a, b = lt.operand(a_vals, fa)[0], lt.operand(b_vals, fb)[0]
                tpl, pa, pb, epi = lt.gemm_path(a, b, None, None)
                want = {True: "straddle" if k % 4 else "b128", False: "dword"}
                assert (pa, pb) == (want[lt.is_fast(a)], want[lt.is_fast(b)]) and epi == "lds"         # n = 4, fresh out
                assert (tpl == "aligned") == (lt.is_fast(a) and lt.is_fast(b) and k % 4 == 0)
                seen.add((tpl, pa, pb))
        a, b = lt.operand(a_vals, "slice_ld4")[0], lt.operand(b_vals, "slice_ld4")[0]
        for fo in lt.OUT_FLAVOURS:
            out = lt.out_operand(5, 4, fo)[0]
            bias = lt.bias_operand(torch.zeros(4), fo == "bias_off1")
            epi = lt.gemm_path(a, b, out, bias)[3]
            assert epi == ("lds" if fo in ("fresh", "slice_ld4") else "scalar"), fo
            assert lt.gemm_path(a, b, out, None)[3] == ("scalar" if fo in ("base_off1", "slice_ld_odd") else "lds")
            assert lt.gemm_path(a, b, out, bias)[0] == ("aligned" if epi == "lds" and k % 4 == 0 else "general")
    forms = {"b128", "straddle", "dword"}
    assert {(pa, pb) for _, pa, pb in seen} >= {(x, y) for x in forms for y in forms if {x, y} != {"b128", "straddle"}}
    assert ("aligned", "b128", "b128") in seen and ("general", "dword", "straddle") in seen
    assert lt.gemm_path(torch.zeros(5, 8), torch.zeros(130, 8), None, None)[3] == "scalar"            # N % 4 != 0


def test_gemm_values_are_fixed_once_per_shape():
    a, b, bias, c0 = lt.gemm_values(5, 4, 3)
    assert a.shape == (5, 3) and b.shape == (4, 3) and bias.shape == (4,) and c0.shape == (5, 4)
    assert lt.gemm_values(5, 4, 3)[0] is a and not torch.equal(lt.gemm_values(5, 4, 4)[0][:, :3], a)
    assert 0.3 < float((lt.gemm(a.numpy(), b.numpy()) > 0).mean()) < 0.7 or a.numel() < 100


# ---------------------------------------------------------------------------------------------------------- decode cases
@pytest.mark.parametrize("hdim,layers", lt.NARROW + lt.WIDE)
def test_decode_cases_are_alive_and_float32_reachable(hdim, layers):
    """Every case: the shapes the kernels require, logits that vary (std >= 0.3 for H >= 36, asserted by the builder too),
    about half of the hidden units dead, and a plain float32 evaluation well inside the gate the kernels are held to."""
    c = lt.decode_case(hdim, layers)
    assert lt.decode_case(hdim, layers) is c
    assert c["h"].shape == (lt.DECODE_NODES, hdim) and c["h"].dtype == np.float32 and len(c["ws"]) == len(c["bs"]) == layers
    assert [w.shape for w in c["ws"]] == [(hdim, hdim)] * (layers - 1) + [(1, hdim)]
    assert [b.shape for b in c["bs"]] == [(hdim,)] * (layers - 1) + [(1,)]
    assert c["u"].dtype == np.int32 and len(c["u"]) == len(c["v"]) == lt.DECODE_PAIRS == len(c["logit"])
    assert 0 <= min(c["u"].min(), c["v"].min()) and max(c["u"].max(), c["v"].max()) < lt.DECODE_NODES
    if hdim >= 36:
        assert float(c["logit"].std()) >= 0.3
        assert 1e-4 < c["prob"].min() and c["prob"].max() < 1 - 1e-4   # no saturated sigmoid hides an error in the logit
    if layers >= 2 and hdim >= 36:
        z = c["h"][c["u"]].astype(np.float64) * c["h"][c["v"]]
        for w, b in zip(c["ws"][:-1], c["bs"][:-1]):
            z = np.maximum(z @ w.astype(np.float64).T + b, 0.0)
        assert 0.3 < float((z == 0).mean()) < 0.7
    err = float(np.abs(lt.decode_float32(c["h"], c["u"], c["v"], c["ws"], c["bs"]) - c["logit"]).max())
    assert err <= 0.25 * 2e-5 * max(1.0, float(np.abs(c["logit"]).max())), err


def test_decode_lengths_make_a_second_trip():
    for wide, tile in ((False, 64), (True, 32)):
        short, long = lt.decode_lengths(wide, 256)
        assert short == [1, tile - 1, tile, tile + 1]
        n_tiles = (long + tile - 1) // tile
        assert n_tiles == 2 * 256 + 2 and n_tiles > 2 * 256 and long % tile == 1     # two workgroups take a second trip, the last tile is one pair
    ids = np.arange(500, dtype=np.int32)
    rep = lt.repeated(ids, 1203)
    assert rep.dtype == np.int32 and np.array_equal(rep[:500], ids) and np.array_equal(rep[500:1000], ids) and np.array_equal(rep[1000:], ids[:203])
