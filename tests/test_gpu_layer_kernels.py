"""GPU: the four kernels a GNN's INFERENCE runs through -- ops.gemm, ops.spmm_csr on the eval path, ops.gcn_norm, ops.mlp_decode
-- against the float64 truths of tests/layer_truth.py (validated on the CPU by test_layer_truth_host.py) on every dispatch path:
every storage flavour of the GEMM operands inside NaN / sentinel guard bands, TAGConv.hops' two-blocks-of-one-buffer SpMM and the
fused epilogues on exact row lengths, gcn_norm on long fractional rows, a zero-sum row and the unit branch, the decode kernels at
every depth up to D_MAXL with a second persistent trip -- and the shape contract of the four wrappers.

Every test prints one line that starts with ``LK`` and gives the largest error / bound ratio it saw."""
import numpy as np
import pytest
import torch

import layer_truth as lt
from conftest import rel_err

pytestmark = pytest.mark.gpu

I32 = torch.int32


def _ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; ``got`` is finite everywhere, and an element whose bound is 0 is exact."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    err = np.abs(got - ref)
    zero = bound == 0
    assert float(err[zero].max(initial=0.0)) == 0.0
    return float((err[~zero] / bound[~zero]).max(initial=0.0))


def _same_bits(x, y):
    return x.shape == y.shape and bool(torch.equal(x.contiguous().view(I32), y.contiguous().view(I32)))


# ====================================================================================================================
# GEMM
# ====================================================================================================================
# what eps_gemm_f32 makes of an input flavour: (is it "fast", ld % 4 == 0, base % 16) -- None where it depends on K
_IN_EXPECT = {"ld_odd": (False, False, None), "slice_ld4": (True, True, 0), "slice_ld_odd": (False, False, None),
              "base_off1": (False, True, 4)}


def _check_flavour(t, flavour, k):
    if flavour == "contig":
        assert t.is_contiguous() and t.data_ptr() % 16 == 0 and lt.is_fast(t) == (k % 4 == 0)
        return
    fast, ld4, rem = _IN_EXPECT[flavour]
    assert lt.is_fast(t) == fast and (t.stride(0) % 4 == 0) == ld4 and (rem is None or t.data_ptr() % 16 == rem), flavour
    assert not t.is_contiguous() or t.shape[0] == 1 or (flavour == "ld_odd" and k % 4 != 0)


def _untouched(buf, view):
    """An INPUT's buffer after the calls: still NaN everywhere around the view, the view still finite."""
    return int(torch.isnan(buf).sum()) == buf.numel() - view.numel() and bool(torch.isfinite(view).all())


@pytest.mark.parametrize("k", lt.GEMM_K)
def test_gemm_every_input_flavour_pair(eps, dev, k):
    """All 25 (A flavour, B flavour) pairs at the 20 (M, N) of the grid and this K, fresh ``out``: the contiguous call is held per
    element to float64 under (K + 2) U (|a| |b|^T), every other call is bit-identical to it -- so no NaN of a guard band beside
    or around a sliced operand reached the result -- and the flavour pairs are shown, from the operands' strides and address
    remainders, to land on the tile_load4 forms they are meant for (b128 / straddle / dword, for A and for B).
    Largest error / bound on the MI355X: 0.50 (K = 3) ... 0.08 (K = 58); no bit differs between the flavours."""
    ops = eps.ops
    forms, worst = set(), 0.0
    for m in lt.GEMM_M:
        for n in lt.GEMM_N:
            a, b, _, _ = lt.gemm_values(m, n, k)
            ref = ops.gemm(a.to(dev), b.to(dev))
            worst = max(worst, _ratio(ref.cpu().numpy(), lt.gemm(a.numpy(), b.numpy()), lt.gemm_bound(a.numpy(), b.numpy())))
            avs = {fl: lt.operand(a, fl, dev) for fl in lt.IN_FLAVOURS}
            bvs = {fl: lt.operand(b, fl, dev) for fl in lt.IN_FLAVOURS}
            for fl in lt.IN_FLAVOURS:
                _check_flavour(avs[fl][0], fl, k); _check_flavour(bvs[fl][0], fl, k)
            for fa, (av, _) in avs.items():
                for fb, (bv, _) in bvs.items():
                    tpl, pa, pb, epi = lt.gemm_path(av, bv, None, None)
                    got = ops.gemm(av, bv)
                    assert got.shape == (m, n) and _same_bits(got, ref), (m, n, k, fa, fb, tpl, pa, pb, epi)
                    forms.add((tpl, pa, pb))
            for fl in lt.IN_FLAVOURS[1:]:
                assert _untouched(*avs[fl][::-1]) and _untouched(*bvs[fl][::-1]), fl
    fast, slow = ("b128" if k % 4 == 0 else "straddle"), "dword"
    want = {("general", x, y) for x in (fast, slow) for y in (fast, slow)}       # (N = 1, 130: the scalar epilogue, whatever A and B)
    if k % 4 == 0:
        want.add(("aligned", fast, fast))
    assert forms == want, (forms, want)
    print(f"\nLK gemm input flavours K={k}: largest error / bound {worst:.3f} over {len(lt.GEMM_M) * len(lt.GEMM_N)} shapes x 25 pairs, "
          f"forms {sorted(forms)}")
    assert worst <= 1.0


_MODES = {"bias": (True, False, False), "relu": (False, True, False), "accumulate": (False, False, True),
          "accumulate_relu": (False, True, True)}                       # -> (bias, relu, accumulate)


def _contiguous_call(ops, dev, vals, with_bias, relu, acc, cache, worst):
    """The contiguous call of one (bias, relu, accumulate) on a shape's values, held to float64 once and kept."""
    key = (with_bias, relu, acc)
    if key not in cache:
        a, b, bias, c0 = vals
        ref = ops.gemm(a.to(dev), b.to(dev), bias=bias.to(dev) if with_bias else None, relu=relu, out=c0.to(dev) if acc else None,
                       accumulate=acc)
        bn, cn = (bias.numpy() if with_bias else None), (c0.numpy() if acc else None)
        worst[0] = max(worst[0], _ratio(ref.cpu().numpy(), lt.gemm(a.numpy(), b.numpy(), bn, relu, cn), lt.gemm_bound(a.numpy(), b.numpy(), bn, cn)))
        cache[key] = ref
    return cache[key]


@pytest.mark.parametrize("k", lt.GEMM_K)
def test_gemm_every_out_flavour(eps, dev, k):
    """Every ``out`` flavour (fresh; a slice with 16-byte aligned rows; one with a misaligned base; one with ldc % 4 != 0; a fresh
    one with ``bias`` taken as big[1:1 + n]) against bias / relu / accumulate / accumulate + relu, A and B both fast slices, at the
    20 (M, N) of the grid: bit-identical to the contiguous call on the same values, which is held to float64 under the project's
    bound ((K + 2) U (|a||b|^T + |bias|); one more unit and + |C| under accumulate) -- and every sentinel word around a sliced
    ``out`` is unchanged.  Both epilogues run under both templates (asserted from strides and address remainders).
    Largest error / bound on the MI355X: 0.61 (K = 1) ... 0.09 (K = 58); no bit differs, no sentinel word changed."""
    ops = eps.ops
    seen, worst = set(), [0.0]
    for m in lt.GEMM_M:
        for n in lt.GEMM_N:
            vals = lt.gemm_values(m, n, k)
            a, b, bias, c0 = vals
            (av, abuf), (bv, bbuf) = lt.operand(a, "slice_ld4", dev), lt.operand(b, "slice_ld4", dev)
            cache = {}
            for fo in lt.OUT_FLAVOURS:
                for mode, (with_bias, relu, acc) in _MODES.items():
                    with_bias = with_bias or fo == "bias_off1"
                    ref = _contiguous_call(ops, dev, vals, with_bias, relu, acc, cache, worst)
                    bias_t = lt.bias_operand(bias, fo == "bias_off1", dev) if with_bias else None
                    out, obuf = lt.out_operand(m, n, fo, dev, init=c0 if acc else None)
                    tpl, _, _, epi = lt.gemm_path(av, bv, out, bias_t)
                    # the epilogue this flavour is there for
                    lds = n % 4 == 0 and fo in ("fresh", "slice_ld4")
                    assert epi == ("lds" if lds else "scalar") and (tpl == "aligned") == (lds and k % 4 == 0), (fo, mode, tpl, epi)
                    if fo == "bias_off1":
                        assert bias_t.data_ptr() % 16 == 4
                    elif fo == "slice_ld4":
                        assert lt.is_fast(out)
                    elif fo == "base_off1":
                        assert out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 4
                    elif fo == "slice_ld_odd":
                        assert out.stride(0) % 4 == 1
                    got = ops.gemm(av, bv, bias=bias_t, relu=relu, out=out, accumulate=acc)
                    assert _same_bits(got, ref), (m, n, k, fo, mode, tpl, epi)
                    if obuf is not None:
                        assert got.data_ptr() == out.data_ptr() and lt.guard_intact(obuf, out), (m, n, k, fo, mode)
                    seen.add((tpl, epi))
            assert _untouched(abuf, av) and _untouched(bbuf, bv)
    assert seen == {("aligned" if k % 4 == 0 else "general", "lds"), ("general", "scalar")}, seen
    print(f"\nLK gemm out flavours K={k}: largest error / bound {worst[0]:.3f}, paths {sorted(seen)}")
    assert worst[0] <= 1.0


@pytest.mark.parametrize("k", [19, 20, 58])
def test_gemm_lower_only_on_the_scalar_epilogue(eps, dev, k):
    """M = N = 257 (3 x 3 tiles) with ``lower_only`` into a strided ``out`` that takes the scalar epilogue, with bias / relu / accumulate:
    the six tiles on and below the diagonal hold the bits of the contiguous full product (held to float64), the three above it
    hold what was there before -- the sentinel, or C under accumulate -- and so does the guard band.
    Largest error / bound on the MI355X: 0.19."""
    ops = eps.ops
    m = n = 257
    vals = lt.gemm_values(m, n, k)
    a, b, bias, c0 = vals
    av, bv = lt.operand(a, "slice_ld4", dev)[0], lt.operand(b, "base_off1", dev)[0]
    tile = torch.arange(m, device=dev) // 128
    upper = tile[None, :] > tile[:, None]                               # n0 > m0: the workgroup returns at once
    assert int(upper.sum()) == 128 * 129 + 128 * 1
    cache, worst = {}, [0.0]
    for fo in ("slice_ld_odd", "base_off1"):
        for mode in ("bias", "relu", "accumulate"):
            with_bias, relu, acc = _MODES[mode]
            full = _contiguous_call(ops, dev, vals, with_bias, relu, acc, cache, worst)
            out, obuf = lt.out_operand(m, n, fo, dev, init=c0 if acc else None)
            before = out.contiguous().view(I32).clone()
            bias_t = bias.to(dev) if with_bias else None
            assert lt.gemm_path(av, bv, out, bias_t)[3] == "scalar"
            ops.gemm(av, bv, bias=bias_t, relu=relu, out=out, accumulate=acc, lower_only=True)
            assert bool(torch.equal(torch.where(upper, before, full.view(I32)), out.contiguous().view(I32))), (fo, mode)
            assert lt.guard_intact(obuf, out), (fo, mode)
            if not acc:
                assert bool((out.contiguous().view(I32)[upper] == lt.SENTINEL).all())
    print(f"\nLK gemm lower_only K={k}: largest error / bound {worst[0]:.3f}")
    assert worst[0] <= 1.0


# ====================================================================================================================
# SpMM on the eval path, gcn_norm
# ====================================================================================================================
def _graph(eps, dev, A, unit=False):
    """The CSRGraph of a scipy matrix with its explicit zeros kept (the constructor, not from_scipy)."""
    return eps.CSRGraph(torch.from_numpy(A.indptr.astype(np.int64)).to(dev), torch.from_numpy(A.indices.astype(np.int32)).to(dev),
                        None if unit else torch.from_numpy(A.data.astype(np.float32)).to(dev), A.shape[0], A.shape[1])


@pytest.fixture(scope="module")
def layer(eps, dev):
    A = lt.layer_graph()
    return A, _graph(eps, dev, A)


SPMM_WIDTHS = [3, 58, 64, 257]                    # scalar kernel; ppa's feature width; float4 kernel; scalar with five column passes


@pytest.mark.parametrize("k", SPMM_WIDTHS)
def test_spmm_hops_between_blocks_of_one_buffer(eps, dev, layer, k):
    """TAGConv.hops' own call: input block and output block are column slices of ONE buffer (ldx = ldy = 3 k4, blocks 16-byte
    aligned, f % 4 != 0 for three of the widths), on rows of exactly 0, 1, 31, 32, 33, 63, 64, 65, 129 and 2049 fractional
    entries.  Each hop is held per element to float64 under gamma(deg) |B| |x| with x the block the kernel read; block 0 is x,
    bit for bit; the pad columns are still exactly zero.  Largest error / bound on the MI355X: 0.90 (k = 3) ... 1.00 (k = 257:
    0.996, on the one-entry row, whose single product is one rounding against a bound of one rounding)."""
    from eps_amd import models
    A, g = layer
    n = A.shape[0]
    conv = models.TAGConv(k, 8, K=2)
    x = np.random.default_rng(100 + k).standard_normal((n, k)).astype(np.float32)
    buf = conv.hops(torch.from_numpy(x).to(dev), g)
    k4 = (k + 3) // 4 * 4
    assert buf.shape == (n, 3 * k4) and buf.is_contiguous() and buf.data_ptr() % 16 == 0
    got = buf.cpu().numpy()
    blocks = [got[:, j * k4:j * k4 + k] for j in range(3)]
    assert np.array_equal(blocks[0].view(np.int32), x.view(np.int32))
    for j in range(3):
        pad = got[:, j * k4 + k:(j + 1) * k4]
        assert pad.shape[1] == k4 - k and not pad.view(np.int32).any()           # +0.0 bits: nothing was written there
    deg = np.diff(A.indptr)
    assert deg[:len(lt.LAYER_ROWS)].tolist() == lt.LAYER_ROWS
    worst = 0.0
    for j in (1, 2):
        worst = max(worst, _ratio(blocks[j], lt.spmm(A, blocks[j - 1]), lt.spmm_bound(A, blocks[j - 1])))
    assert not blocks[1][0].any() and not blocks[2][0].any()                     # the empty row
    print(f"\nLK spmm hops k={k}: largest error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("k", SPMM_WIDTHS)
def test_spmm_fused_epilogues_vs_float64(eps, dev, layer, k):
    """bias + relu on the weighted sum, and mean + bias, per element under gamma(deg + 1) (|B| |x| + |bias|).

    ``mean=True`` with a ``val`` tensor passed: the kernel ignores the values.  That is the reference's behaviour -- its SAGE
    aggregation drops the adjacency's values (``adj_t.set_value(None)``) before the mean -- so the truth is the plain average
    over the stored pattern, and the call gives the bits of the same call with ``val=None``.  Largest error / bound on the
    MI355X: bias + relu 0.89, mean + bias 0.68."""
    ops = eps.ops
    A, g = layer
    n = A.shape[0]
    rng = np.random.default_rng(200 + k)
    x, bias = rng.standard_normal((n, k)).astype(np.float32), rng.standard_normal(k).astype(np.float32)
    xd, bd = torch.from_numpy(x).to(dev), torch.from_numpy(bias).to(dev)
    y = ops.spmm_csr(g.rowptr, g.col, g.val, xd, bias=bd, relu=True)
    r_sum = _ratio(y.cpu().numpy(), lt.spmm(A, x, bias, True, False), lt.spmm_bound(A, x, bias, False, extra=1))
    ym = ops.spmm_csr(g.rowptr, g.col, g.val, xd, bias=bd, mean=True)
    r_mean = _ratio(ym.cpu().numpy(), lt.spmm(A, x, bias, False, True), lt.spmm_bound(A, x, bias, True, extra=1))
    assert _same_bits(ym, ops.spmm_csr(g.rowptr, g.col, None, xd, bias=bd, mean=True))
    assert np.array_equal(ym[0].cpu().numpy().view(np.int32), bias.view(np.int32))         # the empty row: 0 / 1 + bias
    print(f"\nLK spmm epilogues k={k}: largest error / bound bias+relu {r_sum:.3f}, mean+bias {r_mean:.3f}")
    assert r_sum <= 1.0 and r_mean <= 1.0


@pytest.mark.parametrize("variant", ["gcn", "tag", "tag_unit", "tag_zero_row"])
def test_gcn_norm_vs_float64(eps, dev, variant):
    """eps_gcn_norm per entry against val / sqrt(s_r s_c) with float64 row sums of the float32 values:
    |got - truth| <= ((deg_r + deg_c) / 2 U + 1e-6) |truth|, on rows of up to 2049 fractional values in (0.05, 3) (the wave-sum
    path), through gcn_normalized() (self loops added) and tag_normalized() (none), with unit values (``val=None``), and with one
    row whose 33 stored values are all 0.0: its entries, and the entries of its column, are exactly 0.0 and nothing is NaN.
    Largest error / bound on the MI355X: gcn 0.21, tag 0.19, tag_unit 0.06, tag_zero_row 0.19."""
    A = lt.layer_graph(zero_row=variant == "tag_zero_row")
    g = _graph(eps, dev, A, unit=variant == "tag_unit")
    if variant == "gcn":
        src, out = g.with_self_loops(1.0), g.gcn_normalized()
        import scipy.sparse as ssp
        assert not A.diagonal().any()
        Al = (A + ssp.identity(A.shape[0], format="csr")).tocsr(); Al.sort_indices()      # the self-loop plumbing, against scipy
        assert np.array_equal(src.rowptr.cpu().numpy(), Al.indptr) and np.array_equal(src.col.cpu().numpy(), Al.indices)
        assert np.array_equal(src.val.cpu().numpy(), Al.data.astype(np.float32))
    else:
        src, out = g, g.tag_normalized()
    rowptr, col = src.rowptr.cpu().numpy(), src.col.cpu().numpy()
    val = None if src.val is None else src.val.cpu().numpy()
    assert (val is None) == (variant == "tag_unit")
    assert np.diff(rowptr)[:len(lt.LAYER_ROWS)].tolist() == [d + (variant == "gcn") for d in lt.LAYER_ROWS]
    truth = lt.gcn_norm(rowptr, col, val)
    got = out.val.cpu().numpy()
    assert got.shape == truth.shape and np.array_equal(out.col.cpu().numpy(), col)
    worst = _ratio(got, truth, lt.gcn_norm_bound(rowptr, col, truth))
    if variant == "tag_zero_row":
        lo, hi = rowptr[lt.ZERO_ROW], rowptr[lt.ZERO_ROW + 1]
        assert hi - lo == 33 and not got[lo:hi].view(np.int32).any() and not got[col == lt.ZERO_ROW].any()
        assert int((col == lt.ZERO_ROW).sum()) == 33 and (val[col == lt.ZERO_ROW] > 0).all()
    print(f"\nLK gcn_norm {variant}: largest error / bound {worst:.3f} over {len(got)} entries")
    assert worst <= 1.0


# ====================================================================================================================
# decode
# ====================================================================================================================
def _on(dev, c):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t(c["h"]), [t(w) for w in c["ws"]], [t(b) for b in c["bs"]]


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


@pytest.mark.parametrize("hdim,layers", lt.NARROW + lt.WIDE)
def test_decode_depth_and_second_trip(eps, dev, hdim, layers):
    """mlp_decode_kernel (H <= 256) and mlp_decode_wide_kernel at 1 .. D_MAXL = 8 layers -- ``pick`` returns every slot -- on a
    list of (2 n_cu + 1) tile + 1 pairs: more tiles than the 2 n_cu persistent workgroups (asserted), so the second trip and the
    ids fetched one trip ahead run.  The list is the 500 truth pairs over and over: every copy is bit-identical to the first (a
    pair's output depends on its ids alone), the first is held to float64 -- logits within 2e-5 max(1, max|logit|),
    probabilities within rel_err 1e-5 -- and the lists of 1 and tile - 1, tile, tile + 1 pairs give the same bits again.
    Largest error / tolerance over the cases on the MI355X: logits 0.09 (H = 512, L = 8), probabilities 0.19 (H = 260, L = 4)."""
    ops = eps.ops
    c = lt.decode_case(hdim, layers)
    wide = hdim > 256
    tile = lt.WIDE_TILE if wide else lt.NARROW_TILE
    n_cu = ops.device_info()[0]
    short, long = lt.decode_lengths(wide, n_cu)
    n_tiles = (long + tile - 1) // tile
    assert n_tiles > 2 * n_cu and n_cu > 0 and long > 2 * lt.DECODE_PAIRS
    h, ws, bs = _on(dev, c)
    u, v = (torch.from_numpy(lt.repeated(c[key], long)).to(dev) for key in "uv")
    worst = {}
    for sig in (False, True):
        out = ops.mlp_decode(h, u, v, ws, bs, apply_sigmoid=sig).cpu().numpy()
        assert out.shape == (long,) and np.isfinite(out).all()
        first = out[:lt.DECODE_PAIRS]
        assert np.array_equal(_bits(out), _bits(lt.repeated(first, long))), "a pair's output depends on where in the list it stands"
        if sig:
            worst["prob"] = rel_err(first, c["prob"]) / 1e-5
        else:
            worst["logit"] = float(np.abs(first - c["logit"]).max()) / (2e-5 * max(1.0, float(np.abs(c["logit"]).max())))
        for n in short:
            o = ops.mlp_decode(h, u[:n], v[:n], ws, bs, apply_sigmoid=sig).cpu().numpy()
            assert o.shape == (n,) and np.array_equal(_bits(o), _bits(first[:n])), (n, sig)
    print(f"\nLK decode H={hdim} L={layers}: {n_tiles} tiles on {2 * n_cu} workgroups, error / tolerance logits {worst['logit']:.3f}, "
          f"probabilities {worst['prob']:.3f}")
    assert worst["logit"] <= 1.0 and worst["prob"] <= 1.0


@pytest.mark.parametrize("hdim,deep", [(4, 2), (100, 5), (256, 8), (260, 4), (512, 8)])
def test_decode_special_values(eps, dev, hdim, deep):
    """An all-zero row of ``h`` with one layer gives exactly the last bias; a last bias of +-200 gives probabilities of exactly 1.0
    and 0.0 and no NaN (one layer and ``deep`` layers); -0.0 in place of +0.0 entries of ``h`` changes no output bit."""
    ops = eps.ops
    rng = np.random.default_rng(300 + hdim)
    for layers in (1, deep):
        c = lt.decode_case(hdim, layers)
        h, ws, bs = _on(dev, c)
        u, v = (torch.from_numpy(c[key]).to(dev) for key in "uv")
        if layers == 1:
            hz = h.clone(); hz[7] = 0.0
            uz = torch.tensor([7, 7, 3, 7, 299], dtype=I32, device=dev)
            vz = torch.tensor([7, 5, 7, 299, 7], dtype=I32, device=dev)
            got = ops.mlp_decode(hz, uz, vz, ws, bs, apply_sigmoid=False).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(np.repeat(c["bs"][-1], 5))), got
        for shift, want in ((200.0, 1.0), (-200.0, 0.0)):
            assert float(np.abs(c["logit"]).max()) < 50.0
            b2 = bs[:-1] + [bs[-1] + shift]
            p = ops.mlp_decode(h, u, v, ws, b2).cpu().numpy()
            assert np.array_equal(_bits(p), _bits(np.full(len(p), want, np.float32))), (layers, shift, p[:4])
        zero = torch.from_numpy(rng.random(c["h"].shape) < 0.1).to(dev)
        hp, hn = h.masked_fill(zero, 0.0), h.masked_fill(zero, -0.0)
        assert bool((hn[zero].view(I32) == -2 ** 31).all()) and bool((hp[zero].view(I32) == 0).all()) and int(zero.sum()) > 0
        for sig in (False, True):
            assert _same_bits(ops.mlp_decode(hp, u, v, ws, bs, apply_sigmoid=sig), ops.mlp_decode(hn, u, v, ws, bs, apply_sigmoid=sig)), (layers, sig)
    print(f"\nLK decode special values H={hdim}: exact (error / bound 0.000)")


# ====================================================================================================================
# the wrappers' shape contract
# ====================================================================================================================
@pytest.fixture(scope="module")
def wellformed(eps, dev):
    f32 = dict(dtype=torch.float32, device=dev)
    n, f, hd = 6, 5, 8
    rowptr = torch.tensor([0, 2, 3, 3, 5, 6, 8], dtype=torch.int64, device=dev)
    col = torch.tensor([1, 2, 0, 0, 4, 3, 1, 5], dtype=I32, device=dev)
    return dict(a=torch.zeros((4, 3), **f32), b=torch.zeros((7, 3), **f32), bias=torch.zeros(7, **f32), out=torch.zeros((4, 7), **f32),
                rowptr=rowptr, col=col, val=torch.ones(8, **f32), x=torch.zeros((n, f), **f32), sbias=torch.zeros(f, **f32),
                sout=torch.zeros((n, f), **f32), h=torch.zeros((n, hd), **f32), u=torch.zeros(9, dtype=I32, device=dev),
                v=torch.zeros(9, dtype=I32, device=dev), ws=[torch.zeros((hd, hd), **f32), torch.zeros((1, hd), **f32)],
                bs=[torch.zeros(hd, **f32), torch.zeros(1, **f32)], f32=f32)


def _z(s, *shape):
    return torch.zeros(shape, **s["f32"])


REFUSED = {
    # -> (what the refusal must name, the call)
    "gemm_a_1d": (r"gemm: a must be 2-D", lambda o, s: o.gemm(_z(s, 3), s["b"])),
    "gemm_b_3d": (r"gemm: b must be 2-D", lambda o, s: o.gemm(s["a"], _z(s, 7, 3, 1))),
    "gemm_out_1d": (r"gemm: out must be 2-D", lambda o, s: o.gemm(s["a"], s["b"], out=_z(s, 28))),
    "gemm_bias_long": (r"gemm: bias holds 8 entries, not 7", lambda o, s: o.gemm(s["a"], s["b"], bias=_z(s, 8))),
    "gemm_bias_short": (r"gemm: bias holds 6 entries, not 7", lambda o, s: o.gemm(s["a"], s["b"], bias=_z(s, 6))),
    "gemm_out_wide": (r"gemm: out must be \[4, 7\]", lambda o, s: o.gemm(s["a"], s["b"], out=_z(s, 4, 8))),
    "gemm_out_short": (r"gemm: out must be \[4, 7\]", lambda o, s: o.gemm(s["a"], s["b"], out=_z(s, 3, 7), accumulate=True)),
    "gemm_out_transposed": (r"gemm: out must be \[4, 7\]", lambda o, s: o.gemm(s["a"], s["b"], out=_z(s, 7, 4))),
    "gemm_out_slice": (r"gemm: out must be \[4, 7\]", lambda o, s: o.gemm(s["a"], s["b"], out=_z(s, 4, 16)[:, 1:7])),
    "spmm_x_1d": (r"spmm_csr: x must be 2-D", lambda o, s: o.spmm_csr(s["rowptr"], s["col"], None, _z(s, 6))),
    "spmm_val": (r"spmm_csr: val holds 7 entries, not 8", lambda o, s: o.spmm_csr(s["rowptr"], s["col"], _z(s, 7), s["x"])),
    "spmm_bias": (r"spmm_csr: bias holds 4 entries, not 5", lambda o, s: o.spmm_csr(s["rowptr"], s["col"], None, s["x"], bias=_z(s, 4))),
    "spmm_out_rows": (r"spmm_csr: out must be \[6, 5\]", lambda o, s: o.spmm_csr(s["rowptr"], s["col"], None, s["x"], out=_z(s, 5, 5))),
    "spmm_out_cols": (r"spmm_csr: out must be \[6, 5\]", lambda o, s: o.spmm_csr(s["rowptr"], s["col"], None, s["x"], out=_z(s, 6, 8)[:, :4])),
    "spmm_out_1d": (r"spmm_csr: out must be 2-D", lambda o, s: o.spmm_csr(s["rowptr"], s["col"], None, s["x"], out=_z(s, 30))),
    "gcn_norm_val": (r"gcn_norm: val holds 9 entries, not 8", lambda o, s: o.gcn_norm(s["rowptr"], s["col"], _z(s, 9))),
    "decode_h_1d": (r"mlp_decode: h must be 2-D", lambda o, s: o.mlp_decode(_z(s, 48), s["u"], s["v"], s["ws"], s["bs"])),
    "decode_u_v": (r"mlp_decode: u and v differ in length \(9 vs 8\)", lambda o, s: o.mlp_decode(s["h"], s["u"], s["v"][:8], s["ws"], s["bs"])),
    "decode_hidden_bias": (r"mlp_decode: layer 0 bias holds 7 entries, not 8",
                           lambda o, s: o.mlp_decode(s["h"], s["u"], s["v"], s["ws"], [_z(s, 7), s["bs"][1]])),
    "decode_last_bias": (r"mlp_decode: layer 1 bias holds 8 entries, not 1",
                         lambda o, s: o.mlp_decode(s["h"], s["u"], s["v"], s["ws"], [s["bs"][0], _z(s, 8)])),
    "decode_bias_count": (r"mlp_decode: one bias per weight", lambda o, s: o.mlp_decode(s["h"], s["u"], s["v"], s["ws"], s["bs"][:1])),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_wrong_shape_is_refused_before_any_launch(eps, wellformed, monkeypatch, case):
    """gemm, spmm_csr, gcn_norm and mlp_decode refuse an operand of the wrong shape with an EpsError that names it.  ``ops._call``
    -- the one way into the library -- is replaced by a function that fails the test: a missing check shows as a failed
    assertion, never as a launch that reads or writes past an array."""
    ops = eps.ops
    reached = []
    monkeypatch.setattr(ops, "_call", lambda name, *a, **k: reached.append(name))
    msg, call = REFUSED[case]
    try:
        with pytest.raises(eps.EpsError, match=msg):
            call(ops, wellformed)
    finally:
        assert reached == [], f"{case}: the call went on to {reached}"


REACHES = {
    "gemm": ("eps_gemm_f32", lambda o, s: o.gemm(s["a"], s["b"], bias=s["bias"], out=s["out"], accumulate=True)),
    "gemm_views": ("eps_gemm_f32", lambda o, s: o.gemm(_z(s, 4, 9)[:, 1:4], _z(s, 7, 5)[:, :3], out=_z(s, 6, 16)[1:5, 2:9])),
    "spmm_csr": ("eps_spmm_csr", lambda o, s: o.spmm_csr(s["rowptr"], s["col"], s["val"], s["x"], bias=s["sbias"], out=s["sout"])),
    "spmm_csr_row_block": ("eps_spmm_csr", lambda o, s: o.spmm_csr(s["rowptr"][2:5], s["col"], s["val"], s["x"], out=_z(s, 2, 5))),
    "gcn_norm": ("eps_gcn_norm", lambda o, s: o.gcn_norm(s["rowptr"], s["col"], s["val"])),
    "gcn_norm_unit": ("eps_gcn_norm", lambda o, s: o.gcn_norm(s["rowptr"], s["col"], None)),
    "mlp_decode": ("eps_mlp_decode", lambda o, s: o.mlp_decode(s["h"], s["u"], s["v"], s["ws"], s["bs"])),
}


@pytest.mark.parametrize("case", sorted(REACHES))
def test_well_formed_call_reaches_the_library(eps, wellformed, monkeypatch, case):
    """The checks refuse nothing that is well formed: views, a row block of the graph (GCNConv.forward_rows), ``val=None``.  One
    call per wrapper arrives at the patched ``_call`` under the expected symbol, exactly once."""
    ops = eps.ops
    reached = []
    monkeypatch.setattr(ops, "_call", lambda name, *a, **k: reached.append(name))
    symbol, call = REACHES[case]
    call(ops, wellformed)
    assert reached == [symbol]
