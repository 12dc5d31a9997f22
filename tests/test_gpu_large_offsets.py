"""GPU: kernels on operands whose byte offsets need more than 31 and more than 32 bits.  The cases come from
tests/large_offset_cases.py (validated at small marks on the CPU by tests/test_large_offset_cases_host.py): periodic ballast
filled on the device with a few hundred live rows over it, the mark rows / entries straddling 2^31 and 2^32 bytes.

Every kernel is held to two standards, neither with a number of its own:
  * the float64 truth and the bound of its own test module (layer_truth, gat_truth, pair_score_truth, weighted_truth,
    sketch_truth, cn_list_truth, local_community_truth, the decode and cosine training cases), on the live outputs;
  * bit identity with the COMPACTED TWIN: the same live rows at low offsets (the arithmetic order of these kernels does not
    depend on ids or addresses).  Where a twin is another problem -- an output that needs rows the twin drops -- the test says so.
Ballast outputs are checked too: sampled next to every mark, and -- where the expected value is periodic or constant -- over the
whole output by a reduction on the device, so a store that wrapped into the ballast shows.  ``out=`` buffers are sentinel-filled
with guard rows and columns.  Every test asserts from its own operands' sizes and the mark rows' / entries' offsets that it is
beyond the marks.  Nothing of an operand's size crosses to the host or is generated there.

Group A: tall tables (row index x leading dimension crosses the marks).  Group B: long entry arrays (rowptr crosses 2^29 and
2^30 entries).  Group C: the entry points that address col[] with 32 bits refuse a size at their limit before any launch.

At most ~20 GiB of device memory is live at a time (every test states its footprint, held to 24 GiB); each test frees its tensors and the cache is emptied after every test."""
import gc

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import large_offset_cases as lo
import layer_truth as lt
import pair_score_truth as pt
import weighted_truth as wt
from conftest import rel_err

pytestmark = pytest.mark.gpu

MARKS = lo.GPU_MARKS
GIB = 1 << 30
I32 = torch.int32


@pytest.fixture(autouse=True)
def _release_device_memory():
    """The big tensors of a test die with its frame; the allocator's cached blocks are returned after every test, so the rest of
    the suite (and EPS_TEST_POISON=1 runs) does not carry gigabytes of them."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _need(dev, footprint):
    """Skip only when the device cannot hold the test: less free memory than its footprint + 4 GiB (both figures printed)."""
    assert footprint <= 24 * GIB, "a test of this module keeps at most 24 GiB live"
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < footprint + 4 * GIB:
        print(f"\nLO skip: {free / GIB:.1f} GiB free, the test needs {footprint / GIB:.1f} GiB + 4 GiB")
        pytest.skip(f"{free / GIB:.1f} GiB free < {footprint / GIB:.1f} + 4 GiB")


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(t):
    return t.contiguous().view(I32 if t.element_size() == 4 else torch.int64)


def _same_bits(x, y):
    return x.shape == y.shape and bool(torch.equal(_bits(x), _bits(y)))


def _ratio(got, ref, bound):
    """layer kernels' measure: max |got - ref| / bound; an element whose bound is 0 is exact."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    err = np.abs(got - ref)
    zero = bound == 0
    assert float(err[zero].max(initial=0.0)) == 0.0
    return float((err[~zero] / bound[~zero]).max(initial=0.0))


def _beyond_marks(case, table, buf=None):
    """The table's mark rows straddle both marks and the operand is larger than the highest one -- from the operand itself."""
    case.check_straddle(table)
    whole = table if buf is None else buf
    assert whole.numel() * whole.element_size() > max(MARKS) > min(MARKS) >= 1 << 31
    off = case.mark_rows * table.stride(0) * table.element_size()
    for m in MARKS:
        assert (off < m).any() and (off >= m).any()


def _rows_off_value(y, value):
    """ids of the rows of ``y`` (2-D, row-strided, on the device) that differ anywhere from the row vector ``value``."""
    return torch.nonzero((y != value.unsqueeze(0)).any(1)).flatten().cpu().numpy()


# ====================================================================================================================
# Group A: tall tables
# ====================================================================================================================
SPMM = {   # name -> (values, mean, bias + relu, (out ld, first column)); f = 256 throughout
    "sum_values": (True, False, False, (256, 0)),          # float4 kernel with values
    "mean": (False, True, False, (260, 4)),                # float4 kernel, 16-byte aligned block of a wider buffer
    "bias_relu": (True, False, True, (257, 1)),            # scalar kernel (ldy % 4 != 0), four column passes
    "sum_unit": (False, False, False, (257, 1)),           # no stored values, scalar kernel
    "mean_values_bias_relu": (True, True, True, (256, 0)), # every option at once, float4 kernel
    "mean_unit_bias_relu": (False, True, True, (260, 4)),
}


@pytest.mark.parametrize("name", list(SPMM))
def test_spmm_tall_x_and_out(eps, dev, name):
    """ops.spmm_csr with ``x`` [n, 256] and ``out`` both beyond 4 GiB; the graph is over all n rows, only kept rows have entries.
    Kept rows: the twin's bits, the twin within gamma(deg (+1)) (|B| |x| + |bias|) of float64.  Every other row of the output is
    the empty row's value, over the WHOLE output; guard rows and columns keep the sentinel."""
    ops = eps.ops
    with_val, mean, epi, (ldy, c0) = SPMM[name]
    case = lo.TallCase(MARKS, 256, more_pitches=(ldy * 4,) if ldy != 256 else ())
    _need(dev, case.n_rows * (256 + ldy) * 4 + case.n_rows * 300)
    g = lo.tall_graph(case)
    x, _ = case.build(dev)
    out, obuf = lo.out_buffer(case.n_rows, ldy, c0, 256, dev)
    _beyond_marks(case, x)
    _beyond_marks(case, out, obuf)
    rowptr, col, val = lo.tall_graph_device(case, g, dev)
    rng = np.random.default_rng(7)
    bias = rng.standard_normal(256).astype(np.float32) if epi else None
    bd = None if bias is None else _t(bias, dev)
    y = ops.spmm_csr(rowptr, col, val if with_val else None, x, bias=bd, relu=epi, mean=mean, out=out)
    assert y.data_ptr() == out.data_ptr()
    # the twin: the kept rows at low offsets
    T = lo.tall_graph_twin(case, g)
    tw = ops.spmm_csr(_t(T.indptr.astype(np.int64), dev), _t(T.indices.astype(np.int32), dev),
                      _t(T.data.astype(np.float32), dev) if with_val else None, case.twin(dev), bias=bd, relu=epi, mean=mean)
    kept = _t(case.rows, dev)
    assert _same_bits(out[kept], tw), "a kept row differs from the same row at low offsets"
    B = T if with_val else lt._pattern(T)
    worst = _ratio(tw.cpu().numpy(), lt.spmm(B, case.values, bias, epi, mean), lt.spmm_bound(B, case.values, bias, mean, extra=int(epi)))
    # every row without entries, over the whole output
    empty = torch.zeros(256, device=dev) if bias is None else torch.relu(bd)
    off = _rows_off_value(out, empty)
    assert np.array_equal(off, g["rows"]), (len(off), len(g["rows"]))      # (no row of 256 random sums equals the empty row's value)
    assert _same_bits(out[_t(case.samples(), dev)], empty.expand(len(case.samples()), 256))
    assert lo.guards_intact(obuf, out)
    print(f"\nLO spmm tall {name}: {case.n_rows} rows, x {x.numel() * 4 / GIB:.2f} GiB, out {obuf.numel() * 4 / GIB:.2f} GiB, "
          f"largest error / bound {worst:.3f}")
    assert worst <= 1.0


def test_spmm_tall_hop_block_of_one_buffer(eps, dev):
    """TAGConv.hops' call: ``x`` and ``out`` are 64-column blocks of ONE buffer [n, 192] beyond 4 GiB.  The third block keeps its
    sentinel, the x block its values."""
    ops = eps.ops
    k = 64
    case = lo.TallCase(MARKS, 3 * k, k)
    _need(dev, case.n_rows * 3 * k * 4 + case.n_rows * 300)
    g = lo.tall_graph(case)
    x, buf = case.build(dev)
    words = buf.view(I32)
    words[:, k:] = lo.SENTINEL
    out = buf[:, k:2 * k]
    _beyond_marks(case, x, buf)
    _beyond_marks(case, out, buf)
    rowptr, col, val = lo.tall_graph_device(case, g, dev)
    ops.spmm_csr(rowptr, col, val, x, out=out)
    T = lo.tall_graph_twin(case, g)
    tw = ops.spmm_csr(_t(T.indptr.astype(np.int64), dev), _t(T.indices.astype(np.int32), dev), _t(T.data.astype(np.float32), dev), case.twin(dev))
    kept = _t(case.rows, dev)
    assert _same_bits(out[kept], tw)
    worst = _ratio(tw.cpu().numpy(), lt.spmm(T, case.values), lt.spmm_bound(T, case.values))
    off = _rows_off_value(out, torch.zeros(k, device=dev))
    assert np.array_equal(off, g["rows"]), (len(off), len(g["rows"]))
    assert bool((words[:, 2 * k:] == lo.SENTINEL).all()) and not bool((words[:, k:2 * k] == lo.SENTINEL).any())
    assert _same_bits(x[kept], case.twin(dev))
    print(f"\nLO spmm tall hop block: {case.n_rows} rows, one buffer of {buf.numel() * 4 / GIB:.2f} GiB, largest error / bound {worst:.3f}")
    assert worst <= 1.0


GEMM = {   # name -> (lda, ldc, first column of out, bias + relu, accumulate)
    "aligned": (256, 256, 0, False, False),                # gemm_f32_kernel<true>
    "unaligned_ld": (257, 257, 1, True, False),            # general template: dword loads of A, scalar epilogue
    "accumulate": (256, 256, 0, False, True),
}


@pytest.mark.parametrize("name", list(GEMM))
def test_gemm_tall_a_and_out(eps, dev, name):
    """ops.gemm with ``a`` [M, 256] and ``out`` [M, 256] both beyond 4 GiB.  Live rows: the twin's bits, the twin within the
    project's (K + 2) U (|a| |b|^T + |bias|) (+ |C| and one unit under accumulate) of float64.  Ballast rows are periodic, so the
    WHOLE output is compared on the device with the product of one ballast block: exactly the live rows differ."""
    ops = eps.ops
    lda, ldc, c0, epi, acc = GEMM[name]
    case = lo.TallCase(MARKS, lda, 256, more_pitches=(ldc * 4,) if ldc != lda else ())
    _need(dev, case.n_rows * (lda + ldc) * 4 + 3 * case.n_rows * 256)
    a, abuf = case.build(dev)
    _beyond_marks(case, a, abuf)
    rng = np.random.default_rng(11)
    b = (rng.standard_normal((256, 256)) / 16).astype(np.float32)
    bias = rng.standard_normal(256).astype(np.float32) if epi else None
    bd, biasd = _t(b, dev), None if bias is None else _t(bias, dev)
    if acc:
        out, obuf = case.build(dev)                       # C starts as a second copy of the table
        c0_twin, c0_host = case.twin(dev), case.values
    else:
        out, obuf = lo.out_buffer(case.n_rows, ldc, c0, 256, dev)
        c0_twin = c0_host = None
    _beyond_marks(case, out, obuf)
    ops.gemm(a, bd, bias=biasd, relu=epi, out=out, accumulate=acc)
    tw = ops.gemm(case.twin(dev), bd, bias=biasd, relu=epi, out=c0_twin, accumulate=acc)
    kept = _t(case.rows, dev)
    assert _same_bits(out[kept], tw), "a kept row differs from the same row at low offsets"
    worst = _ratio(tw.cpu().numpy(), lt.gemm(case.values, b, bias, epi, c0_host), lt.gemm_bound(case.values, b, bias, c0_host))
    # the whole output against the product of one ballast block
    nb = case.ballast_rows
    block = _t(lo.ballast_values(np.arange(nb), 256), dev)
    ref = ops.gemm(block, bd, bias=biasd, relu=epi, out=block.clone() if acc else None, accumulate=acc)
    full = case.n_rows // nb
    neq = (out[:full * nb].unflatten(0, (full, nb)) != ref.unsqueeze(0)).any(-1).flatten()
    tail = (out[full * nb:] != ref[:case.n_rows - full * nb]).any(-1)
    off = torch.nonzero(torch.cat([neq, tail])).flatten().cpu().numpy()
    assert np.array_equal(off, case.live), (len(off), len(case.live))
    if not acc:
        assert lo.guards_intact(obuf, out)
    print(f"\nLO gemm tall {name}: M = {case.n_rows}, a {abuf.numel() * 4 / GIB:.2f} GiB, out {obuf.numel() * 4 / GIB:.2f} GiB, "
          f"largest error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("hdim,layers", [(256, 5), (260, 4)])
def test_decode_tall_h(eps, dev, hdim, layers):
    """ops.mlp_decode (the narrow kernel at H = 256, the wide one at H = 260, whose pitch does not divide the marks) gathering
    rows of ``h`` beyond 4 GiB: u and v run over the mark rows, further live rows and ballast rows; 197 pairs (a tile tail of
    both kernels).  The twin's bits; the twin within the decode tests' tolerance of float64 (logits 2e-5 max(1, max |logit|),
    probabilities rel_err 1e-5)."""
    ops = eps.ops
    case = lo.TallCase(MARKS, hdim)
    _need(dev, case.n_rows * hdim * 4)
    h, _ = case.build(dev)
    assert h.is_contiguous()
    _beyond_marks(case, h)
    c = lt.decode_case(hdim, layers)
    ws, bs = [_t(w, dev) for w in c["ws"]], [_t(b, dev) for b in c["bs"]]
    rng = np.random.default_rng(13)
    m = case.mark_rows
    u = np.concatenate([m, rng.choice(case.rows, 197 - len(m))])
    v = np.concatenate([rng.choice(case.rows, 197 - len(m)), m[::-1]])
    assert len(u) == len(v) == 197 and 197 % lt.NARROW_TILE and 197 % lt.WIDE_TILE
    for mm in MARKS:
        for ids in (u, v):
            assert (ids * case.pitch < mm).any() and ((ids + 1) * case.pitch > mm).any() and (ids * case.pitch >= mm).any()
    ud, vd = _t(u.astype(np.int32), dev), _t(v.astype(np.int32), dev)
    uc, vc = case.twin_ids(u), case.twin_ids(v)
    ht = case.twin(dev)
    worst = {}
    for sig in (False, True):
        got = ops.mlp_decode(h, ud, vd, ws, bs, apply_sigmoid=sig)
        tw = ops.mlp_decode(ht, _t(uc.astype(np.int32), dev), _t(vc.astype(np.int32), dev), ws, bs, apply_sigmoid=sig)
        assert _same_bits(got, tw), sig
        logit, prob = lt.decode(case.values, uc, vc, c["ws"], c["bs"])
        if sig:
            worst["prob"] = rel_err(tw.cpu().numpy(), prob) / 1e-5
        else:
            worst["logit"] = float(np.abs(tw.cpu().numpy() - logit).max()) / (2e-5 * max(1.0, float(np.abs(logit).max())))
    print(f"\nLO decode tall H={hdim}: {case.n_rows} rows, h {h.numel() * 4 / GIB:.2f} GiB, error / tolerance logits "
          f"{worst['logit']:.3f}, probabilities {worst['prob']:.3f}")
    assert worst["logit"] <= 1.0 and worst["prob"] <= 1.0


def test_decode_train_and_backward_tall_h(eps, dev):
    """ops.mlp_decode_train gathering rows of ``h`` [n, 256] beyond 4 GiB and ops.mlp_decode_backward writing its gradient, a
    second table of that size.  Three layers with dropout masks; 197 pairs over the mark rows, further kept rows, a self pair and
    a duplicated pair.  Scores, parameter gradients and the kept rows of grad_h: the twin's bits (grad_h sums a node's incidences
    in the order of a stable sort of cat(u, v), which the monotone remap keeps).  The twin within the training decode's own bars
    of float64: scores 1e-5, gradients by decode_train_cases.check_grads.  Every row of grad_h without an incidence is zero,
    over the WHOLE table."""
    import decode_train_cases as dc
    ops = eps.ops
    H, L, B = 256, 3, 197
    case = lo.TallCase(MARKS, H)
    _need(dev, 2 * case.n_rows * H * 4 + case.n_rows * 64)
    h, _ = case.build(dev)
    assert h.is_contiguous()
    _beyond_marks(case, h)
    _, _, ws, bs, keep = dc.make_case(H, L, B, 4242)
    rng = np.random.default_rng(43)
    m = case.mark_rows
    u = np.concatenate([m, rng.choice(case.rows, B - len(m))])
    v = np.concatenate([rng.choice(case.rows, B - len(m)), m[::-1]])
    v[0] = u[0]                                                            # a self pair
    u[2], v[2] = u[1], v[1]                                                # the same pair twice
    for mm in MARKS:
        for ids in (u, v):
            assert (ids * case.pitch < mm).any() and ((ids + 1) * case.pitch > mm).any() and (ids * case.pitch >= mm).any()
    uc, vc = case.twin_ids(u), case.twin_ids(v)
    i32 = lambda a: _t(np.asarray(a).astype(np.int32), dev)               # noqa: E731
    wd, bd, kw = [w.to(dev) for w in ws], [b.to(dev) for b in bs], ops.pack_mask(keep.to(dev))
    ht = case.twin(dev)

    def run(table, a, b):
        out, taken = ops.mlp_decode_train(table, a, b, wd, bd, keep=kw, keep_scale=2.0, want_taken=True)
        leaf = out.clone().requires_grad_(True)
        dc.loss_of(leaf).backward()
        return out, taken, ops.mlp_decode_backward(table, a, b, wd, bd, leaf.grad.contiguous(), keep=kw, keep_scale=2.0)

    out, taken, (gh, gw, gb) = run(h, i32(u), i32(v))
    assert gh.shape == h.shape and gh.is_contiguous()
    _beyond_marks(case, gh)
    tout, ttaken, (tgh, tgw, tgb) = run(ht, i32(uc), i32(vc))
    assert _same_bits(out, tout) and torch.equal(taken, ttaken)
    assert all(_same_bits(a, b) for a, b in zip(gw + gb, tgw + tgb))
    assert _same_bits(gh[_t(case.rows, dev)], tgh), "a kept row of grad_h differs from the same row at low offsets"
    touched = torch.nonzero(gh.view(I32).any(1)).flatten().cpu().numpy()
    assert np.array_equal(touched, np.unique(np.concatenate([u, v])))
    # the twin against float64
    ht_cpu, edges = torch.from_numpy(case.values), torch.from_numpy(np.stack([uc, vc]))
    ref = dc.decode_forward(ht_cpu.double(), edges, [w.double() for w in ws], [b.double() for b in bs], keep, 2.0)
    err = float((tout.double().cpu() - ref).abs().max())
    branch = list(ops.unpack_mask(ttaken, H).cpu())
    g64 = dc.reference_grads(ht_cpu, edges, ws, bs, keep, 2.0, branch, torch.float64)
    g32 = dc.reference_grads(ht_cpu, edges, ws, bs, keep, 2.0, branch, torch.float32)
    got = {"h": tgh}
    got.update({f"w{i}": g for i, g in enumerate(tgw)})
    got.update({f"b{i}": g for i, g in enumerate(tgb)})
    print(f"\nLO decode train tall: {case.n_rows} rows, h and grad_h {h.numel() * 4 / GIB:.2f} GiB each, max |scores - f64| {err:.3g}")
    assert err <= 1e-5
    dc.check_grads("LO decode train tall", got, g64, g32)


def test_decode_bf16_tall_h(eps, dev):
    """ops.mlp_decode_bf16 gathering rows of a bf16 ``h`` [n, 256] beyond 4 GiB (twice the rows of the float32 table; built by
    ops.to_bf16 from the float32 case, whose kept rows must come out as the host's round-to-nearest-even bits).  Two layers, where
    the only rounding to bf16 is the deterministic Hadamard one: the twin's bits, and the twin within the bf16 decode's own bar
    (1e-5 of the sum of the magnitudes of the final dot's terms) of the float64 emulation of its rounding points."""
    from test_decode_bf16_host import emulate_decode_bf16, rne_bf16_bits
    ops = eps.ops
    H = 256
    case = lo.TallCase(MARKS, H, itemsize=2)
    _need(dev, case.n_rows * H * (4 + 2))
    x, _ = case.build(dev)
    h = ops.to_bf16(x)
    del x
    assert h.is_contiguous() and h.dtype == torch.int16
    _beyond_marks(case, h)
    i16 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16))                  # noqa: E731
    hb = rne_bf16_bits(case.values)
    assert torch.equal(h[_t(case.rows, dev)].cpu(), i16(hb))
    g = torch.Generator().manual_seed(29)
    ws = [rne_bf16_bits((torch.randn(H, H, generator=g) / H ** 0.5).numpy()), (torch.randn(1, H, generator=g) / H ** 0.5).numpy()]
    bs = [(torch.randn(H, generator=g) * 0.1).numpy(), (torch.randn(1, generator=g) * 0.1).numpy()]
    dw, db = [i16(ws[0]).to(dev), _t(ws[1], dev)], [_t(b, dev) for b in bs]
    rng = np.random.default_rng(31)
    m = case.mark_rows
    u = np.concatenate([m, rng.choice(case.rows, 197 - len(m))])
    v = np.concatenate([rng.choice(case.rows, 197 - len(m)), m[::-1]])
    uc, vc = case.twin_ids(u), case.twin_ids(v)
    got = ops.mlp_decode_bf16(h, _t(u.astype(np.int32), dev), _t(v.astype(np.int32), dev), dw, db, apply_sigmoid=False)
    tw = ops.mlp_decode_bf16(i16(hb).to(dev), _t(uc.astype(np.int32), dev), _t(vc.astype(np.int32), dev), dw, db, apply_sigmoid=False)
    assert _same_bits(got, tw)
    want, tsum = emulate_decode_bf16(hb, uc, vc, ws, bs)
    err = float((np.abs(tw.cpu().numpy().astype(np.float64) - want) / tsum).max())
    print(f"\nLO decode bf16 tall: {case.n_rows} rows, h {h.numel() * 2 / GIB:.2f} GiB, max err / sum|terms| {err:.3e} (bar 1e-5)")
    assert err <= 1e-5


def _symmetric_tall_graph(case, dev):
    """tall_graph and its mirror: a SYMMETRIC unit pattern over the kept rows -> (P scipy CSR over the twin's ids, the table
    rows that hold entries, rowptr / col over all n rows on the device, rowptr / col of the twin on the device).  The big graph
    stores the same entries in the same order as the twin, so entry positions (reverse positions too) are the twin's."""
    T = lo.tall_graph_twin(case, lo.tall_graph(case))
    P = ((T + T.T) != 0).astype(np.float64).tocsr()
    P.sort_indices()
    assert (abs(P - P.T)).nnz == 0 and P.nnz > T.nnz
    with_entries = case.rows[np.diff(P.indptr) > 0]
    assert set(case.mark_rows) <= set(with_entries)
    deg = torch.zeros(case.n_rows + 1, dtype=torch.int64, device=dev)
    deg[_t(case.rows + 1, dev)] = _t(np.diff(P.indptr).astype(np.int64), dev)
    rowptr, col = torch.cumsum(deg, 0), _t(case.rows[P.indices].astype(np.int32), dev)
    return P, with_entries, rowptr, col, _t(P.indptr.astype(np.int64), dev), _t(P.indices.astype(np.int32), dev)


def test_cosine_features_backward_tall(eps, dev):
    """ops.cos_features_backward with ``xhat`` and the returned gradient [n, 256] beyond 4 GiB (and ``x`` of the forward that
    made xhat and nrm), on the symmetric pattern of tall_graph and its mirror with its reverse positions, for a random dL/dc.
    Kept rows: the twin's bits; the twin within the cosine training tests' bar (grad_tolerance) of the float64 closed form.
    A row without entries gets a zero gradient, over the WHOLE table."""
    from test_cosine_train_host import cosine_grad_truth, grad_tolerance
    ops = eps.ops
    F = 256
    case = lo.TallCase(MARKS, F)
    _need(dev, 3 * case.n_rows * F * 4 + case.n_rows * (F + 200))
    P, with_entries, rowptr, col, trp, tcol = _symmetric_tall_graph(case, dev)
    M = ssp.csr_matrix((np.arange(P.nnz) + 1.0, P.indices, P.indptr), shape=P.shape).T.tocsr()
    M.sort_indices()
    mirror = (M.data - 1).astype(np.int64)                                  # entry e = (i, j) -> the entry (j, i)
    row = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    assert np.array_equal(P.indices[mirror], row) and np.array_equal(row[mirror], P.indices)
    revpos_np = (mirror - P.indptr[P.indices]).astype(np.int32)             # include/eps_abi.h: its position INSIDE row j
    assert (revpos_np >= 0).all() and (revpos_np < np.diff(P.indptr)[P.indices]).all()
    revpos = _t(revpos_np, dev)
    gc_np = np.random.default_rng(53).standard_normal(P.nnz).astype(np.float32)
    gce = _t(gc_np, dev)
    x, _ = case.build(dev)
    _beyond_marks(case, x)
    xhat, nrm = ops.cos_node_features(rowptr, col, None, x, want_norm=True)
    del x
    _beyond_marks(case, xhat)
    gxp = ops.cos_features_backward(rowptr, col, None, xhat, nrm, revpos, gce)
    assert gxp.stride(0) == F
    _beyond_marks(case, gxp)
    txhat, tnrm = ops.cos_node_features(trp, tcol, None, case.twin(dev), want_norm=True)
    tg = ops.cos_features_backward(trp, tcol, None, txhat, tnrm, revpos, gce)
    kept = _t(case.rows, dev)
    assert _same_bits(xhat[kept], txhat) and _same_bits(nrm[kept], tnrm)
    assert _same_bits(gxp[kept], tg), "a kept row of the gradient differs from the same row at low offsets"
    Gd = np.zeros(P.shape)
    Gd[row, P.indices] = gc_np
    t = cosine_grad_truth(P, case.values.astype(np.float64), np.zeros((2, 0), np.int64), np.zeros(0), gc_given=Gd)
    truth, mag = t["gxp"]
    got = tg.cpu().numpy()
    assert np.isfinite(got).all()
    worst = float((np.abs(got.astype(np.float64) - truth) / grad_tolerance(mag, F, 1.0)).max())
    touched = torch.nonzero((gxp != 0).any(1)).flatten().cpu().numpy()
    assert np.array_equal(touched, with_entries), (len(touched), len(with_entries))
    print(f"\nLO cosine backward tall: {case.n_rows} rows, xhat and gradient {gxp.numel() * 4 / GIB:.2f} GiB each, {P.nnz} entries, "
          f"largest error / bar {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("heads", [1, 8])
def test_gat_aggregate_and_backward_tall(eps, dev, heads):
    """ops.gat_aggregate and ops.gat_aggregate_backward with ``z``, ``out`` (= ``out_nobias``), ``gout`` and the returned gz all
    [n, 256] beyond 4 GiB, on a SYMMETRIC pattern over the kept rows (tall_graph and its mirror).  The scores are regime
    "quarters" of gat_truth (no raw score near the LeakyReLU kink), a function of the row id.  Kept rows: the twin's bits; the
    twin within gat_truth's forward and backward bounds.  A row without entries attends to itself alone: out = z and gz = gout
    there, over the WHOLE tables."""
    import gat_truth as gt
    ops = eps.ops
    F = 256
    case = lo.TallCase(MARKS, F)
    _need(dev, 4 * case.n_rows * F * 4 + case.n_rows * (F + 200))
    P, with_entries, rowptr, col, trp, tcol = _symmetric_tall_graph(case, dev)
    k = len(case.rows)

    def scores(ids, hh):
        r, hh = ids[:, None], hh[None, :]
        return ((r * 5 + hh * 3) % 17 - 8) / 4.0, ((r * 7 + hh) % 17 - 8) / 4.0 + 0.125

    s_src, s_dst = (t.to(torch.float32) for t in scores(torch.arange(case.n_rows, device=dev), torch.arange(heads, device=dev)))
    ts, td = (t.astype(np.float32) for t in scores(case.rows, np.arange(heads)))
    z, _ = case.build(dev)
    _beyond_marks(case, z)
    out, lse = ops.gat_aggregate(rowptr, col, z, s_src, s_dst, heads, want_lse=True)
    _beyond_marks(case, out)
    kept = _t(case.rows, dev)
    tout, tlse = ops.gat_aggregate(trp, tcol, case.twin(dev), _t(ts, dev), _t(td, dev), heads, want_lse=True)
    assert _same_bits(out[kept], tout) and _same_bits(lse[kept], tlse), "a kept row differs from the same row at low offsets"
    fw = gt.aggregate(P.indptr.astype(np.int64), P.indices, case.values, ts, td, heads, parts=True)
    worst = {"out": float((np.abs(tout.cpu().numpy() - fw["out"]) / np.maximum(fw["bound"], 1e-300)).max()),
             "lse": float((np.abs(tlse.cpu().numpy() - fw["lse"]) / np.maximum(fw["lse_bound"], 1e-300)).max())}
    differ = torch.nonzero((out != z).any(1)).flatten().cpu().numpy()
    assert np.array_equal(differ, with_entries), (len(differ), len(with_entries))
    # backward: gout a second tall table with its own kept rows
    gvals = np.random.default_rng(47).standard_normal((k, F)).astype(np.float32)
    gout, _ = case.build(dev)
    gout[kept] = _t(gvals, dev)
    _beyond_marks(case, gout)
    gz, gs, gd = ops.gat_aggregate_backward(rowptr, col, z, s_src, s_dst, heads, lse, out, gout)
    assert gz.is_contiguous() and gz.shape == z.shape
    _beyond_marks(case, gz)
    tgz, tgs, tgd = ops.gat_aggregate_backward(trp, tcol, case.twin(dev), _t(ts, dev), _t(td, dev), heads, tlse, tout, _t(gvals, dev))
    assert _same_bits(gz[kept], tgz) and _same_bits(gs[kept], tgs) and _same_bits(gd[kept], tgd)
    tr = gt.aggregate_backward(P.indptr.astype(np.int64), P.indices, case.values, ts, td, heads, tout.cpu().numpy(), gvals)
    for name, got in (("gz", tgz), ("g_s_src", tgs), ("g_s_dst", tgd)):
        worst[name] = float((np.abs(got.double().cpu().numpy() - tr[name]) / np.maximum(tr[name + "_bound"], 1e-300)).max())
        assert tr[name + "_bound"].max() <= 1e-2 * float(np.abs(tr[name]).max())
    differ = torch.nonzero((gz != gout).any(1)).flatten().cpu().numpy()
    assert np.array_equal(differ, with_entries), (len(differ), len(with_entries))
    print(f"\nLO gat tall heads={heads}: {case.n_rows} rows, four tables of {z.numel() * 4 / GIB:.2f} GiB, {P.nnz} entries, "
          f"largest error / bound {({a: round(b, 3) for a, b in worst.items()})}")
    assert max(worst.values()) <= 1.0


def test_cosine_features_and_edge_cosines_tall(eps, dev):
    """ops.cos_node_features with ``x`` [n, 256] and its output ``xhat`` both beyond 4 GiB, then ops.edge_cosines gathering rows of
    that xhat.  Kept rows and their entries: the twin's bits, the twin within the cosine tests' bars of float64 (xhat 1e-5
    (1 + F / 64) (|terms| + 1e-3), cosines 1e-5 (2 + F / 64) (|terms| + 1e-3)).  A row without entries is x / ||x||: ballast
    rows are periodic, so the WHOLE xhat is compared on the device with the kernel's output for one ballast block."""
    from test_cosine_cn_host import edge_cosines_truth, smoothed_unit_features
    ops = eps.ops
    F = 256
    case = lo.TallCase(MARKS, F)
    _need(dev, case.n_rows * F * 4 * 2 + case.n_rows * (F + 300))
    g = lo.tall_graph(case)
    x, _ = case.build(dev)
    _beyond_marks(case, x)
    rowptr, col, val = lo.tall_graph_device(case, g, dev)
    xhat = ops.cos_node_features(rowptr, col, val, x)
    assert xhat.stride(0) == F
    _beyond_marks(case, xhat)
    c = ops.edge_cosines(rowptr, col, xhat)
    T = lo.tall_graph_twin(case, g)
    trp, tcol, tval = _t(T.indptr.astype(np.int64), dev), _t(T.indices.astype(np.int32), dev), _t(T.data.astype(np.float32), dev)
    tw = ops.cos_node_features(trp, tcol, tval, case.twin(dev))
    kept = _t(case.rows, dev)
    assert _same_bits(xhat[kept], tw), "a kept row of xhat differs from the same row at low offsets"
    ctw = ops.edge_cosines(trp, tcol, tw)
    assert _same_bits(c, ctw), "an edge cosine differs from the same entry at low offsets"      # (same rows, same order: same entries)
    xv = case.values.astype(np.float64)
    truth = smoothed_unit_features(T, xv)
    deg = np.asarray(T.sum(1)).ravel() + 1e-6
    xp = xv + (T @ xv) / deg[:, None]
    mag = (np.abs(xv) + (T @ np.abs(xv)) / deg[:, None]) / np.maximum(np.linalg.norm(xp, axis=1), 1e-8)[:, None]
    worst_x = float((np.abs(tw.cpu().numpy() - truth) / (1e-5 * (1 + F / 64) * (mag + 1e-3))).max())
    c_truth, c_mag = edge_cosines_truth(T, truth)
    worst_c = float((np.abs(ctw.cpu().numpy() - c_truth) / (1e-5 * (2 + F / 64) * (c_mag + 1e-3))).max())
    # the whole xhat against one period of itself (a row without entries is x / ||x||, and the ballast is periodic): the first
    # block, its kept rows taken from the next period in which they are not kept; sampled rows of it against float64
    nb = case.ballast_rows
    ref = xhat[:nb].clone()
    low = case.rows[case.rows < nb]
    stand_in = low + nb
    while np.isin(stand_in, case.rows).any():
        stand_in = np.where(np.isin(stand_in, case.rows), stand_in + nb, stand_in)
    assert stand_in.max() < case.n_rows
    ref[_t(low, dev)] = xhat[_t(stand_in, dev)]
    smp = np.setdiff1d(np.arange(0, nb, 97), case.rows)
    bx = lo.ballast_values(smp, F).astype(np.float64)
    bn = np.maximum(np.linalg.norm(bx, axis=1), 1e-8)[:, None]
    worst_b = float((np.abs(ref[_t(smp, dev)].cpu().numpy() - bx / bn) / (1e-5 * (1 + F / 64) * (np.abs(bx) / bn + 1e-3))).max())
    assert worst_b <= 1.0, worst_b
    full = case.n_rows // nb
    neq = (xhat[:full * nb].unflatten(0, (full, nb)) != ref.unsqueeze(0)).any(-1).flatten()
    tail = (xhat[full * nb:] != ref[:case.n_rows - full * nb]).any(-1)
    off = torch.nonzero(torch.cat([neq, tail])).flatten().cpu().numpy()
    # exactly the live rows differ -- and the kept BALLAST rows that hold entries (none: tall_graph gives entries to live rows)
    assert set(g["rows"]) <= set(case.live) and np.array_equal(off, case.live), (len(off), len(case.live))
    print(f"\nLO cosine tall: {case.n_rows} rows, x and xhat {x.numel() * 4 / GIB:.2f} GiB each, {c.numel()} entries, error / bar "
          f"xhat {worst_x:.3f}, cosines {worst_c:.3f}")
    assert worst_x <= 1.0 and worst_c <= 1.0


def test_sketches_tall_tables(eps, dev):
    """ops.sketch_propagate and ops.sketch_pair_stats on n = 2^23 + 162 nodes: a MinHash table [n, 128] uint32 crosses 2^32
    bytes, a HyperLogLog table [n, 256] uint8 2^31, and in the [2, n, .] tables every row of the second hop lies beyond them
    (MinHash: beyond 2^32).  The graph gives entries to a few live rows (the mark rows among them, read and written).  Integers
    throughout: sketch_truth bit for bit, the twin bit for bit; a row without entries is the empty sketch in both hops, over the
    WHOLE tables."""
    import sketch_truth as st
    ops = eps.ops
    case = lo.TallCase(MARKS, st.P, itemsize=4)                     # the MinHash pitch: 512 bytes
    n = case.n_rows
    _need(dev, n * (256 + 512) * 3 + n * 700)
    g = lo.tall_graph(case)
    rowptr, col, _ = lo.tall_graph_device(case, g, dev)
    hll = torch.empty((2, n, st.R), dtype=torch.uint8, device=dev)
    mh = torch.empty((2, n, st.P), dtype=torch.uint32, device=dev)
    # beyond the marks, from the operands: the mark rows of the 512-byte pitch straddle 2^31 and 2^32 in mh[0], and -- at half
    # the pitch -- the rows at the upper mark straddle 2^31 in hll[0]; hop 2 starts beyond the upper mark (mh) / 2^31 (hll)
    case.check_straddle(mh[0].view(torch.int32))
    assert mh[0].numel() * 4 > MARKS[1] and hll[0].numel() > MARKS[0] and n * st.P * 4 > MARKS[1] and n * st.R > MARKS[0]
    top = np.array([case.roles[(k, MARKS[1])] for k in ("below", "at", "after")], np.int64)
    assert (top[0] + 1) * st.R == MARKS[0] == top[1] * st.R and np.isin(top, g["rows"]).all()
    own = ops.sketch_own(0, n, dev)
    ops.sketch_propagate(rowptr, col, n, own[0], own[1], keep_own=False, out=(hll[0], mh[0]))
    del own
    ops.sketch_propagate(rowptr, col, n, hll[0], mh[0], keep_own=True, out=(hll[1], mh[1]))
    # truth and twin: the kept rows alone, their own sketches those of their REAL ids
    T = lo.tall_graph_twin(case, g)
    k = len(case.rows)
    own_h, own_m = st.own_sketch(case.rows)
    h1 = st.propagate(T, own_h, own_m, keep_own=False)
    h2 = st.propagate(T, *h1, keep_own=True)
    th, tm = np.stack([h1[0], h2[0]]), np.stack([h1[1], h2[1]])
    trp, tcol = _t(T.indptr.astype(np.int64), dev), _t(T.indices.astype(np.int32), dev)
    thll = torch.empty((2, k, st.R), dtype=torch.uint8, device=dev)
    tmh = torch.empty((2, k, st.P), dtype=torch.uint32, device=dev)
    own_md = _t(own_m.view(np.int32), dev).view(torch.uint32)
    ops.sketch_propagate(trp, tcol, k, _t(own_h, dev), own_md, keep_own=False, out=(thll[0], tmh[0]))
    ops.sketch_propagate(trp, tcol, k, thll[0], tmh[0], keep_own=True, out=(thll[1], tmh[1]))
    kept = _t(case.rows, dev)
    mh32, tmh32 = mh.view(I32), tmh.view(I32)                       # (the same words, in a type torch indexes and compares)
    for hop in (0, 1):
        assert torch.equal(hll[hop][kept], thll[hop]) and torch.equal(mh32[hop][kept], tmh32[hop]), hop
        assert np.array_equal(thll[hop].cpu().numpy(), th[hop]) and np.array_equal(tmh32[hop].cpu().numpy().view(np.uint32), tm[hop]), hop
        # every row without entries is empty, over the whole table
        used = torch.nonzero((hll[hop] != 0).any(1)).flatten().cpu().numpy()
        assert np.array_equal(used, g["rows"]), hop
        used = torch.nonzero((mh32[hop] != -1).any(1)).flatten().cpu().numpy()
        assert np.array_equal(used, g["rows"]), hop
    # pair statistics: u and v over the mark rows, further graph rows and rows without entries
    rng = np.random.default_rng(37)
    m = case.mark_rows
    u = np.concatenate([m, rng.choice(g["rows"], 60), rng.choice(case.rows, 30)])
    v = np.concatenate([m[::-1], rng.choice(g["rows"], 60), rng.choice(g["rows"], 30)])
    uc, vc = case.twin_ids(u), case.twin_ids(v)
    S, Z, M = ops.sketch_pair_stats(hll, mh, n, _t(u.astype(np.int32), dev), _t(v.astype(np.int32), dev))
    tS, tZ, tM = ops.sketch_pair_stats(thll, tmh, k, _t(uc.astype(np.int32), dev), _t(vc.astype(np.int32), dev))
    assert torch.equal(S, tS) and torch.equal(Z, tZ) and torch.equal(M, tM)
    wS, wZ, wM = st.pair_stats(th, tm, uc, vc)
    assert np.array_equal(S.cpu().numpy(), wS) and np.array_equal(Z.cpu().numpy(), wZ) and np.array_equal(M.cpu().numpy(), wM)
    assert (wM > 0).any() and (wM < st.P).any() and (wZ < st.R).any()
    print(f"\nLO sketches tall: n = {n}, hll {hll.numel() / GIB:.2f} GiB, mh {mh.numel() * 4 / GIB:.2f} GiB, {len(u)} pairs: exact")


def test_to_bf16_beyond_2g_elements(eps, dev):
    """ops.to_bf16 on more than 2^31 elements: the input crosses 2^31, 2^32 and 2^33 bytes, the output 2^31 and 2^32.  The live
    rows (with ties and values next to ties in their first columns) against the host's round-to-nearest-even, bit for bit; the
    WHOLE output against torch's own conversion on the device, and the ballast -- exact in bfloat16 -- against its own high halves."""
    ops = eps.ops
    marks = MARKS + (1 << 33,)
    case = lo.TallCase(marks, 256)
    _need(dev, case.n_rows * 256 * (4 + 2 + 2 + 1))
    ties = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0x7F7FFFFF, 0x00000001, 0x80000000], np.uint32).view(np.float32)
    case.values[~case.is_ballast, :len(ties)] = ties
    x, _ = case.build(dev)
    case.check_straddle(x)
    assert x.is_contiguous() and x.numel() > 1 << 31 and x.numel() * 4 > 1 << 33
    out = ops.to_bf16(x)
    assert out.shape == x.shape and out.dtype == torch.int16 and out.numel() * 2 > 1 << 32
    off = case.mark_rows * out.stride(0) * out.element_size()              # (the output's pitch is half the input's: x's rows at
    for m in MARKS:                                                        #  2^32 and 2^33 are the output's rows at 2^31 and 2^32)
        assert (off + 512 == m).any() and (off == m).any() and out.stride(0) * out.element_size() == 512
    kept = _t(case.rows, dev)
    want = torch.from_numpy(case.values).to(torch.bfloat16).view(torch.int16)
    assert torch.equal(out[kept].cpu(), want)
    assert torch.equal(out[-1].cpu(), want[-1]) and torch.equal(out[0].cpu(), want[0])
    assert torch.equal(out, x.to(torch.bfloat16).view(torch.int16))
    smp = _t(case.samples(), dev)
    assert torch.equal(out[smp].to(I32), x[smp].view(I32) >> 16)
    print(f"\nLO to_bf16: {x.numel()} elements, x {x.numel() * 4 / GIB:.2f} GiB, out {out.numel() * 2 / GIB:.2f} GiB: exact")


# ====================================================================================================================
# Group B: long entry arrays
# ====================================================================================================================
L_RUN = 1 << 20
LENS = [1, 64, 129, 1025, 513, 2049, 2, 65, 128, 1024]      # every route of the generic pair kernel; rows 3 and 4 sit at the marks
B_ROW = 3


def _long_case(phase):
    return lo.LongCSR(MARKS, LENS, L_RUN, B_ROW, phase=phase)


def _beyond_entry_marks(case, rowptr, col, val=None):
    case.check_straddle(col)
    for t in (col, val):
        if t is not None:
            assert t.numel() * t.element_size() > max(MARKS)
    assert int(rowptr[-1]) == col.numel() > 1 << 30
    live_start = np.array([s for _, s, _, _ in case.live], np.int64) * 4
    live_end = live_start + np.array([len(c) for _, _, c, _ in case.live], np.int64) * 4
    for m in MARKS:
        assert ((live_start <= m) & (live_end >= m)).any() and (live_start > m).any() and (live_end < m).any()


def _twin_device(T, dev, weighted=True):
    return (_t(T.indptr.astype(np.int64), dev), _t(T.indices.astype(np.int32), dev), _t(T.data.astype(np.float32), dev) if weighted else None)


@pytest.fixture(scope="module")
def pair_limits(eps):
    from eps_amd import ops
    S, C, Q, R, _, _ = ops.pair_scores_limits()
    K, GQ, B, RING = ops.pair_scores_grouped_limits()
    return dict(S=S, C=C, R=R, K=K, B=B)


@pytest.mark.parametrize("kind", ["unit", "val"])
@pytest.mark.parametrize("phase", [0, 1])
def test_pair_scores_rows_beyond_the_marks(eps, dev, pair_limits, phase, kind):
    """ops.pair_scores, generic and column-run kernel, float32 and float64 weights, on pairs of rows that end at, start at and
    span the entry indices 2^29 and 2^30 (2^31 and 2^32 bytes of col / val), of rows far beyond them, and of ballast rows of
    2^20 entries.  The list goes beyond one chunk of the column-run kernel and covers every route of the generic one
    (asserted from ops.pair_scores_limits).  Counts exact; sums: the twin's bits, and within gamma(count + 2) sum |terms| of the
    extended-precision truth (cn: gamma(count + 1))."""
    ops = eps.ops
    weighted = kind == "val"
    case = _long_case(phase)
    _need(dev, case.nnz * (8 if weighted else 4) + 64 * case.n)
    rowptr, col, val = case.build(dev, weighted)
    _beyond_entry_marks(case, rowptr, col, val)
    T, keep = case.twin()
    u0, v0 = lo.pair_lists(case)
    deg = np.diff(case.rowptr)
    routes = {pt.route(deg[a], deg[b], pair_limits["S"], pair_limits["C"], pair_limits["R"]) for a, b in zip(u0, v0)}
    assert routes >= {"small", "one", "multi", "inplace"}, routes
    # every pair once, and the pairs of two live rows again and again until the list exceeds one chunk of the column-run kernel
    # (a pair with a ballast row walks 2^20 entries: those go in once, not a thousand times over)
    both_live = np.flatnonzero(np.isin(u0, case.live_rows) & np.isin(v0, case.live_rows))
    pick = np.concatenate([np.arange(len(u0)), np.tile(both_live, pair_limits["K"] // len(both_live) + 1)])
    pick = pick[np.argsort(v0[pick], kind="stable")]
    u, v = u0[pick], v0[pick]
    assert len(u) > pair_limits["K"] and (np.diff(v) >= 0).all() and case.n <= pair_limits["B"]
    ud, vd = _t(u, dev), _t(v, dev)
    trp, tcol, tval = _twin_device(T, dev, weighted)
    rng = np.random.default_rng(17)
    w64 = rng.uniform(0.05, 1.0, case.n).astype(np.float32).astype(np.float64)       # one table, exact in both precisions: one truth
    t = {key: x[pick] for key, x in lo.pair_truth(case, weighted, w64, u0, v0).items()}
    assert t["count"].max() >= 1 << 19 and (t["count"] == 0).any()
    worst = 0.0
    for dtype, gam in ((np.float32, pt.gamma), (np.float64, pt.gamma64)):
        wd = _t(w64.astype(dtype), dev)
        bound = gam(t["count"] + 2) * t["abs"]
        for grouped in (False, True):
            where = (phase, kind, dtype.__name__, "grouped" if grouped else "generic")
            count, cn, ws = ops.pair_scores(rowptr, col, val, wd, case.n, ud, vd, grouped=grouped)
            c2, cn2, ws2 = ops.pair_scores(trp, tcol, tval, wd, case.n, ud, vd, grouped=grouped)
            assert torch.equal(count, c2) and _same_bits(ws, ws2) and (cn is None or _same_bits(cn, cn2)), where
            assert np.array_equal(count.cpu().numpy(), t["count"]), where
            err = np.abs(ws.cpu().numpy().astype(np.float64) - t["ws"])
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
            assert (err <= bound).all(), where
            if cn is not None:
                assert (np.abs(cn.cpu().numpy().astype(np.float64) - t["cn"]) <= pt.gamma(t["count"] + 1) * t["abs_cn"]).all(), where
    print(f"\nLO pair_scores phase {phase} {kind}: nnz {case.nnz}, {len(u)} pairs, routes {sorted(routes)}, largest error / bound {worst:.4f}")


@pytest.mark.parametrize("phase", [0, 1])
def test_rescore_weighted_rows_beyond_the_marks(eps, dev, phase):
    """ops.rescore_weighted (64-bit entry indices) on the same rows: float32 of the int64 sum of the 2^-40 fixed-point terms, bit
    for bit the truth's (weighted_truth.pair_exact) and the twin's."""
    ops = eps.ops
    case = _long_case(phase)
    _need(dev, case.nnz * 8 + 64 * case.n)
    rowptr, col, val = case.build(dev)
    _beyond_entry_marks(case, rowptr, col, val)
    T, _ = case.twin()
    u, v = lo.pair_lists(case)
    # eps_rescore_weighted has ONE path and no *_limits entry point (ops.rescore_limits are eps_rescore_runs', which refuses a
    # graph of this size -- Group C): the shorter row goes over the 64 lanes, each entry searched in the longer one.  What can
    # differ is which row is the shorter and how many trips of 64 it takes: below, exactly and above one trip, either way round.
    deg = np.diff(case.rowptr)
    short = np.minimum(deg[u], deg[v])
    at_mark = np.isin(u, np.concatenate(case.set_rows[:2])) | np.isin(v, np.concatenate(case.set_rows[:2]))
    for name, m in (("under a trip", short < 64), ("one trip", short == 64), ("a trip and one", short == 65), ("many trips", short > 1024)):
        assert (m & at_mark & (deg[u] <= deg[v])).any() and (m & at_mark & (deg[u] > deg[v])).any(), name
    w = np.random.default_rng(19).uniform(0.05, 1.0, case.n).astype(np.float32)
    keys = _t((u.astype(np.int64) << 32) | v.astype(np.int64), dev)
    got = ops.rescore_weighted(rowptr, col, val, _t(w, dev), case.n, keys)
    tw = ops.rescore_weighted(*_twin_device(T, dev), _t(w, dev), case.n, keys)
    assert _same_bits(got, tw)
    live = np.isin(u, case.live_rows) & np.isin(v, case.live_rows)
    check = np.concatenate([np.flatnonzero(live), np.flatnonzero(~live)[::9][:24]])
    tr, tc, tv = T.indptr.astype(np.int64), T.indices, T.data
    want = np.array([wt.pair_exact(tr, tc, tv, w, u[i], v[i]) for i in check], np.float32)
    assert np.array_equal(got.cpu().numpy()[check].view(np.int32), want.view(np.int32))
    assert (want > 0).sum() > 100 and len(check) > live.sum() > 0
    print(f"\nLO rescore_weighted phase {phase}: nnz {case.nnz}, {len(u)} pairs, {len(check)} against the fixed-point truth: exact")


@pytest.mark.parametrize("phase", [0, 1])
def test_pair_cn_list_rows_beyond_the_marks(eps, dev, phase):
    """ops.pair_cn_list, count and fill, on the same pairs: pointers and lists equal the twin's, and the truth's -- cn_list_truth.cn_lists
    for the pairs of two live rows; for a pair with a ballast row (the ramp 0 .. l - 1) the other row's ids below l."""
    import cn_list_truth as cl
    ops = eps.ops
    case = _long_case(phase)
    _need(dev, case.nnz * 4 + 64 * case.n)
    rowptr, col, _ = case.build(dev, weighted=False)
    _beyond_entry_marks(case, rowptr, col)
    T, _ = case.twin()
    u, v = lo.pair_lists(case)
    # every path of the walk (ops.pair_cn_list_limits): the long row staged in one pass, in several, searched in place
    cap, ratio = ops.pair_cn_list_limits()
    deg = np.diff(case.rowptr)
    short, long_ = np.minimum(deg[u], deg[v]), np.maximum(deg[u], deg[v])
    at_mark = np.isin(u, case.set_rows[0]) | np.isin(u, case.set_rows[1])
    for name, m in (("one pass", long_ <= cap), ("several passes", (long_ > cap) & (long_ < ratio * short)),
                    ("in place", (long_ > cap) & (long_ >= ratio * short))):
        assert (m & at_mark & (short > 0)).any(), name
    assert (long_ == cap).any() and (long_ == cap + 1).any()
    ud, vd = _t(u, dev), _t(v, dev)
    ptr, w = ops.pair_cn_list(rowptr, col, case.n, ud, vd)
    trp, tcol, _ = _twin_device(T, dev, weighted=False)
    ptr2, w2 = ops.pair_cn_list(trp, tcol, case.n, ud, vd)
    assert torch.equal(ptr, ptr2) and torch.equal(w, w2)
    live = np.isin(u, case.live_rows) & np.isin(v, case.live_rows)
    lptr, lw = cl.cn_lists(T, u[live], v[live])
    segs, j = [], 0
    for i in range(len(u)):
        if live[i]:
            segs.append(lw[lptr[j]:lptr[j + 1]]); j += 1
        else:
            (ca, _), (cb, _) = case.row(int(u[i])), case.row(int(v[i]))
            a_ramp, b_ramp = u[i] not in case.live_rows, v[i] not in case.live_rows
            segs.append(np.arange(min(len(ca), len(cb)), dtype=np.int32) if a_ramp and b_ramp else cb[cb < len(ca)] if a_ramp else ca[ca < len(cb)])
    want_ptr = np.concatenate([[0], np.cumsum([len(x) for x in segs])])
    assert np.array_equal(ptr.cpu().numpy(), want_ptr) and np.array_equal(w.cpu().numpy(), np.concatenate(segs))
    assert (~live).sum() > 20 and max(len(x) for x in segs) == L_RUN
    print(f"\nLO pair_cn_list phase {phase}: nnz {case.nnz}, {len(u)} pairs, {len(w)} listed ids: exact")


@pytest.mark.parametrize("phase", [0, 1])
def test_local_community_degrees_rows_beyond_the_marks(eps, dev, phase):
    """ops.local_community_degrees on the lists ops.pair_cn_list gives for the same pairs (all but the pairs of two ballast rows,
    whose list of 2^20 members -- a thousand of them rows of 2^20 entries -- is a pass of its own): the rows of the members that
    are live rows lie at, across and beyond the marks, those that are ballast rows are searched in place.  Integers: equal to
    local_community_truth.gammas restated from the host data (lo.gammas_truth).  (gamma needs the row of EVERY member, ballast
    rows included, so the compacted twin is another problem: no twin here.)  Paths, from ops.local_community_limits: short
    lists, one staged pass, several passes, a member searched in place."""
    ops = eps.ops
    case = _long_case(phase)
    _need(dev, case.nnz * 4 + 64 * case.n)
    rowptr, col, _ = case.build(dev, weighted=False)
    _beyond_entry_marks(case, rowptr, col)
    u, v = lo.pair_lists(case)
    some_live = np.isin(u, case.live_rows) | np.isin(v, case.live_rows)
    u, v = u[some_live], v[some_live]
    ptr, w = ops.pair_cn_list(rowptr, col, case.n, _t(u, dev), _t(v, dev))
    gamma = ops.local_community_degrees(rowptr, col, case.n, ptr, w)
    hp, hw = ptr.cpu().numpy(), w.cpu().numpy()
    short, cap, ratio = ops.local_community_limits()
    cnt, deg = np.diff(hp), np.diff(case.rowptr)
    staged = np.minimum(np.repeat(cnt, cnt), cap)
    assert ((cnt > 0) & (cnt <= short)).any() and ((cnt > short) & (cnt <= cap)).any() and (cnt > cap).any()
    assert (deg[hw] >= ratio * staged).any() and ((deg[hw] > 0) & (deg[hw] < ratio * staged)).any()
    at_mark = np.isin(hw, np.concatenate(case.set_rows[:2]))
    assert at_mark.any() and np.isin(hw, case.set_rows[-1]).any()
    want = lo.gammas_truth(case, hp, hw)
    got = gamma.cpu().numpy()
    assert np.array_equal(got, want)
    assert want[at_mark].max() > 0 and want.max() > 8
    print(f"\nLO local_community_degrees phase {phase}: nnz {case.nnz}, {len(u)} lists, {len(hw)} members, largest gamma {int(want.max())}: exact")


@pytest.mark.parametrize("phase", [0, 1])
def test_spmm_narrow_x_over_a_long_entry_array(eps, dev, phase):
    """ops.spmm_csr with x [n, 4] over col / val of more than 4 GiB each -- a whole pass.  The twin's rows (live rows and the
    kept ballast rows) bit for bit; the twin within gamma(deg) |B| |x| of float64; every full ballast row of the big graph
    equals the first one; the rows after the last stored one are zero."""
    ops = eps.ops
    case = _long_case(phase)
    _need(dev, case.nnz * 8 + 64 * case.n)
    rowptr, col, val = case.build(dev)
    _beyond_entry_marks(case, rowptr, col, val)
    T, keep = case.twin()
    x = np.random.default_rng(23).standard_normal((case.n, 4)).astype(np.float32)
    xd = _t(x, dev)
    y = ops.spmm_csr(rowptr, col, val, xd)
    tw = ops.spmm_csr(*_twin_device(T, dev), xd)
    kd = _t(keep, dev)
    assert _same_bits(y[kd], tw[kd])
    worst = _ratio(tw[kd].cpu().numpy(), lt.spmm(T, x)[keep], lt.spmm_bound(T, x)[keep])
    fb = _t(case.full_ballast_rows, dev)
    assert len(fb) > 1000 and bool((_bits(y[fb]) == _bits(y[fb[:1]])).all())
    assert not bool(y[case.n_used:].view(I32).any())
    print(f"\nLO spmm narrow phase {phase}: nnz {case.nnz}, {len(fb)} ballast rows of {L_RUN} entries, largest error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("kind", ["unit", "val"])
@pytest.mark.parametrize("phase", [0, 1])
def test_col_sums_over_a_long_entry_array(eps, dev, phase, kind):
    """ops.col_sums over more than 2^30 entries.  Unit values: the float64 sums are the stored entries per column, exactly (known
    on the host from the rows' lengths).  Stored values: the ballast values are multiples of 1/4, the live ones float32 in
    (0.05, 3), so every term is a multiple of 2^-28 and every column sum is below 2^12: each float64 partial sum is exact in
    whatever order the atomics arrive, and the result is the host's float64 sum BIT FOR BIT (the bar of test_gpu_guards.py's
    col_sums test; an exact sum is also what a twin would give).  The float32 table is the float64 one rounded once."""
    ops = eps.ops
    weighted = kind == "val"
    case = _long_case(phase)
    _need(dev, case.nnz * (8 if weighted else 4) + 64 * case.n)
    rowptr, col, val = case.build(dev, weighted)
    _beyond_entry_marks(case, rowptr, col, val)
    wide = ops.col_sums(rowptr, col, val, case.n, f64=True)
    s, _, k = case.col_sums(weighted)
    got = wide.cpu().numpy()
    assert float(s.max()) < 1 << 12 and np.array_equal(s * 2.0 ** 28, np.rint(s * 2.0 ** 28))       # exact sums, as the docstring says
    if not weighted:
        assert np.array_equal(s, k.astype(np.float64))
    worst = float(np.abs(got - s).max())
    print(f"\nLO col_sums phase {phase} {kind}: nnz {case.nnz}, largest column {int(k.max())} entries, largest |got - sum| {worst:.3e}")
    assert np.array_equal(got, s)
    assert int(k.sum()) == case.nnz and k.max() > 1000
    narrow = ops.col_sums(rowptr, col, val, case.n)
    assert narrow.dtype == torch.float32 and torch.equal(narrow, wide.to(torch.float32))


@pytest.mark.parametrize("kind", ["unit", "val"])
@pytest.mark.parametrize("phase", [0, 1])
def test_gcn_norm_output_as_long_as_the_entries(eps, dev, phase, kind):
    """ops.gcn_norm: the OUTPUT has one float per stored entry and crosses both marks.  Entries next to every mark, at both ends
    and at the head of the ballast row below every live set (whose columns are stored rows: non-zero terms), and all live entries,
    against val / sqrt(s_r s_c) from the host's float64 row sums under the project's ((deg_r + deg_c) / 2 U + 1e-6) |truth|.
    Every full ballast row's output equals the first one's, over the whole array.  (Each entry needs the sums of two rows of the
    whole graph: a compacted graph is another problem, so there is no twin.)"""
    ops = eps.ops
    weighted = kind == "val"
    case = _long_case(phase)
    _need(dev, case.nnz * (12 if weighted else 8) + 64 * case.n)
    rowptr, col, val = case.build(dev, weighted)
    _beyond_entry_marks(case, rowptr, col, val)
    out = ops.gcn_norm(rowptr, col, val)
    assert out.numel() == case.nnz and out.numel() * 4 > max(MARKS)
    ks = np.unique(np.concatenate([case.sample_entries()] + [s + np.arange(len(c)) for _, s, c, _ in case.live]))
    truth, bound = lo.gcn_norm_at(case, ks, weighted)
    got = out[_t(ks, dev)].cpu().numpy()
    worst = _ratio(got, truth, bound)
    assert (truth != 0).sum() > 100
    rows = 0
    for r0, e0, cnt in case.ballast:
        full = cnt // L_RUN
        if full:
            blk = _bits(out[e0:e0 + full * L_RUN]).view(full, L_RUN)
            assert bool((blk == blk[:1]).all()), (r0, e0)
            rows += full
    assert rows == len(case.full_ballast_rows)
    print(f"\nLO gcn_norm phase {phase} {kind}: nnz {case.nnz}, {len(ks)} entries against float64, largest error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("phase", [0, 1])
def test_edge_cosines_output_as_long_as_the_entries(eps, dev, phase):
    """ops.edge_cosines over more than 2^30 entries: col is read and the OUTPUT (one float per entry) written across both marks.
    xhat [n, 5] comes from ops.cos_node_features on the graph without entries (x / ||x||).  The live rows' entries equal the
    twin's bits; they, and the entries next to every mark, at both ends and at the head of the ballast row below every live
    set, are within the cosine tests' bar 1e-5 (2 + F / 64) (|terms| + 1e-3) of the float64 dot products of x / ||x||."""
    ops = eps.ops
    F = 5
    case = _long_case(phase)
    _need(dev, case.nnz * 8 + 256 * case.n)
    rowptr, col, _ = case.build(dev, weighted=False)
    _beyond_entry_marks(case, rowptr, col)
    x = np.random.default_rng(41).standard_normal((case.n, F)).astype(np.float32)
    T, keep = case.twin()
    trp, tcol, _ = _twin_device(T, dev, weighted=False)
    none = torch.zeros_like(trp)
    xhat = ops.cos_node_features(none, tcol, None, _t(x, dev))             # (no row holds an entry: tcol is never read)
    out = ops.edge_cosines(rowptr, col, xhat)
    assert out.numel() == case.nnz and out.numel() * 4 > max(MARKS)
    tw = ops.edge_cosines(trp, tcol, xhat)
    for r, s, c, _ in case.live:
        t0 = int(T.indptr[r])
        assert _same_bits(out[s:s + len(c)], tw[t0:t0 + len(c)]), r
    ks = np.unique(np.concatenate([case.sample_entries()] + [s + np.arange(len(c)) for _, s, c, _ in case.live]))
    row, cid, _ = case.entry(ks)
    xh = x.astype(np.float64) / np.maximum(np.linalg.norm(x.astype(np.float64), axis=1), 1e-8)[:, None]
    prod = xh[row] * xh[cid]
    err = np.abs(out[_t(ks, dev)].cpu().numpy() - prod.sum(1))
    worst = float((err / (1e-5 * (2 + F / 64) * (np.abs(prod).sum(1) + 1e-3))).max())
    for m in MARKS:
        assert (ks * 4 < m).any() and (ks * 4 == m).any() and (ks * 4 > m).any()
    print(f"\nLO edge_cosines phase {phase}: nnz {case.nnz}, {len(ks)} entries against float64, largest error / bar {worst:.3f}")
    assert worst <= 1.0


def _merge_keys(case):
    """A small sorted batch ``row << 32 | col`` for ops.csr_merge: at the rows at every mark and the row that ends the arrays,
    three stored pairs (once each: a fractional value takes ONE float32 add) and five new ones, one of them three times; at
    ballast rows of 2^20 entries (which hold every id) stored pairs, one twice (multiples of 1/4: exact); at the remainder
    ballast row stored and new pairs; at two rows without entries new pairs."""
    keys = []
    add = lambda r, ids: keys.extend((int(r) << 32) | int(c) for c in ids)               # noqa: E731
    rows = [case.set_rows[i][case.b + k] for i in range(len(case.marks)) for k in (0, 1)] + [case.set_rows[-1][-1]]
    for r in rows:
        ids = case.row(int(r))[0]
        fresh = np.setdiff1d(np.arange(3, case.n, case.n // 11), ids)[:5]
        add(r, list(ids[[0, len(ids) // 2, -1]]) + list(fresh) + [fresh[1], fresh[1]])
    for r in case.pair_ballast():
        ln = len(case.row(int(r))[0])
        if ln == case.L:
            add(r, [0, 12345, 12345, case.L - 1])
        else:
            add(r, [0, ln - 1, ln, ln + 5, case.n - 1, ln + 5])
    add(case.n_used + 3, [5, 77, 77])
    add(case.n - 1, [0])
    return np.sort(np.array(keys, np.int64))


@pytest.mark.parametrize("phase", [0, 1])
def test_csr_merge_rewrites_a_long_entry_array(eps, dev, phase):
    """ops.csr_merge of a small batch into the graph of more than 2^30 entries: col and val are rewritten whole, every entry
    behind the first new one moved.  The new row pointer against the host's; every row the twin holds (live rows, kept ballast
    rows, the rows the batch touches) against the twin's merge bit for bit, and the twin's merge against scipy's sum of the
    two patterns; every ballast region compared WHOLE on the device with the old arrays at its new place (values differ at
    the batch's stored pairs alone)."""
    ops = eps.ops
    case = _long_case(phase)
    _need(dev, case.nnz * 16 + 64 * case.n)
    rowptr, col, val = case.build(dev)
    _beyond_entry_marks(case, rowptr, col, val)
    keys = _merge_keys(case)
    krow, kcol = keys >> 32, keys & 0xFFFFFFFF
    T, keep = case.twin()
    assert set(krow) <= set(keep) | set(range(case.n_used, case.n))
    K = ssp.coo_matrix((np.ones(len(keys)), (krow, kcol)), shape=(case.n, case.n)).tocsr()
    S = (T.astype(np.float64) + K).tocsr()
    S.sum_duplicates(); S.sort_indices()
    new_rp, new_col, new_val = ops.csr_merge(rowptr, col, val, case.n, _t(keys, dev), True)
    added = np.zeros(case.n, np.int64)
    rk = np.unique(krow)
    added[rk] = np.diff(S.indptr)[rk] - np.diff(case.rowptr)[rk]
    want_rp = case.rowptr + np.concatenate([[0], np.cumsum(added)])
    assert added.sum() > 30 and torch.equal(new_rp, _t(want_rp, dev))
    assert new_col.numel() == new_val.numel() == want_rp[-1] > case.nnz and new_col.numel() * 4 > max(MARKS)
    # the twin's merge: scipy's, bit for bit
    trp, tcol, tval = _twin_device(T, dev)
    rp2, c2, v2 = ops.csr_merge(trp, tcol, tval, case.n, _t(keys, dev), True)
    assert np.array_equal(rp2.cpu().numpy(), S.indptr) and np.array_equal(c2.cpu().numpy(), S.indices)
    assert np.array_equal(v2.cpu().numpy().view(np.int32), S.data.astype(np.float32).view(np.int32))
    # every row the twin holds, in the big result
    for r in np.union1d(keep, rk):
        a, b, ta = int(want_rp[r]), int(want_rp[r + 1]), int(S.indptr[r])
        assert b - a == S.indptr[r + 1] - ta
        assert torch.equal(new_col[a:b], c2[ta:ta + b - a]) and _same_bits(new_val[a:b], v2[ta:ta + b - a]), r
    # every ballast region whole, at its new place
    for r0, e0, cnt in case.ballast:
        s = int(want_rp[r0])
        assert torch.equal(new_col[s:s + cnt], col[e0:e0 + cnt]), r0
        rows_in = (krow >= r0) & (krow < np.searchsorted(case.rowptr, e0 + cnt, side="left"))
        stored = len({(int(a), int(b)) for a, b in zip(krow[rows_in], kcol[rows_in]) if b < case.rowptr[a + 1] - case.rowptr[a]})
        assert int((new_val[s:s + cnt] != val[e0:e0 + cnt]).sum()) == stored, r0
    shifts = {int(want_rp[r0] - case.rowptr[r0]) for r0, _, _ in case.ballast}
    assert len(shifts) >= 3 and max(shifts) > 0
    print(f"\nLO csr_merge phase {phase}: nnz {case.nnz} -> {int(want_rp[-1])}, {len(keys)} keys, ballast regions moved by {sorted(shifts)}")


# ====================================================================================================================
# Group C: documented limits are enforced
# ====================================================================================================================
# Each of these entry points compares the STATED nnz with its limit before it launches anything (at most a 4-byte status word is
# cleared first); profiles/large_offsets/coverage.txt gives file:line of every check.
NNZ_LIMIT = 1 << 30
TEXT = "col[] is addressed with 32-bit byte offsets (nnz < 2^30)"


def _small(dev):
    d = dict(rowptr=torch.tensor([0, 1, 2], dtype=torch.int64, device=dev), col=torch.tensor([1, 0], dtype=I32, device=dev),
             i32=torch.zeros(64, dtype=I32, device=dev), i64=torch.zeros(64, dtype=torch.int64, device=dev),
             i16=torch.zeros(64, dtype=torch.int16, device=dev), f32=torch.ones(64, device=dev))
    return d


@pytest.mark.parametrize("name", ["eps_filter_scan", "eps_expand_unit_count", "eps_expand_unit_fill", "eps_expand_unit_list",
                                  "eps_scan_screen", "eps_scan_screen_weighted", "eps_relabel_graph", "eps_reverse_positions_sorted"])
def test_stated_nnz_at_the_limit_is_refused(eps, dev, name):
    """A two-node graph with a STATED nnz at the limit: EpsError with the documented text, nothing launched (the status words the
    calls may clear stay 0, the outputs keep their fill)."""
    ops = eps.ops
    d = _small(dev)
    rp, col, i32, i64, i16, f32 = d["rowptr"], d["col"], d["i32"], d["i64"], d["i16"], d["f32"]
    mark = torch.full((64,), -7, dtype=I32, device=dev)
    surv = ops.Survivors(16, 0.0, dev)
    ws = torch.zeros(512, dtype=torch.int64, device=dev)
    n, nnz = 2, NNZ_LIMIT
    calls = {
        "eps_filter_scan": (TEXT, (rp, col, i32, i64, None, n, nnz, 1, i32, 2, surv.rec, ws, ws.numel() * 8)),
        "eps_expand_unit_count": (TEXT, (rp, col, None, None, n, nnz, 1, 0, 2, None, i64, ws, ws.numel() * 8)),
        "eps_expand_unit_fill": (TEXT, (rp, col, None, i64, None, n, nnz, 1, 0, 2, None, i64, None, mark, None, None, i32, ws, ws.numel() * 8)),
        "eps_expand_unit_list": (TEXT, (rp, col, None, i64, None, n, nnz, 1, 0, 2, None, i64, i64, mark, None, i32, ws, ws.numel() * 8)),
        "eps_scan_screen": (TEXT, (rp, col, i32, i32, i16, i32, None, None, None, None, None, None, None, i32, n, nnz, i32, None, 2,
                                   -1, -1, -1, -1, 20, 2, surv.rec, i32)),
        "eps_scan_screen_weighted": (TEXT, (rp, col, f32, i32, f32, i16, i32, i32, n, nnz, i32, 2, 20, 2, surv.rec, i32)),
        "eps_relabel_graph": ("eps_relabel_graph: bad size", (rp, col, None, i64, i32, rp, n, 1 << 31, 2, mark, None, ws, ws.numel() * 8)),
        "eps_reverse_positions_sorted": ("eps_reverse_positions_sorted: bad size", (rp, col, n, 1 << 31, 2, mark, i64, i32, None, ws, ws.numel() * 8)),
    }
    text, args = calls[name]
    with pytest.raises(eps._lib.EpsError) as e:
        ops._call(name, dev, *args)
    assert text in str(e.value) and name.replace("_weighted", "") in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((mark == -7).all()) and not bool(i32.any()) and not bool(i64.any())
    assert surv.counts() == (0, 0)


def test_row_records_refuse_a_stated_nnz_at_the_limit(eps, dev):
    """ops.scan_row_records (whose ABI call takes no nnz and keeps rowptr's low word) refuses a stated nnz of 2^30 before any
    launch, and builds the records one entry below it: word 16 of a record is the row's first entry."""
    ops = eps.ops
    cuts = torch.zeros((2, 32), dtype=torch.int16, device=dev)
    rowptr = torch.tensor([0, 1, 2], dtype=torch.int64, device=dev)
    fx32 = torch.tensor([5, 7], dtype=I32, device=dev)
    assert ops.SCAN_MAX_NNZ == NNZ_LIMIT
    with pytest.raises(eps._lib.EpsError, match="scan_row_records: .*nnz < 2\\^30"):
        ops.scan_row_records(cuts, rowptr, fx32, nnz=NNZ_LIMIT)
    rec = ops.scan_row_records(cuts, rowptr, fx32, nnz=NNZ_LIMIT - 1)
    assert rec[:, 16].tolist() == [0, 1] and rec[:, 17].tolist() == [5, 7]


def test_rescore_runs_refuses_a_graph_of_2_30_entries(eps, dev):
    """The live case: the Group B graph has more than 2^30 entries.  scan.scan_available is false for it (scan_plausible, before
    any table is built), and ops.rescore_runs / rescore_runs_dev -- whose ABI calls take no nnz to check and address col[] with
    32-bit byte offsets -- raise before they launch (``out`` is never allocated: the check comes first)."""
    from eps_amd import scan
    ops = eps.ops
    case = _long_case(0)
    _need(dev, case.nnz * 4 + 64 * case.n)
    rowptr, col, _ = case.build(dev, weighted=False)
    _beyond_entry_marks(case, rowptr, col)
    assert col.numel() >= ops.RESCORE_MAX_NNZ == NNZ_LIMIT
    g = eps.CSRGraph(rowptr, col, None, case.n, case.n)
    assert not scan.scan_plausible(g) and not scan.scan_available(g)
    fixw = torch.ones(case.n, dtype=torch.int64, device=dev)
    u, v = case.set_rows[0][3], case.set_rows[0][4]
    keys = torch.tensor([(int(u) << 32) | int(v)], dtype=torch.int64, device=dev)
    with pytest.raises(eps._lib.EpsError, match="rescore_runs: .*32-bit byte offsets.*nnz < 2\\^30"):
        ops.rescore_runs(rowptr, col, fixw, case.n, keys)
    with pytest.raises(eps._lib.EpsError, match="rescore_runs_dev: .*32-bit byte offsets.*nnz < 2\\^30"):
        ops.rescore_runs_dev(rowptr, col, fixw, case.n, keys, torch.ones(1, dtype=torch.int64, device=dev))
    # one entry below the limit the wrappers let the call through: checked on the small twin, against the pair kernel's count
    T, _ = case.twin()
    trp, tcol, _ = _twin_device(T, dev, weighted=False)
    assert tcol.numel() < NNZ_LIMIT
    fx = ops.fixed_weights(torch.ones(case.n, device=dev))
    got = ops.rescore_runs(trp, tcol, fx, case.n, keys)
    cnt, _, _ = ops.pair_scores(trp, tcol, None, None, case.n, keys.new_tensor([u]).to(I32), keys.new_tensor([v]).to(I32), grouped=False)
    assert float(got[0]) == float(cnt[0]) > 0
