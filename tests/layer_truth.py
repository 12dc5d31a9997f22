"""The truth the GNN layer kernels of the INFERENCE path (ops.gemm, ops.spmm_csr, ops.gcn_norm, ops.mlp_decode) are held to:
plain numpy float64 restatements of the four operations, the per-element error bounds that go with them, and the builders of
the cases the GPU tests run -- operands in every storage flavour the kernels dispatch on, the row-length graph, the decode
stacks.  A plain helper module (no fixtures); tests/test_layer_truth_host.py validates it on the CPU against triple loops and
holds every builder to what it promises, tests/test_gpu_layer_kernels.py compares the HIP kernels with it."""
import math

import numpy as np
import scipy.sparse as ssp
import torch

U = 2.0 ** -24                                   # unit roundoff of float32


def gamma(k):
    """The standard bound of k correctly rounded float32 operations in a chain."""
    return k * U / (1.0 - k * U)


# ====================================================================================================================
# truths
# ====================================================================================================================
def gemm(a, b, bias=None, relu=False, acc_c=None):
    """act(a b^T + bias + acc_c) in float64; ``b`` is [N, K] (torch.nn.Linear layout)."""
    c = np.asarray(a, np.float64) @ np.asarray(b, np.float64).T
    if bias is not None:
        c = c + np.asarray(bias, np.float64)[None, :]
    if acc_c is not None:
        c = c + np.asarray(acc_c, np.float64)
    return np.maximum(c, 0.0) if relu else c


def gemm_bound(a, b, bias=None, acc_c=None):
    """Per element: (K + 2) U (|a| |b|^T + |bias|) -- K products and additions of the fma chain, the bias add, one to spare;
    with ``acc_c`` one more unit and + |C|.  (ReLU is 1-Lipschitz: it needs no term.)"""
    k = np.asarray(a).shape[1]
    s = np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(b, np.float64)).T
    if bias is not None:
        s = s + np.abs(np.asarray(bias, np.float64))[None, :]
    if acc_c is None:
        return (k + 2) * U * s
    return (k + 3) * U * (s + np.abs(np.asarray(acc_c, np.float64)))


def _csr64(B):
    B = ssp.csr_matrix(B, dtype=np.float64)
    B.sort_indices()
    return B


def _pattern(B):
    B = _csr64(B)
    return ssp.csr_matrix((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)


def spmm(B, x, bias=None, relu=False, mean=False):
    """act(B x + bias) in float64.  ``mean``: the stored VALUES are ignored -- every row is the plain average of the x rows
    of its stored entries (an empty row averages to 0), which is what SAGEConv's aggregation does with a weighted adjacency."""
    x = np.asarray(x, np.float64)
    if mean:
        P = _pattern(B)
        y = (P @ x) / np.maximum(np.diff(P.indptr), 1).astype(np.float64)[:, None]
    else:
        y = _csr64(B) @ x
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[None, :]
    return np.maximum(y, 0.0) if relu else y


def spmm_bound(B, x, bias=None, mean=False, extra=0):
    """Per element: gamma(deg_row + extra) (|B| |x| + |bias|); ``extra`` = 1 with a fused bias (one more addition; the mean's
    division is counted in deg, whose chain has only deg - 1 additions)."""
    deg = np.diff(_csr64(B).indptr).astype(np.float64)[:, None]
    s = spmm(abs(_csr64(B)), np.abs(np.asarray(x, np.float64)), None if bias is None else np.abs(bias), False, mean)
    return gamma(deg + extra) * s


def gcn_norm(rowptr, col, val):
    """val / sqrt(s_r s_c), s the row sums in float64 of the float32 values (``val`` None: ones), 0 where either sum is 0."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    v = np.ones(len(col)) if val is None else np.asarray(val, np.float32).astype(np.float64)
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    s = np.zeros(n)
    np.add.at(s, row, v)
    den = s[row] * s[col]
    out = np.zeros(len(col))
    ok = den != 0
    out[ok] = v[ok] / np.sqrt(den[ok])
    return out


def gcn_norm_bound(rowptr, col, truth):
    """((deg_r + deg_c) / 2 U + 1e-6) |truth| per entry: the two float32 row sums of positive terms err by at most deg U
    relative each and enter under a square root; 1e-6 is the project's own gate for the device powf and the two products."""
    deg = np.diff(np.asarray(rowptr, np.int64)).astype(np.float64)
    row = np.repeat(np.arange(len(deg)), deg.astype(np.int64))
    return ((deg[row] + deg[np.asarray(col, np.int64)]) / 2 * U + 1e-6) * np.abs(truth)


def decode(h, u, v, ws, bs):
    """LinkPredictor in eval mode: Hadamard -> (L - 1) x [Linear, ReLU] -> Linear(H, 1).  -> (logits, probabilities), float64."""
    h = np.asarray(h, np.float64)
    z = h[np.asarray(u, np.int64)] * h[np.asarray(v, np.int64)]
    for w, b in zip(ws[:-1], bs[:-1]):
        z = np.maximum(z @ np.asarray(w, np.float64).T + np.asarray(b, np.float64), 0.0)
    logit = (z @ np.asarray(ws[-1], np.float64).T + np.asarray(bs[-1], np.float64))[:, 0]
    return logit, 1.0 / (1.0 + np.exp(-logit))


def decode_float32(h, u, v, ws, bs):
    """The same chain in plain float32 numpy -> logits: the distance a careful float32 evaluation keeps from the truth."""
    z = h[u] * h[v]
    for w, b in zip(ws[:-1], bs[:-1]):
        z = np.maximum(z @ w.T + b, np.float32(0))
    return (z @ ws[-1].T + bs[-1])[:, 0]


# ====================================================================================================================
# graphs
# ====================================================================================================================
def symmetric_weights(A, rng, lo=1, hi=4):
    """Integer weights on a symmetric pattern, the same on both copies of an edge."""
    up = ssp.triu(ssp.csr_matrix(A), 1).tocoo()
    w = rng.integers(lo, hi + 1, up.nnz).astype(np.float64)
    W = ssp.coo_matrix((w, (up.row, up.col)), shape=A.shape).tocsr()
    return (W + W.T).tocsr()


def rows_graph(rng, lengths, n):
    """Symmetric weighted graph in which node i < len(lengths) has EXACTLY lengths[i] stored entries: the special nodes'
    neighbours are drawn from the other ('filler') nodes only, which are also joined among themselves
    (like test_gpu_fuzz._graph_with_row_lengths, whose lengths are lower limits)."""
    k = len(lengths)
    rows, cols = [], []
    for i, L in enumerate(lengths):
        nb = rng.choice(np.arange(k, n), size=L, replace=False)
        rows.append(np.full(L, i)); cols.append(nb)
    extra = rng.integers(k, n, (2, 3 * n))
    extra = extra[:, extra[0] != extra[1]]
    r, c = np.concatenate(rows + [extra[0]]), np.concatenate(cols + [extra[1]])
    P = ssp.coo_matrix((np.ones(len(r)), (r, c)), shape=(n, n)).tocsr()
    P = ((P + P.T) > 0).astype(np.float64).tocsr()
    A = symmetric_weights(P, rng)
    assert np.diff(A.indptr)[:k].tolist() == list(lengths)
    return A


LAYER_ROWS = [0, 1, 31, 32, 33, 63, 64, 65, 129, 2049]      # SP_FLIGHT = 32 rows, fetches of 64 entries, one hub
LAYER_NODES = 4500
ZERO_ROW = 4                                                 # the 33-entry row: the one ``layer_graph(zero_row=True)`` zeroes


def fractional_weights(A, rng, lo=0.05, hi=3.0):
    """float32-representable values in (lo, hi) on a symmetric pattern, the same on both copies of an edge."""
    up = ssp.triu(ssp.csr_matrix(A), 1).tocoo()
    w = rng.uniform(lo + 1e-3, hi - 1e-3, up.nnz).astype(np.float32).astype(np.float64)   # (the cast cannot reach lo or hi)
    W = ssp.coo_matrix((w, (up.row, up.col)), shape=A.shape).tocsr()
    return (W + W.T).tocsr()


def layer_graph(zero_row=False, seed=41):
    """The 4500-node graph of the SpMM and gcn_norm tests: rows 0..9 hold exactly LAYER_ROWS entries, values fractional in
    (0.05, 3) and symmetric.  ``zero_row``: the stored values of row ZERO_ROW (not its mirror entries) are all 0.0 -- the row
    sums to zero while its entries stay stored.  float64 scipy CSR with explicit zeros kept."""
    rng = np.random.default_rng(seed)
    A = fractional_weights(rows_graph(rng, LAYER_ROWS, LAYER_NODES), rng)
    A.sort_indices()
    assert np.diff(A.indptr)[:len(LAYER_ROWS)].tolist() == LAYER_ROWS
    assert A.data.min() > 0.05 and A.data.max() < 3.0 and not np.all(A.data == np.round(A.data))
    if zero_row:
        A.data[A.indptr[ZERO_ROW]:A.indptr[ZERO_ROW + 1]] = 0.0
    return A


# ====================================================================================================================
# GEMM operands: the storage flavours eps_gemm_f32 dispatches on
# ====================================================================================================================
GEMM_M = [1, 127, 129, 257]                      # one row either side of the 128 tile; a third tile row
GEMM_N = [1, 4, 130, 132, 260]                   # the same for columns, N % 4 both ways
GEMM_K = [1, 3, 4, 15, 17, 19, 20, 58]           # either side of the 16 chunk and of a float4

GUARD_ROWS = 2                                   # rows of guard band before and after a sliced operand
SENTINEL = 0x7FC5A5A5                            # the word an ``out`` buffer is filled with (a NaN pattern no kernel produces)

# name -> (first column of the slice, what ld is beyond the width rounded up to 4)
_GEOMETRY = {
    "slice_ld4": (4, 8),                         # ld % 4 == 0, base 16-byte aligned: a "fast" operand; K % 4 != 0 -> straddle form
    "slice_ld_odd": (4, 9),                      # ld % 4 == 1
    "base_off1": (1, 8),                         # ld % 4 == 0 but the base sits one float into an aligned row
}
IN_FLAVOURS = ("contig", "ld_odd", "slice_ld4", "slice_ld_odd", "base_off1")
OUT_FLAVOURS = ("fresh", "slice_ld4", "base_off1", "slice_ld_odd", "bias_off1")


def _ceil4(k):
    return (k + 3) // 4 * 4


def _layout(flavour, k):
    """-> (first column, ld) of a [*, k] operand stored in ``flavour``."""
    if flavour == "ld_odd":                      # rows as tight as ld % 4 != 0 allows: contiguous memory when k % 4 != 0
        return 0, (k if k % 4 else k + 1)
    c0, extra = _GEOMETRY[flavour]
    return c0, _ceil4(k) + extra


def operand(values, flavour, device="cpu"):
    """An input operand [R, K] holding ``values`` (a float32 torch tensor) in one of IN_FLAVOURS -> (view, buffer).
    "contig" is a contiguous tensor of its own.  Every other flavour is a view into a buffer with GUARD_ROWS rows before and
    after it whose every other word -- the guard rows and the columns beside the view -- is NaN."""
    r, k = values.shape
    if flavour == "contig":
        t = values.to(device).contiguous().clone()
        return t, t
    c0, ld = _layout(flavour, k)
    buf = torch.full((r + 2 * GUARD_ROWS, ld), float("nan"), dtype=torch.float32, device=device)
    view = buf[GUARD_ROWS:GUARD_ROWS + r, c0:c0 + k]
    view.copy_(values)
    return view, buf


def out_operand(m, n, flavour, device="cpu", init=None):
    """The ``out=`` of a gemm call in one of OUT_FLAVOURS -> (view or None, buffer or None).  "fresh" / "bias_off1": None (the
    wrapper allocates), or a contiguous copy of ``init`` when the call accumulates.  Otherwise a view into an int32-SENTINEL
    filled buffer (GUARD_ROWS rows before and after, columns beside), holding ``init`` if given."""
    if flavour in ("fresh", "bias_off1"):
        t = None if init is None else init.to(device).contiguous().clone()
        return t, None
    c0, ld = _layout(flavour, n)
    buf = torch.full((m + 2 * GUARD_ROWS, ld), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    view = buf[GUARD_ROWS:GUARD_ROWS + m, c0:c0 + n]
    if init is not None:
        view.copy_(init)
    return view, buf


def bias_operand(values, misaligned, device="cpu"):
    """``values`` [n] contiguous, or as big[1:1 + n] of a NaN-filled vector: one float past a 16-byte boundary."""
    if not misaligned:
        return values.to(device).contiguous().clone()
    big = torch.full((values.numel() + 8,), float("nan"), dtype=torch.float32, device=device)
    big[1:1 + values.numel()] = values
    return big[1:1 + values.numel()]


def guard_intact(buf, view):
    """Every word of ``buf`` outside ``view`` still holds SENTINEL, bit for bit (compared on the buffer's device)."""
    words = buf.view(torch.int32)
    off = (view.data_ptr() - buf.data_ptr()) // 4
    r0, c0 = off // buf.stride(0), off % buf.stride(0)
    inside = torch.zeros(words.shape, dtype=torch.bool, device=buf.device)
    inside[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = True
    return bool(((words == SENTINEL) | inside).all()) and int(inside.sum()) == view.numel()


def is_fast(t):
    """eps_gemm_f32's test of an operand: 16-byte aligned rows (ld % 4 == 0 and an aligned base)."""
    return t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def gemm_path(a, b, out, bias):
    """The dispatch of eps_gemm_f32 restated from the operands the wrapper is handed -> (template, A form, B form, epilogue):
    template "aligned" (gemm_f32_kernel<true>) or "general"; tile_load4's form per operand, "b128" (one 16-byte load),
    "straddle" (a fast row with a K tail) or "dword"; epilogue "lds" (float4 stores) or "scalar".  ``out`` None: a fresh
    contiguous allocation."""
    k, n = a.shape[1], b.shape[0]
    fa, fb = is_fast(a), is_fast(b)
    fc = (n % 4 == 0) if out is None else (is_fast(out) and n % 4 == 0)
    fc = fc and (bias is None or bias.data_ptr() % 16 == 0)
    if fa and fb and fc and k % 4 == 0:
        return "aligned", "b128", "b128", "lds"

    def form(fast):
        return ("straddle" if k % 4 else "b128") if fast else "dword"
    return "general", form(fa), form(fb), "lds" if fc else "scalar"


_GEMM_VALUES = {}


def gemm_values(m, n, k):
    """The values of one shape, fixed once: a [m, k], b [n, k], bias [n], c0 [m, n] (what ``out`` holds before an
    accumulating call) as float32 torch tensors on the CPU.  Signs are mixed so that ReLU cuts about half the entries."""
    key = (m, n, k)
    if key not in _GEMM_VALUES:
        gen = torch.Generator().manual_seed(1000003 * m + 1009 * n + k)
        _GEMM_VALUES[key] = tuple(torch.randn(s, generator=gen) for s in ((m, k), (n, k), (n,), (m, n)))
    return _GEMM_VALUES[key]


# ====================================================================================================================
# decode cases
# ====================================================================================================================
DECODE_NODES, DECODE_PAIRS = 300, 500
NARROW = [(h, l) for h in (36, 100, 256) for l in (1, 5, 8)] + [(4, 1), (4, 2)]
WIDE = [(h, l) for h in (260, 512) for l in (1, 4, 8)]
NARROW_TILE, WIDE_TILE = 64, 32                  # D_BM / D_WBM of csrc/mlp_decode.hip

_DECODE = {}


def decode_case(hdim, layers):
    """h [300, H], 500 random pairs, ``layers`` Linear layers of He scale (weights sqrt(2) randn / sqrt(H), biases
    0.1 randn), and the float64 logits / probabilities of the 500 pairs.  For H >= 36 the logits' standard deviation is at
    least 0.3 (asserted): the stack does not die on the way down, so a depth-8 case cannot go vacuous."""
    key = (hdim, layers)
    if key not in _DECODE:
        rng = np.random.default_rng(7919 * hdim + layers)
        h = rng.standard_normal((DECODE_NODES, hdim)).astype(np.float32)
        outs = [hdim] * (layers - 1) + [1]
        ws = [(math.sqrt(2.0) * rng.standard_normal((o, hdim)) / math.sqrt(hdim)).astype(np.float32) for o in outs]
        bs = [(0.1 * rng.standard_normal(o)).astype(np.float32) for o in outs]
        u, v = rng.integers(0, DECODE_NODES, (2, DECODE_PAIRS)).astype(np.int32)
        logit, prob = decode(h, u, v, ws, bs)
        if hdim >= 36:
            assert float(logit.std()) >= 0.3, (hdim, layers, float(logit.std()))
        _DECODE[key] = dict(h=h, u=u, v=v, ws=ws, bs=bs, logit=logit, prob=prob)
    return _DECODE[key]


def decode_lengths(wide, n_cu):
    """The list lengths a decode kernel is run at: one pair, a pair either side of a tile, and (2 n_cu + 1) tile + 1 pairs:
    two tiles more than the 2 n_cu persistent workgroups, so that the first two take a SECOND trip on the ids they fetched one
    trip ahead (the last tile holds one pair) while every other workgroup's look-ahead falls past the end of the list."""
    tile = WIDE_TILE if wide else NARROW_TILE
    return [1, tile - 1, tile, tile + 1], (2 * n_cu + 1) * tile + 1


def repeated(ids, n):
    """The pair list of length ``n`` made of the truth pairs over and over."""
    return np.resize(ids, n)
