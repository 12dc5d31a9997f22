"""The truth the graph-attention kernels (ops.gat_aggregate, ops.gat_aggregate_backward, models.GATConv / GAT) are held to: float64
restatements of the published GATConv layer -- a dense per-row loop for the aggregate, the closed forms for its backward, a dense
masked-softmax torch formulation for autograd --, the per-element error bounds that go with them, and the builders of the cases the
tests run.  A plain helper module (no fixtures); tests/test_gat_host.py validates it on the CPU and holds every builder to what it
promises, tests/test_gpu_gat.py compares the HIP kernels with it.

Semantics (restated): the neighbourhood of row i is its stored entries with col != i plus i itself exactly once (a stored self loop
is not counted twice, stored values are ignored, an empty row attends to itself alone); e_ij = LeakyReLU_slope(s_src[j,h] +
s_dst[i,h]); alpha_i.h = softmax_j e_ij; out[i,h,:] = sum_j alpha_ijh z[j,h,:] + bias, optionally ReLU."""
import numpy as np
import scipy.sparse as ssp
import torch

import layer_truth as lt
import training_truth as tt

U = lt.U
SLOPE = 0.2

# ---- the error model's one measured number ---------------------------------------------------------------------------------------
# Twice the worst error, in units in the last place, of numpy's float32 ``exp`` against float64 on the cases' own arguments (every
# e - m of every case below; ``worst_exp_ulps``, asserted in tests/test_gat_host.py).  Measured worst: 2.257 ulp (numpy's
# vectorised float32 exp, whose documented maximum is 2.52); the factor 2 is margin for a different implementation of the same
# accuracy class (the device's expf), rounded up to a tenth.  One ulp is at most 2 U relative.
EXP_ULPS = 4.6

# K of the forward bound, in units of U, from named terms (``forward_k``):
K_SCORE_OPS = 3          # the two additions and the multiply that form e (s_src + s_dst, the LeakyReLU product, e - m)
K_ARGUMENT = 3           # ... as an ABSOLUTE error of exp's argument: <= 3 U max|e| of the row, which IS a relative error of exp
K_DIVISION = 1           # acc / l


def forward_k(emax):
    """K per (row, head): the score operations, the argument error 3 max|e| turned relative, the division, expf."""
    return K_SCORE_OPS + K_ARGUMENT * emax + K_DIVISION + 2.0 * EXP_ULPS


def leaky(raw, slope=SLOPE):
    return np.where(raw > 0, raw, slope * raw)


def neighbourhood(rowptr_block, col, r, i):
    """Row r of the block (absolute node i): i first, then the stored columns other than i."""
    c = np.asarray(col[rowptr_block[r]:rowptr_block[r + 1]], np.int64)
    return np.concatenate([[i], c[c != i]])


# ====================================================================================================================
# truths
# ====================================================================================================================
def aggregate(rowptr, col, z, s_src, s_dst, heads, bias=None, relu=False, row0=0, slope=SLOPE, parts=False):
    """Rows [row0, row0 + len(rowptr) - 1) of the attention aggregate in float64, one dense row at a time.  ``rowptr``: the
    block's slice of the graph's (absolute offsets into ``col``).  -> out [rows, f]; with ``parts`` a dict: out, lse [rows,
    heads], bound (the forward bound per element), lse_bound, emax [rows, heads], rho [rows, heads] (see
    ``aggregate_backward``)."""
    z, s_src, s_dst = (np.asarray(t, np.float64) for t in (z, s_src, s_dst))
    n_rows, f = len(rowptr) - 1, z.shape[1]
    C = f // heads
    b64 = np.zeros(f) if bias is None else np.asarray(bias, np.float64)
    out, absum = np.zeros((n_rows, f)), np.zeros((n_rows, f))
    lse, emax, m_abs, logl = (np.zeros((n_rows, heads)) for _ in range(4))
    for r in range(n_rows):
        i = row0 + r
        J = neighbourhood(rowptr, col, r, i)
        e = leaky(s_src[J] + s_dst[i][None, :], slope)                   # [|J|, heads]
        m = e.max(0)
        p = np.exp(e - m)
        l = p.sum(0)
        a = p / l
        zJ = z[J].reshape(len(J), heads, C)
        out[r] = np.einsum("jh,jhc->hc", a, zJ).reshape(f)
        absum[r] = np.einsum("jh,jhc->hc", a, np.abs(zJ)).reshape(f)
        lse[r], emax[r], m_abs[r], logl[r] = m + np.log(l), np.abs(e).max(0), np.abs(m), np.abs(np.log(l))
    res = out + b64[None, :]
    if relu:
        res = np.maximum(res, 0.0)
    if not parts:
        return res
    deg = np.diff(np.asarray(rowptr, np.int64)).astype(np.float64)[:, None]
    k = forward_k(emax)                                                   # [rows, heads]
    bound = np.repeat(deg + 1 + k, C, axis=1) * U * (absum + np.abs(b64)[None, :])
    # lse = m + logf(l): m carries the score operations' 2 U |m|; l is a chain of deg + 1 terms, each relative K U off, and its
    # relative error is log's absolute one; logf is in expf's accuracy class (2 EXP_ULPS U |log l|); the last addition U |lse|
    lse_bound = U * (2 * m_abs + (deg + 1 + k) + 2 * EXP_ULPS * logl + np.abs(lse))
    # rho (units of U): the relative error of alpha = expf(e - lse) as the BACKWARD recomputes it -- the argument error 3 max|e|,
    # lse's own error, the subtraction U (|e| + |lse|), expf
    rho = K_ARGUMENT * emax + lse_bound / U + (emax + np.abs(lse)) + 2.0 * EXP_ULPS
    return dict(out=res, lse=lse, bound=bound, lse_bound=lse_bound, emax=emax, rho=rho)


def aggregate_float32(rowptr, col, z, s_src, s_dst, heads, bias=None, relu=False, row0=0, slope=SLOPE):
    """The same aggregate in plain float32 numpy, max-subtracted: the distance a careful float32 evaluation keeps from the truth."""
    f32 = np.float32
    z, s_src, s_dst = (np.asarray(t, f32) for t in (z, s_src, s_dst))
    n_rows, f = len(rowptr) - 1, z.shape[1]
    C = f // heads
    out = np.zeros((n_rows, f), f32)
    for r in range(n_rows):
        i = row0 + r
        J = neighbourhood(rowptr, col, r, i)
        raw = s_src[J] + s_dst[i][None, :]
        e = np.where(raw > 0, raw, f32(slope) * raw).astype(f32)
        p = np.exp(e - e.max(0))
        acc = (p[:, :, None] * z[J].reshape(len(J), heads, C)).sum(0, dtype=f32)
        out[r] = (acc / p.sum(0, dtype=f32)[:, None]).reshape(f)
    if bias is not None:
        out = out + np.asarray(bias, f32)[None, :]
    return np.maximum(out, f32(0)) if relu else out


def exp_arguments(rowptr, col, s_src, s_dst, slope=SLOPE):
    """Every e - m a float32 evaluation of the case hands to exp (float32)."""
    f32 = np.float32
    s_src, s_dst = np.asarray(s_src, f32), np.asarray(s_dst, f32)
    args = []
    for i in range(len(rowptr) - 1):
        J = neighbourhood(rowptr, col, i, i)
        raw = s_src[J] + s_dst[i][None, :]
        e = np.where(raw > 0, raw, f32(slope) * raw).astype(f32)
        args.append((e - e.max(0)).ravel())
    return np.concatenate(args)


def worst_exp_ulps(args32):
    """The worst error of numpy's float32 exp on ``args32`` against float64, in units in the last place of the true value."""
    want = np.exp(args32.astype(np.float64))
    got = np.exp(args32).astype(np.float64)
    ulp = np.spacing(np.maximum(want, 2.0 ** -126).astype(np.float32)).astype(np.float64)
    return float((np.abs(got - want) / ulp).max())


def aggregate_backward(rowptr, col, z, s_src, s_dst, heads, out_nobias, gout, slope=SLOPE):
    """The closed forms of the backward over the whole graph in float64:
        alpha_ij = softmax_j e_ij, d_alpha_ij = <gout[i,h,:], z[j,h,:]>, D_ih = <gout[i,h,:], out_nobias[i,h,:]>,
        ds_ij = alpha_ij (d_alpha_ij - D_ih) (raw_ij > 0 ? 1 : slope);
        g_s_dst[i] = sum_j ds_ij, g_s_src[j] = sum_i ds_ij, gz[j] = sum_i alpha_ij gout[i].
    ``out_nobias`` is an INPUT (the forward's output as the caller holds it), as it is for the kernel.
    -> dict: gz, g_s_src, g_s_dst and their bounds gz_bound, g_s_src_bound, g_s_dst_bound.

    Bounds, from the kernel's operation counts (units of U; t = the row's terms, self loop included; rho_i = the relative error of
    a recomputed alpha of row i, ``aggregate``; w = alpha (1 or slope), one more product; a per-head dot product over C columns
    is 4 products and 3 additions per lane, then C/4 additions: C/4 + 5):
      gz[j]       sum_i (t_j + rho_i) alpha_ij |gout_i|
      g_s_dst[i]  = <gout_i, A> - D W, A = sum_j w z_j, W = sum_j w:
                  (t_i + rho_i + C/4 + 8) S1 + (t_i + rho_i + 4) |D| W + (C/4 + 5) W sum_c |gout_i| |out_i|,  S1 = sum_c |gout_ic| sum_j w |z_jc|
      g_s_src[j]  = <z_j, B> - sum_i w D_i, B = sum_i w gout_i:
                  sum_i (t_j + rho_i + C/4 + 9) w |z_j| |gout_i| + sum_i (t_j + rho_i + 4) w |D_i| + sum_i w (C/4 + 5) sum_c |gout_i| |out_i|."""
    z, s_src, s_dst, outnb, gout = (np.asarray(t, np.float64) for t in (z, s_src, s_dst, out_nobias, gout))
    n, f = z.shape
    C = f // heads
    fw = aggregate(rowptr, col, z, s_src, s_dst, heads, slope=slope, parts=True)
    rho = fw["rho"]
    gz, gs, gd = np.zeros((n, heads, C)), np.zeros((n, heads)), np.zeros((n, heads))
    gz_b, gs_b, gd_b = np.zeros((n, heads, C)), np.zeros((n, heads)), np.zeros((n, heads))
    t = np.array([len(neighbourhood(rowptr, col, i, i)) for i in range(n)], np.float64)
    dot = C / 4 + 5
    z3, g3, o3 = z.reshape(n, heads, C), gout.reshape(n, heads, C), outnb.reshape(n, heads, C)
    for i in range(n):
        J = neighbourhood(rowptr, col, i, i)
        raw = s_src[J] + s_dst[i][None, :]
        e = leaky(raw, slope)
        p = np.exp(e - e.max(0))
        a = p / p.sum(0)                                                  # [|J|, heads]
        w = a * np.where(raw > 0, 1.0, slope)
        zJ, gi = z3[J], g3[i]                                             # [|J|, heads, C], [heads, C]
        D = (gi * o3[i]).sum(1)                                           # [heads]
        Dabs = (np.abs(gi) * np.abs(o3[i])).sum(1)
        dal = np.einsum("hc,jhc->jh", gi, zJ)
        ds = w * (dal - D[None, :])
        gd[i] = ds.sum(0)
        np.add.at(gs, J, ds)
        np.add.at(gz, J, a[:, :, None] * gi[None])
        # bounds
        S1 = np.einsum("hc,jh,jhc->h", np.abs(gi), w, np.abs(zJ))
        W = w.sum(0)
        gd_b[i] = (t[i] + rho[i] + dot + 3) * S1 + (t[i] + rho[i] + 4) * np.abs(D) * W + dot * W * Dabs
        tj = t[J][:, None]
        np.add.at(gz_b, J, ((tj + rho[i][None, :]) * a)[:, :, None] * np.abs(gi)[None])
        zg = np.einsum("jhc,hc->jh", np.abs(zJ), np.abs(gi))
        np.add.at(gs_b, J, (tj + rho[i][None, :] + dot + 4) * w * zg + (tj + rho[i][None, :] + 4) * w * np.abs(D)[None, :]
                  + w * dot * Dabs[None, :])
    return dict(gz=gz.reshape(n, f), g_s_src=gs, g_s_dst=gd, gz_bound=U * gz_b.reshape(n, f), g_s_src_bound=U * gs_b,
                g_s_dst_bound=U * gd_b)


# ---- torch float64, dense: autograd's view of the same layer -------------------------------------------------------
def dense_mask(A, device="cpu"):
    """bool [N, N]: the neighbourhoods as a dense mask -- the stored pattern off the diagonal, plus the whole diagonal."""
    A = ssp.csr_matrix(A)
    n = A.shape[0]
    M = torch.zeros((n, n), dtype=torch.bool, device=device)
    coo = A.tocoo()
    M[torch.from_numpy(coo.row.astype(np.int64)), torch.from_numpy(coo.col.astype(np.int64))] = True
    M.fill_diagonal_(True)
    return M


def dense_aggregate(mask, z, s_src, s_dst, heads, slope=SLOPE, want_raw=False):
    """The aggregate as a dense masked softmax (torch, any float dtype, differentiable): -> out [N, f]."""
    n, f = z.shape
    raw = s_src[None, :, :] + s_dst[:, None, :]                          # [i, j, h]
    e = torch.nn.functional.leaky_relu(raw, slope).masked_fill(~mask[:, :, None], float("-inf"))
    a = torch.softmax(e, dim=1)
    out = torch.einsum("ijh,jhc->ihc", a, z.view(n, heads, f // heads)).reshape(n, f)
    return (out, raw) if want_raw else out


def gat_conv(params, mask, x, heads, relu=False, raws=None):
    """GATConv on ``params`` = dict(lin.weight, att_src, att_dst, bias) in the dtype of its tensors (float64 for the truth, float32
    for the dense torch yardstick).  ``raws``: a list that collects the raw scores [N, N, heads] of the layer."""
    z = x @ params["lin.weight"].t()
    n, f = z.shape
    z3 = z.view(n, heads, f // heads)
    s_src = (z3 * params["att_src"]).sum(-1)
    s_dst = (z3 * params["att_dst"]).sum(-1)
    out, raw = dense_aggregate(mask, z, s_src, s_dst, heads, want_raw=True)
    if raws is not None:
        raws.append(raw)
    out = out + params["bias"]
    return torch.relu(out) if relu else out


def link_gnn_forward(p, mask, edges, heads, branch=None, pre=None, raws=None):
    """LinkGNN(emb, GAT, LinkPredictor) in training mode with dropout 0 on ``p``, a dict of the model's own state-dict keys (any
    float dtype) -> scores [B] in (0, 1).  ``branch`` / ``pre``: see training_truth._relu (masks in forward order: the GNN's
    ReLUs, then the decoder's); ``raws`` collects the raw attention scores [N, N, heads] of every layer."""
    branch = None if branch is None else iter(branch)
    h = p["emb.weight"]
    L = tt._count(p, "gnn.convs.{}.lin.weight")
    for k in range(L):
        h = gat_conv({key: p[f"gnn.convs.{k}.{key}"] for key in ("lin.weight", "att_src", "att_dst", "bias")}, mask, h, heads, raws=raws)
        if k + 1 < L:
            h = tt._relu(h, branch, pre)
    M = tt._count(p, "linkpred.lins.{}.weight")
    return tt.link_predictor(h, edges, [p[f"linkpred.lins.{i}.weight"] for i in range(M)],
                             [p[f"linkpred.lins.{i}.bias"] for i in range(M)], branch, pre)


# ====================================================================================================================
# cases
# ====================================================================================================================
ROW_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 300]     # rows 0..9: an empty row, either side of a 32 group and of a 64 chunk, a hub
EMPTY_ROW, CHUNK_ROW, HUB_ROW = 0, 7, 9
LOOP_ONLY_ROW = 10                                       # a row holding only a stored self loop
LOOP_ROW, LOOP_ROW_OTHERS = 11, 20                       # a row with a stored self loop among 20 others
N_SPECIAL = 12
N_NODES = 640
SHAPES = [(8, 2), (64, 1), (64, 8), (256, 4), (300, 3)]  # (f, heads)
REGIMES = ("normal", "quarters", "wide")
EQUAL_ROW = 3                                            # regime "wide": the row whose scores are all equal

_GRAPH = {}


def graph(seed=5):
    """The symmetric 640-node graph of the tests (scipy CSR, sorted, float64 values that nothing reads): rows 0..9 hold exactly
    ROW_LENGTHS entries, row LOOP_ONLY_ROW its own self loop alone, row LOOP_ROW a self loop among LOOP_ROW_OTHERS others; the
    special rows' ids sort before all their neighbours, the last node's after all of its, ``between_row(A)``'s in between."""
    if seed not in _GRAPH:
        rng = np.random.default_rng(seed)
        A = lt.rows_graph(rng, ROW_LENGTHS + [0, LOOP_ROW_OTHERS], N_NODES)
        loops = ssp.coo_matrix((np.ones(2), ([LOOP_ONLY_ROW, LOOP_ROW], [LOOP_ONLY_ROW, LOOP_ROW])), shape=A.shape)
        A = (A + loops).tocsr()
        A.sort_indices()
        _GRAPH[seed] = A
    return _GRAPH[seed]


def between_row(A):
    """A row with stored neighbours on both sides of its own id (the first such filler row)."""
    for i in range(N_SPECIAL, A.shape[0] - 1):
        c = A.indices[A.indptr[i]:A.indptr[i + 1]]
        if len(c) and c.min() < i < c.max():
            return i
    raise AssertionError("no row with neighbours on both sides")


def asymmetric(A):
    """``A`` without the entries (i, j), i < j, of every third row: a pattern that is not its own transpose."""
    B = ssp.csr_matrix(A).tolil()
    for i in range(N_SPECIAL, A.shape[0], 3):
        B.rows[i], B.data[i] = [c for c in B.rows[i] if c <= i], [v for c, v in zip(B.rows[i], B.data[i]) if c <= i]
    B = B.tocsr()
    B.sort_indices()
    return B


_CASES = {}


def case(f, heads, regime, seed=5):
    """dict(A, rowptr int64, col int32, z [N, f], s_src, s_dst [N, heads], bias [f], gout [N, f]) -- float32 arrays, fixed per key.
      "normal"    z ~ N(0,1), scores = the layer's own: z times N(0,1)/sqrt(C) attention vectors, rounded to float32;
      "quarters"  s_src in {k/4}, s_dst in {k/4 + 1/8}, |k| <= 8: every raw score is an odd multiple of 1/8, so no LeakyReLU
                  argument sits near its kink (the backward's regime);
      "wide"      s_src, s_dst uniform in [-45, 45] (raw scores up to +-90 within one row; the hub row reaches +90 exactly) and
                  row EQUAL_ROW's scores all equal: exp without the max subtracted overflows float32, the truth stays finite."""
    key = (f, heads, regime, seed)
    if key not in _CASES:
        A = graph(seed)
        n, C = A.shape[0], f // heads
        rng = np.random.default_rng(100003 * f + 1009 * heads + REGIMES.index(regime) + seed)
        z = rng.standard_normal((n, f)).astype(np.float32)
        if regime == "normal":
            att = (rng.standard_normal((2, heads, C)) / np.sqrt(C)).astype(np.float32)
            z3 = z.reshape(n, heads, C).astype(np.float64)
            s_src, s_dst = ((z3 * att[k][None]).sum(-1).astype(np.float32) for k in (0, 1))
        elif regime == "quarters":
            s_src = (rng.integers(-8, 9, (n, heads)) / 4.0).astype(np.float32)
            s_dst = (rng.integers(-8, 9, (n, heads)) / 4.0 + 0.125).astype(np.float32)
        else:
            s_src = rng.uniform(-45, 45, (n, heads)).astype(np.float32)
            s_dst = rng.uniform(-45, 45, (n, heads)).astype(np.float32)
            eq = np.concatenate([[EQUAL_ROW], A.indices[A.indptr[EQUAL_ROW]:A.indptr[EQUAL_ROW + 1]]])
            s_src[eq] = 40.0
            hub_nb = A.indices[A.indptr[HUB_ROW]:A.indptr[HUB_ROW + 1]]
            s_dst[HUB_ROW] = 45.0
            s_src[hub_nb[~np.isin(hub_nb, eq)][0]] = 45.0
        _CASES[key] = dict(A=A, rowptr=A.indptr.astype(np.int64), col=A.indices.astype(np.int32), z=z, s_src=s_src, s_dst=s_dst,
                           bias=rng.standard_normal(f).astype(np.float32), gout=rng.standard_normal((n, f)).astype(np.float32))
    return _CASES[key]


_TRUTH = {}


def forward_truth(f, heads, regime, bias, relu):
    """``aggregate(..., parts=True)`` of a case, computed once and shared (read-only) among the tests that need it."""
    key = (f, heads, regime, bool(bias), bool(relu))
    if key not in _TRUTH:
        c = case(f, heads, regime)
        _TRUTH[key] = aggregate(c["rowptr"], c["col"], c["z"], c["s_src"], c["s_dst"], heads, c["bias"] if bias else None, relu,
                                parts=True)
    return _TRUTH[key]
