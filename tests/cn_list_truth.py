"""The truth the common-neighbour lists (csrc/pair_cn_list.hip, ops.pair_cn_list / cn_list_transpose), models.cn_embed_sum and
the NCN models are held to.  numpy / torch-CPU only, a plain helper module (no fixtures); tests/test_cn_list_host.py validates
it on the CPU against a brute-force dense statement, the GPU tests compare the HIP path with it.

A graph is a scipy CSR matrix with sorted indices; only its PATTERN counts (stored values, explicit zeros included, are
neighbours like any other)."""
import numpy as np
import scipy.sparse as ssp
import torch

import training_truth as tt

U = 2.0 ** -24                                   # unit roundoff of float32


def gamma(n):
    """gamma_n = n U / (1 - n U): the bound of a float32 sum of n terms, in units of the sum of absolute values."""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------- lists
def cn_lists(A, u, v):
    """-> (ptr int64[B + 1], w int32[M]): per pair np.intersect1d of the stored rows u[b] and v[b], ascending; a pair with an id
    outside [0, n) lists nothing."""
    A = ssp.csr_matrix(A)
    A.sort_indices()
    n, ip, ix = A.shape[0], A.indptr, A.indices
    segs = []
    for a, b in zip(np.asarray(u, np.int64), np.asarray(v, np.int64)):
        if 0 <= a < n and 0 <= b < n:
            segs.append(np.intersect1d(ix[ip[a]:ip[a + 1]], ix[ip[b]:ip[b + 1]], assume_unique=True))
        else:
            segs.append(np.zeros(0, ix.dtype))
    ptr = np.zeros(len(segs) + 1, np.int64)
    np.cumsum(np.asarray([len(s) for s in segs], np.int64), out=ptr[1:])
    w = np.concatenate(segs).astype(np.int32) if segs else np.zeros(0, np.int32)
    return ptr, w


def transpose_stable(ptr, w, n):
    """-> (tptr int64[n + 1], tb int32[M]): for every node the pairs that list it, ascending in b (a stable sort of (w, b))."""
    ptr, w = np.asarray(ptr, np.int64), np.asarray(w, np.int64)
    b_of = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    order = np.argsort(w, kind="stable")
    tptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(w, minlength=n), out=tptr[1:])
    return tptr, b_of[order].astype(np.int32)


def incidence(ptr, w, n):
    """The lists as a scipy CSR [B x n] of float64 ones."""
    return ssp.csr_matrix((np.ones(len(w)), np.asarray(w, np.int64), np.asarray(ptr, np.int64)), shape=(len(ptr) - 1, n))


# ---------------------------------------------------------------------------------------------------------- sums
def seq_sum_f32(ptr, idx, x):
    """out[r] = the float32 sum of the rows x[idx[k]], k = ptr[r] .. ptr[r + 1] - 1, added ONE AFTER THE OTHER in that order
    starting from 0 (every add rounded to float32): what a sequential fma chain with unit factors computes, bit for bit."""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((len(ptr) - 1, x.shape[1]), np.float32)
    length = np.diff(ptr)
    rows = np.argsort(-length, kind="stable")                # longest first: the active rows are a prefix
    n_active = len(rows)
    for t in range(int(length.max(initial=0))):
        while n_active and length[rows[n_active - 1]] <= t:
            n_active -= 1
        act = rows[:n_active]
        out[act] = out[act] + x[idx[ptr[act] + t]]
    return out


def sum_f64(ptr, idx, x, n_cols):
    """-> (the same sums in float64, the sums of absolute values): the truth and the scale of its rounding bound."""
    C = incidence(ptr, idx, n_cols)
    x = np.asarray(x, np.float64)
    return C @ x, C @ np.abs(x)


# ---------------------------------------------------------------------------------------------------------- the model
def ncn_predictor(hij, z, p, beta=1.0, prefix="linkpred.", branch=None, pre=None):
    """NCNPredictor without dropout, in the dtype of its inputs -> [B]:
    t = relu(xij_lin(hij)) + beta relu(xcn_lin(z)); t = relu(lin(t)) for lins[:-1]; sigmoid(lins[-1](t))."""
    t = (tt._relu(hij @ p[prefix + "xij_lin.weight"].t() + p[prefix + "xij_lin.bias"], branch, pre)
         + beta * tt._relu(z @ p[prefix + "xcn_lin.weight"].t() + p[prefix + "xcn_lin.bias"], branch, pre))
    m = tt._count(p, prefix + "lins.{}.weight")
    for i in range(m - 1):
        t = tt._relu(t @ p[prefix + f"lins.{i}.weight"].t() + p[prefix + f"lins.{i}.bias"], branch, pre)
    return torch.sigmoid(t @ p[prefix + f"lins.{m - 1}.weight"].t() + p[prefix + f"lins.{m - 1}.bias"]).squeeze(1)


def ncn_forward(kind, p, A, P, x, edges, beta=1.0, branch=None, pre=None):
    """NCNLinkGNN(emb, GCN | SAGE, NCNPredictor) in training mode with dropout 0 -> scores [B], dense: the encoder of
    ``training_truth.link_gnn_forward``, then z = (P[u] * P[v]) @ h -- the common STORED neighbours of the adjacency's pattern
    P -- and ``ncn_predictor``.  ``branch`` / ``pre``: see ``training_truth._relu`` (forward order: the GNN's ReLUs, xij_lin,
    xcn_lin, lins[:-1])."""
    branch = None if branch is None else iter(branch)
    dt = A.dtype
    xin = x.to(dt) if "emb.weight" not in p else (p["emb.weight"] if x is None else torch.cat([p["emb.weight"], x.to(dt)], 1))
    if kind == "gcn":
        L = tt._count(p, "gnn.convs.{}.weight")
        h = tt.gcn_stack(tt.gcn_matrix(A), xin, [p[f"gnn.convs.{i}.weight"] for i in range(L)],
                         [p[f"gnn.convs.{i}.bias"] for i in range(L)], branch, pre)
    else:
        L = tt._count(p, "gnn.convs.{}.lin_l.weight")
        h = tt.sage_stack(tt.mean_matrix(P), xin, [p[f"gnn.convs.{i}.lin_l.weight"] for i in range(L)],
                          [p[f"gnn.convs.{i}.lin_l.bias"] for i in range(L)], [p[f"gnn.convs.{i}.lin_r.weight"] for i in range(L)],
                          branch, pre)
    z = (P[edges[0]] * P[edges[1]]) @ h
    return ncn_predictor(h[edges[0]] * h[edges[1]], z, p, beta, "linkpred.", branch, pre)


# ---------------------------------------------------------------------------------------------------------- the boundary graph
def boundary_lengths(cap, ratio):
    """The row lengths at which the list kernel changes its path: empty, one entry, around a 64-lane slice, around the staging
    capacity, a second and third pass, and a hub that every other row searches in place."""
    return [0, 1, 63, 64, 65, cap - 1, cap, cap + 1, 2 * cap + 1, max(40000, ratio * 65 + 1)]


def boundary_graph(cap, ratio, seed=5):
    """-> (A scipy CSR float32 symmetric pattern with values in 1..3, special node ids, stranger id).

    Node i < k has EXACTLY boundary_lengths()[i] stored entries, all among the 'filler' nodes; its first ceil(L / 2) entries
    are a prefix of one fixed order of the filler nodes, so any two non-empty special rows share common neighbours.  Node k,
    the stranger, has 64 entries in a reserved block no special row touches: paired with a special row it runs the same path
    and finds nothing.  Filler nodes are joined among themselves too (random pairs have matches)."""
    rng = np.random.default_rng(seed)
    lengths = boundary_lengths(cap, ratio)
    k = len(lengths)
    n = max(lengths) + 2200
    reserved = np.arange(k + 1, k + 65)                       # the stranger's neighbours
    pool = rng.permutation(np.arange(k + 65, n))
    assert len(pool) >= max(lengths)
    rows, cols = [np.full(64, k)], [reserved]
    for i, L in enumerate(lengths):
        head = (L + 1) // 2
        rest = rng.choice(pool[head:], size=L - head, replace=False) if L > head else np.zeros(0, np.int64)
        rows.append(np.full(L, i)); cols.append(np.concatenate([pool[:head], rest]))
    extra = rng.integers(k + 65, n, (2, 2 * n))
    extra = extra[:, extra[0] != extra[1]]
    r, c = np.concatenate(rows + [extra[0]]), np.concatenate(cols + [extra[1]])
    P = ssp.coo_matrix((np.ones(len(r)), (r, c)), shape=(n, n)).tocsr()
    P = ((P + P.T) > 0).astype(np.float64).tocsr()
    up = ssp.triu(P, 1).tocoo()
    W = ssp.coo_matrix((rng.integers(1, 4, up.nnz).astype(np.float64), (up.row, up.col)), shape=(n, n)).tocsr()
    A = (W + W.T).tocsr().astype(np.float32)
    A.sort_indices()
    assert np.diff(A.indptr)[:k].tolist() == lengths and np.diff(A.indptr)[k] == 64
    return A, np.arange(k), k


def boundary_pairs(A, special, stranger, n_random=1000, seed=6):
    """Every ordered pair of the boundary rows and the stranger, u == v for each of them, and ``n_random`` random pairs drawn
    with duplicates -> (u, v) int32."""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([special, [stranger]])
    uu, vv = np.meshgrid(ids, ids, indexing="ij")             # (every ordered pair, the diagonal included)
    rnd = rng.integers(0, A.shape[0], (2, n_random - 100))
    dup = rnd[:, rng.integers(0, rnd.shape[1], 100)]
    u = np.concatenate([uu.ravel(), rnd[0], dup[0]]).astype(np.int32)
    v = np.concatenate([vv.ravel(), rnd[1], dup[1]]).astype(np.int32)
    return u, v
