"""The truth the GNN training path (models._SpMM, GCNConv / SAGEConv / TAGConv in training mode, training.train) is held to:
dense, differentiable restatements of the training forwards on torch autograd, and the closed forms of the SpMM backward for a
GENERAL matrix in scipy float64.  A plain helper module (no fixtures); tests/test_training_host.py validates it on the CPU
against the oracle and against autograd, the GPU tests compare the HIP path with it.

The dense restatements compute in the dtype of the tensors they are given: float64 is the truth, the same functions on float32
tensors are the "plain float32 torch formulation" whose own distance to float64 some gates are relative to.

Parameters come as a dict keyed like ``model.named_parameters()`` / ``model.state_dict()`` (``params_as``)."""
import numpy as np
import scipy.sparse as ssp
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def params_as(model, dtype, buffers=False):
    """Leaf copies of the model's parameters (and, with ``buffers``, its floating-point buffers, without grad) in ``dtype``."""
    out = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in model.named_parameters()}
    if buffers:
        out.update({k: v.detach().to(dtype).clone() for k, v in model.named_buffers() if v.dtype.is_floating_point})
    return out


# ---------------------------------------------------------------------------------------------------------- matrices
def dense_adjacency(adj, dtype=torch.float64, device=None):
    """The stored matrix of a CSRGraph as a dense tensor (implicit values are ones; stored zeros stay zeros)."""
    A = torch.from_numpy(adj.to_scipy().toarray()).to(dtype)
    return A if device is None else A.to(device)


def dense_pattern(adj, dtype=torch.float64, device=None):
    """1 at every STORED entry of a CSRGraph (a stored value of 0 still counts: the mean runs over the pattern)."""
    g = adj.cpu()
    P = ssp.csr_matrix((np.ones(g.nnz()), g.col.numpy(), g.rowptr.numpy()), shape=(g.n_rows, g.n_cols)).toarray()
    P = torch.from_numpy(P).to(dtype)
    return P if device is None else P.to(device)


def _inv_sqrt(deg):
    return torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))      # (A takes no gradient: the inf branch is inert)


def gcn_matrix(A):
    """GCNConv's aggregate: A with its diagonal SET to 1, scaled D^-1/2 . D^-1/2 with D its row sums (any positive values)."""
    Ah = A.clone()
    Ah.fill_diagonal_(1.0)
    dis = _inv_sqrt(Ah.sum(1))
    return dis[:, None] * Ah * dis[None, :]


def tag_matrix(A):
    """TAGConv's aggregate: D^-1/2 A D^-1/2 with D the row sums of A as stored (no self loops added), inf -> 0."""
    dis = _inv_sqrt(A.sum(1))
    return dis[:, None] * A * dis[None, :]


def mean_matrix(P):
    """SAGEConv's aggregate over the pattern P: D^-1 P with D = clamp(row count, min=1) (an isolated row aggregates to 0)."""
    return P / P.sum(1).clamp(min=1)[:, None]


# ---------------------------------------------------------------------------------------------------------- forwards
def _relu(z, branch, pre):
    """ReLU.  ``pre`` (a list) collects the pre-activation.  ``branch`` (an iterator of boolean masks) replaces the ReLU by
    z * mask: the piecewise-linear function restricted to the branch ANOTHER forward took.  ReLU has no derivative at 0, so
    where a float32 forward and this one disagree on the sign of a pre-activation that float32 cannot tell from 0, only the
    gradients on a common branch can be compared."""
    if pre is not None:
        pre.append(z.detach())
    return torch.relu(z) if branch is None else z * next(branch).to(z.dtype)


def gcn_stack(An, x, weights, biases, branch=None, pre=None):
    """h <- An (h W) + b, ReLU after every layer but the last.  ``weights[l]`` is [in, out]."""
    h = x
    for l, (w, b) in enumerate(zip(weights, biases)):
        h = An @ (h @ w) + b
        if l + 1 < len(weights):
            h = _relu(h, branch, pre)
    return h


def sage_stack(Dn, x, w_l, b_l, w_r, branch=None, pre=None):
    """h <- lin_l(Dn h) + lin_r(h), ReLU after every layer but the last.  Linear layout [out, in]; lin_r has no bias."""
    h = x
    for l in range(len(w_l)):
        h = (Dn @ h) @ w_l[l].t() + b_l[l] + h @ w_r[l].t()
        if l + 1 < len(w_l):
            h = _relu(h, branch, pre)
    return h


def link_predictor(h, edges, ws, bs, branch=None, pre=None):
    """LinkPredictor's training forward without dropout: Hadamard -> (L-1) x [Linear, ReLU] -> Linear -> sigmoid, [B]."""
    z = h[edges[0]] * h[edges[1]]
    for w, b in zip(ws[:-1], bs[:-1]):
        z = _relu(z @ w.t() + b, branch, pre)
    return torch.sigmoid(z @ ws[-1].t() + bs[-1]).squeeze(1)


def _count(p, fmt):
    n = 0
    while fmt.format(n) in p:
        n += 1
    return n


def link_gnn_forward(kind, p, A, P, x, edges, branch=None, pre=None):
    """LinkGNN(emb, GCN | SAGE, LinkPredictor) in training mode with dropout 0 -> scores [B] in (0, 1).  ``A``: the dense
    adjacency (values), ``P``: its dense pattern; ``x``: features or None; the embedding comes FIRST in the input.
    ``branch`` / ``pre``: see ``_relu`` (masks in forward order: the GNN's ReLUs, then the decoder's)."""
    branch = None if branch is None else iter(branch)
    dt = A.dtype
    xin = x.to(dt) if "emb.weight" not in p else (p["emb.weight"] if x is None else torch.cat([p["emb.weight"], x.to(dt)], 1))
    if kind == "gcn":
        L = _count(p, "gnn.convs.{}.weight")
        h = gcn_stack(gcn_matrix(A), xin, [p[f"gnn.convs.{i}.weight"] for i in range(L)],
                      [p[f"gnn.convs.{i}.bias"] for i in range(L)], branch, pre)
    else:
        L = _count(p, "gnn.convs.{}.lin_l.weight")
        h = sage_stack(mean_matrix(P), xin, [p[f"gnn.convs.{i}.lin_l.weight"] for i in range(L)],
                       [p[f"gnn.convs.{i}.lin_l.bias"] for i in range(L)], [p[f"gnn.convs.{i}.lin_r.weight"] for i in range(L)],
                       branch, pre)
    M = _count(p, "linkpred.lins.{}.weight")
    return link_predictor(h, edges, [p[f"linkpred.lins.{i}.weight"] for i in range(M)],
                          [p[f"linkpred.lins.{i}.bias"] for i in range(M)], branch, pre)


def _batch_norm(z, p, pre):
    return F.batch_norm(z, p[pre + ".running_mean"], p[pre + ".running_var"], p[pre + ".weight"], p[pre + ".bias"],
                        training=True, momentum=0.1, eps=BN_EPS)


def dea_forward(p, A, x, edges, jk_mode="max"):
    """DEA_GNN_JK in training mode with dropout 0 -> logits [B]: [emb || x] -> layers x [TAGConv(K=2), BatchNorm, ReLU] ->
    jumping knowledge -> Hadamard -> (L-1) x [Linear, BatchNorm, ReLU] -> Linear.  BatchNorm runs on batch statistics and
    updates the running statistics in ``p`` in place, like the module does."""
    dt = A.dtype
    An = tag_matrix(A)
    cur = p["emb.weight"] if x is None else torch.cat([p["emb.weight"], x.to(dt)], 1)
    outs = []
    for i in range(_count(p, "convs.{}.lin.weight")):
        hs = torch.cat([cur, An @ cur, An @ (An @ cur)], 1)
        z = hs @ p[f"convs.{i}.lin.weight"].t() + p[f"convs.{i}.lin.bias"]
        cur = torch.relu(_batch_norm(z, p, f"gnn_bns.{i}"))
        outs.append(cur)
    if jk_mode == "max":
        h = torch.stack(outs).max(0).values
    else:
        h = torch.stack(outs).sum(0)
        if jk_mode == "mean":
            h = h / len(outs)
    z = h[edges[0]] * h[edges[1]]
    M = _count(p, "lins.{}.weight")
    for i in range(M - 1):
        z = torch.relu(_batch_norm(z @ p[f"lins.{i}.weight"].t() + p[f"lins.{i}.bias"], p, f"mlp_bns.{i}"))
    return (z @ p[f"lins.{M - 1}.weight"].t() + p[f"lins.{M - 1}.bias"]).squeeze(1)


# ---------------------------------------------------------------------------------------------------------- losses
def log_loss(out, n_pos):
    """training.train for gcn / sage: -log(pos + 1e-8).mean() - log(1 - neg + 1e-8).mean(); the first n_pos scores are positives."""
    return -torch.log(out[:n_pos] + 1e-8).mean() - torch.log(1 - out[n_pos:] + 1e-8).mean()


def bce_logits_loss(logits, label):
    """training.train for dea / dea_512: BCEWithLogitsLoss against 1 / 0 labels."""
    return F.binary_cross_entropy_with_logits(logits, label.to(logits.dtype))


# ---------------------------------------------------------------------------------------------------------- SpMM closed forms
def _f64(A):
    A = ssp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def pattern_of(A):
    """1.0 at every stored entry of a scipy matrix (explicit zeros included)."""
    A = _f64(A)
    return ssp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)


def row_counts(A):
    return np.diff(_f64(A).indptr).astype(np.float64)


def spmm_forward(A, X, mean):
    """sum: Y = A X;  mean: Y = D^-1 P X with P the pattern of A and D = max(stored entries per row, 1).  float64."""
    X = np.asarray(X, np.float64)
    if not mean:
        return _f64(A) @ X
    return (pattern_of(A) @ X) / np.maximum(row_counts(A), 1.0)[:, None]


def spmm_backward(A, dY, mean):
    """The gradient of ``spmm_forward`` in X for a GENERAL (square or not, symmetric or not) A:
    sum: dX = A^T dY;  mean: dX = P^T (D^-1 dY)."""
    dY = np.asarray(dY, np.float64)
    if not mean:
        return _f64(A).T @ dY
    return pattern_of(A).T @ (dY / np.maximum(row_counts(A), 1.0)[:, None])


def spmm_backward_shortcut(A, dY, mean):
    """What models._SpMM.backward computes: the product with A itself in place of A^T (sum: A dY; mean: P (D^-1 dY)).
    Equal to ``spmm_backward`` exactly when A (the pattern, for mean) equals its transpose."""
    dY = np.asarray(dY, np.float64)
    if not mean:
        return _f64(A) @ dY
    return pattern_of(A) @ (dY / np.maximum(row_counts(A), 1.0)[:, None])
