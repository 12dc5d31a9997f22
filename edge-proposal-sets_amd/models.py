"""GCN / SAGE / LinkPredictor / LinkGNN / DEA_GNN_JK / CommonNeighborsPredictor with the reference's class
names, constructor signatures, ``forward`` signatures and state-dict keys (models.py:36-133, :163-187,
:417-440, :461-485, :487-506, :508-575, :578-670, :673-790) -- the forward passes run on the
hand-written HIP kernels (csrc/) instead of torch_geometric / torch_sparse / cuBLAS.

Scoring signature kept: ``model(x, edges[2,B], adj_t) -> scores`` ([B,1] for LinkGNN, [B] for
CommonNeighborsPredictor('simple')).

Scope: the scoring loops (filter.py:113-121, train_and_eval.py:108-136: ``model.eval()`` / ``torch.no_grad()``)
run entirely on the HIP kernels.  Training (train_and_eval.py:31-96) runs on torch autograd
with the HIP SpMM as a custom autograd Function (forward and backward) and the dense layers on torch.

What differs from the reference on purpose: ``LinkGNN`` computes the node embeddings ``h`` ONCE per
(parameters, x, adjacency) and reuses them for every scoring batch; the reference re-runs the whole
GNN for each batch (models.py:505 called from filter.py:118).  Results are identical in eval mode.

Beyond the reference: ``NCNPredictor`` / ``NCNLinkGNN`` (``--model ncn | ncn_sage``), Neural Common Neighbor on the
common-neighbour lists of csrc/pair_cn_list.hip (``cn_embed_sum``); ``BuddyPredictor`` / ``BuddyLinkModel`` (``--model buddy``),
BUDDY on the subgraph sketches of csrc/sketch.hip (``heuristics.sketch_features``); ``GATConv`` / ``GAT`` (``--model gat``), a
graph-attention encoder on the fused softmax-and-gather kernels of csrc/gat_attend.hip.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import ops
from .graph import CSRGraph
from . import heuristics


class _SpMM(torch.autograd.Function):
    """Differentiable CSR x dense aggregate for TRAINING (train_and_eval.py:31-96): forward and backward both run
    eps_spmm_csr.  The gradient of Y = A X is dX = A^T dY; the backward multiplies by A itself, which is that gradient only
    when A equals its transpose:
      sum : Y = A X          ->  dX = A dY               (pattern AND values symmetric)
      mean: Y = D^-1 P X     ->  dX = P (D^-1 dY)        (P the pattern, symmetric; values are not read)
    Every adjacency the reference builds is symmetric (rank.py:33), and the convs refuse any other one in training mode
    (``_check_trainable``) BEFORE they get here: this Function itself checks nothing.  The normalised copies the convs pass
    (graph.gcn_normalized / tag_normalized) hold (val * dis[r]) * dis[c], so their mirrored entries can differ in the last
    bit; that is rounding of the same size as the product's own and is accepted."""

    @staticmethod
    def forward(ctx, x, graph, mean):
        ctx.graph, ctx.mean = graph, mean
        return ops.spmm_csr(graph.rowptr, graph.col, None if mean else graph.val, x.contiguous(), mean=mean)

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.graph
        grad_out = grad_out.contiguous()
        if ctx.mean:
            inv = 1.0 / g.degree().clamp(min=1).to(torch.float32)
            grad_out = (grad_out * inv[:, None]).contiguous()
        return ops.spmm_csr(g.rowptr, g.col, None if ctx.mean else g.val, grad_out), None, None


def _pad4_full(x: torch.Tensor):
    """-> (view [N,K], full [N,ld]) with ld = K rounded up to a multiple of 4 floats and zero pad columns:
    16-B aligned rows let the GEMM / SpMM kernels use 16-byte loads; K itself is unchanged."""
    n, k = x.shape
    ld = (k + 3) // 4 * 4
    if ld == k and x.is_contiguous() and x.data_ptr() % 16 == 0:
        return x, x
    buf = torch.zeros((n, ld), dtype=torch.float32, device=x.device)
    buf[:, :k] = x
    return buf[:, :k], buf


def _pad4(x: torch.Tensor) -> torch.Tensor:
    if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0:
        return x
    return _pad4_full(x)[0]


def _check_rows(x: torch.Tensor, adj_t: CSRGraph, who: str) -> None:
    """The SpMM gathers x[col] unchecked: x must have one row per column of the adjacency."""
    if x.dim() != 2 or x.shape[0] != adj_t.n_cols:
        raise ValueError(f"{who}: x must have one row per column of the adjacency ({adj_t.n_cols}), got {tuple(x.shape)}")


def _check_trainable(adj_t: CSRGraph, who: str, values: bool) -> None:
    """Training through _SpMM needs the adjacency THE CALLER PASSED to equal its transpose: its pattern, and for the convs
    that read them (``values``) its stored values.  (Not the normalised copy: that one is symmetric only up to a rounding.)
    Both verdicts are cached on the graph, so only the first step pays for them."""
    from . import scan
    from ._lib import EpsError
    if adj_t.n_rows != adj_t.n_cols or not scan.is_symmetric(adj_t):
        raise EpsError(f"{who}: training needs an adjacency with a symmetric pattern (the backward multiplies by A in "
                       f"place of A^T); scoring under eval() / no_grad() takes any graph")
    if values and not heuristics.values_are_symmetric(adj_t):
        raise EpsError(f"{who}: training needs an adjacency with symmetric values (the backward multiplies by A in place "
                       f"of A^T); scoring under eval() / no_grad() takes any graph")


# ----------------------------------------------------------------------------------- convs
class GCNConv(torch.nn.Module):
    """torch_geometric 1.7.0 GCNConv [third-party, restated]: out = D^-1/2 (A with diag := 1) D^-1/2 (x W) + b.
    Parameters as in PyG 1.7: ``weight`` [in,out] (glorot), ``bias`` [out] (zeros).  Checkpoints written by
    PyG >= 2.0 (``lin.weight`` [out,in]) load too."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = torch.nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))  # glorot
        with torch.no_grad():
            self.weight.uniform_(-a, a)
            self.bias.zero_()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k_new = prefix + "lin.weight"
        if k_new in state_dict and prefix + "weight" not in state_dict:
            state_dict[prefix + "weight"] = state_dict.pop(k_new).t()
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x: torch.Tensor, adj_t: CSRGraph, relu: bool = False) -> torch.Tensor:
        _check_rows(x, adj_t, "GCNConv")
        training = torch.is_grad_enabled() and self.training
        if training:
            _check_trainable(adj_t, "GCNConv", values=True)
        gn = adj_t.gcn_normalized()                      # cached per adjacency (eps_gcn_norm)
        if training:                                     # training: HIP SpMM inside autograd, dense part on torch
            out = _SpMM.apply(x @ self.weight, gn, False) + self.bias
            return F.relu(out) if relu else out
        with torch.no_grad():
            return self._forward_hip(x, gn, relu)

    def _forward_hip(self, x, gn, relu, rows=None):
        w_nk = self.weight.detach().t().contiguous()     # [out,in]: the GEMM takes Linear layout
        xw = ops.gemm(_pad4(x), w_nk)                    # transform ...
        rowptr = gn.rowptr if rows is None else gn.rowptr[rows[0]:rows[1] + 1]   # row block: absolute offsets into col
        return ops.spmm_csr(rowptr, gn.col, gn.val, xw, bias=self.bias.detach(), relu=relu)   # ... then aggregate

    @torch.no_grad()
    def forward_rows(self, x: torch.Tensor, adj_t: CSRGraph, lo: int, hi: int, relu: bool = False) -> torch.Tensor:
        """Rows [lo, hi) of the layer output from the FULL input (multi-GPU row sharding, dist.py)."""
        _check_rows(x, adj_t, "GCNConv")
        return self._forward_hip(x, adj_t.gcn_normalized(), relu, rows=(lo, hi))

    def __repr__(self):
        return f"GCNConv({self.in_channels}, {self.out_channels})"


class SAGEConv(torch.nn.Module):
    """torch_geometric 1.7.0 SAGEConv [third-party; semantics witnessed in-tree by models.py:347-349,
    :358-384]: out = lin_l(mean_{j in N(i)} x_j) + lin_r(x_i); mean ignores edge values, no self loop;
    lin_r has no bias."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_l = torch.nn.Linear(in_channels, out_channels, bias=True)
        self.lin_r = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()

    def forward(self, x: torch.Tensor, adj_t: CSRGraph, relu: bool = False) -> torch.Tensor:
        _check_rows(x, adj_t, "SAGEConv")
        if torch.is_grad_enabled() and self.training:
            _check_trainable(adj_t, "SAGEConv", values=False)     # the mean reads the pattern only
            out = self.lin_l(_SpMM.apply(x, adj_t, True)) + self.lin_r(x)
            return F.relu(out) if relu else out
        with torch.no_grad():
            return self._forward_hip(x, adj_t, relu)

    TRANSFORM_FIRST = True     # aggregate lin_l(x) instead of x when the layer narrows (see _forward_hip)

    def _forward_hip(self, x, adj_t, relu, rows=None):
        k = x.shape[1]
        x, x_full = _pad4_full(x)                      # pad columns are zero: aggregate the padded width (float4 path)
        rowptr = adj_t.rowptr if rows is None else adj_t.rowptr[rows[0]:rows[1] + 1]
        x_rows = x if rows is None else x[rows[0]:rows[1]]
        if self.TRANSFORM_FIRST and self.in_channels > self.out_channels and self.out_channels % 4 == 0:
            # the mean commutes with lin_l: mean_j(x_j) W^T == mean_j(x_j W^T).  A layer that narrows (ppa: 58 features +
            # 256-d embedding = 314 -> 256; collab: 384 -> 256) then gathers ONE 1-KiB row of z = x W_l^T per neighbour
            # instead of a 256-column pass plus a partial-row pass over x; lin_l's bias rides in the SpMM's epilogue.
            z = ops.gemm(x, self.lin_l.weight.detach())
            out = ops.spmm_csr(rowptr, adj_t.col, None, z, bias=self.lin_l.bias.detach(), mean=True)
        else:
            agg = ops.spmm_csr(rowptr, adj_t.col, None, x_full, mean=True)[:, :k]
            out = ops.gemm(agg, self.lin_l.weight.detach(), bias=self.lin_l.bias.detach())
        return ops.gemm(x_rows, self.lin_r.weight.detach(), out=out, accumulate=True, relu=relu)

    @torch.no_grad()
    def forward_rows(self, x: torch.Tensor, adj_t: CSRGraph, lo: int, hi: int, relu: bool = False) -> torch.Tensor:
        """Rows [lo, hi) of the layer output from the FULL input (multi-GPU row sharding, dist.py)."""
        _check_rows(x, adj_t, "SAGEConv")
        return self._forward_hip(x, adj_t, relu, rows=(lo, hi))

    def __repr__(self):
        return f"SAGEConv({self.in_channels}, {self.out_channels})"


class _GATAggregate(torch.autograd.Function):
    """Differentiable attention aggregate for TRAINING: ``apply(z, s_src, s_dst, graph, heads)`` -> the aggregate without bias
    and ReLU, on eps_gat_aggregate; the backward is eps_gat_aggregate_backward and returns the gradients of ``z`` (the gathered
    features), ``s_src`` and ``s_dst``.  The two score tables are functions of ``z`` on torch, so autograd carries their
    gradients on to ``att_*`` and ``lin.weight``.  The backward sums over the rows that attend to a node along that node's own
    row: the pattern must be symmetric, which GATConv checks (``_check_trainable``) BEFORE it gets here."""

    @staticmethod
    def forward(ctx, z, s_src, s_dst, graph, heads):
        z, s_src, s_dst = z.contiguous(), s_src.contiguous(), s_dst.contiguous()
        out, lse = ops.gat_aggregate(graph.rowptr, graph.col, z, s_src, s_dst, heads, want_lse=True)
        ctx.save_for_backward(z, s_src, s_dst, lse, out)
        ctx.graph, ctx.heads = graph, heads
        return out

    @staticmethod
    def backward(ctx, grad_out):
        z, s_src, s_dst, lse, out = ctx.saved_tensors
        g = ctx.graph
        gz, gs, gd = ops.gat_aggregate_backward(g.rowptr, g.col, z, s_src, s_dst, ctx.heads, lse, out, grad_out.contiguous())
        return gz, gs, gd, None, None


class GATConv(torch.nn.Module):
    """The graph attention layer of Velickovic et al. (ICLR 2018) as torch_geometric publishes it [third-party, restated]:
    ``GATConv(in_channels, out_channels, heads)`` with C = out_channels / heads; the heads are concatenated, so the output
    is ``out_channels`` wide.

    Parameters (the state-dict keys of the published layer): ``lin.weight`` [heads * C, in] (no bias in ``lin``), ``att_src``
    [1, heads, C], ``att_dst`` [1, heads, C], ``bias`` [heads * C]; glorot for ``lin.weight`` and the two ``att_*``, zeros for
    ``bias``.
    Features and scores: z = x W^T viewed as [N, heads, C]; s_src[j,h] = <z[j,h,:], att_src[h,:]>, s_dst[i,h] = <z[i,h,:],
    att_dst[h,:]>.
    Neighbourhood of row i: the stored entries of row i with col != i, plus i itself exactly once -- a stored self loop is not
    counted twice; stored values are ignored; an empty row attends to itself alone, so its output is z[i] + bias.  The
    adjacency must be square.
    Attention: e_ij = LeakyReLU_0.2(s_src[j,h] + s_dst[i,h]), alpha_i.h = softmax_j e_ij.
    Output: out[i,h,:] = sum_j alpha_ijh z[j,h,:] + bias, optionally followed by ReLU.
    Not built: attention dropout, edge features, ``concat=False``, GATv2.

    Eval runs on the HIP kernels: the transform is ``ops.gemm``, the two score tables are a second small product of z with the
    block-diagonal [2 heads, heads * C] matrix of ``att_src`` / ``att_dst`` (the same sums, over the same z, as training
    forms), the aggregate is eps_gat_aggregate with the bias and the ReLU in its epilogue.  Training runs the aggregate and its
    backward on the HIP kernels inside autograd (``_GATAggregate``) and the dense part on torch."""

    SLOPE = ops.GAT_SLOPE

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1):
        super().__init__()
        if heads < 1 or out_channels % heads:
            raise ValueError(f"GATConv: out_channels {out_channels} is not a multiple of heads {heads}")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels // heads))
        self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels // heads))
        self.bias = torch.nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            torch.nn.init.xavier_uniform_(self.lin.weight)       # glorot
            torch.nn.init.xavier_uniform_(self.att_src)
            torch.nn.init.xavier_uniform_(self.att_dst)
            self.bias.zero_()

    def _att_matrix(self, pad: bool) -> torch.Tensor:
        """[2 heads (rounded up to 4 rows with ``pad``), heads * C]: row h holds att_src[h, :] in head h's columns, row heads + h
        att_dst[h, :], zeros elsewhere -- z times its transpose is [s_src || s_dst].  Differentiable in ``att_*``."""
        h, c = self.heads, self.out_channels // self.heads
        eye = torch.eye(h, dtype=self.att_src.dtype, device=self.att_src.device)[:, :, None]
        rows = [(eye * a.view(1, h, c)).reshape(h, h * c) for a in (self.att_src, self.att_dst)]
        if pad and (2 * h) % 4:
            rows.append(rows[0].new_zeros((4 - (2 * h) % 4, h * c)))
        return torch.cat(rows, 0)

    @staticmethod
    def _check_square(adj_t: CSRGraph) -> None:
        if adj_t.n_rows != adj_t.n_cols:
            raise ValueError(f"GATConv: the self loop needs a square adjacency, got {adj_t.n_rows} x {adj_t.n_cols}")

    def forward(self, x: torch.Tensor, adj_t: CSRGraph, relu: bool = False) -> torch.Tensor:
        _check_rows(x, adj_t, "GATConv")
        self._check_square(adj_t)
        if torch.is_grad_enabled() and self.training:
            _check_trainable(adj_t, "GATConv", values=False)      # the attention reads the pattern only
            h = self.heads
            z = self.lin(x)
            s = z @ self._att_matrix(False).t()
            out = _GATAggregate.apply(z, s[:, :h], s[:, h:2 * h], adj_t, h) + self.bias
            return F.relu(out) if relu else out
        with torch.no_grad():
            return self._forward_hip(x, adj_t, relu)

    def _forward_hip(self, x, adj_t, relu, rows=None):
        h = self.heads
        z = ops.gemm(_pad4(x), self.lin.weight.detach())         # transform ...
        s = ops.gemm(z, self._att_matrix(True).detach().contiguous())         # ... the two score tables, [N, 2 heads (+ pad)] ...
        lo, hi = (0, adj_t.n_rows) if rows is None else rows
        rowptr = adj_t.rowptr if rows is None else adj_t.rowptr[lo:hi + 1]     # row block: absolute offsets into col
        return ops.gat_aggregate(rowptr, adj_t.col, z, s[:, :h], s[:, h:2 * h], h, row0=lo, slope=self.SLOPE,
                                 bias=self.bias.detach(), relu=relu)           # ... then attend

    @torch.no_grad()
    def forward_rows(self, x: torch.Tensor, adj_t: CSRGraph, lo: int, hi: int, relu: bool = False) -> torch.Tensor:
        """Rows [lo, hi) of the layer output from the FULL input (multi-GPU row sharding, dist.py)."""
        _check_rows(x, adj_t, "GATConv")
        self._check_square(adj_t)
        return self._forward_hip(x, adj_t, relu, rows=(lo, hi))

    def __repr__(self):
        return f"GATConv({self.in_channels}, {self.out_channels}, heads={self.heads})"


class _ConvStack(torch.nn.Module):
    conv_cls = None

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__()
        self.convs = torch.nn.ModuleList()
        self.convs.append(self.conv_cls(in_channels, hidden_channels))
        for _ in range(num_layers - 2):
            self.convs.append(self.conv_cls(hidden_channels, hidden_channels))
        self.convs.append(self.conv_cls(hidden_channels, out_channels))
        self.dropout = dropout

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x, adj_t):
        # models.py:181-187 / :434-440: ReLU (+ dropout, identity in eval) after every layer but the last;
        # the ReLU rides in the producing kernel's epilogue.
        for conv in self.convs[:-1]:
            x = conv(x, adj_t, relu=True)
            x = F.dropout(x, p=self.dropout, training=self.training)   # identity in eval mode
        return self.convs[-1](x, adj_t)


    @torch.no_grad()
    def forward_sharded(self, x, adj_t, rank: int, world: int, gather):
        """Multi-GPU forward (inference): the last layer -- the one whose output every rank needs in full for the
        decode -- is computed for this rank's row block only and exchanged with ONE all-gather (``gather(local,
        bounds)``, dist.all_gather_rows: N x H x 4 B over xGMI); the layers before it are replicated (tens of ms at
        these sizes: cheaper than an all-gather per layer)."""
        for conv in self.convs[:-1]:
            x = conv(x, adj_t, relu=True)
        n = adj_t.n_rows
        bounds = [n * r // world for r in range(world + 1)]
        local = self.convs[-1].forward_rows(x, adj_t, bounds[rank], bounds[rank + 1])
        return gather(local, bounds)


class GCN(_ConvStack):
    """models.py:163-187."""
    conv_cls = GCNConv


class SAGE(_ConvStack):
    """models.py:417-440."""
    conv_cls = SAGEConv


GAT_HEADS = 4                    # --gat_heads default


class GAT(_ConvStack):
    """A stack of GATConv layers in the mould of GCN / SAGE (beyond the reference): every layer concatenates its ``heads`` heads,
    so the stack keeps the width ``hidden_channels`` throughout; ReLU (+ dropout) after every layer but the last."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, heads=GAT_HEADS):
        import functools
        object.__setattr__(self, "conv_cls", functools.partial(GATConv, heads=int(heads)))   # (bound before the stack is built)
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout)
        self.heads = int(heads)


REORDER_MIN_NODES = 100_000      # graphs from this size on run their GNN layers on the hubs-first relabelling


# ----------------------------------------------------------------------------------- decode
DECODE_PRECISIONS = ("fp32", "bf16")


class _FusedDecode(torch.autograd.Function):
    """The training decode on csrc/mlp_decode_train.hip: ``apply(h, edges, keep, keep_scale, *weights, *biases)`` -> scores [B].
    ``edges``: int32 [2, B], ids checked by the caller; ``keep``: packed dropout masks (ops.pack_mask) or None.  The backward
    recomputes the forward tile by tile (nothing but the inputs is saved) and is reproducible bit for bit."""

    @staticmethod
    def forward(ctx, h, edges, keep, keep_scale, *wb):
        L = len(wb) // 2
        h = h.contiguous()
        ws, bs = [w.contiguous() for w in wb[:L]], [b.contiguous() for b in wb[L:]]
        ctx.save_for_backward(h, edges, keep, *ws, *bs)
        ctx.keep_scale = keep_scale
        return ops.mlp_decode_train(h, edges[0], edges[1], ws, bs, keep=keep, keep_scale=keep_scale)

    @staticmethod
    def backward(ctx, grad_out):
        h, edges, keep, *wb = ctx.saved_tensors
        L = len(wb) // 2
        need = ctx.needs_input_grad
        gh, gw, gb = ops.mlp_decode_backward(h, edges[0], edges[1], wb[:L], wb[L:], grad_out.contiguous(), keep=keep,
                                             keep_scale=ctx.keep_scale, want_h=need[0], want_params=any(need[4:]))
        return (gh, None, None, None, *(gw or [None] * L), *(gb or [None] * L))


def fold_batch_statistics(weight, bias, gamma, beta, mean, var, eps: float):
    """(W', b') such that x W'^T + b' == gamma (x W^T + b - mean) / sqrt(var + eps) + beta: ``fold_batchnorm`` on the statistics of
    the batch at hand.  Formed in float64, returned in W's dtype; parameter-sized."""
    f = torch.float64
    s = gamma.to(f) / torch.sqrt(var.to(f) + eps)
    return ((weight.to(f) * s[:, None]).to(weight.dtype).contiguous(),
            (s * (bias.to(f) - mean.to(f)) + beta.to(f)).to(bias.dtype).contiguous())


class _FusedDecodeBN(torch.autograd.Function):
    """DEA_GNN_JK's two-layer training decode on csrc/mlp_decode_train.hip: ``apply(h, edges, keep, keep_scale, mean, var, eps,
    W0, b0, gamma, beta, w1, b1)`` -> logits [B].  ``mean`` / ``var``: the batch statistics of the hidden pre-activation
    (ops.mlp_decode_bn_stats), constants here: the backward carries the statistics' own dependence on h and W0 itself.  The
    forward folds the BatchNorm into the hidden layer (``fold_batch_statistics``) and is
    eps_mlp_decode_train on the folded layer; nothing but the inputs and that layer is saved."""

    @staticmethod
    def forward(ctx, h, edges, keep, keep_scale, mean, var, eps, w0, b0, gamma, beta, w1, b1):
        h = h.contiguous()
        w0, b0, gamma, beta, w1, b1 = (t.detach().contiguous() for t in (w0, b0, gamma, beta, w1, b1))
        wf, bf = fold_batch_statistics(w0, b0, gamma, beta, mean, var, eps)
        ctx.save_for_backward(h, edges, keep, mean, var, w0, b0, gamma, w1, b1, wf, bf)
        ctx.keep_scale, ctx.eps = keep_scale, eps
        return ops.mlp_decode_train(h, edges[0], edges[1], [wf, w1], [bf, b1], keep=keep, keep_scale=keep_scale, apply_sigmoid=False)

    @staticmethod
    def backward(ctx, grad_out):
        h, edges, keep, mean, var, w0, b0, gamma, w1, b1, wf, bf = ctx.saved_tensors
        gh, gw, gb, gg, gbeta = ops.mlp_decode_bn_backward(h, edges[0], edges[1], [w0, w1], [b0, b1], wf, bf, gamma, mean, var, ctx.eps,
                                                           grad_out.contiguous(), keep=keep, keep_scale=ctx.keep_scale,
                                                           want_h=ctx.needs_input_grad[0])
        return (gh, None, None, None, None, None, None, gw[0], gb[0], gg, gbeta, gw[1], gb[1])


def _check_precision(precision: str) -> None:
    if precision not in DECODE_PRECISIONS:
        raise ValueError(f"decode precision '{precision}': one of {', '.join(DECODE_PRECISIONS)}")


def _bf16_decoder(module, layers):
    """(weights, biases) of a decoder for eps_mlp_decode_bf16: ``layers()`` gives the float32 layers (any BatchNorm folded in
    already, in float32); the hidden weights are rounded to bf16 AFTER that, the last layer and the biases stay float32.
    Cached on ``module`` per version of its parameters and buffers."""
    key = (tuple((p.data_ptr(), p._version) for p in module.parameters()),
           tuple((b.data_ptr(), b._version) for b in module.buffers()))
    if getattr(module, "_bf16_key", None) != key:
        ws, bs = layers()
        module._bf16_layers = ([ops.to_bf16(w) for w in ws[:-1]] + [ws[-1]], bs)
        module._bf16_key = key
    return module._bf16_layers


class LinkPredictor(torch.nn.Module):
    """models.py:461-485: Hadamard -> (L-1) x [Linear, ReLU, dropout] -> Linear(hidden, out) -> sigmoid."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__()
        self.lins = torch.nn.ModuleList()
        self.lins.append(torch.nn.Linear(in_channels, hidden_channels))
        for _ in range(num_layers - 2):
            self.lins.append(torch.nn.Linear(hidden_channels, hidden_channels))
        self.lins.append(torch.nn.Linear(hidden_channels, out_channels))
        self.dropout = dropout

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()

    @torch.no_grad()
    def decode(self, h: torch.Tensor, edges: torch.Tensor, apply_sigmoid: bool = True, precision: str = "fp32") -> torch.Tensor:
        """Fused gather + MLP + sigmoid over edges [2,B] (eps_mlp_decode) -> float32 [B].  Inference only.
        ``precision="bf16"``: the screening decode on the bf16 matrix cores (eps_mlp_decode_bf16); ``h`` is then the float32
        table (converted here) or its bf16 bit patterns (int16, ``_CachedEmbeddings.embeddings_bf16``: converted once)."""
        heuristics.check_node_ids(edges, h.shape[0], "decode edges")   # the kernel gathers h[u], h[v] unchecked
        e = edges.to(device=h.device, dtype=torch.int32)
        if precision == "bf16":
            ws, bs = _bf16_decoder(self, self._decoder_layers)
            hb = h.contiguous() if h.dtype == torch.int16 else ops.to_bf16(h.contiguous())
            return ops.mlp_decode_bf16(hb, e[0].contiguous(), e[1].contiguous(), ws, bs, apply_sigmoid)
        _check_precision(precision)
        ws, bs = self._decoder_layers()
        return ops.mlp_decode(h.contiguous(), e[0].contiguous(), e[1].contiguous(), ws, bs, apply_sigmoid)

    def _decoder_layers(self):
        return ([lin.weight.detach().contiguous() for lin in self.lins], [lin.bias.detach().contiguous() for lin in self.lins])

    def decode_train(self, h: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
        """The training forward over edges [2,B] on the fused kernels (eps_mlp_decode_train / eps_mlp_decode_backward) ->
        float32 [B], differentiable in ``h`` and in the layers.  Dropout: the keep masks are drawn here with torch's current
        device generator (``torch.rand(B, H) >= p`` per hidden layer) and go to the kernel as bits."""
        hd, L = h.shape[1], len(self.lins)
        if h.dim() != 2 or hd % 4 != 0 or not ops.TRAIN_MIN_HIDDEN <= hd <= ops.TRAIN_MAX_HIDDEN or not 2 <= L <= 8 or any(
                tuple(lin.weight.shape) != ((1 if i == L - 1 else hd), hd) for i, lin in enumerate(self.lins)):
            raise ValueError(f"fused training decode: width {hd} with layers {[tuple(lin.weight.shape) for lin in self.lins]} is "
                             f"outside the kernel's domain (one width H for the embedding and every hidden layer, H % 4 == 0, "
                             f"{ops.TRAIN_MIN_HIDDEN} <= H <= {ops.TRAIN_MAX_HIDDEN}, 2 to 8 layers, one output); leave fused_decode off for this model")
        heuristics.check_node_ids(edges, h.shape[0], "decode edges")   # the kernels gather h[u], h[v] unchecked
        e = edges.to(device=h.device, dtype=torch.int32).contiguous()
        keep, scale, p = None, 1.0, float(self.dropout)
        if p > 0:
            b = e.shape[1]
            keep = torch.stack([ops.pack_mask(torch.rand(b, hd, device=h.device) >= p) for _ in range(L - 1)])
            scale = 1.0 / (1.0 - p) if p < 1 else 0.0
        return _FusedDecode.apply(h, e, keep, scale, *[lin.weight for lin in self.lins], *[lin.bias for lin in self.lins])

    def forward(self, x_i: torch.Tensor, x_j: torch.Tensor) -> torch.Tensor:
        """Reference signature: two gathered [B,H] blocks -> [B,1].  (LinkGNN uses decode(), which gathers
        inside the kernel instead of materialising the two blocks.)"""
        if torch.is_grad_enabled() and self.training:   # models.py:478-485 on autograd
            x = x_i * x_j
            for lin in self.lins[:-1]:
                x = F.dropout(F.relu(lin(x)), p=self.dropout, training=True)
            return torch.sigmoid(self.lins[-1](x))
        b = x_i.shape[0]
        h2 = torch.cat([x_i, x_j], 0)
        idx = torch.arange(b, device=x_i.device, dtype=torch.int32)
        return self.decode(h2, torch.stack([idx, idx + b])).unsqueeze(1)


class _CachedEmbeddings:
    """The node embeddings ``h`` of a GNN link model in eval mode, computed ONCE per (parameter and buffer versions, x,
    adjacency) and reused for every scoring batch -- the reference recomputes them for each batch.  Graphs from
    REORDER_MIN_NODES nodes on run the layers on the hubs-first relabelling (graph.degree_ordered: the SpMM's gathers hit
    the cache more often); ``h`` comes back in the caller's node order.  A model supplies ``_node_input(x)`` and
    ``_node_forward(xin, adj)``."""
    _h_key = None
    _h = None

    @torch.no_grad()
    def embeddings(self, x: Optional[torch.Tensor], adj: CSRGraph) -> torch.Tensor:
        key = (adj.uid, None if x is None else (x.data_ptr(), x._version),
               tuple((p.data_ptr(), p._version) for p in self.parameters()),
               tuple((b.data_ptr(), b._version) for b in self.buffers()))
        if key != self._h_key:
            xin = self._node_input(x)
            relabel = adj.n_rows >= REORDER_MIN_NODES and adj.n_rows == adj.n_cols
            if relabel:
                adj_run, perm, inv = adj.degree_ordered()
                xin = xin[perm].contiguous()
            else:
                adj_run = adj
            h = self._node_forward(xin, adj_run)
            self._h = h[inv].contiguous() if relabel else h
            self._h_key = key
        return self._h

    _hb_key = None
    _hb = None

    @torch.no_grad()
    def embeddings_bf16(self, x: Optional[torch.Tensor], adj: CSRGraph) -> torch.Tensor:
        """The bf16 bit patterns (int16 [N, H]) of ``embeddings(x, adj)``, under the same cache key: built on the first bf16
        decode after ``h`` changed, kept until it changes again."""
        h = self.embeddings(x, adj)
        if self._hb is None or self._hb_key != self._h_key:
            self._hb = ops.to_bf16(h.contiguous())
            self._hb_key = self._h_key
        return self._hb


class LinkGNN(_CachedEmbeddings, torch.nn.Module):
    """models.py:487-506.  ``fused_decode`` (off by default): the training branch decodes through
    ``LinkPredictor.decode_train`` (the fused HIP forward and backward) instead of the torch ops."""
    fused_decode = False

    def __init__(self, emb, gnn, linkpred):
        super().__init__()
        self.gnn = gnn
        self.linkpred = linkpred
        self.emb = emb
        self._h_key = None
        self._h = None

    def reset_parameters(self):
        self.gnn.reset_parameters()
        self.linkpred.reset_parameters()
        if self.emb is not None:
            self.emb.reset_parameters()
        self._h_key = None

    def _node_input(self, x):
        """[emb.weight || x], embedding FIRST (models.py:501-505)."""
        if x is None:
            return self.emb.weight.detach()
        if self.emb is not None:
            return torch.cat([self.emb.weight.detach(), x], dim=1)
        return x

    def _node_forward(self, xin, adj):
        from . import dist as epd
        rank, world = epd.world_info()
        if world > 1 and hasattr(self.gnn, "forward_sharded"):
            return self.gnn.forward_sharded(xin, adj, rank, world, epd.all_gather_rows)
        return self.gnn(xin, adj)

    def forward(self, x, edges, adj):
        if torch.is_grad_enabled() and self.training:   # models.py:500-506 on autograd (no caching while training)
            if x is None:
                x = self.emb.weight
            elif self.emb is not None:
                x = torch.cat([self.emb.weight, x], dim=1)
            h = self.gnn(x, adj)
            if self.fused_decode:
                return self.linkpred.decode_train(h, edges).unsqueeze(1)
            return self.linkpred(h[edges[0]], h[edges[1]])
        h = self.embeddings(x, adj)
        return self.linkpred.decode(h, edges).unsqueeze(1)


# ----------------------------------------------------------------------------------- Neural Common Neighbor
CN_LIST_BUDGET = 1 << 26         # common neighbours listed per launch (4 bytes each, twice in training: the list and its transpose)


class _CNEmbedSum(torch.autograd.Function):
    """Z = C H for one list of pairs, C the [pairs x nodes] common-neighbour incidence (ops.pair_cn_list), and dH = C^T dZ: both
    products are eps_spmm_csr without values, which adds sequentially in entry order -- Z[b] is the float32 sum of the rows h[w]
    in ascending w, dH[w] that of dZ[b] in ascending b, bit for bit (fmaf(1, x, acc) is an exact add).  The transpose is built
    in the backward, and only when h wants a gradient."""

    @staticmethod
    def forward(ctx, h, adj, u, v, count):
        ptr, w = ops.pair_cn_list(adj.rowptr, adj.col, adj.n_rows, u, v, check=False, count=count)
        ctx.lists, ctx.n = (ptr, w), h.shape[0]
        return ops.spmm_csr(ptr, w, None, _pad4(h))

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        ptr, w = ctx.lists
        tptr, tb = ops.cn_list_transpose(ptr, w, ctx.n, check=False)
        return ops.spmm_csr(tptr, tb, None, _pad4(grad_out)), None, None, None, None


def cn_embed_sum(h: torch.Tensor, adj: CSRGraph, edges: torch.Tensor) -> torch.Tensor:
    """-> float32 [B, H]: z_b = sum of h[w] over the common STORED neighbours w of the pair (edges[0, b], edges[1, b]) in ``adj``
    (the pattern: stored values are not read), added in ascending w; differentiable in ``h`` (any width).  At most
    CN_LIST_BUDGET common neighbours are listed at a time: a longer batch is cut on its cumulative counts, each piece with a
    list of its own (a pair's sum does not depend on where the cuts fall; a single pair beyond the budget is a piece)."""
    _check_rows(h, adj, "cn_embed_sum")
    if adj.n_rows != adj.n_cols:
        raise ValueError(f"cn_embed_sum: common neighbours need a square adjacency, got {adj.n_rows} x {adj.n_cols}")
    heuristics.check_node_ids(edges, adj.n_rows, "cn_embed_sum edges")
    e = edges.to(device=h.device, dtype=torch.int32)
    u, v = e[0].contiguous(), e[1].contiguous()
    b = u.numel()
    if b == 0:
        return h.new_zeros((0, h.shape[1]))
    count = ops.pair_cn_list_count(adj.rowptr, adj.col, adj.n_rows, u, v, check=False)
    cum = torch.cumsum(count, 0, dtype=torch.int64)
    budget = int(CN_LIST_BUDGET)
    if int(cum[-1].item()) <= budget:
        return _CNEmbedSum.apply(h, adj, u, v, count)
    cum, cuts, s, base = cum.cpu(), [0], 0, 0
    while s < b:
        # the longest run of pairs from s whose counts fit the budget -- at least one pair
        s = max(s + 1, int(torch.searchsorted(cum, base + budget, right=True)))
        cuts.append(s)
        base = int(cum[s - 1])
    return torch.cat([_CNEmbedSum.apply(h, adj, u[lo:hi], v[lo:hi], count[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])])


class NCNPredictor(torch.nn.Module):
    """The decoder of Neural Common Neighbor (Wang, Yang, Zhang): the pair's Hadamard product and the sum of its common
    neighbours' embeddings each get a first layer,
        t = relu(xij_lin(h_u * h_v)) + beta * relu(xcn_lin(z_cn)),
    then dropout, relu(lin(t)) + dropout for each of lins[:-1], and sigmoid(lins[-1](t)).  ``lins`` holds num_layers - 1 layers
    (num_layers >= 2); ``beta`` is a plain float.  The dense layers run on torch in training and in eval."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, beta=1.0):
        super().__init__()
        if num_layers < 2:
            raise ValueError(f"NCNPredictor: num_layers {num_layers}: the two first layers and an output layer make at least 2")
        self.xij_lin = torch.nn.Linear(in_channels, hidden_channels)
        self.xcn_lin = torch.nn.Linear(in_channels, hidden_channels)
        self.lins = torch.nn.ModuleList()
        for _ in range(num_layers - 2):
            self.lins.append(torch.nn.Linear(hidden_channels, hidden_channels))
        self.lins.append(torch.nn.Linear(hidden_channels, out_channels))
        self.dropout = dropout
        self.beta = float(beta)

    def reset_parameters(self):
        self.xij_lin.reset_parameters()
        self.xcn_lin.reset_parameters()
        for lin in self.lins:
            lin.reset_parameters()

    def forward(self, x_i: torch.Tensor, x_j: torch.Tensor, z_cn: torch.Tensor) -> torch.Tensor:
        drop = self.training and torch.is_grad_enabled()
        t = F.relu(self.xij_lin(x_i * x_j)) + self.beta * F.relu(self.xcn_lin(z_cn))
        t = F.dropout(t, p=self.dropout, training=drop)
        for lin in self.lins[:-1]:
            t = F.dropout(F.relu(lin(t)), p=self.dropout, training=drop)
        return torch.sigmoid(self.lins[-1](t))


NCN_EVAL_TILE = 1 << 15          # pairs per dense-layer call of NCNLinkGNN in eval: every call has this ONE shape
NCN_EVAL_TILES_PER_LIST = 32     # ... and tiles per cn_embed_sum call (its host reads are per call: 2^20 pairs, 1 GiB of sums at H = 256)


class NCNLinkGNN(LinkGNN):
    """LinkGNN whose decoder also sees the pair's common neighbours: scores = linkpred(h_u, h_v, sum_{w in N(u) & N(v)} h_w), the
    common neighbours being those of the ``adj`` passed in (no target-edge masking: v in N(u) puts neither u nor v into the
    intersection).  Same state-dict prefixes, embedding-first input and eval-mode embedding cache as LinkGNN.

    In eval the dense layers run on tiles of NCN_EVAL_TILE pairs, the last one padded: every GEMM then has one shape, so a
    pair's score does not depend on the batch it arrives in -- the filter stage may cut its candidate blocks anywhere.  The list
    of (u, v) equals that of (v, u) and h_u * h_v commutes, so score(u, v) == score(v, u) bit for bit."""

    def forward(self, x, edges, adj):
        if torch.is_grad_enabled() and self.training:
            if x is None:
                x = self.emb.weight
            elif self.emb is not None:
                x = torch.cat([self.emb.weight, x], dim=1)
            h = self.gnn(x, adj)
            return self.linkpred(h[edges[0]], h[edges[1]], cn_embed_sum(h, adj, edges))
        with torch.no_grad():
            h = self.embeddings(x, adj)
            e = edges.to(device=h.device, dtype=torch.int64)     # (cn_embed_sum checks the ids before anything gathers with them)
            n, tile = e.shape[1], int(NCN_EVAL_TILE)
            out = torch.empty((n, self.linkpred.lins[-1].out_features), dtype=torch.float32, device=h.device)
            for s0 in range(0, n, tile * NCN_EVAL_TILES_PER_LIST):
                z_all = cn_embed_sum(h, adj, e[:, s0:s0 + tile * NCN_EVAL_TILES_PER_LIST])
                for s in range(s0, s0 + z_all.shape[0], tile):
                    u, v, z = e[0, s:s + tile], e[1, s:s + tile], z_all[s - s0:s - s0 + tile]
                    xi, xj = h[u], h[v]
                    if u.numel() < tile:
                        pad = (0, 0, 0, tile - u.numel())
                        xi, xj, z = F.pad(xi, pad), F.pad(xj, pad), F.pad(z, pad)
                    out[s:s + tile] = self.linkpred(xi, xj, z)[:u.numel()]
            return out


# ----------------------------------------------------------------------------------- BUDDY (subgraph sketches)
SKETCH_FEATURES = {1: 2, 2: 5}   # hops -> structural features per pair (heuristics.sketch_feature_formulas)


class BuddyPredictor(torch.nn.Module):
    """The decoder of BUDDY (Chamberlain et al., ICLR 2023) in the mould of ``NCNPredictor``: the pair's Hadamard product and its
    structural features from the subgraph sketches each get a first layer,
        t = relu(xij_lin(h_u * h_v)) + relu(xs_lin(F(u, v))),
    then dropout, relu(lin(t)) + dropout for each of lins[:-1], and sigmoid(lins[-1](t)).  ``lins`` holds num_layers - 1 layers
    (num_layers >= 2).  The dense layers run on torch in training and in eval."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, num_features=5):
        super().__init__()
        if num_layers < 2:
            raise ValueError(f"BuddyPredictor: num_layers {num_layers}: the two first layers and an output layer make at least 2")
        self.xij_lin = torch.nn.Linear(in_channels, hidden_channels)
        self.xs_lin = torch.nn.Linear(num_features, hidden_channels)
        self.lins = torch.nn.ModuleList()
        for _ in range(num_layers - 2):
            self.lins.append(torch.nn.Linear(hidden_channels, hidden_channels))
        self.lins.append(torch.nn.Linear(hidden_channels, out_channels))
        self.dropout = dropout

    def reset_parameters(self):
        self.xij_lin.reset_parameters()
        self.xs_lin.reset_parameters()
        for lin in self.lins:
            lin.reset_parameters()

    def forward(self, x_i: torch.Tensor, x_j: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
        drop = self.training and torch.is_grad_enabled()
        t = F.relu(self.xij_lin(x_i * x_j)) + F.relu(self.xs_lin(f))
        t = F.dropout(t, p=self.dropout, training=drop)
        for lin in self.lins[:-1]:
            t = F.dropout(F.relu(lin(t)), p=self.dropout, training=drop)
        return torch.sigmoid(self.lins[-1](t))


class BuddyLinkModel(_CachedEmbeddings, torch.nn.Module):
    """BUDDY: node side h = feat_lin(dropout([xin || A^ xin || ... || A^hops xin])) with A^ = ``adj.gcn_normalized()`` and xin =
    [emb.weight || x] (embedding first, as in LinkGNN) -- fixed propagation, one Linear((hops + 1) in_dim, hidden); pair side
    the structural features of ``heuristics.sketch_features`` (estimated from the graph's HyperLogLog / MinHash sketches at a
    cost that depends on no degree; constants of the graph, no gradient); decoder ``BuddyPredictor``.  The sketches are those of
    the ``adj`` passed in (no target-edge masking).  NOT a LinkGNN: the filter scores it block by block through ``forward``.

    Eval: ``h`` is cached per (parameters, x, adjacency) like LinkGNN's, the sketches per adjacency on the graph; the dense
    layers run on tiles of NCN_EVAL_TILE pairs, the last one padded, so a pair's score does not depend on the batch it arrives
    in.  The features of (u, v) and (v, u) are the same bits and h_u * h_v commutes: score(u, v) == score(v, u) bit for bit."""

    def __init__(self, emb, in_dim, hidden, num_layers, dropout, hops=2):
        super().__init__()
        if hops not in SKETCH_FEATURES:
            raise ValueError(f"BuddyLinkModel: hops {hops}: 1 or 2")
        self.emb = emb
        self.hops = int(hops)
        self.dropout = dropout
        self.feat_lin = torch.nn.Linear((self.hops + 1) * in_dim, hidden)
        self.linkpred = BuddyPredictor(hidden, hidden, 1, num_layers, dropout, SKETCH_FEATURES[self.hops])
        self._h_key = None
        self._h = None

    def reset_parameters(self):
        self.feat_lin.reset_parameters()
        self.linkpred.reset_parameters()
        if self.emb is not None:
            self.emb.reset_parameters()
        self._h_key = None

    _node_input = LinkGNN._node_input

    def _node_forward(self, xin, adj):
        gn = adj.gcn_normalized()
        xs = [xin.contiguous()]
        for _ in range(self.hops):
            xs.append(ops.spmm_csr(gn.rowptr, gn.col, gn.val, xs[-1]))
        return ops.gemm(_pad4(torch.cat(xs, 1)), self.feat_lin.weight.detach().contiguous(), bias=self.feat_lin.bias.detach())

    def forward(self, x, edges, adj):
        if torch.is_grad_enabled() and self.training:
            if x is None:
                x = self.emb.weight
            elif self.emb is not None:
                x = torch.cat([self.emb.weight, x], dim=1)
            _check_rows(x, adj, "BuddyLinkModel")
            _check_trainable(adj, "BuddyLinkModel", values=True)
            gn = adj.gcn_normalized()
            xs = [x]
            for _ in range(self.hops):
                xs.append(_SpMM.apply(xs[-1], gn, False))
            h = self.feat_lin(F.dropout(torch.cat(xs, 1), p=self.dropout, training=True))
            f = heuristics.sketch_features(adj, edges, self.hops)
            return self.linkpred(h[edges[0]], h[edges[1]], f)
        with torch.no_grad():
            h = self.embeddings(x, adj)
            f_all = heuristics.sketch_features(adj, edges, self.hops)     # (once per call: it checks the ids before anything gathers with them)
            e = edges.to(device=h.device, dtype=torch.int64)
            n, tile = e.shape[1], int(NCN_EVAL_TILE)
            out = torch.empty((n, self.linkpred.lins[-1].out_features), dtype=torch.float32, device=h.device)
            for s in range(0, n, tile):
                u, v = e[0, s:s + tile], e[1, s:s + tile]
                xi, xj, f = h[u], h[v], f_all[s:s + tile]
                if u.numel() < tile:
                    pad = (0, 0, 0, tile - u.numel())
                    xi, xj, f = F.pad(xi, pad), F.pad(xj, pad), F.pad(f, pad)
                out[s:s + tile] = self.linkpred(xi, xj, f)[:u.numel()]
            return out


# ----------------------------------------------------------------------------------- DEA_GNN_JK
def fold_batchnorm(weight: torch.Tensor, bias: torch.Tensor, bn: torch.nn.BatchNorm1d):
    """(W', b') such that x W'^T + b' == bn(x W^T + b) with bn in eval mode (running statistics):
    s = gamma / sqrt(var + eps), W' = s W, b' = s b + beta - s mu.  Formed in float64, returned in W's dtype."""
    f = torch.float64
    s = bn.weight.detach().to(f) / torch.sqrt(bn.running_var.to(f) + bn.eps)
    w = s[:, None] * weight.detach().to(f)
    b = s * bias.detach().to(f) + bn.bias.detach().to(f) - s * bn.running_mean.to(f)
    return w.to(weight.dtype).contiguous(), b.to(weight.dtype).contiguous()


class TAGConv(torch.nn.Module):
    """torch_geometric 1.7.0 TAGConv(in, out, K) with normalize=True [third-party, restated]: with
    A^ = D^-1/2 A D^-1/2 (no self loops, inf -> 0; graph.tag_normalized), out = lin([x || A^ x || ... || A^K x]),
    ``lin`` = Linear(in * (K + 1), out) with bias.  Checkpoints in the PyG >= 2.0 layout (``lins.{k}.weight`` [out,in],
    optional ``lins.{k}.bias`` and ``bias``) load too: the weights are concatenated along ``in`` in k order and every
    bias is summed into ``lin.bias``."""

    def __init__(self, in_channels: int, out_channels: int, K: int = 3):
        super().__init__()
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.lin = torch.nn.Linear(in_channels * (K + 1), out_channels)

    def reset_parameters(self):
        self.lin.reset_parameters()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if prefix + "lin.weight" not in state_dict and prefix + "lins.0.weight" in state_dict:
            ws = [state_dict.pop(f"{prefix}lins.{k}.weight") for k in range(self.K + 1)]
            b = torch.zeros(ws[0].shape[0], dtype=ws[0].dtype, device=ws[0].device)
            for k in [f"{prefix}lins.{k}.bias" for k in range(self.K + 1)] + [prefix + "bias"]:
                if k in state_dict:
                    b = b + state_dict.pop(k)
            state_dict[prefix + "lin.weight"] = torch.cat(ws, 1)
            state_dict[prefix + "lin.bias"] = b
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x: torch.Tensor, adj_t: CSRGraph) -> torch.Tensor:
        """Training mode with grad enabled: the hops through the HIP SpMM Function (a symmetric adjacency is required: A^ is
        then symmetric, so its backward holds).  Otherwise the same hops without autograd."""
        _check_rows(x, adj_t, "TAGConv")
        training = torch.is_grad_enabled() and self.training
        if training:
            _check_trainable(adj_t, "TAGConv", values=True)
        an = adj_t.tag_normalized()
        xs = [x]
        for _ in range(self.K):
            if training:
                xs.append(_SpMM.apply(xs[-1], an, False))
            else:       # eval() / no_grad(): any graph; no gradient reaches x through the hops (like GCNConv / SAGEConv)
                xs.append(ops.spmm_csr(an.rowptr, an.col, an.val, xs[-1].detach().contiguous()))
        return self.lin(torch.cat(xs, 1))

    @torch.no_grad()
    def hops(self, x: torch.Tensor, an: CSRGraph) -> torch.Tensor:
        """[x || A^ x || ... || A^K x] in ONE [N, (K + 1) * k4] buffer (k4 = in rounded up to 4 floats, zero pad columns:
        every block starts 16-byte aligned); each hop is an SpMM from the previous block into the next."""
        _check_rows(x, an, "TAGConv")
        n, k = x.shape
        k4 = (k + 3) // 4 * 4
        buf = (torch.empty if k4 == k else torch.zeros)((n, (self.K + 1) * k4), dtype=torch.float32, device=x.device)
        buf[:, :k] = x
        for j in range(1, self.K + 1):
            ops.spmm_csr(an.rowptr, an.col, an.val, buf[:, (j - 1) * k4:(j - 1) * k4 + k], out=buf[:, j * k4:j * k4 + k])
        return buf

    def hop_weight(self, w: torch.Tensor) -> torch.Tensor:
        """``w`` [out, (K + 1) * in] laid out for ``hops``' buffer (zero columns at the pad of each block)."""
        k, k4 = self.in_channels, (self.in_channels + 3) // 4 * 4
        if k4 == k:
            return w
        wp = torch.zeros((w.shape[0], self.K + 1, k4), dtype=w.dtype, device=w.device)
        wp[:, :, :k] = w.view(w.shape[0], self.K + 1, k)
        return wp.view(w.shape[0], -1)

    def __repr__(self):
        return f"TAGConv({self.in_channels}, {self.out_channels}, K={self.K})"


_JK_MODES = ('max', 'sum', 'mean')


class DEA_GNN_JK(_CachedEmbeddings, torch.nn.Module):
    """models.py:36-133: a learnable embedding (FIRST in the input, [emb.weight || x]), ``gnn_num_layers`` x [TAGConv(K),
    BatchNorm, ReLU, dropout], jumping knowledge over the layer outputs, then the decoder h[u] * h[v] -> (mlp_num_layers - 1)
    x [Linear, BatchNorm, ReLU, dropout] -> Linear(hidden, out).squeeze(1).  The output is a LOGIT; ``loss`` is
    BCEWithLogitsLoss.

    Training mode runs on torch autograd with the hops through the HIP SpMM.  Eval mode runs on the HIP kernels: per layer
    the hop buffer (TAGConv.hops) and one GEMM with the BatchNorm folded into its weights and ReLU in its epilogue; the
    embeddings are cached like LinkGNN's; the decode is eps_mlp_decode (logits) with the decoder's BatchNorms folded in.

    ``fused_decode`` (off by default): the training branch decodes through ``decode_train`` (the fused HIP statistics pass,
    forward and backward, BatchNorm on batch statistics included) instead of the torch ops; the GNN half stays on autograd."""
    fused_decode = False

    def __init__(self, num_nodes, embed_dim, gnn_in_dim, gnn_hidden_dim, gnn_out_dim, gnn_num_layers, mlp_in_dim,
                 mlp_hidden_dim, mlp_out_dim=1, mlp_num_layers=2, dropout=0.5, gnn_batchnorm=False, mlp_batchnorm=False, K=2,
                 jk_mode='max'):
        super().__init__()
        if jk_mode not in _JK_MODES:
            # the reference accepts 'lstm' / 'cat' too and then fails in its decoder or in JumpingKnowledge: say so here
            raise ValueError(f"DEA_GNN_JK: jk_mode '{jk_mode}' is not supported (one of {', '.join(_JK_MODES)})")
        self.emb = torch.nn.Embedding(num_nodes, embedding_dim=embed_dim)
        self.convs = torch.nn.ModuleList([TAGConv(gnn_in_dim, gnn_hidden_dim, K)] +
                                         [TAGConv(gnn_hidden_dim, gnn_hidden_dim, K) for _ in range(gnn_num_layers - 2)] +
                                         [TAGConv(gnn_hidden_dim, gnn_out_dim, K)])
        self.lins = torch.nn.ModuleList([torch.nn.Linear(mlp_in_dim, mlp_hidden_dim)] +
                                        [torch.nn.Linear(mlp_hidden_dim, mlp_hidden_dim) for _ in range(mlp_num_layers - 2)] +
                                        [torch.nn.Linear(mlp_hidden_dim, mlp_out_dim)])
        self.gnn_batchnorm, self.mlp_batchnorm = gnn_batchnorm, mlp_batchnorm
        if gnn_batchnorm:
            self.gnn_bns = torch.nn.ModuleList([torch.nn.BatchNorm1d(gnn_hidden_dim) for _ in range(gnn_num_layers)])
        if mlp_batchnorm:
            self.mlp_bns = torch.nn.ModuleList([torch.nn.BatchNorm1d(mlp_hidden_dim) for _ in range(mlp_num_layers - 1)])
        self.jk_mode = jk_mode
        self.dropout = dropout
        self.loss_fn = torch.nn.BCEWithLogitsLoss()
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.emb.weight)
        for conv in self.convs:
            conv.reset_parameters()
        for lin in self.lins:
            lin.reset_parameters()
        for bn in (list(self.gnn_bns) if self.gnn_batchnorm else []) + (list(self.mlp_bns) if self.mlp_batchnorm else []):
            bn.reset_parameters()
        self._h_key = None

    def _jk(self, outs):
        if self.jk_mode == 'max':
            return torch.stack(outs).max(0).values
        s = torch.stack(outs).sum(0)
        return s / len(outs) if self.jk_mode == 'mean' else s

    def _node_input(self, x):
        w = self.emb.weight.detach()
        return w if x is None else torch.cat([w, x], 1)

    def _node_forward(self, xin, adj):
        """Eval: per layer the hop buffer, then ONE GEMM with the BatchNorm folded in and ReLU in the epilogue."""
        an = adj.tag_normalized()
        x, h, n_out = xin, None, len(self.convs)
        for i, conv in enumerate(self.convs):
            w, b = conv.lin.weight.detach(), conv.lin.bias.detach()
            if self.gnn_batchnorm:
                w, b = fold_batchnorm(w, b, self.gnn_bns[i])
            x = ops.gemm(conv.hops(x, an), conv.hop_weight(w), bias=b.contiguous(), relu=True)
            if h is None:
                h = x
            elif self.jk_mode == 'max':
                h = torch.maximum(h, x, out=h)        # (x of the layer before is in this layer's hop buffer already)
            else:
                h = h + x
        return h / n_out if self.jk_mode == 'mean' else h

    @torch.no_grad()
    def decode(self, h: torch.Tensor, edges: torch.Tensor, precision: str = "fp32") -> torch.Tensor:
        """Logits of the decoder over edges [2,B] (eps_mlp_decode with the BatchNorms folded in) -> float32 [B].
        ``precision="bf16"``: eps_mlp_decode_bf16 on ``h`` (float32, or its bf16 bit patterns from ``embeddings_bf16``); the
        BatchNorm is folded into ``lins.0`` in float32 first, the hidden weights are rounded to bf16 after."""
        heuristics.check_node_ids(edges, h.shape[0], "decode edges")   # the kernel gathers h[u], h[v] unchecked
        e = edges.to(device=h.device, dtype=torch.int32)
        if precision == "bf16":
            ws, bs = _bf16_decoder(self, self._decoder_layers)
            hb = h.contiguous() if h.dtype == torch.int16 else ops.to_bf16(h.contiguous())
            return ops.mlp_decode_bf16(hb, e[0].contiguous(), e[1].contiguous(), ws, bs, apply_sigmoid=False)
        _check_precision(precision)
        ws, bs = self._decoder_layers()
        return ops.mlp_decode(h.contiguous(), e[0].contiguous(), e[1].contiguous(), ws, bs, apply_sigmoid=False)

    def _decoder_layers(self):
        ws, bs = [], []
        for i, lin in enumerate(self.lins):
            w, b = lin.weight.detach(), lin.bias.detach()
            if self.mlp_batchnorm and i < len(self.lins) - 1:
                w, b = fold_batchnorm(w, b, self.mlp_bns[i])
            ws.append(w.contiguous())
            bs.append(b.contiguous())
        return ws, bs

    def decode_train(self, h: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
        """The training decode over edges [2,B] on the fused kernels (eps_mlp_decode_bn_stats, eps_mlp_decode_train on the
        folded layer, eps_mlp_decode_bn_backward) -> logits float32 [B], differentiable in ``h``, the two Linear layers and the
        BatchNorm's weight and bias.  The BatchNorm's running statistics and ``num_batches_tracked`` are updated in place as
        torch.nn.BatchNorm1d updates them.  Dropout masks: as ``LinkPredictor.decode_train`` draws them."""
        hd, L, B = h.shape[1], len(self.lins), edges.shape[1]
        if (h.dim() != 2 or L != 2 or not self.mlp_batchnorm or hd % 4 != 0 or not ops.TRAIN_MIN_HIDDEN <= hd <= ops.TRAIN_MAX_HIDDEN
                or tuple(self.lins[0].weight.shape) != (hd, hd) or tuple(self.lins[1].weight.shape) != (1, hd)):
            raise ValueError(f"fused BatchNorm training decode: width {hd} with layers {[tuple(lin.weight.shape) for lin in self.lins]}"
                             f"{'' if self.mlp_batchnorm else ' without mlp_batchnorm'} is outside the kernel's domain (Linear(H, H), "
                             f"BatchNorm, ReLU, Linear(H, 1): exactly two layers, H % 4 == 0, {ops.TRAIN_MIN_HIDDEN} <= H <= "
                             f"{ops.TRAIN_MAX_HIDDEN}); leave fused_decode off for this model")
        if B < 2:
            raise ValueError(f"fused BatchNorm training decode: B={B} edges; batch statistics need at least 2")
        heuristics.check_node_ids(edges, h.shape[0], "decode edges")   # the kernels gather h[u], h[v] unchecked
        e = edges.to(device=h.device, dtype=torch.int32).contiguous()
        bn, (lin0, lin1) = self.mlp_bns[0], self.lins
        with torch.no_grad():
            mean, var = ops.mlp_decode_bn_stats(h.detach().contiguous(), e[0], e[1], [lin0.weight.contiguous(), lin1.weight.contiguous()],
                                                [lin0.bias.contiguous(), lin1.bias.contiguous()])
            if bn.track_running_stats and bn.running_mean is not None:
                bn.num_batches_tracked.add_(1)
                m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                bn.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
                bn.running_var.mul_(1.0 - m).add_(var, alpha=m * B / (B - 1))
        keep, scale, p = None, 1.0, float(self.dropout)
        if p > 0:
            keep = ops.pack_mask(torch.rand(B, hd, device=h.device) >= p).unsqueeze(0)
            scale = 1.0 / (1.0 - p) if p < 1 else 0.0
        return _FusedDecodeBN.apply(h, e, keep, scale, mean, var, float(bn.eps), lin0.weight, lin0.bias, bn.weight, bn.bias,
                                    lin1.weight, lin1.bias)

    def forward(self, x_feature, edge_label_index, adj_t):
        if not self.training:
            return self.decode(self.embeddings(x_feature, adj_t), edge_label_index)
        out = self.emb.weight if x_feature is None else torch.cat([self.emb.weight, x_feature], dim=1)
        outs = []
        for i, conv in enumerate(self.convs):
            out = conv(out, adj_t)
            if self.gnn_batchnorm:
                out = self.gnn_bns[i](out)
            out = F.dropout(F.relu(out), p=self.dropout, training=True)
            outs.append(out)
        out = self._jk(outs)
        if self.fused_decode:
            return self.decode_train(out, edge_label_index)
        out = out[edge_label_index[0]] * out[edge_label_index[1]]
        for i, lin in enumerate(self.lins[:-1]):
            out = lin(out)
            if self.mlp_batchnorm:
                out = self.mlp_bns[i](out)
            out = F.dropout(F.relu(out), p=self.dropout, training=True)
        return self.lins[-1](out).squeeze(1)

    def loss(self, y_pred, y_true):
        return self.loss_fn(y_pred, y_true)


class MLP(torch.nn.Module):
    """models.py:136-163 (the layers and state-dict keys ``lins.*``).  Only 'mlpcos' constructs it, and -- like the
    reference, whose call is commented out (models.py:564) -- never applies it: it exists so that a reference checkpoint
    (``mlp.lins.*``, ``emb.weight``) loads."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__()
        self.lins = torch.nn.ModuleList()
        self.lins.append(torch.nn.Linear(in_channels, hidden_channels))
        for _ in range(num_layers - 2):
            self.lins.append(torch.nn.Linear(hidden_channels, hidden_channels))
        self.lins.append(torch.nn.Linear(hidden_channels, out_channels))
        self.dropout = dropout

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()


_COSINE = ('mlpcos', 'simplecos')


class CommonNeighborsPredictor(torch.nn.Module):
    """models.py:508-575.  'simple' (CN) and 'adamic' run on eps_pair_scores; 'adamic_ogb',
    'resource_allocation', 'katz' return None exactly like the reference (those heuristics are evaluated by
    AA()/resource_allocation(), not by the module).  The cosine variants ('mlpcos', 'simplecos') score the edge-valued
    common-neighbour sum of the cosine graph (heuristics.cosine_common_neighbors: csrc/cosine_cn.hip + eps_pair_scores).
    The local indices, the local-community indices and 'ppr' (heuristics.ppr with ``ppr_alpha`` / ``ppr_eps``) return the index
    itself: no parameters, no sigmoid.
    Scoring (``model.eval()`` or ``torch.no_grad()``) builds no autograd graph.  In ``model.train()`` with grad enabled and a
    learnable embedding the cosine variants are differentiable in emb.weight (heuristics.cosine_common_neighbors_raw:
    csrc/cosine_cn_bwd.hip), which is how the reference trains mlpcos (train_and_eval.py:31-96)."""

    def __init__(self, emb, in_channels, hidden_channels, out_channels, num_layers, dropout, model_type='weighted',
                 ppr_alpha=heuristics.PPR_ALPHA, ppr_eps=heuristics.PPR_EPS):
        super().__init__()
        assert model_type in ['mlpcos', 'simplecos', 'adamic', 'simple', 'adamic_ogb', "resource_allocation", 'katz', 'ppr',
                              *heuristics.LOCAL_INDICES, *heuristics.LOCAL_COMMUNITY_INDICES]
        self.type = model_type
        self.ppr_alpha, self.ppr_eps = float(ppr_alpha), float(ppr_eps)
        if self.type == 'ppr':
            heuristics.ppr_parameters(self.ppr_alpha, self.ppr_eps)       # (a refused pair stops here, before any data is scored)
        if self.type == 'mlpcos':
            self.mlp = MLP(in_channels, hidden_channels, out_channels, num_layers, dropout)
        else:
            self.mlp = torch.nn.Identity()
        self.emb = emb
        self._x_key = self._x_src = self._x = None

    def reset_parameters(self):
        if self.type == 'mlpcos':
            self.mlp.reset_parameters()
        if self.emb is not None:
            self.emb.reset_parameters()

    @torch.no_grad()
    def cosine_input(self, x: Optional[torch.Tensor]) -> torch.Tensor:
        """The node features the cosine variants smooth (models.py:529-532): emb.weight when x is None, else
        [emb.weight || x] with an embedding, else x.  The concatenation is kept per (embedding version, x), so the cosine
        graph cached on the adjacency (keyed on this tensor) serves every scoring batch."""
        if x is None and self.emb is None:
            raise ValueError(f"CommonNeighborsPredictor('{self.type}') needs node features or a learnable embedding")
        if self.emb is None:
            return x
        w = self.emb.weight
        key = (w.data_ptr(), w._version, None if x is None else x._version)
        if key != self._x_key or self._x_src is not x:     # (x itself is held: an address can be recycled)
            self._x = w.detach() if x is None else torch.cat([w.detach(), x], dim=1)
            self._x_key, self._x_src = key, x
        return self._x

    def forward(self, x, edges, adj):
        if (self.type in _COSINE and self.training and torch.is_grad_enabled() and self.emb is not None
                and self.emb.weight.requires_grad):
            # training (train_and_eval.py:31-96): the gradient reaches emb.weight through the cosines (csrc/cosine_cn_bwd.hip);
            # the feature columns take none, and self.mlp is never applied (models.py:564): its parameters keep grad None
            return torch.sigmoid(heuristics.cosine_common_neighbors_raw(adj, self.emb.weight, edges, feat=x))
        with torch.no_grad():
            return self._score(x, edges, adj)

    def _score(self, x, edges, adj):
        if self.type in ['adamic_ogb', "resource_allocation", 'katz']:
            return None                                                      # models.py:534-535
        if self.type == 'simple':
            return heuristics.common_neighbors(adj, edges)                   # models.py:536-542
        if self.type in heuristics.LOCAL_INDICES:                            # (no parameters, no sigmoid: the index itself)
            return heuristics.local_index(adj, edges, self.type)
        if self.type in heuristics.LOCAL_COMMUNITY_INDICES:                  # (likewise: car, cpa, caa, cra, cjc)
            return heuristics.local_community(adj, edges, self.type)
        if self.type == 'ppr':                                               # (likewise: pi_u(v) + pi_v(u), the pair entry)
            return heuristics.ppr(adj, edges, alpha=self.ppr_alpha, eps=self.ppr_eps, device_out=True)
        if self.type == 'adamic':
            # models.py:547-554: weight 1/log(rowsum(adj) + 1e-6) per common neighbour (edge values of the two
            # rows are NOT used: only the indices of the product), no inf guard, then sigmoid
            key = ("adamic_model_w",)
            if key not in adj._cache:
                adj._cache[key] = (1.0 / torch.log(adj.sum(-1) + 1e-6)).contiguous()
            g = adj if adj.val is None else adj.fill_value(1.0)
            heuristics.check_node_ids(edges, g.n_rows)
            e = edges.to(device=adj.device, dtype=torch.int32)
            _, _, ws = ops.pair_scores(g.rowptr, g.col, None, adj._cache[key], g.n_rows, e[0].contiguous(),
                                       e[1].contiguous(), want_count=False, want_cn=False)
            return torch.sigmoid(ws)
        # 'simplecos' / 'mlpcos' (models.py:556-575; self.mlp stays unused, :564)
        return heuristics.cosine_common_neighbors(adj, self.cosine_input(x), edges)


# ----------------------------------------------------------------------------------- factory
DECODE_MAX_HIDDEN = 256          # csrc/mlp_decode.hip: hdim % 4 == 0 && hdim <= 256
_MODELS = ['sage', 'sage2', 'gcn', 'dea', 'dea_512', 'mlpcos', 'simplecos', 'adamic', 'simple', 'adamic_ogb',
           "resource_allocation", 'katz', 'ensemble_gcn_sage', *heuristics.LOCAL_INDICES, *heuristics.LOCAL_COMMUNITY_INDICES, 'ncn', 'ncn_sage', 'buddy',
           'ppr', 'gat']
_NCN = {'ncn': 'gcn', 'ncn_sage': 'sage'}       # Neural Common Neighbor: name -> the encoder whose arguments and defaults it takes
_ENCODER_ROW = {**_NCN, 'buddy': 'gcn', 'gat': 'gcn'}         # models beyond the reference: name -> the row of the defaults table they take
_HEURISTICS = ['mlpcos', 'simplecos', 'adamic', 'simple', 'adamic_ogb', 'katz', "resource_allocation", *heuristics.LOCAL_INDICES, *heuristics.LOCAL_COMMUNITY_INDICES,
               'ppr']


def _flag(args, name: str, default):
    """An optional command-line value: the default when the namespace does not carry it (or carries None)."""
    x = getattr(args, name, None)
    return default if x is None else x


def build_model(args, data, device):
    """models.py:578-670 for the models on the accelerated path (gcn, sage, dea, dea_512, heuristics)."""
    assert args.model in _MODELS
    if args.model in _COSINE:
        # the reference would fail inside its forward (emb.weight of None, models.py:529-532): say why here
        if args.use_feature and data.x is None:
            raise ValueError(f"--model {args.model} --use_feature: the dataset carries no node features "
                             "(ddi has none; collab and ppa do)")
        if not args.use_feature and not args.use_learnable_embedding:
            raise ValueError(f"--model {args.model} needs node features: pass --use_feature True (on a dataset that has "
                             "them) or --use_learnable_embedding True")
    if args.model in ('dea', 'dea_512'):
        return _build_dea(args, data, device)
    if args.model == 'gat':
        _check_gat_args(args)
    if args.model in _ENCODER_ROW:
        # (before anything is allocated: ppa has no defaults, and the decoder's two first layers and its output layer make 2)
        if args.hidden_channels is None:
            raise UnsupportedModelConfig(f"--model {args.model} needs --hidden_channels (there is no "
                                         f"{getattr(args, 'dataset', '')} default for it)")
        if args.num_layers is None or args.num_layers < 2:
            raise UnsupportedModelConfig(f"--model {args.model}: --num_layers {args.num_layers}: the decoder has at least 2 layers")
    emb = None
    if args.use_learnable_embedding:
        emb = torch.nn.Embedding(data.num_nodes, args.hidden_channels).to(device)
    input_dim = 0
    if args.use_learnable_embedding:
        input_dim += args.hidden_channels
    if args.use_feature:
        input_dim += data.x.shape[1]
    if args.model in ('sage', 'gcn'):
        hc = args.hidden_channels
        if hc is None or hc % 4 != 0 or hc > DECODE_MAX_HIDDEN:
            # eps_mlp_decode keeps a 64-edge tile of width H in LDS: fail here, before any training time is spent
            raise ValueError(f"--hidden_channels {hc}: the fused decode kernel takes a multiple of 4 up to "
                             f"{DECODE_MAX_HIDDEN} (the reference's ogbl defaults are 256)")
        gnn_cls = SAGE if args.model == 'sage' else GCN
        gnn = gnn_cls(input_dim, args.hidden_channels, args.hidden_channels, args.num_layers, args.dropout).to(device)
        linkpred = LinkPredictor(args.hidden_channels, args.hidden_channels, 1, args.num_layers,
                                 args.dropout).to(device)
        return LinkGNN(emb, gnn, linkpred)
    if args.model == 'gat':
        gnn = GAT(input_dim, args.hidden_channels, args.hidden_channels, args.num_layers, args.dropout,
                  heads=int(_flag(args, "gat_heads", GAT_HEADS))).to(device)
        linkpred = LinkPredictor(args.hidden_channels, args.hidden_channels, 1, args.num_layers, args.dropout).to(device)
        return LinkGNN(emb, gnn, linkpred)
    if args.model in _NCN:
        gnn_cls = SAGE if args.model == 'ncn_sage' else GCN
        gnn = gnn_cls(input_dim, args.hidden_channels, args.hidden_channels, args.num_layers, args.dropout).to(device)
        linkpred = NCNPredictor(args.hidden_channels, args.hidden_channels, 1, args.num_layers, args.dropout).to(device)
        return NCNLinkGNN(emb, gnn, linkpred)
    if args.model == 'buddy':
        if input_dim == 0:
            raise UnsupportedModelConfig("--model buddy needs node features: pass --use_feature True (on a dataset that has them) or "
                                         "--use_learnable_embedding True")
        return BuddyLinkModel(emb, input_dim, args.hidden_channels, args.num_layers, args.dropout,
                              hops=int(getattr(args, "sketch_hops", 2) or 2)).to(device)
    if args.model in _HEURISTICS:
        ppr_kw = {}
        if args.model == 'ppr':
            ppr_kw = dict(ppr_alpha=_flag(args, "ppr_alpha", heuristics.PPR_ALPHA), ppr_eps=_flag(args, "ppr_eps", heuristics.PPR_EPS))
        return CommonNeighborsPredictor(emb, input_dim, args.hidden_channels, args.hidden_channels, args.num_layers,
                                        args.dropout, model_type=args.model, **ppr_kw).to(device)
    raise NotImplementedError(f"model '{args.model}' (sage2 / ensemble_gcn_sage) is outside the accelerated path "
                              "(SURVEY 2.1: alternative / experimental models, not in the north star)")


def _check_gat_args(args) -> None:
    """The rules of --model gat, each refused by name before anything is allocated."""
    heads = int(_flag(args, "gat_heads", GAT_HEADS))
    hc, nl = args.hidden_channels, args.num_layers
    if not 1 <= heads <= ops.GAT_MAX_HEADS:
        raise UnsupportedModelConfig(f"--model gat: --gat_heads {heads}: the attention kernel takes 1 to {ops.GAT_MAX_HEADS} heads")
    if hc is None:
        raise UnsupportedModelConfig(f"--model gat needs --hidden_channels (there is no {getattr(args, 'dataset', '')} default for it)")
    if hc % (4 * heads) != 0:
        fit = [h for h in range(1, ops.GAT_MAX_HEADS + 1) if hc % (4 * h) == 0]
        raise UnsupportedModelConfig(f"--model gat: --hidden_channels {hc} is not a multiple of 4 * heads = {4 * heads} (every head is a "
                                     f"whole number of float4 columns); with this width pass --gat_heads {' or '.join(map(str, fit)) or '(none fits)'}")
    if hc > DECODE_MAX_HIDDEN:
        raise UnsupportedModelConfig(f"--model gat: --hidden_channels {hc}: the fused decode kernel takes a width up to {DECODE_MAX_HIDDEN}")
    if nl is None or nl < 2:
        raise UnsupportedModelConfig(f"--model gat: --num_layers {nl}: the encoder stack and the decoder have at least 2 layers")


DEA_MAX_HIDDEN = 512             # csrc/mlp_decode.hip: hdim % 4 == 0 && hdim <= 512


class UnsupportedModelConfig(ValueError, NotImplementedError):
    """A model configuration refused at build time (the reference would fail later, or the kernels do not take it).  A
    ValueError; also a NotImplementedError, which is what build_model raised for every 'dea' configuration before the
    model was supported."""


def _build_dea(args, data, device):
    """models.py:629-636: 3 TAGConv(K=2) layers and a 2-layer decoder of width --hidden_channels, BatchNorm in both, JK max
    (--num_layers does not change the depth).  The reference fails later on the combinations refused here."""
    hc = args.hidden_channels
    if hc is None:
        raise UnsupportedModelConfig(f"--model {args.model} needs --hidden_channels (the reference has no {getattr(args, 'dataset', '')} default for it)")
    if hc % 4 != 0 or hc > DEA_MAX_HIDDEN:
        raise UnsupportedModelConfig(f"--hidden_channels {hc}: the fused decode kernel takes a multiple of 4 up to {DEA_MAX_HIDDEN}")
    if not args.use_learnable_embedding:
        # its forward always puts emb.weight first; without the flag the first layer's input width would not count it
        raise UnsupportedModelConfig(f"--model {args.model} needs --use_learnable_embedding True (its input is [embedding || x])")
    input_dim = hc + (data.x.shape[1] if args.use_feature else 0)
    return DEA_GNN_JK(num_nodes=data.num_nodes, embed_dim=hc, gnn_in_dim=input_dim, gnn_hidden_dim=hc, gnn_out_dim=hc,
                      gnn_num_layers=3, mlp_in_dim=hc, mlp_hidden_dim=hc, mlp_out_dim=1, mlp_num_layers=2,
                      dropout=args.dropout, gnn_batchnorm=True, mlp_batchnorm=True, K=2, jk_mode='max').to(device)


# per-dataset defaults, one row per (dataset group, model group): restates the table of models.py:673-790
_GNNS = ('sage', 'sage2', 'gcn', 'dea', 'dea_512', 'ensemble_gcn_sage', 'ncn', 'ncn_sage', 'buddy', 'gat')
_KEYS = ["num_layers", "hidden_channels", "dropout", "batch_size", "lr", "epochs", "use_feature",
         "use_learnable_embedding"]


def _defaults_for(dataset: str, model: str) -> dict:
    model = _ENCODER_ROW.get(model, model)       # (ncn / ncn_sage / buddy: the row of their encoder)
    d = dict.fromkeys(_KEYS)

    def put(**kw):
        d.update(kw)

    if dataset == 'ddi':
        put(use_feature=False, use_learnable_embedding=True, batch_size=64 * 1024)
        if model in _GNNS:
            put(num_layers=2, hidden_channels=256, dropout=0.5, lr=0.005, epochs=200)
            if model in ('dea', 'dea_512'):
                put(num_layers=3, epochs=400)
                if model == 'dea_512':
                    put(hidden_channels=512)
        if model in ('mlpcos', 'simplecos'):
            put(num_layers=2, hidden_channels=256, dropout=0.5, lr=0.005, epochs=200)
        if model in ('simple', 'simplecos') + heuristics.LOCAL_INDICES + heuristics.LOCAL_COMMUNITY_INDICES:
            put(batch_size=1024)
            if model == 'simplecos':
                put(use_feature=True)
    if dataset == 'collab':
        put(use_feature=True, use_learnable_embedding=True, batch_size=16 * 1024)
        if model in ('sage', 'sage2', 'gcn', 'dea', 'dea_512'):
            put(num_layers=3, hidden_channels=256, dropout=0.0, lr=0.001, epochs=200)
            if model in ('dea', 'dea_512'):
                put(num_layers=4, epochs=400)
                if model == 'dea_512':
                    put(hidden_channels=512)
        if model in ('mlpcos', 'simplecos'):
            put(num_layers=3, hidden_channels=256, dropout=0.0, lr=0.00001, epochs=400)
    if dataset in ('reddit', 'twitch', 'fb'):
        put(use_feature=True, use_learnable_embedding=True, batch_size=64 * 1024)
        if model in ('sage', 'sage2', 'gcn'):
            put(num_layers=3, hidden_channels=256, dropout=0.0, lr=0.005, epochs=200)
        if model in ('mlpcos', 'simplecos'):
            put(batch_size=1024, num_layers=3, hidden_channels=256, dropout=0.0, lr=0.001, epochs=10)
    if dataset == 'email':
        put(use_feature=False, use_learnable_embedding=True, batch_size=16 * 1024)
        if model in ('sage', 'sage2', 'gcn'):
            put(num_layers=3, hidden_channels=300, dropout=0.0, lr=0.001, epochs=200)
        if model in ('mlpcos', 'simplecos'):
            put(num_layers=3, hidden_channels=256, dropout=0.0, batch_size=1024, lr=0.00004, epochs=30)
    return d


def default_model_configs(args):
    """models.py:673-790: fill every model flag the command line left at None from the per-(dataset, model)
    table; a CLI value wins (:774-778); heuristic models force use_feature / use_learnable_embedding off
    (:783-785).  ppa has no block in the reference: its flags stay None unless given on the CLI."""
    defaults = _defaults_for(args.dataset, args.model)
    for attr in _KEYS:
        if getattr(args, attr) is None:
            setattr(args, attr, defaults[attr])
    if args.model in ['adamic', 'simple', 'adamic_ogb', "resource_allocation", 'katz', "ensemble_gcn_sage", *heuristics.LOCAL_INDICES, *heuristics.LOCAL_COMMUNITY_INDICES,
                      'ppr']:
        args.use_feature = False
        args.use_learnable_embedding = False
    if args.model == 'simplecos' and args.dataset != "email":
        args.use_learnable_embedding = False
    return args
