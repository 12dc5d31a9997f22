"""Common-Neighbours / Adamic-Adar / Resource-Allocation pair scoring on the MI355X.

Drop-ins for the reference's heuristic entry points, same names, argument meaning and return
types:

* ``get_A(adj, num_nodes)``                          <- adamic_utils.py:8-11
* ``AA(A, edge_index, batch_size=2000)``             <- adamic_utils.py:13-25
* ``resource_allocation(adj_matrix, link_list, batch_size=32768)``  <- train_and_eval.py:195-216
* ``common_neighbors(adj, edges)``                   <- models.py:536-542 ('simple')
* ``local_index(adj, edges, index)``                 <- the degree-normalised local indices of Zhou, Lu, Zhang (``LOCAL_INDICES``)
* ``local_index_columns``                            <- the same for a filter's column-major candidate blocks
* ``local_community(adj, edges, index)``             <- the local-community indices of Cannistraci, Alanis-Lobato, Ravasi
                                                        (``LOCAL_COMMUNITY_INDICES``: car, cpa, caa, cra, cjc)
* ``local_community_columns``                        <- the same for a filter's column-major candidate blocks
* ``truncated_katz`` / ``exact_katz``                <- the two branches of test_katz, train_and_eval.py:272-343
* ``truncated_katz_columns``                        <- the truncated series for a filter's column-major candidate blocks
* ``ppr`` / ``ppr_columns`` / ``ppr_mass``           <- personalized PageRank by a fixed-point forward push (pair entry, a filter's
                                                        column entry, the integer mass per directed request)
* ``cosine_common_neighbors(adj, x, edges)``         <- models.py:556-575 ('simplecos' / 'mlpcos')
* ``cosine_common_neighbors_raw(adj, x, edges)``     <- the same before the sigmoid, differentiable in x (training)

Where the reference loops over 2000-pair batches on one CPU thread through SciPy, these upload
the pair list once, run ``eps_pair_scores`` (csrc/pair_intersect.hip) over all of it and hand
back the same ``torch.FloatTensor``.  ``batch_size`` is accepted for signature compatibility;
it does not change results (the reference's batching does not either).  There is no CPU path.
"""
from __future__ import annotations

from fractions import Fraction
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops
from ._lib import EpsError
from .graph import CSRGraph

# pairs scored per launch when streaming a very large candidate list through HBM
_STREAM_CHUNK = 1 << 26


def _default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise EpsError("no HIP device visible: the edge-proposal-sets_amd scoring path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _as_graph(A, device: Optional[torch.device] = None) -> CSRGraph:
    """Accept what the reference passes as ``A``: the object returned by get_A, or a SciPy matrix
    (filter.py:136-139 builds one by hand, possibly int64)."""
    if isinstance(A, CSRGraph):
        g = A
    elif hasattr(A, "tocsr"):
        g = CSRGraph.from_scipy(A)
    else:
        raise TypeError(f"unsupported adjacency type {type(A)}")
    if not g.device.type == "cuda":
        g = g.to(device or _default_device())
    return g


def check_node_ids(edge_index: torch.Tensor, n_nodes: int, what: str = "edge list") -> None:
    """The kernels index rowptr / the embedding table with the ids they are given: an id outside [0, n_nodes) must stop
    here (the reference raises IndexError in the same case), before it is narrowed to int32 or reaches the device."""
    if edge_index.numel() == 0:
        return
    lo, hi = torch.aminmax(edge_index)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi >= n_nodes:
        raise EpsError(f"{what}: node ids must lie in [0, {n_nodes}), got [{lo}, {hi}]")


def _as_pairs(edge_index, device: torch.device, n_nodes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """[2,E] integer tensor/array -> two contiguous int32 device vectors (ids range-checked against ``n_nodes``)."""
    if isinstance(edge_index, np.ndarray):
        edge_index = torch.from_numpy(edge_index)
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise EpsError(f"expected a [2,E] edge list, got {tuple(edge_index.shape)}")
    if n_nodes is not None:
        check_node_ids(edge_index, n_nodes)
    e = edge_index.to(device=device, dtype=torch.int32, non_blocking=True)
    return e[0].contiguous(), e[1].contiguous()


def get_A(adj: CSRGraph, num_nodes: int) -> CSRGraph:
    """adamic_utils.py:8-11.  The reference converts the SparseTensor to a host SciPy CSR (keeping
    edge values); here the adjacency simply stays in HBM -- the returned object is what AA() and
    resource_allocation() take as ``A``."""
    if adj.n_rows != num_nodes or adj.n_cols != num_nodes:
        raise EpsError(f"get_A: adjacency is {adj.sparse_sizes()}, expected [{num_nodes},{num_nodes}]")
    return adj if adj.device.type == "cuda" else adj.to(_default_device())


def node_weight_table(g: CSRGraph, mode: int, f64: bool = False) -> torch.Tensor:
    """K2: mult[w] = 1/log(colsum[w]) (AA) or 1/colsum[w] (RA), inf -> 0; cached on the graph."""
    key = ("node_w", mode, f64)
    if key not in g._cache:
        colsum = ops.col_sums(g.rowptr, g.col, g.val, g.n_cols, f64=f64)
        g._cache[key] = ops.node_weights(colsum, mode, f64=f64)
    return g._cache[key]


def pair_scores_streamed(g: CSRGraph, u: torch.Tensor, v: torch.Tensor, node_w: Optional[torch.Tensor],
                         want_count=False, want_cn=False, grouped=None):
    """Run eps_pair_scores over an arbitrarily long pair list in HBM-sized pieces."""
    n = u.numel()
    if n <= _STREAM_CHUNK:
        return ops.pair_scores(g.rowptr, g.col, g.val, node_w, g.n_rows, u, v, want_count=want_count, want_cn=want_cn,
                               grouped=grouped)
    outs = [[], [], []]
    for s in range(0, n, _STREAM_CHUNK):
        r = ops.pair_scores(g.rowptr, g.col, g.val, node_w, g.n_rows, u[s:s + _STREAM_CHUNK].contiguous(),
                            v[s:s + _STREAM_CHUNK].contiguous(), want_count=want_count, want_cn=want_cn,
                            grouped=grouped)
        for k in range(3):
            if r[k] is not None:
                outs[k].append(r[k])
    return tuple(torch.cat(o) if o else None for o in outs)


def AA(A, edge_index, batch_size: int = 2000, device_out: bool = False):
    """The Adamic-Adar heuristic score (adamic_utils.py:13-25).

    ``A``: adjacency from get_A (or a SciPy CSR).  ``edge_index``: LongTensor [2,E].
    Returns ``(torch.FloatTensor[E], edge_index)`` exactly like the reference; weighted when A
    carries non-unit values (collab): score = sum_w A[u,w] * (A[v,w] / log(colsum[w]))."""
    g = _as_graph(A)
    u, v = _as_pairs(edge_index, g.device, g.n_rows)
    w = node_weight_table(g, ops.W_AA)
    _, _, ws = pair_scores_streamed(g, u, v, w)
    return (ws if device_out else ws.cpu()), edge_index


def resource_allocation(adj_matrix, link_list, batch_size: int = 32768, device_out: bool = False):
    """Resource-Allocation similarity (train_and_eval.py:195-216); ``link_list`` is [m,2].

    An integer-typed SciPy adjacency (filter.py:130-139 builds int64 ones) makes the reference run
    in float64 before the final FloatTensor cast; that case takes the float64-accumulate kernel."""
    f64 = hasattr(adj_matrix, "dtype") and np.issubdtype(np.dtype(adj_matrix.dtype), np.integer)
    g = _as_graph(adj_matrix)
    if isinstance(link_list, np.ndarray):
        link_list = torch.from_numpy(link_list)
    u, v = _as_pairs(link_list.t(), g.device, g.n_rows)
    w = node_weight_table(g, ops.W_RA, f64=f64)
    _, _, ws = pair_scores_streamed(g, u, v, w)
    ws = ws.to(torch.float32)
    return ws if device_out else ws.cpu()


def common_neighbors(adj: CSRGraph, edges: torch.Tensor) -> torch.Tensor:
    """CN(u,v) = sum_w adj[u,w]*adj[v,w] (models.py:536-542); float32 on the adjacency's device."""
    g = _as_graph(adj)
    u, v = _as_pairs(edges, g.device, g.n_rows)
    _, cn, _ = pair_scores_streamed(g, u, v, None, want_cn=True)
    return cn


# ------------------------------------------------------------------------------------------- degree-normalised local indices
# Zhou, Lu, Zhang, "Predicting missing links via local information" (the paper train_and_eval.py:197 cites for RA) compares ten
# local indices; CN, AA and RA are 'simple', 'adamic_ogb' and 'resource_allocation', these are the other seven.  With c the number
# of common STORED neighbours (stored values are ignored, also on collab) and a, b the numbers of stored entries of rows u, v:
#   salton c/sqrt(ab)  jaccard c/(a+b-c)  sorensen 2c/(a+b)  hpi c/min(a,b)  hdi c/max(a,b)  lhn c/(ab)  pa ab;  0/0 -> 0.
LOCAL_INDICES = tuple(ops.LOCAL_INDEX)


def local_index(A, edge_index, index: str) -> torch.Tensor:
    """The local index ``index`` (one of ``LOCAL_INDICES``) of the pairs ``edge_index`` [2,E]: same argument forms and the same
    kind of tensor as ``common_neighbors`` (float32 on the adjacency's device).  The counts come from eps_pair_scores, the
    scores from eps_local_index_pairs (float64 arithmetic on the integers, one rounding): score(u, v) == score(v, u) bit for
    bit, and equal to what ``local_index_columns`` gives the same pair."""
    if index not in ops.LOCAL_INDEX:
        raise EpsError(f"local index '{index}': one of {', '.join(LOCAL_INDICES)}")
    g = _as_graph(A)
    u, v = _as_pairs(edge_index, g.device, g.n_rows)
    cnt, _, _ = pair_scores_streamed(g, u, v, None, want_count=True, want_cn=False)
    return ops.local_index_pairs(g.rowptr, g.n_rows, u, v, cnt, index)


def local_index_columns(g: CSRGraph, v_lo: int, v_hi: int, block, index: str, bar=None, capacity: int = 0, check: bool = True):
    """``local_index`` for a FILTER's access pattern: ``block`` is a ``candidates.ColumnBlock`` of the columns [v_lo, v_hi) whose
    ``cn`` holds the common-neighbour count of every slot (int32, or the float32 unit-weight score of ``ops.expand_unit``);
    padded blocks bring their ``counts``.  ``bar`` None -> float32 scores per slot; a bar -> ``(positions, scores)`` of the slots
    that EXCEED it in ascending position (what ``ColumnBlock.survivors`` holds), or None when more than ``capacity`` do."""
    if index not in ops.LOCAL_INDEX:
        raise EpsError(f"local index '{index}': one of {', '.join(LOCAL_INDICES)}")
    return ops.local_index_columns(g.rowptr, g.n_rows, v_lo, v_hi, block.colptr, block.cand_u, block.cn, index,
                                   counts=block.counts, bar=bar, capacity=capacity, check=check)


# ------------------------------------------------------------------------------------------- local-community indices
# Cannistraci, Alanis-Lobato, Ravasi (Sci. Rep. 3:1613, 2013): a pair is scored by the links AMONG its common neighbours.  With L
# the ascending list of the common STORED neighbours of u and v (stored values are ignored), c = |L|, a, b, d_w the stored
# entries of rows u, v, w, gamma(w) = the members of L other than w stored in row w, G = sum gamma, CAR = c G / 2:
#   car CAR   cpa ((a-c) + CAR)((b-c) + CAR)   caa sum gamma(w)/log2 d_w   cra sum gamma(w)/d_w   cjc CAR/(a+b-c), 0/0 -> 0.
# Lists from csrc/pair_cn_list.hip, gamma and the scores from csrc/local_community.hip.
LOCAL_COMMUNITY_INDICES = tuple(ops.LOCAL_COMMUNITY_INDEX)
LOCAL_COMMUNITY_BUDGET = 1 << 26     # common neighbours listed per piece (4 bytes each for the list, 4 for gamma)


def _budget_cuts(count: torch.Tensor, budget: int):
    """[(lo, hi)]: the pairs cut on the prefix of ``count`` into the longest runs whose counts fit ``budget`` -- a single pair
    beyond it is a run of its own (``models.cn_embed_sum`` cuts the same way)."""
    b = count.numel()
    cum = torch.cumsum(count, 0, dtype=torch.int64)
    if b == 0 or int(cum[-1].item()) <= budget:
        return [(0, b)]
    cum, cuts, s, base = cum.cpu(), [0], 0, 0
    while s < b:
        s = max(s + 1, int(torch.searchsorted(cum, base + budget, right=True)))
        cuts.append(s)
        base = int(cum[s - 1])
    return list(zip(cuts[:-1], cuts[1:]))


def local_community_pairs(g: CSRGraph, u: torch.Tensor, v: torch.Tensor, count: torch.Tensor, index: str) -> torch.Tensor:
    """float32 scores of the pairs (u[p], v[p]) (int32 device vectors, ids inside the graph) whose numbers of common stored
    neighbours are ``count`` (int32).  Pairs with fewer than two are not listed: no link can lie among their common neighbours,
    their closed form comes from the same device function.  The others are listed LOCAL_COMMUNITY_BUDGET entries at a time
    (cut on the counts' prefix; a pair's score does not depend on where the cuts fall), then degrees, then scores."""
    if index not in ops.LOCAL_COMMUNITY_INDEX:
        raise EpsError(f"local-community index '{index}': one of {', '.join(LOCAL_COMMUNITY_INDICES)}")
    out = torch.empty(u.numel(), dtype=torch.float32, device=u.device)
    if u.numel() == 0:
        return out
    listed = count >= 2
    pos, rest = torch.nonzero(listed).squeeze(1), torch.nonzero(~listed).squeeze(1)
    if rest.numel():
        ptr = torch.zeros(rest.numel() + 1, dtype=torch.int64, device=u.device)
        torch.cumsum(count[rest], 0, dtype=torch.int64, out=ptr[1:])
        out[rest] = ops.local_community_scores(g.rowptr, g.n_rows, u[rest], v[rest], ptr, None, None, index)
    if pos.numel():
        lu, lv, lc = u[pos], v[pos], count[pos]
        for lo, hi in _budget_cuts(lc, int(LOCAL_COMMUNITY_BUDGET)):
            pu, pv = lu[lo:hi], lv[lo:hi]
            ptr, w = ops.pair_cn_list(g.rowptr, g.col, g.n_rows, pu, pv, check=False, count=lc[lo:hi])
            gamma = ops.local_community_degrees(g.rowptr, g.col, g.n_rows, ptr, w, check=False)
            out[pos[lo:hi]] = ops.local_community_scores(g.rowptr, g.n_rows, pu, pv, ptr, w, gamma, index, check=False)
    return out


def local_community(A, edge_index, index: str) -> torch.Tensor:
    """The local-community index ``index`` (one of ``LOCAL_COMMUNITY_INDICES``) of the pairs ``edge_index`` [2,E]: same argument
    forms and the same kind of tensor as ``local_index`` (float32 on the adjacency's device).  Counts from
    eps_pair_cn_list_count, then ``local_community_pairs``: score(u, v) == score(v, u) bit for bit, and equal to what
    ``local_community_columns`` gives the same pair."""
    if index not in ops.LOCAL_COMMUNITY_INDEX:
        raise EpsError(f"local-community index '{index}': one of {', '.join(LOCAL_COMMUNITY_INDICES)}")
    g = _as_graph(A)
    u, v = _as_pairs(edge_index, g.device, g.n_rows)
    count = ops.pair_cn_list_count(g.rowptr, g.col, g.n_rows, u, v, check=False)
    return local_community_pairs(g, u, v, count, index)


def local_community_columns(g: CSRGraph, v_lo: int, v_hi: int, block, index: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``local_community`` for a FILTER's access pattern: ``block`` is a ``candidates.ColumnBlock`` of the columns [v_lo, v_hi)
    whose ``cn`` holds the common-neighbour count of every slot (int32, or the float32 unit-weight score of
    ``ops.expand_unit``).  -> float32 scores per slot, into ``out`` when given; the padding slots of a count-free block are not
    written (-inf without ``out``)."""
    n = block.cand_u.numel()
    if out is not None and (out.dtype != torch.float32 or out.numel() != n):
        raise EpsError(f"local_community_columns: out must hold one float32 per slot of the block ({n})")
    if block.padded:
        score = out if out is not None else torch.full((n,), float("-inf"), dtype=torch.float32, device=block.cand_u.device)
        # the counted entries of every column, by the counts (what a padding slot holds is not defined for every expansion)
        counts = block.counts.to(torch.int64)
        first = torch.cumsum(counts, 0) - counts
        seg = torch.repeat_interleave(torch.arange(counts.numel(), device=counts.device), counts)
        pos = block.colptr[seg] + (torch.arange(seg.numel(), device=counts.device) - first[seg])
        u, cn = block.cand_u[pos], block.cn[pos]
        v = (seg + int(v_lo)).to(torch.int32)
    else:
        u, cn = block.cand_u, block.cn
        cols = torch.arange(int(v_lo), int(v_hi), dtype=torch.int32, device=block.cand_u.device)
        v = torch.repeat_interleave(cols, block.colptr[1:] - block.colptr[:-1], output_size=n)
    got = local_community_pairs(g, u.contiguous(), v, cn.to(torch.int32), index)
    if not block.padded and out is None:
        return got
    if block.padded:
        score[pos] = got
    else:
        score = out.copy_(got)
    return score


# ------------------------------------------------------------------------------------------- subgraph sketches
SKETCH_CHUNK = 1 << 22            # pairs per eps_sketch_pair_stats call of the helpers below (their float64 temporaries are per call)


def sketch_cardinality(S: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
    """The HyperLogLog estimate (float64, any shape) from the integer statistics of a 256-register row: S = the sum of
    2^(33 - M_r), Z = the registers that are 0.  E = alpha m^2 2^33 / S with m = 256, alpha = 0.7213 / (1 + 1.079 / m); when
    E <= 2.5 m and Z > 0, linear counting m ln(m / Z) instead.  The empty set (Z = 256) gives 0."""
    m = 256.0
    alpha = 0.7213 / (1.0 + 1.079 / m)
    e = (alpha * m * m * 8589934592.0) / S.to(torch.float64)
    lin = m * torch.log(m / Z.clamp(min=1).to(torch.float64))
    return torch.where((e <= 2.5 * m) & (Z > 0), lin, e)


def sketch_intersections(S: torch.Tensor, Z: torch.Tensor, match: torch.Tensor) -> torch.Tensor:
    """I = (match / 128) E (float64): the estimated size of the intersection of two sketched sets from the statistics of their
    union row (``sketch_cardinality``) and the count of equal MinHash words."""
    return (match.to(torch.float64) / 128.0) * sketch_cardinality(S, Z)


def sketch_feature_formulas(I: torch.Tensor, cu: torch.Tensor, cv: torch.Tensor) -> torch.Tensor:
    """The structural features of BUDDY from the intersections I (float64 [B, K, K]) and the two endpoints' cardinalities
    (float64 [K, B] each) -> float32 [B, 5] (K = 2) or [B, 2] (K = 1): log1p(clamp_min(., 0)) of
        a11 = I11                                       nodes at distance (1, 1)
        a12 = (I12 - I11) + (I21 - I11)                 ... (1, 2) and (2, 1)
        a22 = (I22 - (I12 + I21)) + I11                 ... (2, 2)
        b1  = (C1(u) - I12) + (C1(v) - I21)             within one hop of one endpoint only
        b2  = (((C2(u) - C1(u)) - I22) + I12) + (((C2(v) - C1(v)) - I22) + I21)
    (K = 1: I11 and (C1(u) - I11) + (C1(v) - I11)), each in exactly this association: swapping u and v gives the same bits."""
    k = I.shape[1]
    i11 = I[:, 0, 0]
    if k == 1:
        f = torch.stack([i11, (cu[0] - i11) + (cv[0] - i11)], 1)
    else:
        i12, i21, i22 = I[:, 0, 1], I[:, 1, 0], I[:, 1, 1]
        f = torch.stack([i11,
                         (i12 - i11) + (i21 - i11),
                         (i22 - (i12 + i21)) + i11,
                         (cu[0] - i12) + (cv[0] - i21),
                         (((cu[1] - cu[0]) - i22) + i12) + (((cv[1] - cv[0]) - i22) + i21)], 1)
    return torch.log1p(f.clamp_min(0.0)).to(torch.float32)


def _sketch_pieces(A, edge_index, hops: int):
    g = _as_graph(A)
    u, v = _as_pairs(edge_index, g.device, g.n_rows)
    hll, mh, card = g.sketches(hops)
    for lo in range(0, max(u.numel(), 1), SKETCH_CHUNK):
        pu, pv = u[lo:lo + SKETCH_CHUNK], v[lo:lo + SKETCH_CHUNK]
        yield sketch_intersections(*ops.sketch_pair_stats(hll, mh, g.n_rows, pu, pv, check=False)), card, pu, pv


def sketch_pair_counts(A, edge_index, hops: int = 2) -> torch.Tensor:
    """-> float64 [E, hops, hops] on the adjacency's device: I[b, i - 1, j - 1] estimates |S_i(u_b) & S_j(v_b)| from the graph's
    sketches (``CSRGraph.sketches``; csrc/sketch.hip) -- I[:, 0, 0] estimates the common-neighbour count.  Same argument forms
    as ``local_index``.  I(u, v)[i, j] == I(v, u)[j, i] bit for bit."""
    return torch.cat([I for I, _, _, _ in _sketch_pieces(A, edge_index, hops)])


@torch.no_grad()
def sketch_features(A, edge_index, hops: int = 2) -> torch.Tensor:
    """-> float32 [E, 5] (hops 2) or [E, 2] (hops 1): the structural features ``sketch_feature_formulas`` of the pairs
    ``edge_index`` [2,E] from the graph's sketches.  A constant of the graph: it carries no gradient."""
    return torch.cat([sketch_feature_formulas(I, card[:, pu.long()], card[:, pv.long()]) for I, card, pu, pv in _sketch_pieces(A, edge_index, hops)])


# ------------------------------------------------------------------------------------------- cosine common neighbours
def cosine_graph(adj: CSRGraph, x: torch.Tensor) -> CSRGraph:
    """The graph whose value at stored entry (u, w) is cos(x'_u, x'_w), x' = x + (adj @ x) / (rowsum(adj) + 1e-6)
    (models.py:556-562; adj's values are used in the smoothing, collab is weighted).  The reference forms two
    F.cosine_similarity per (pair, common neighbour) (:566-569); both depend on one stored entry only, so they are computed
    once per entry here: eps_cos_node_features (normalised x', the per-vector clamp of F.cosine_similarity) and
    eps_edge_cosines (one dot per entry; each undirected entry once on a symmetric pattern).  Shares adj's rowptr / col.
    Cached on adj, keyed on the feature tensor itself and its version: train and test graphs (adj_t / full_adj_t) each
    hold their own."""
    g = _as_graph(adj)
    if x is None or x.dim() != 2 or x.shape[0] != g.n_rows:
        raise EpsError(f"cosine_graph: node features must be [{g.n_rows}, F], got "
                       f"{None if x is None else tuple(x.shape)}")
    if g.n_rows != g.n_cols:
        raise EpsError(f"cosine_graph needs a square adjacency, got {g.sparse_sizes()}")

    def build() -> CSRGraph:
        from . import scan
        xin = x.detach().to(device=g.device, dtype=torch.float32)
        if xin.stride(-1) != 1 or xin.stride(0) % 4 or xin.data_ptr() % 16:
            # rows gathered whole as float4 (ppa's 58 features are 232-byte rows): copy into 128-byte aligned rows first
            f = xin.shape[1]
            buf = torch.zeros((xin.shape[0], (f + ops.COS_ROW_FLOATS - 1) // ops.COS_ROW_FLOATS * ops.COS_ROW_FLOATS),
                              dtype=torch.float32, device=g.device)
            buf[:, :f] = xin
            xin = buf[:, :f]
        xhat = ops.cos_node_features(g.rowptr, g.col, g.val, xin)
        revpos = None
        if g.nnz() and g.nnz() < 1 << 31:
            rev = scan.reverse_positions(g)                     # (cached per graph; the filter scan shares the table)
            revpos = rev if scan.is_symmetric(g) else None
        c = ops.edge_cosines(g.rowptr, g.col, xhat, revpos)
        return CSRGraph(g.rowptr, g.col, c, g.n_rows, g.n_cols)

    return g.weight_cached("cosine_graph", x, build)


def cosine_common_neighbors(adj: CSRGraph, x: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """sigmoid(sum_{w in N(u) & N(v)} cos(x'_u, x'_w) * cos(x'_v, x'_w)) per pair (models.py:556-575): the edge-valued
    common-neighbour sum of ``cosine_graph`` (eps_pair_scores), then torch.sigmoid; pairs without a common neighbour
    score 0.5.  float32 [E] on the adjacency's device."""
    g = _as_graph(adj)
    u, v = _as_pairs(edges, g.device, g.n_rows)
    cg = cosine_graph(g, x)
    _, cn, _ = pair_scores_streamed(cg, u, v, None, want_cn=True)
    return torch.sigmoid(cn)


def _aligned_rows(x: torch.Tensor) -> torch.Tensor:
    """x as float32 rows the gathers can read whole as float4: a copy into 128-byte aligned rows where x is not already so."""
    if x.stride(-1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and x.dtype == torch.float32:
        return x
    f = x.shape[1]
    buf = torch.zeros((x.shape[0], (f + ops.COS_ROW_FLOATS - 1) // ops.COS_ROW_FLOATS * ops.COS_ROW_FLOATS),
                      dtype=torch.float32, device=x.device)
    buf[:, :f] = x
    return buf[:, :f]


class _CosineCN(torch.autograd.Function):
    """raw[p] = sum_{w in N(u_p) & N(v_p)} cos(x'_u, x'_w) cos(x'_v, x'_w) with a gradient for the LEADING columns of the
    features: x = [w || feat], w [N, H] the differentiable part (an embedding), feat constant columns or None.  Forward: the
    kernels of ``cosine_graph`` + eps_pair_scores; backward: eps_pair_cn_backward (-> dL/dc per entry),
    eps_cos_features_backward (-> dL/dx' and dL/dx' / deg), and the smoothing's transpose as one eps_spmm_csr over the H columns
    (the adjacency is symmetric, values included: the assumption models._SpMM makes)."""

    @staticmethod
    def forward(ctx, w, feat, g, revpos, u, v):
        x = w.detach() if feat is None else torch.cat([w.detach(), feat.detach().to(w.dtype)], dim=1)
        xhat, nrm = ops.cos_node_features(g.rowptr, g.col, g.val, _aligned_rows(x), want_norm=True)
        c = ops.edge_cosines(g.rowptr, g.col, xhat, revpos)
        _, raw, _ = pair_scores_streamed(CSRGraph(g.rowptr, g.col, c, g.n_rows, g.n_cols), u, v, None, want_cn=True)
        ctx.save_for_backward(xhat, nrm, c, u, v)
        ctx.graph, ctx.revpos, ctx.hidden = g, revpos, w.shape[1]
        return raw

    @staticmethod
    def backward(ctx, grad_raw):
        xhat, nrm, c, u, v = ctx.saved_tensors
        g, h = ctx.graph, ctx.hidden
        gc = ops.pair_cn_backward(g.rowptr, g.col, c, u, v, grad_raw.to(torch.float32).contiguous())
        gxp, gxs = ops.cos_features_backward(g.rowptr, g.col, g.val, xhat, nrm, ctx.revpos, gc, want_scaled=True)
        gx = ops.spmm_csr(g.rowptr, g.col, g.val, gxs[:, :h])
        return gx.add_(gxp[:, :h]), None, None, None, None, None


def cosine_common_neighbors_raw(adj: CSRGraph, x: torch.Tensor, edges: torch.Tensor,
                                feat: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw (pre-sigmoid) cosine common-neighbour sums of ``cosine_common_neighbors`` over the features [x || feat],
    DIFFERENTIABLE in ``x`` (float32 [N, H] on the device, e.g. emb.weight; ``feat`` takes no gradient): what training mlpcos /
    simplecos-with-embedding needs (train_and_eval.py:31-96).  Same forward kernels as the scoring path; nothing is cached --
    the embedding changes every step -- and the backward needs a symmetric adjacency."""
    from . import scan
    g = _as_graph(adj)
    if x is None or x.dim() != 2 or x.shape[0] != g.n_rows or x.shape[1] < 1 or x.dtype != torch.float32:
        raise EpsError(f"cosine_common_neighbors_raw: x must be float32 [{g.n_rows}, H], got "
                       f"{None if x is None else (tuple(x.shape), x.dtype)}")
    if not x.is_cuda:
        raise EpsError("cosine_common_neighbors_raw: x must be on the HIP device (there is no CPU fallback)")
    if feat is not None and (feat.dim() != 2 or feat.shape[0] != g.n_rows):
        raise EpsError(f"cosine_common_neighbors_raw: feat must be [{g.n_rows}, F], got {tuple(feat.shape)}")
    if g.n_rows != g.n_cols:
        raise EpsError(f"cosine_common_neighbors_raw needs a square adjacency, got {g.sparse_sizes()}")
    if g.nnz() >= 1 << 31:
        raise EpsError("cosine_common_neighbors_raw: the reverse-position table takes fewer than 2^31 stored entries")
    if not scan.is_symmetric(g) or not values_are_symmetric(g):
        raise EpsError("cosine_common_neighbors_raw: the backward needs a symmetric adjacency (pattern and values): it "
                       "reads each cosine's gradient at both stored copies and multiplies by A in place of A^T")
    u, v = _as_pairs(edges, g.device, g.n_rows)
    revpos = scan.reverse_positions(g)
    return _CosineCN.apply(x, None if feat is None else feat.to(g.device), g, revpos, u, v)


def values_are_symmetric(g: CSRGraph) -> bool:
    """Whether val[(r, w)] == val[(w, r)] on a graph with a symmetric pattern (cached; unit-valued graphs trivially)."""
    if g.val is None or g.nnz() == 0:
        return True
    if "values_symmetric" not in g._cache:
        from . import scan
        row, col, _ = g.coo()
        rev = g.rowptr[col.long()] + scan.reverse_positions(g).long()
        g._cache["values_symmetric"] = bool(torch.equal(g.val[rev], g.val))
    return g._cache["values_symmetric"]


def sigmoid_raw_cut(bar: float) -> float:
    """A raw threshold t for a bar on sigmoid scores: every float32 raw sum r whose torch.sigmoid(r) exceeds ``bar`` has
    r > t (conservative: candidates at or a little below the bar may pass too, none above it is cut).  The fused kernels
    compare raw sums; the cosine filters' scores are sigmoid(raw).  float32 sigmoid never exceeds 1.0, so a bar that has
    saturated at 1.0 admits nothing (+inf).  Otherwise the bar is lowered by 4 x 2^-24 (four ulps of the float32 scores
    near 1; more than the rounding of any sigmoid implementation) before the exact float64 logit, and the result is
    rounded down to float32."""
    b = float(bar)
    if not b < 1.0:
        return float("inf")
    lo = b - 4.0 * 2.0 ** -24
    if lo <= 0.0:
        return float("-inf")
    t = np.float32(np.log(lo) - np.log1p(-lo))
    if float(t) > np.log(lo) - np.log1p(-lo):
        t = np.nextafter(t, np.float32(-np.inf))
    return float(t)


# ----------------------------------------------------------------------------------------------------------- Katz
KATZ_BETA = 0.05                  # train_and_eval.py:284
EXACT_KATZ_MAX_NODES = 16384      # one dense float64 N x N matrix is 2 GiB at the cap


def katz_coefficients(beta: float = KATZ_BETA, iterations: int = 2) -> Tuple[float, float, float]:
    """Coefficients of A, A^2, A^3 in the reference's truncated series (train_and_eval.py:285-291): ``H = beta*A``, then
    ``H += beta*(A @ H)`` ``iterations`` times.  Each step adds beta*A*H to the WHOLE running H, so two steps give
    beta*A + 2*beta^2*A^2 + beta^3*A^3 (not the textbook series).  Computed exactly from the decimal beta, rounded once."""
    if not 0 <= int(iterations) <= 2:
        raise EpsError(f"truncated Katz: iterations must lie in [0, 2] (the kernel sums up to A^3), got {iterations}")
    b = Fraction(repr(float(beta)))
    c = [b]                                            # c[k] is the coefficient of A^(k+1)
    for _ in range(int(iterations)):
        c = [x + y for x, y in zip(c + [Fraction(0)], [Fraction(0)] + [b * x for x in c])]
    c += [Fraction(0)] * (3 - len(c))
    return tuple(float(x) for x in c)


def _katz_transpose(g: CSRGraph):
    """(A^T, paths_out, paths_in) of a device graph, cached on it.  A symmetric A (every graph add_edges builds) is its own
    transpose: the kernel then reads one set of arrays for both ends."""
    if "katz_t" not in g._cache:
        from .graph import _coalesce
        row, col, val = g.coo()
        rowptr_t, col_t, val_t = _coalesce(col, row, val, g.n_cols, g.n_rows)
        sym = torch.equal(rowptr_t, g.rowptr) and torch.equal(col_t, g.col) and (
            val is None or torch.equal(val_t, val))
        gt = g if sym else CSRGraph(rowptr_t, col_t, val_t, g.n_cols, g.n_rows)
        p_out = ops.two_path_counts(g.rowptr, g.col)
        p_in = p_out if sym else ops.two_path_counts(gt.rowptr, gt.col)
        g._cache["katz_t"] = (gt, p_out, p_in)
    return g._cache["katz_t"]


def truncated_katz(A, edge_index, beta: float = KATZ_BETA, iterations: int = 2, device_out: bool = False) -> torch.Tensor:
    """The collab branch of test_katz (train_and_eval.py:285-291) read at the pairs: float32[E] of
    c1*A[u,v] + c2*(A^2)[u,v] + c3*(A^3)[u,v] with ``katz_coefficients(beta, iterations)``, one eps_katz_pair_scores
    launch set (csrc/katz_pairs.hip) -- neither A^2 nor A^3 is formed.  ``A``: get_A output or SciPy; any square
    matrix (a non-symmetric one gets its transpose built once and cached).  ``edge_index``: [2,E]."""
    coeffs = katz_coefficients(beta, iterations)
    g = _as_graph(A)
    if g.n_rows != g.n_cols:
        raise EpsError(f"truncated Katz needs a square adjacency, got {g.sparse_sizes()}")
    u, v = _as_pairs(edge_index, g.device, g.n_rows)
    gt, p_out, p_in = _katz_transpose(g)
    out = ops.katz_pair_scores(g.rowptr, g.col, g.val, gt.rowptr, gt.col, gt.val, p_out, p_in, g.n_rows, u, v, coeffs)
    return out if device_out else out.cpu()


def truncated_katz_columns(A, v_lo: int, v_hi: int, colptr, cand_u, beta: float = KATZ_BETA, iterations: int = 2,
                           device_out: bool = False) -> torch.Tensor:
    """``truncated_katz`` for a FILTER's access pattern: float32[E] scores of the column-major candidates (cand_u[p], v) of the
    columns [v_lo, v_hi) -- ``colptr`` [v_hi - v_lo + 1] gives every column's range, as ``candidates.expand_block`` lays a block
    out.  One eps_katz_column_scores launch (csrc/katz_columns.hip): (A^2)[:, v] is built once per column and every candidate
    costs one pass over its row.  Same score, bit for bit the same under any split into blocks; any u may be listed."""
    coeffs = katz_coefficients(beta, iterations)
    g = _as_graph(A)
    if g.n_rows != g.n_cols:
        raise EpsError(f"truncated Katz needs a square adjacency, got {g.sparse_sizes()}")
    colptr = torch.as_tensor(colptr).to(device=g.device, dtype=torch.int64).contiguous()
    cand_u = torch.as_tensor(cand_u)
    if cand_u.dtype != torch.int32:             # (ids that an int32 cannot hold stop here; ops checks the range of the rest)
        check_node_ids(cand_u, g.n_rows, "candidate list")
    cand_u = cand_u.to(device=g.device, dtype=torch.int32).contiguous()
    gt, _, p_in = _katz_transpose(g)
    out = ops.katz_column_scores(g.rowptr, g.col, g.val, gt.rowptr, gt.col, gt.val, p_in, g.n_rows, v_lo, v_hi, colptr, cand_u,
                                 coeffs)
    return out if device_out else out.cpu()


def katz_column_steps(g: CSRGraph, cand_u: torch.Tensor) -> int:
    """Three-hop steps of the column kernel on a candidate list: one table lookup per stored entry of every candidate's row,
    sum over the candidates of deg(u).  (Plain tensor ops: also on CPU graphs.)"""
    deg = g.rowptr[1:] - g.rowptr[:-1]
    return int(deg[cand_u.to(torch.int64)].sum().item()) if cand_u.numel() else 0


def katz_steps_bound(g: CSRGraph) -> int:
    """Upper bound of ``katz_column_steps`` over ALL 2-hop non-edges of the graph without listing them: node u is the first
    element of at most min(two-paths out of u, N - 1) candidates, each costing deg(u)."""
    from .candidates import path_counts
    deg = g.rowptr[1:] - g.rowptr[:-1]
    return int((deg * torch.clamp(path_counts(g), max=max(g.n_rows - 1, 0))).sum().item()) if g.n_rows else 0


def exact_katz_bytes(n: int) -> int:
    """Device memory the exact branch needs for an n-node graph: I - beta*A and its inverse, float64 n x n each."""
    return 2 * 8 * int(n) * int(n)


_KATZ_SOLVE_COLUMNS = 512   # right-hand-side columns per triangular solve (see _katz_inverse)


def _katz_inverse(g: CSRGraph, beta: float) -> torch.Tensor:
    """inv(I - beta*A) - I, dense float64 on the device, cached on the graph (test_katz reads one graph's H three times).
    One LU factorisation (rocSOLVER through torch.linalg), then the identity's columns are solved in blocks of
    _KATZ_SOLVE_COLUMNS: a single triangular solve over all N columns (what torch.linalg.inv issues) fails in hipBLAS at
    N = 4267 (HIPBLAS_STATUS_ALLOC_FAILED: it needs more than the workspace torch gives the handle), blocks of 512 run at
    N = 4267 and at the 16384 cap."""
    key = ("katz_inv", float(beta))
    if key not in g._cache:
        n = g.n_rows
        m = torch.zeros((n, n), dtype=torch.float64, device=g.device)
        row, col, _ = g.coo()
        # beta*A is formed in float32 like the reference's SciPy product, then the arithmetic is float64 (coalesced: one write
        # per entry)
        m[row, col] = -(g.values_or_ones() * float(beta)).to(torch.float64)
        m.diagonal().add_(1.0)
        lu, piv, info = torch.linalg.lu_factor_ex(m)
        del m
        if int(info.item()) != 0:
            raise EpsError(f"exact Katz: I - {beta}*A is singular (N={n}); the inverse does not exist")
        h = torch.empty((n, n), dtype=torch.float64, device=g.device)
        rhs = torch.empty((n, min(n, _KATZ_SOLVE_COLUMNS)), dtype=torch.float64, device=g.device)
        for s in range(0, n, _KATZ_SOLVE_COLUMNS):
            e = min(n, s + _KATZ_SOLVE_COLUMNS)
            b = rhs[:, :e - s].zero_()
            b[torch.arange(s, e, device=g.device), torch.arange(e - s, device=g.device)] = 1.0
            h[:, s:e] = torch.linalg.lu_solve(lu, piv, b)
        del lu, rhs
        if not bool(torch.isfinite(h).all()):
            raise EpsError(f"exact Katz: I - {beta}*A is numerically singular (N={n}); the inverse is not finite")
        h.diagonal().sub_(1.0)
        g._cache[key] = h
    return g._cache[key]


def exact_katz(A, edge_index, beta: float = KATZ_BETA, device_out: bool = False) -> torch.Tensor:
    """The non-collab branch of test_katz (train_and_eval.py:293-294): ``inv(I - beta*A) - I`` read at the pairs, float64[E]
    like the reference.  One dense float64 LU inverse per graph through torch.linalg (a factorisation per graph, not a
    per-pair hot path); graphs above EXACT_KATZ_MAX_NODES nodes are refused before anything reaches the device."""
    n = A.n_rows if isinstance(A, CSRGraph) else A.shape[0]
    if n > EXACT_KATZ_MAX_NODES:
        raise EpsError(f"exact Katz: N={n} exceeds EXACT_KATZ_MAX_NODES={EXACT_KATZ_MAX_NODES}; the dense inverse would need "
                       f"{exact_katz_bytes(n) / 2**30:.1f} GiB of device memory (two {n} x {n} float64 matrices)")
    g = _as_graph(A)
    if g.n_rows != g.n_cols:
        raise EpsError(f"exact Katz needs a square adjacency, got {g.sparse_sizes()}")
    u, v = _as_pairs(edge_index, g.device, g.n_rows)
    h = _katz_inverse(g, beta)
    out = h[u.long(), v.long()]
    return out if device_out else out.cpu()


# ------------------------------------------------------------------------------------------ personalized PageRank
# The forward push of Andersen, Chung and Lang in integers and synchronous rounds (csrc/ppr_push.hip, include/eps_abi.h): mass in
# units of 2^-48, alpha = a16 / 65536, a node u pushes while r[u] >= T d(u) with T = ceil(eps * 2^48).  The walk is on the stored
# PATTERN (stored values are ignored, also on collab, as 'simple' and 'adamic' ignore them).  With eps' = T / 2^48 and pi_s the
# exact PPR vector at the effective alpha, on a symmetric pattern and a source that was not capped: 0 <= pi_s(x) - p_s(x) < eps' d(x).
PPR_ALPHA = 0.15                  # common practice (PPRGo, HeaRT), not a measurement
PPR_EPS = 1e-4                    # likewise
PPR_MAX_ROUNDS = 1024             # bounds the kernel's loop by an argument (the golden graphs need at most 86 rounds): not a tuning knob
PPR_SOURCE_CHUNK = 1 << 16        # sources per eps_ppr_push call of ppr_mass ...
PPR_QUERY_CHUNK = 1 << 24         # ... and query nodes (8 bytes of mass each), whichever comes first
PPR_SCALE = 2.0 ** -48


def ppr_parameters(alpha: float = PPR_ALPHA, eps: float = PPR_EPS) -> Tuple[int, int]:
    """(a16, thr) of eps_ppr_push: a16 = round(alpha * 65536) in [1, 32768] (the effective alpha is a16 / 65536 exactly), thr =
    ceil(eps * 2^48) in [1, 2^48].  Refused: thr * (65536 - a16) < 65536, where the share of a push could be 0."""
    alpha, eps = float(alpha), float(eps)
    a16 = int(round(alpha * 65536)) if np.isfinite(alpha) else 0
    if not 1 <= a16 <= 32768:
        raise EpsError(f"ppr: alpha = {alpha} gives a16 = {a16}, outside [1, 32768] (alpha in (0, 1/2])")
    if not (np.isfinite(eps) and 0.0 < eps <= 1.0):
        raise EpsError(f"ppr: eps = {eps} outside (0, 1]")
    thr = int(np.ceil(eps * 2.0 ** 48))          # (a power-of-two scaling of a float is exact)
    if thr * (65536 - a16) < 65536:
        raise EpsError(f"ppr: eps = {eps} (thr = {thr}) is too small for alpha = {alpha}: thr * (65536 - a16) < 65536, a share "
                       "could be 0")
    return a16, thr


def ppr_queries(src: torch.Tensor, dst: torch.Tensor):
    """Directed requests (src[i] -> dst[i]) grouped by source, as eps_ppr_push takes them: -> (sources int32 [S], the unique
    sources ascending; qptr int64 [S + 1]; qnode int32 [E], the targets of source j at qptr[j] : qptr[j + 1] in request order;
    back int64 [E], with mass_of_request = mass[back]).  Plain tensor ops: also on CPU tensors."""
    src, dst = torch.as_tensor(src).reshape(-1), torch.as_tensor(dst).reshape(-1)
    if src.numel() != dst.numel():
        raise EpsError(f"ppr_queries: {src.numel()} sources for {dst.numel()} targets")
    order = torch.sort(src.to(torch.int64), stable=True).indices
    sources, counts = torch.unique_consecutive(src[order].to(torch.int64), return_counts=True)
    qptr = torch.zeros(sources.numel() + 1, dtype=torch.int64, device=src.device)
    qptr[1:] = torch.cumsum(counts, 0)
    back = torch.empty_like(order)
    back[order] = torch.arange(order.numel(), dtype=order.dtype, device=order.device)
    return sources.to(torch.int32), qptr, dst[order].to(torch.int32).contiguous(), back


def _ppr_report(where: str, n_capped: int, n_sources: int, max_rounds: int) -> None:
    if n_capped:
        print(f'{where}: {n_capped} of {n_sources} sources stopped at max_rounds = {max_rounds} with a non-empty frontier '
              '(their estimates keep the bound of the rounds they ran, not eps)')


def ppr_mass(A, src, dst, alpha: float = PPR_ALPHA, eps: float = PPR_EPS, max_rounds: int = PPR_MAX_ROUNDS, table: str = 'auto',
             stats: Optional[dict] = None, where: str = 'ppr') -> torch.Tensor:
    """int64 [E] on the graph's device: p_src[i](dst[i]) in units of 2^-48 for every directed request, one push per DISTINCT
    source (``ppr_queries``), at most PPR_SOURCE_CHUNK sources and PPR_QUERY_CHUNK query nodes per launch so that the query and
    workspace memory stay bounded.  ``stats`` receives sources, capped, pushes, steps and global_sources; capped sources are
    printed once per call."""
    a16, thr = ppr_parameters(alpha, eps)
    g = _as_graph(A)
    if g.n_rows != g.n_cols:
        raise EpsError(f"ppr needs a square adjacency, got {g.sparse_sizes()}")
    src, dst = torch.as_tensor(src).reshape(-1), torch.as_tensor(dst).reshape(-1)
    check_node_ids(src, g.n_rows, "ppr sources"); check_node_ids(dst, g.n_rows, "ppr targets")
    sources, qptr, qnode, back = ppr_queries(src.to(g.device), dst.to(g.device))
    st = {"sources": int(sources.numel()), "capped": 0, "pushes": 0, "steps": 0, "global_sources": 0}
    mass = torch.empty(qnode.numel(), dtype=torch.int64, device=g.device)
    ends = qptr.cpu()
    i, n_s = 0, int(sources.numel())
    while i < n_s:
        j = int(torch.searchsorted(ends, ends[i] + PPR_QUERY_CHUNK, right=True).item()) - 1
        j = max(i + 1, min(j, i + PPR_SOURCE_CHUNK, n_s))
        q0, q1 = int(ends[i]), int(ends[j])
        m, _, pushes, steps, capped = ops.ppr_push(g.rowptr, g.col, g.n_rows, sources[i:j].contiguous(), (qptr[i:j + 1] - q0).contiguous(),
                                                   qnode[q0:q1].contiguous(), a16, thr, max_rounds, table=table, check=False, stats=st)
        mass[q0:q1] = m
        c, p, s = torch.stack([capped.sum().to(torch.int64), pushes.sum(), steps.sum()]).tolist()
        st["capped"] += int(c); st["pushes"] += int(p); st["steps"] += int(s)
        i = j
    _ppr_report(where, st["capped"], n_s, max_rounds)
    if stats is not None:
        stats.update(st)
    return mass[back]


def ppr(A, edge_index, alpha: float = PPR_ALPHA, eps: float = PPR_EPS, device_out: bool = False, max_rounds: int = PPR_MAX_ROUNDS,
        table: str = 'auto', stats: Optional[dict] = None) -> torch.Tensor:
    """The PAIR entry (rank, evaluation lists, the module's forward): float32 [E] of
        score(u, v) = float32(float64(M[u -> v] + M[v -> u]) * 2^-48)
    with M the integer mass of ``ppr_mass`` -- SEAL's pi_u(v) + pi_v(u).  Both directions come out of one set of pushes over the
    union of the endpoints.  The integer sum is below 2^49, so there is exactly one rounding, and score(u, v) == score(v, u) bit
    for bit.  Stored values are ignored.  ``A``: get_A output or SciPy; ``edge_index``: [2, E]."""
    g = _as_graph(A)
    u, v = _as_pairs(edge_index, g.device, g.n_rows)
    n = u.numel()
    m = ppr_mass(g, torch.cat([u, v]), torch.cat([v, u]), alpha, eps, max_rounds, table, stats, where='ppr (pair entry)')
    out = ((m[:n] + m[n:]).to(torch.float64) * PPR_SCALE).to(torch.float32)
    return out if device_out else out.cpu()


def ppr_columns(A, v_lo: int, v_hi: int, colptr, cand_u, alpha: float = PPR_ALPHA, eps: float = PPR_EPS, device_out: bool = False,
                max_rounds: int = PPR_MAX_ROUNDS, table: str = 'auto', stats: Optional[dict] = None, check: bool = True) -> torch.Tensor:
    """The COLUMN entry (a filter's column-major candidate blocks: ``colptr`` [v_hi - v_lo + 1], ``cand_u`` [E], as
    ``candidates.expand_block`` lays a block out): the block already is "sources with query lists", so the source is the column v
    and, by reversibility (d(v) pi_v(u) = d(u) pi_u(v) on a symmetric pattern), one push per column estimates both directions:
        score(u, v) = float32(float64(M[v -> u]) * float64(d(u) + d(v)) / float64(d(u)) * 2^-48)
    as float64 tensor ops in exactly this order.  It is NOT bitwise the pair score and is not claimed to be: from the bound of
    the push, |column - pair| < eps' d(v) plus the float32 rounding.  A graph whose pattern is not symmetric is refused.
    ``check``: the list's ids and the column pointers' ends and order are verified on the host first (``check=False``: a list
    that has just come out of the expansion)."""
    from . import scan
    a16, thr = ppr_parameters(alpha, eps)
    g = _as_graph(A)
    if g.n_rows != g.n_cols:
        raise EpsError(f"ppr needs a square adjacency, got {g.sparse_sizes()}")
    if not scan.is_symmetric(g):
        raise EpsError("ppr_columns: the column entry reads pi_u(v) off pi_v(u) by reversibility, which needs a symmetric "
                       "pattern; score this graph with the pair entry (heuristics.ppr)")
    v_lo, v_hi = int(v_lo), int(v_hi)
    if not 0 <= v_lo <= v_hi <= g.n_rows:
        raise EpsError(f"ppr_columns: columns [{v_lo}, {v_hi}) outside [0, {g.n_rows}]")
    colptr = torch.as_tensor(colptr).to(device=g.device, dtype=torch.int64).contiguous()
    cand_u = torch.as_tensor(cand_u)
    if cand_u.dtype != torch.int32:
        check_node_ids(cand_u, g.n_rows, "candidate list")
    cand_u = cand_u.to(device=g.device, dtype=torch.int32).contiguous()
    if colptr.numel() != v_hi - v_lo + 1:
        raise EpsError(f"ppr_columns: colptr must hold {v_hi - v_lo + 1} entries, got {colptr.numel()}")
    sources = torch.arange(v_lo, v_hi, dtype=torch.int32, device=g.device)
    st = {"sources": v_hi - v_lo, "global_sources": 0}
    m, _, pushes, steps, capped = ops.ppr_push(g.rowptr, g.col, g.n_rows, sources, colptr, cand_u, a16, thr, max_rounds, table=table,
                                               check=check, stats=st)
    c, p, s = torch.stack([capped.sum().to(torch.int64), pushes.sum(), steps.sum()]).tolist() if v_hi > v_lo else (0, 0, 0)
    st.update(capped=int(c), pushes=int(p), steps=int(s))
    _ppr_report(f'ppr (columns [{v_lo}, {v_hi}))', int(c), v_hi - v_lo, max_rounds)
    if stats is not None:
        stats.update(st)
    deg = g.rowptr[1:] - g.rowptr[:-1]
    du = deg[cand_u.long()].to(torch.float64)
    dv = torch.repeat_interleave(deg[v_lo:v_hi], colptr[1:] - colptr[:-1]).to(torch.float64)
    out = (m.to(torch.float64) * (du + dv) / du * PPR_SCALE)
    out = torch.where(du > 0, out, torch.zeros_like(out)).to(torch.float32)       # (a node without entries is never reached: 0)
    return out if device_out else out.cpu()
