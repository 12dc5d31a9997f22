"""The filter stage (drop-in for filter.py:26-166): score every 2-hop non-edge with the filter model,
order the candidates, save the proposal file.

Same command line (filter.py:27-47), same checkpoint-name protocol ``spec|edges|num|run.pt`` (:72-76), same
output ``filtered_edges/{spec}_{edges}_{num}_{run}_sorted_edges.pt`` = float32 [E,3] rows (u, v, score)
(:160-165).  Differences, all on purpose:
  * candidates are generated in column blocks on the device and streamed to the scoring kernels; A @ A is
    never materialised on the host;
  * GNN filters compute the node embeddings once, not once per scoring batch;
  * the order is the declared rule (score desc, candidate index asc) instead of an unstable sort;
  * extensions: ``--synthetic`` (seeded stand-in data), ``--keep_top K`` (save only the best K rows -- rank.py
    never reads past ``num_sorted_edge``).
"""
from __future__ import annotations

import argparse
import math
import time
from pathlib import Path

import torch

from . import _lib, candidates, ops, proposals, scan
from .datasets import get_data
from .graph import CSRGraph, add_edges
from .heuristics import (KATZ_BETA, LOCAL_COMMUNITY_INDICES, LOCAL_INDICES, PPR_ALPHA, PPR_EPS, cosine_graph, katz_steps_bound,
                         local_community_columns, local_community_pairs, local_index_columns, node_weight_table, pair_scores_streamed,
                         ppr_columns, sigmoid_raw_cut, truncated_katz, truncated_katz_columns)
from .models import DECODE_PRECISIONS, build_model, default_model_configs


def make_parser():
    parser = argparse.ArgumentParser(description='filter stage (MI355X)')
    parser.add_argument('--dataset', type=str, required=True)
    parser.add_argument('--model', type=str, required=True)
    parser.add_argument('--checkpoint', type=str, required=True)
    parser.add_argument('--num_layers', type=int)
    parser.add_argument('--hidden_channels', type=int)
    parser.add_argument('--dropout', type=float)
    parser.add_argument('--batch_size', type=int)
    parser.add_argument('--lr', type=float)
    parser.add_argument('--epochs', type=int)
    parser.add_argument('--use_feature', type=bool)
    parser.add_argument('--use_learnable_embedding', type=bool)
    parser.add_argument('--device', type=int, default=None)
    # extensions
    parser.add_argument('--dist_backend', type=str, default=None, choices=[None, 'nccl', 'gloo'])
    parser.add_argument('--synthetic', action="store_true", default=False)
    parser.add_argument('--keep_top', type=int, default=0)
    parser.add_argument('--keep_per_node', type=int, default=0, metavar='k',
                        help='for every node v, save only the k best of its candidates (u, v): score descending, then u ascending '
                             '-- exactly the first k rows with second column v of the file the same command writes without the '
                             'flag, in that file\'s order.  A node with fewer than k candidates keeps all of them.  With '
                             '--keep_top K as well: the first K rows of that result.  Default 0: off, nothing changes')
    parser.add_argument('--shard_proposals', action='store_true',
                        help='sharded runs (torchrun) under --keep_top: every rank writes the chunk of the sorted list it ordered '
                             '(<file>.shard{r}of{N}; rank.py reads the shards in rank order) instead of sending its rows to rank 0')
    parser.add_argument('--decode_precision', type=str, default='fp32', choices=list(DECODE_PRECISIONS),
                        help='GNN filters (gcn, sage, dea) under --keep_top K: bf16 screens every candidate block by its LOGIT on the '
                             'bf16 matrix cores, keeps the ceil(G * ceil(K/2)) best unordered pairs, and decodes those once more in '
                             'fp32, exactly as the fp32 run would.  Every score in the file is bit-identical to the fp32 decode of its '
                             'pair and the rows follow the declared tie rule; only MEMBERSHIP can differ from the fp32 run: a pair '
                             'whose bf16 rank falls beyond the kept ones is lost.  Single-process runs only.  Default fp32: the bare '
                             'command is unchanged')
    parser.add_argument('--sketch_hops', type=int, default=2, choices=[1, 2],
                        help='--model buddy: hops of the subgraph sketches and of the node-feature propagation (default 2)')
    parser.add_argument('--gat_heads', type=int, default=None,
                        help='--model gat: attention heads per layer, 1 to 8; --hidden_channels must be a multiple of 4 * heads '
                             '(default 4)')
    parser.add_argument('--ppr_alpha', type=float, default=PPR_ALPHA,
                        help=f'--model ppr: the teleport probability, rounded to a 16-bit fraction in (0, 1/2] (default {PPR_ALPHA})')
    parser.add_argument('--ppr_eps', type=float, default=PPR_EPS,
                        help=f'--model ppr: a node pushes while its residual is at least eps times its degree (default {PPR_EPS})')
    parser.add_argument('--decode_guard', type=float, default=None, metavar='G',
                        help=f'with --decode_precision bf16: the screening pass keeps ceil(G * ceil(K/2)) pairs, G >= 1 '
                             f'(default {DECODE_GUARD_DEFAULT:g}: see DESIGN 4.5d)')
    return parser


DECODE_GUARD_DEFAULT = 4.0     # the rule: twice the smallest measured guard with recall 1.0 on both stand-ins; DESIGN 4.5d says what is measured
BF16_FILTER_MODELS = ('gcn', 'sage', 'dea', 'dea_512', 'gat')


def screen_size(keep: int, guard: float) -> int:
    """M = ceil(G * ceil(K/2)): the unordered pairs the bf16 screening pass keeps for the fp32 decode."""
    k2 = (int(keep) + 1) // 2
    return max(k2, int(math.ceil(float(guard) * k2)))


def check_decode_args(args) -> None:
    """--decode_precision / --decode_guard against the rest of the command line (model flags filled in by
    ``default_model_configs``): a ValueError with the reason for every combination the bf16 screening pass does not serve --
    raised before the dataset is read."""
    precision = getattr(args, "decode_precision", "fp32") or "fp32"
    guard = getattr(args, "decode_guard", None)
    if precision not in DECODE_PRECISIONS:
        raise ValueError(f"--decode_precision {precision}: one of {', '.join(DECODE_PRECISIONS)}")
    if precision == "fp32":
        if guard is not None:
            raise ValueError("--decode_guard goes with --decode_precision bf16 (the fp32 decode screens nothing)")
        return
    if args.model not in BF16_FILTER_MODELS:
        raise ValueError(f"--decode_precision bf16: --model {args.model} has no MLP decode (GNN filters only: gcn, sage, dea)")
    if int(getattr(args, "keep_top", 0) or 0) <= 0:
        raise ValueError("--decode_precision bf16 needs --keep_top K > 0: it screens for the K best rows; the whole file is fp32 work")
    if int(args.keep_top) > scan.MAX_K:
        raise ValueError(f"--decode_precision bf16: --keep_top {args.keep_top} is beyond the selection's {scan.MAX_K} rows")
    if guard is not None and not guard >= 1.0:          # (NaN fails too)
        raise ValueError(f"--decode_guard {guard}: the screening pass keeps G * ceil(K/2) pairs, G >= 1")
    hc = args.hidden_channels
    if hc is None or hc % 16 != 0 or hc > ops.BF16_MAX_HIDDEN:
        raise ValueError(f"--decode_precision bf16: --model {args.model} with --hidden_channels {hc}: the bf16 decode kernel takes "
                         f"a multiple of 16 up to {ops.BF16_MAX_HIDDEN} (wider or odd widths decode in fp32)")
    if args.model in ('gcn', 'sage', 'gat') and (args.num_layers is None or args.num_layers < 2):
        raise ValueError(f"--decode_precision bf16: --num_layers {args.num_layers}: a one-layer decoder has no matrix work")
    import os
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("--decode_precision bf16 runs in one process: sharded runs would have to decode the kept pairs again "
                         "on every rank before the gather (DESIGN 8)")


def check_per_node_args(args) -> None:
    """--keep_per_node against the rest of the command line: a ValueError that names the value for what the per-node cut
    does not serve -- raised before the dataset is read."""
    k = int(getattr(args, "keep_per_node", 0) or 0)
    if k < 0:
        raise ValueError(f"--keep_per_node {k}: the number of proposals kept per node is >= 0 (0: no per-node cut)")
    if k and (getattr(args, "decode_precision", "fp32") or "fp32") == "bf16":
        raise ValueError(f"--keep_per_node {k} with --decode_precision bf16: the bf16 pass screens for ONE global K "
                         "(--keep_top); a per-node cut decodes in fp32")
    if k >= 1 << 31:
        raise ValueError(f"--keep_per_node {k}: the selection takes k < 2^31")


NCN_MODELS = ('ncn', 'ncn_sage')
ONE_PROCESS_MODELS = NCN_MODELS + ('buddy',)


def check_ncn_args(args) -> None:
    """--model ncn / ncn_sage / buddy scores through the model's forward in one process: a sharded run is refused before the
    dataset is read (the row-sharded embedding forward has not been tried with the common-neighbour sums or the sketch features
    on top)."""
    import os
    if args.model in ONE_PROCESS_MODELS and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError(f"--model {args.model} runs in one process: sharded filter runs are not supported for it")


def per_node_positions(pairs, score: torch.Tensor, v_lo: int, v_hi: int, k: int) -> torch.Tensor:
    """Positions (ascending) of the candidates of one block of ``scored_blocks`` that the per-node cut keeps: for every column
    of [v_lo, v_hi) its k best in the declared order (``ops.segment_topk``).  A ``ColumnBlock`` brings its column pointers; an
    int [2,E] pair tensor is column-major, so its pointers are a search of its v row."""
    if not isinstance(pairs, torch.Tensor):
        return ops.segment_topk(pairs.colptr, score, k, counts=pairs.counts)
    v = pairs[1].contiguous()
    colptr = torch.searchsorted(v, torch.arange(v_lo, v_hi + 1, dtype=v.dtype, device=v.device)).to(torch.int64)
    return ops.segment_topk(colptr, score.contiguous(), k)


def train_only_graph(split_edge, num_nodes: int, device) -> CSRGraph:
    """filter.py:130-139: the RA filter scores on a graph built from the TRAIN edges only (both directions,
    integer ones, duplicates summed by the csr_matrix constructor), ignoring proposal edges and adj_t."""
    e = split_edge['train']['edge'].t().to(device)
    both = torch.cat([e, e.flip(0)], 1)
    g = CSRGraph.from_edge_index(both, torch.ones(both.shape[1], device=device), (num_nodes, num_nodes))
    if g.val is not None and bool((g.val == 1).all()):      # every undirected edge listed once (ddi, ppa): unit graph
        g = g.fill_value(1.0)
    return g


def score_block(args, model, data, pairs: torch.Tensor, ra_graph=None) -> torch.Tensor:
    """Scores of one candidate block [2,E_blk] (int64, on device) -> float32 [E_blk] on device."""
    u = pairs[0].to(torch.int32).contiguous()
    v = pairs[1].to(torch.int32).contiguous()
    if args.model == "adamic_ogb":                       # filter.py:122-126
        g = data.adj_t
        return pair_scores_streamed(g, u, v, node_weight_table(g, ops.W_AA), grouped=True)[2]   # column-major blocks
    if args.model == "resource_allocation":              # filter.py:127-142 (float64 math, FloatTensor out)
        w = node_weight_table(ra_graph, ops.W_RA, f64=True)
        return pair_scores_streamed(ra_graph, u, v, w, grouped=True)[2].to(torch.float32)
    if args.model == "katz":                             # (CommonNeighborsPredictor('katz') returns None, as in the reference)
        return truncated_katz(data.adj_t, pairs, beta=KATZ_BETA, device_out=True)
    return model(data.x, pairs, data.adj_t).reshape(-1)  # filter.py:116-121


def rank_column_range(g: CSRGraph, rank: int, world: int):
    """Contiguous column shard of this rank, balanced by 2-hop path counts (the cost of generating + scoring a column)."""
    if world == 1:
        return 0, g.n_rows
    from . import dist as epd
    b = epd.balanced_bounds(epd.column_work(g.rowptr, g.col), world)
    return b[rank], b[rank + 1]


def fused_node_weights(args, g: CSRGraph, ra_graph):
    """Per-node weights that make the fused kernels' sum_w A[u,w]*A[v,w]*node_w[w] the filter model's score, or None
    when the model does not score on the candidate graph itself (GNN filters; RA after proposal edges were added).
    AA: filter.py:122-126; CN 'simple': :116-121 with models.py:536-542 (unit weights); RA: :130-141 scores on the
    train-only graph -- when no proposal edges were added that IS the candidate graph (unit values), with 1/deg formed
    in float64 like the reference's int64 adjacency makes it, then rounded once to float32."""
    if args.model == "adamic_ogb":
        return node_weight_table(g, ops.W_AA)
    if args.model == "simple":
        return torch.ones(g.n_rows, dtype=torch.float32, device=g.device)
    if (args.model == "resource_allocation" and ra_graph is not None and g.val is None and ra_graph.val is None
            and g.nnz() == ra_graph.nnz() and torch.equal(g.rowptr, ra_graph.rowptr) and torch.equal(g.col, ra_graph.col)):
        return node_weight_table(ra_graph, ops.W_RA, f64=True).to(torch.float32)
    return None


GNN_HALF = True            # GNN filters under --keep_top on symmetric graphs: decode every unordered pair once (gnn_half_topk)
GNN_PRUNE_SLACK = 1 << 20  # gnn_half_topk re-cuts its kept pairs to the running bar when it holds more than 4 x ceil(K/2) + this


def _decode(model, data, pairs, precision: str = "fp32"):
    """The filter's scores of ``pairs`` as the model's forward gives them (sigmoid for LinkGNN, logits for DEA_GNN_JK), or, with
    ``precision="bf16"``, the screening LOGITS of the bf16 kernel on the cached bf16 table."""
    if precision != "bf16":
        return model(data.x, pairs, data.adj_t).reshape(-1)
    hb = model.embeddings_bf16(data.x, data.adj_t)
    if hasattr(model, "linkpred"):
        return model.linkpred.decode(hb, pairs, apply_sigmoid=False, precision="bf16")
    return model.decode(hb, pairs, precision="bf16")


def gnn_half_topk(args, model, data, keep: int, rank: int, world: int, precision: str = "fp32", guard: float = None):
    """The ``keep`` best proposals of a GNN filter, decoding each unordered candidate pair ONCE.

    The reference scores both orientations of a pair (filter.py:96-121), but LinkPredictor and DEA_GNN_JK decode h_u * h_v
    (models.py:478-485, :118-120): the product commutes bit for bit, so score(u, v) == score(v, u) (DEA_GNN_JK's scores are
    logits, as the reference writes them).  On a symmetric pattern column v
    therefore lists only its candidates u < v (eps_expand_unit_* with revpos: half the list), the decoder runs on those
    (half the MFMA work -- the decode is all of this filter's time: 39.5 -> 20 s on the ppa stand-in), the pairs whose score
    reaches the running ceil(keep/2)-th best are kept, and the final selection mirrors them and orders the rows by the
    declared rule (score descending, then candidate order), exactly as the threshold scan's does (scan.select_topk).
    -> (pairs int64 [2,<=keep], scores float32), candidates seen (both orientations counted).

    ``precision="bf16"`` (--decode_precision; one process): the blocks are decoded by the bf16 kernel on LOGITS (a saturated
    sigmoid of 1.0f would tie thousands of candidates), the running selection keeps the M = ceil(guard * ceil(keep/2)) best by
    that logit, and the <= M (+ ties) kept pairs are decoded once more in fp32, exactly as the fp32 run calls it; selection,
    mirroring and row order then run on those fp32 scores.  Every score written is therefore the fp32 decode of its pair bit
    for bit and the order is the declared one; only membership can differ: a pair whose bf16 rank falls beyond M is lost."""
    bf16 = precision == "bf16"
    if bf16 and world > 1:
        raise ValueError("--decode_precision bf16 runs in one process")
    g = data.adj_t
    dev = g.device
    revpos, md, sp = scan.reverse_positions(g), scan.max_degree(g), scan.window_splits(g)
    col_lo, col_hi = rank_column_range(g, rank, world)
    blocks = [(max(lo, col_lo), min(hi, col_hi)) for lo, hi in candidates.column_blocks(g) if lo < col_hi and hi > col_lo]
    k2 = screen_size(keep, DECODE_GUARD_DEFAULT if guard is None else guard) if bf16 else (keep + 1) // 2
    keys_l, vals_l, held, bar, n_seen = [], [], 0, None, 0
    if world > 1 and hasattr(model, "embeddings"):
        model.embeddings(data.x, data.adj_t)         # the row-sharded forward holds a collective: every rank reaches it

    def prune():
        nonlocal keys_l, vals_l, held, bar
        keys, vals = torch.cat(keys_l), torch.cat(vals_l)
        if vals.numel() > k2:
            bar = ops.kth_largest(vals, k2)
            m = vals >= bar
            keys, vals = keys[m], vals[m]
        keys_l, vals_l, held = [keys], [vals], keys.numel()

    for v_lo, v_hi in blocks:
        r = ops.expand_unit(g.rowptr, g.col, None, g.n_rows, v_lo, v_hi, md, sp, want_score=False, want_v=True,
                            col_order=candidates.heaviest_first(g, v_lo, v_hi), revpos=revpos)
        pairs = r.pairs                                          # int32 [2, E]: (u; v), u < v
        if pairs.shape[1] == 0:
            continue
        n_seen += 2 * pairs.shape[1]
        sc = _decode(model, data, pairs, precision)
        if bar is not None:
            m = sc >= bar
            pairs, sc = pairs[:, m], sc[m]
        keys_l.append((pairs[1].to(torch.int64) << 32) | pairs[0].to(torch.int64))
        vals_l.append(sc)
        held += sc.numel()
        if held > 4 * k2 + GNN_PRUNE_SLACK:
            prune()
    if keys_l:
        prune()
        keys, vals = keys_l[0], vals_l[0]
    else:
        keys, vals = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    if bf16 and keys.numel():
        # the kept pairs, decoded in fp32 (a pair's score does not depend on what else is in the call)
        vals = _decode(model, data, torch.stack([keys & 0xFFFFFFFF, keys >> 32]).to(torch.int32))
    if world > 1:
        keys, vals = scan._gather_varlen(keys, world), scan._gather_varlen(vals, world)
        n_seen = _sum_over_ranks(n_seen)
    keys, vals = scan.select_topk(keys, vals, keep, g.n_rows)
    return torch.stack([keys & 0xFFFFFFFF, keys >> 32]), vals, n_seen


def _sum_over_ranks(x: int) -> int:
    from . import dist as epd
    t = torch.tensor([x], dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
    return int(sum(int(v.item()) for v in epd.all_gather_list(t)))


CUT_CAPACITY = 1 << 23     # survivors per block the expansion kernel may report (96 MB); more -> the block is redone in full


COSINE_MODELS = ('simplecos', 'mlpcos')
COSINE_FUSED = True        # cosine filters: fused signed expansion (False: candidate lists + the pair kernel, for comparisons)
LAST_COSINE_CUTS = []      # the last fused cosine run, per column block: (v_lo, v_hi, raw threshold or None, "scored" / "cut" / "skipped")


KATZ_COLUMNS = True         # the Katz filter: the column kernel (False: candidate lists + the pair kernel, for comparisons)


def cosine_blocks(args, model, data, blocks, bar=None, fused: bool = True):
    """``scored_blocks`` of the cosine filters (models.py:556-575): candidates of the graph as it is, scores
    sigmoid(sum_w c[u,w] * c[v,w]) with c the stored cosines of ``heuristics.cosine_graph``.  The fused expansion walks
    the cosine graph (same pattern, so the same candidates in the same order) with node_w = 1 through the SIGNED entry
    point -- cosines may be negative, which is why these filters skip the threshold scan, whose screen bounds sums from
    above.  The kernel's cut compares raw sums, so the streaming top-K's bar is translated first
    (``heuristics.sigmoid_raw_cut``: conservative, +inf once the bar has saturated at 1.0).  ``fused=False``, or sums
    whose bound leaves the fixed-point range: candidate lists + the pair kernel (the model's own forward)."""
    g = data.adj_t
    LAST_COSINE_CUTS.clear()
    gc = cosine_graph(g, model.cosine_input(data.x))
    ones = torch.ones(g.n_rows, dtype=torch.float32, device=g.device)
    if fused and not (candidates.hip_expand_available(gc) and candidates.fused_scores_fit(gc, ones)):
        print(f'fused scoring disabled: score bound {candidates.fused_score_bound(gc, ones):.3e} >= 2^22')
        fused = False
    if not fused:
        for v_lo, v_hi in blocks:
            pairs = candidates.expand_block(g, v_lo, v_hi)[0]
            yield v_lo, v_hi, pairs, (score_block(args, model, data, pairs) if pairs.shape[1] else None)
        return
    print(f'fused candidate generation + signed scoring ({args.model})')
    for v_lo, v_hi in blocks:
        thr = bar() if bar is not None else None
        raw_thr = None if thr is None else sigmoid_raw_cut(thr)
        if raw_thr == float("inf"):
            # the K-th score is 1.0f and no float32 sigmoid exceeds it: no later candidate can enter the top-K (an equal
            # score of a later candidate never displaces an earlier one), so the remaining columns are not expanded
            LAST_COSINE_CUTS.append((v_lo, blocks[-1][1], raw_thr, "skipped"))
            print(f'bar saturated at 1.0: columns [{v_lo}, {blocks[-1][1]}) skipped')
            return
        blk = None
        if raw_thr is not None:
            blk = candidates.expand_block_lazy(gc, v_lo, v_hi, ones, want_score=False, cut=(raw_thr, CUT_CAPACITY),
                                               count_free=True, signed=True)
            if blk.survivors is None:
                blk = None
            else:
                pos, raw = blk.survivors
                blk.survivors = (pos, torch.sigmoid(raw))
        if blk is None:
            blk = candidates.expand_block_lazy(gc, v_lo, v_hi, ones, want_score=True, signed=True)
            blk.score = torch.sigmoid(blk.score)
            LAST_COSINE_CUTS.append((v_lo, v_hi, raw_thr, "scored"))
        else:
            LAST_COSINE_CUTS.append((v_lo, v_hi, raw_thr, "cut"))
        yield v_lo, v_hi, blk, blk.score


def katz_blocks(args, data, blocks):
    """``scored_blocks`` of the Katz filter: candidates of the graph as it is (list-only expansion), scores
    beta*A + 2 beta^2 A^2 + beta^3 A^3 at every one of them from the column kernel (csrc/katz_columns.hip), on EVERY dataset --
    the truncated series of test_katz's collab branch (train_and_eval.py:285-291); the exact inverse of its other branch is a
    dense N x N object, and a filter needs an ordering of the 2-hop candidates only.  Blocks are [2,E] pair tensors, so the
    streaming top-K, the per-node cut, column shards and the full sort take them as they take any other block."""
    g = data.adj_t
    print(f'Katz filter: truncated series, beta = {KATZ_BETA}; at most {katz_steps_bound(g):.3e} three-hop steps '
          f'(sum over the candidates of deg(u), bounded from the two-hop path counts of the whole graph)')
    for v_lo, v_hi in blocks:
        pairs = candidates.expand_block(g, v_lo, v_hi)[0]
        if pairs.shape[1] == 0:
            yield v_lo, v_hi, pairs, None
            continue
        v = pairs[1].contiguous()
        colptr = torch.searchsorted(v, torch.arange(v_lo, v_hi + 1, dtype=v.dtype, device=v.device)).to(torch.int64)
        yield v_lo, v_hi, pairs, truncated_katz_columns(g, v_lo, v_hi, colptr, pairs[0], beta=KATZ_BETA, device_out=True)


PPR_COLUMNS = True          # the PPR filter on a symmetric graph: one push per column (False: candidate lists + the pair entry, for comparisons)


def ppr_blocks(model, data, blocks):
    """``scored_blocks`` of the personalized-PageRank filter: candidates of the graph as it is (list-only expansion), then the
    block's column pointers, then the COLUMN entry (``heuristics.ppr_columns``: one fixed-point push per column v, csrc/ppr_push.hip,
    read at the column's candidates and scaled by (d(u) + d(v)) / d(u)).  Blocks are [2,E] pair tensors, so the streaming top-K,
    the per-node cut, column shards and the full sort take them as they take Katz's.  Graphs that do not take this route (a
    pattern that is not symmetric) are scored by the generic list + ``score_block`` route through the PAIR entry
    (``heuristics.ppr``: pi_u(v) + pi_v(u) from two pushes); the two routes estimate the same quantity and differ within
    |column - pair| < eps' d(v) plus the float32 rounding, eps' = ceil(eps 2^48) / 2^48 -- they are not bitwise equal."""
    g = data.adj_t
    alpha, eps = model.ppr_alpha, model.ppr_eps          # (what build_model took from --ppr_alpha / --ppr_eps: the pair entry's too)
    print(f'PPR filter: alpha = {alpha}, eps = {eps}; one push per column, stored values ignored')
    for v_lo, v_hi in blocks:
        pairs = candidates.expand_block(g, v_lo, v_hi)[0]
        if pairs.shape[1] == 0:
            yield v_lo, v_hi, pairs, None
            continue
        v = pairs[1].contiguous()
        colptr = torch.searchsorted(v, torch.arange(v_lo, v_hi + 1, dtype=v.dtype, device=v.device)).to(torch.int64)
        # (the list has just come out of the expansion: its ids and column pointers are the kernels' own)
        yield v_lo, v_hi, pairs, ppr_columns(g, v_lo, v_hi, colptr, pairs[0], alpha=alpha, eps=eps, device_out=True, check=False)


LOCAL_INDEX_CUT = True      # local-index filters under --keep_top: the kernel's survivor lists (False: every block scored in full, for comparisons)
LAST_LOCAL_INDEX_CUTS = []  # the last local-index run, per column block: (v_lo, v_hi, bar or None, "scored" / "cut")


def _counted_block(g: CSRGraph, v_lo: int, v_hi: int, count_free: bool) -> candidates.ColumnBlock:
    """The candidates of columns [v_lo, v_hi) with the number of common stored neighbours of every one in ``cn``: on graphs
    without values the float32 unit-weight score of the list kernels (``ops.expand_unit``: that integer exactly, below 2^24
    nodes), on graphs with values the int32 count of the fused expansion (``want_cn``; stored values play no part).
    ``count_free``: the padded upper-bound layout (``candidates.segment_bounds``), no counting pass."""
    if g.val is None and 0 < g.n_rows < 1 << 24 and g.nnz() < 1 << 30:
        kw = {}
        if count_free:
            pre, pre_host = candidates.segment_bounds(g)
            kw = dict(colptr_ub=(pre[v_lo:v_hi + 1] - pre[v_lo]).contiguous(), total_ub=int(pre_host[v_hi] - pre_host[v_lo]))
        r = ops.expand_unit(g.rowptr, g.col, None, g.n_rows, v_lo, v_hi, scan.max_degree(g), scan.window_splits(g), want_score=True,
                            want_v=False, col_order=candidates.heaviest_first(g, v_lo, v_hi), **kw)
        if count_free and int(r.status.item()):
            raise _lib.EpsError(f"local index filter: the one-pass list of columns [{v_lo}, {v_hi}) reported status {int(r.status.item())}")
        return candidates.ColumnBlock(v_lo, r[0], r[1], r[4], None, counts=r.counts)
    blk = candidates.expand_block_lazy(g, v_lo, v_hi, None, want_cn=True, count_free=count_free)
    blk.score = None
    return blk


def local_index_blocks(args, data, blocks, bar=None):
    """``scored_blocks`` of the degree-normalised local indices (``heuristics.LOCAL_INDICES``): candidates of the graph as it
    is, each with its exact common-neighbour count out of the expansion, scored by the column kernel (csrc/local_index.hip).  A
    degree-normalised score is no sum of per-neighbour weights, so there is no column bound for the threshold scan to screen
    with: every candidate's score is formed.  Once the streaming top-K holds K proposals the kernel hands back only the
    candidates above its bar (``ColumnBlock.survivors``; the count-free layout then costs nothing, nothing scans the block
    afterwards); a block with more than CUT_CAPACITY of them is scored in full instead.  Graphs whose heaviest column outgrows
    the fused expansion's scratch take list + pair-kernel counts, then the same kernel."""
    g = data.adj_t
    LAST_LOCAL_INDEX_CUTS.clear()
    print(f'local index filter ({args.model}): expansion with common-neighbour counts + column kernel')
    fused = candidates.hip_expand_available(g)
    for v_lo, v_hi in blocks:
        if not fused:
            pairs, cn, _ = candidates.expand_block(g, v_lo, v_hi, want_cn=True)
            if pairs.shape[1] == 0:
                yield v_lo, v_hi, pairs, None
                continue
            v = pairs[1].contiguous()
            colptr = torch.searchsorted(v, torch.arange(v_lo, v_hi + 1, dtype=v.dtype, device=v.device)).to(torch.int64)
            blk = candidates.ColumnBlock(v_lo, colptr, pairs[0].to(torch.int32).contiguous(), cn, None)
            yield v_lo, v_hi, pairs, local_index_columns(g, v_lo, v_hi, blk, args.model, check=False)
            continue
        thr = bar() if bar is not None and LOCAL_INDEX_CUT else None
        blk = None
        if thr is not None:
            blk = _counted_block(g, v_lo, v_hi, count_free=True)
            blk.survivors = local_index_columns(g, v_lo, v_hi, blk, args.model, bar=thr, capacity=CUT_CAPACITY, check=False)
            if blk.survivors is None:
                blk = None                           # more survivors than the list holds: score the block in full
        if blk is None:
            blk = _counted_block(g, v_lo, v_hi, count_free=False)
            # (the list has just come out of the expansion: its ids and column pointers are the kernels' own)
            blk.score = local_index_columns(g, v_lo, v_hi, blk, args.model, check=False)
            LAST_LOCAL_INDEX_CUTS.append((v_lo, v_hi, thr, "scored"))
        else:
            LAST_LOCAL_INDEX_CUTS.append((v_lo, v_hi, thr, "cut"))
        yield v_lo, v_hi, blk, blk.score


def local_community_blocks(args, data, blocks):
    """``scored_blocks`` of the local-community indices (``heuristics.LOCAL_COMMUNITY_INDICES``): candidates of the graph as it
    is, each with its exact common-neighbour count out of the expansion (``_counted_block``).  The candidates with two or more
    common neighbours are compacted, listed with their counts given (no counting launch: csrc/pair_cn_list.hip), their lists
    run through the degree and the score kernels (csrc/local_community.hip) a budget of list entries at a time, and the scores
    scattered back; the others get their closed form from the same device function (``heuristics.local_community_pairs``).
    Every candidate's score is written: these scores are no sum of per-node weights, so there is no bound to screen with, and
    a survivor-only path under the running bar is not built.  Graphs whose heaviest column outgrows the fused expansion's
    scratch take list + pair-kernel counts, then the same kernels."""
    g = data.adj_t
    print(f'local-community filter ({args.model}): expansion with common-neighbour counts + list, degree and score kernels')
    fused = candidates.hip_expand_available(g)
    for v_lo, v_hi in blocks:
        if not fused:
            pairs, cn, _ = candidates.expand_block(g, v_lo, v_hi, want_cn=True)
            if pairs.shape[1] == 0:
                yield v_lo, v_hi, pairs, None
                continue
            yield v_lo, v_hi, pairs, local_community_pairs(g, pairs[0].to(torch.int32).contiguous(), pairs[1].to(torch.int32).contiguous(),
                                                           cn.to(torch.int32), args.model)
            continue
        blk = _counted_block(g, v_lo, v_hi, count_free=False)
        blk.score = local_community_columns(g, v_lo, v_hi, blk, args.model)
        yield v_lo, v_hi, blk, blk.score


def scored_blocks(args, model, data, ra_graph, col_lo: int = 0, col_hi: int = None, bar=None):
    """(v_lo, v_hi, pairs, scores) per column block.  Heuristic filters whose scoring graph IS the candidate graph
    (AA: filter.py:122-126; CN 'simple': :116-121 with models.py:536-542) come out of the fused expansion already
    scored; RA scores on the train-only graph (filter.py:130-141) and GNN filters decode the block's pairs; the cosine
    filters score the cosine graph (``cosine_blocks``); the local indices score (count, degrees) per candidate
    (``local_index_blocks``), the local-community indices the links among every candidate's common neighbours
    (``local_community_blocks``)."""
    g = data.adj_t
    col_hi = g.n_rows if col_hi is None else col_hi
    blocks = [(max(lo, col_lo), min(hi, col_hi)) for lo, hi in candidates.column_blocks(g) if lo < col_hi and hi > col_lo]
    if args.model in COSINE_MODELS:
        yield from cosine_blocks(args, model, data, blocks, bar, fused=COSINE_FUSED and candidates.hip_expand_available(g))
        return
    if args.model == "katz" and KATZ_COLUMNS and candidates.hip_expand_available(g, scored=False):
        yield from katz_blocks(args, data, blocks)
        return
    if args.model == "ppr" and PPR_COLUMNS and candidates.hip_expand_available(g, scored=False) and scan.is_symmetric(g):
        yield from ppr_blocks(model, data, blocks)
        return
    if args.model in LOCAL_INDICES and candidates.hip_expand_available(g, scored=False):
        yield from local_index_blocks(args, data, blocks, bar)
        return
    if args.model in LOCAL_COMMUNITY_INDICES and candidates.hip_expand_available(g, scored=False):
        yield from local_community_blocks(args, data, blocks)
        return
    node_w = fused_node_weights(args, g, ra_graph) if candidates.hip_expand_available(g) else None
    if node_w is not None and not candidates.fused_scores_fit(g, node_w):
        # weights so large that a score could leave the fused kernels' fixed-point range: float32 / float64 pair kernels
        print(f'fused scoring disabled: score bound {candidates.fused_score_bound(g, node_w):.3e} >= 2^22')
        node_w = None
    if node_w is None:
        for v_lo, v_hi in blocks:
            pairs = candidates.expand_block(g, v_lo, v_hi)[0]      # HIP expansion (list only); scores from score_block
            yield v_lo, v_hi, pairs, (score_block(args, model, data, pairs, ra_graph) if pairs.shape[1] else None)
        return
    print(f'fused candidate generation + scoring ({args.model})')
    for v_lo, v_hi in blocks:
        # once the streaming top-K holds K proposals (``bar()`` is its K-th score) only candidates above that bar matter:
        # the kernel reports them directly and the block's score array is neither written nor scanned
        thr = bar() if bar is not None else None
        blk = None
        if thr is not None:
            # (nothing scans the block afterwards, so the count-free segment layout costs nothing and saves the counting pass)
            blk = candidates.expand_block_lazy(g, v_lo, v_hi, node_w, want_score=False, cut=(thr, CUT_CAPACITY),
                                               count_free=True)
            if blk.survivors is None:
                blk = None                           # more survivors than the list holds: score the block in full
        if blk is None:
            blk = candidates.expand_block_lazy(g, v_lo, v_hi, node_w, want_score=True)
        yield v_lo, v_hi, blk, blk.score


LAST_TIMING = {}      # the last run's scoring section: {"scored_s": host stopwatch, "gpu_ms": HIP events on the stream, "candidates": n}


class _Stopwatch:
    """The scoring section of a run on both clocks: host wall (what the stage prints) and a pair of HIP events on the current
    stream around the same section (bench_configs.py reports both: `wall_s` of a CLI leg also holds stand-in generation,
    checkpoint and file I/O, which say nothing about the engine)."""

    def __init__(self, device):
        self.device = device
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e1 = torch.cuda.Event(enable_timing=True)
        self.e0.record(torch.cuda.current_stream(device))
        self.t0 = time.perf_counter()

    def stop(self, candidates: int) -> float:
        self.e1.record(torch.cuda.current_stream(self.device))
        torch.cuda.synchronize(self.device)
        dt = time.perf_counter() - self.t0
        LAST_TIMING.clear()
        LAST_TIMING.update(scored_s=dt, gpu_ms=self.e0.elapsed_time(self.e1), candidates=int(candidates))
        return dt


def run(args) -> str:
    args = default_model_configs(args)
    check_per_node_args(args)
    check_decode_args(args)
    check_ncn_args(args)
    print(args)
    Path("filtered_edges").mkdir(exist_ok=True)
    if not torch.cuda.is_available():
        raise RuntimeError("filter stage needs a HIP device: the scoring path has no CPU fallback")
    # one process per GPU under torchrun (WORLD_SIZE > 1): candidate COLUMNS are sharded, the graph is replicated, the
    # only exchange is the final merge (top-K lists under --keep_top, else the shards of the full list)
    from . import dist as epd
    rank, world, dist_dev = epd.init_from_env(args.dist_backend, args.device)
    device = dist_dev if world > 1 else torch.device(f'cuda:{args.device or 0}')
    _lib.warm_up_async(device)           # (code objects load in the background while the dataset is read on the host)
    ops._pinned_words([0])               # (... and the pinned staging ring of the survivor records is allocated now, not inside the timed section)

    edge_index, edge_weight, split_edge, data = get_data(args)
    data = data.to(device)
    model = build_model(args, data, device)
    print(f'using model {model}')
    use_params = sum(p.numel() for p in model.parameters() if p.requires_grad) > 0
    print('using params?', use_params)
    if use_params:
        model.load_state_dict(torch.load(f'models/{args.checkpoint}', map_location=device))

    parts = args.checkpoint.split("|")
    spec, sorted_edge_path, num_sorted_edge = parts[0], parts[1], int(parts[2])
    run_id = parts[3].split(".")[0]
    if sorted_edge_path:
        print("Loading corresponding extra edges from ", sorted_edge_path)
        extra_edges = proposals.load_proposals(f"filtered_edges/{sorted_edge_path}.pt", num_sorted_edge)
        assert extra_edges.size(0) == 2 and extra_edges.size(1) == num_sorted_edge
    else:
        extra_edges = torch.zeros([2, 0], dtype=torch.long)
    data.adj_t = add_edges(args.dataset, edge_index.to(device), edge_weight.to(device), extra_edges.to(device),
                           data.num_nodes)
    model.eval()
    ra_graph = train_only_graph(split_edge, data.num_nodes, device) if args.model == "resource_allocation" else None

    _lib.warm_up_join()                  # (the background loads are done -- or given up on -- before anything is timed)
    watch = _Stopwatch(device)
    keep = int(args.keep_top)
    # --keep_per_node: the threshold scan, the dense product and the half lists all cut (or mirror) GLOBALLY, so the run takes
    # the block route with every candidate scored, cuts each column of each block there, and --keep_top is applied to the
    # ordered result at the end (in a sharded run the counts printed are this rank's)
    per_node = int(getattr(args, "keep_per_node", 0) or 0)
    if per_node:
        keep_rows, keep = keep, 0
    if keep == 0 and not per_node and args.model == "simple" and world == 1 and candidates.dense_cn_suits(data.adj_t):
        # configs[0]: a small DENSE graph (ddi: N = 4,267, 11.7 % of all pairs are edges).  Common-neighbour counts = A A^T, ONE
        # product on the matrix cores (exact: counts < 2^24), the reference's candidate list a masked read of it in its own
        # column-major order, and the file's order ONE stable sort by the integer count -- no per-graph table, a dozen launches
        # (csrc/dense_cn.hip; the sparse path took 7.5 ms of GPU time in hundreds of launches for the same 16 M rows)
        g = data.adj_t
        with torch.no_grad():
            got = ops.dense_cn_candidates(g.rowptr, g.col, g.n_rows, directed=True, check_symmetric=True, as_rows=True)
        if got is not None:                      # (an asymmetric pattern takes the general path below)
            rows, cnt = got
            rows = rows[torch.sort(cnt.to(torch.int16), descending=True, stable=True).indices]  # counts <= N - 2 < 2^15
            n_seen = int(rows.shape[0])
            dt = watch.stop(n_seen)
            print('dense common-neighbour product (A A^T on the f32 MFMA)')
            print(f'using {n_seen} edges; scored in {dt:.2f} s ({n_seen / max(dt, 1e-9):.3e} candidate edges/s incl. generation)')
            return _save(args, spec, sorted_edge_path, num_sorted_edge, run_id, rank, world, rows)
    if 0 < keep <= scan.MAX_K and args.model not in COSINE_MODELS + ("katz", "ppr") + LOCAL_INDICES + LOCAL_COMMUNITY_INDICES and scan.scan_plausible(data.adj_t):
        # (the hubs-first copy first: the symmetry check of scan_available then reads the COPY's reverse positions -- the table
        #  the scan needs anyway -- instead of building one for the graph as labelled, 3-5 ms on a ppa-sized graph)
        scan.scan_graph(data.adj_t, build=True)
    scan_w = fused_node_weights(args, data.adj_t, ra_graph) if 0 < keep <= scan.MAX_K and scan.scan_available(data.adj_t) else None
    if scan_w is not None and not scan.scan_usable(data.adj_t, scan_w):
        scan_w = None                    # sums could leave the scan's fixed-point range: the pair kernels score this graph
    if scan_w is not None:
        # --keep_top with a heuristic filter on a symmetric graph (unit-valued, or collab's summed multi-edge weights): one
        # threshold scan of the whole candidate set (csrc/scan_pieces.hip / filter_scan.hip) instead of candidate blocks +
        # streaming top-K; every rank ends with the same list
        # (count=False: a launch with skipped heads counts the candidates its walk TOUCHES; the exact size of the candidate set
        #  would be one more scan of the graph -- a fifth of this one-shot run -- for a number that is only printed)
        st = {"count": False}
        with torch.no_grad():
            # (the file is written by rank 0: the ordered rows travel there alone)
            shards = world > 1 and bool(getattr(args, "shard_proposals", False))
            best_pairs, best_scores = scan.scan_topk(data.adj_t, scan_w, keep, rank, world, stats=st, relabel=True,
                                                     rows_on="shards" if shards else (0 if world > 1 else None))
        n_seen = st["candidates"] if st["candidates"] is not None else st["touched"]
        dt = watch.stop(n_seen)
        bar = None if st["bar"] is None else float(st["bar"])
        print(f'threshold scan ({args.model}): bar {bar}, {st["survivors"]} survivors, {st["launches"]} launches'
              + (f', heads skipped under a budget of {st["head_budget"]:.4f}' if st.get("heads") else ''))
        print(f'using {"at least " if st["candidates"] is None else ""}{n_seen} edges; scored in {dt:.2f} s '
              f'({n_seen / max(dt, 1e-9):.3e} candidate edges/s incl. generation)'
              + (' -- every 2-hop non-edge is covered by the bound; the count is of those the walk touched' if st["candidates"] is None else ''))
        return _save(args, spec, sorted_edge_path, num_sorted_edge, run_id, rank, world,
                     None if best_pairs is None else torch.cat([best_pairs.t().to(torch.float32), best_scores.unsqueeze(1)], 1),
                     sharded=shards)
    full_w = (fused_node_weights(args, data.adj_t, ra_graph)
              if keep == 0 and not per_node and data.adj_t.val is None and scan.scan_available(data.adj_t) else None)
    if (full_w is not None and candidates.fused_scores_fit(data.adj_t, full_w)
            and int(scan.half_paths(data.adj_t).sum().item()) < 1 << 29):      # (unordered pairs <= half paths: lists that fit)
        # the whole [E,3] file of a heuristic filter on a unit-valued symmetric graph: scores are symmetric too, so the list
        # kernels write each unordered pair once (column v: its candidates u < v), and the rows -- both orientations -- come
        # out of the same mirror + declared-order sort the threshold scan's selection uses
        g = data.adj_t
        col_lo, col_hi = rank_column_range(g, rank, world)
        keys_l, vals_l = [], []
        with torch.no_grad():
            for lo, hi in candidates.column_blocks(g):
                lo, hi = max(lo, col_lo), min(hi, col_hi)
                if lo >= hi:
                    continue
                r = ops.expand_unit(g.rowptr, g.col, full_w, g.n_rows, lo, hi, scan.max_degree(g), scan.window_splits(g),
                                    col_order=candidates.heaviest_first(g, lo, hi), revpos=scan.reverse_positions(g))
                keys_l.append((r.pairs[1].to(torch.int64) << 32) | r.pairs[0].to(torch.int64))
                vals_l.append(r[4])
        keys = torch.cat(keys_l) if keys_l else torch.zeros(0, dtype=torch.int64, device=device)
        vals = torch.cat(vals_l) if vals_l else torch.zeros(0, dtype=torch.float32, device=device)
        if world > 1:
            keys, vals = scan._gather_varlen(keys, world), scan._gather_varlen(vals, world)
        if keys.numel():
            rows_k, rows_v = scan.select_topk(keys, vals, 2 * keys.numel(), g.n_rows)
            n_seen = rows_k.numel()
            dt = watch.stop(n_seen)
            print(f'using {n_seen} edges; scored in {dt:.2f} s ({n_seen / max(dt, 1e-9):.3e} candidate edges/s incl. generation)')
            rows = torch.stack([(rows_k & 0xFFFFFFFF).to(torch.float32), (rows_k >> 32).to(torch.float32), rows_v], 1)
            return _save(args, spec, sorted_edge_path, num_sorted_edge, run_id, rank, world, rows)
    from .models import DEA_GNN_JK, LinkGNN
    if (GNN_HALF and not per_node and 0 <= keep <= scan.MAX_K and isinstance(model, (LinkGNN, DEA_GNN_JK)) and data.adj_t.device.type == "cuda"
            and data.adj_t.n_rows == data.adj_t.n_cols and data.adj_t.nnz() < 1 << 30 and scan.is_symmetric(data.adj_t)
            and (keep > 0 or int(scan.half_paths(data.adj_t).sum().item()) < 1 << 29)):     # (the whole file: lists that fit)
        with torch.no_grad():
            best_pairs, best_scores, n_seen = gnn_half_topk(args, model, data, keep if keep else scan.MAX_K, rank, world,
                                                            precision=getattr(args, "decode_precision", "fp32"),
                                                            guard=getattr(args, "decode_guard", None))
        dt = watch.stop(n_seen)
        print(f'GNN filter, each unordered pair decoded once ({args.model})'
              + (f'; bf16 screening, {screen_size(keep, args.decode_guard or DECODE_GUARD_DEFAULT)} pairs decoded again in fp32'
                 if getattr(args, "decode_precision", "fp32") == "bf16" else ''))
        print(f'using {n_seen} edges; scored in {dt:.2f} s ({n_seen / max(dt, 1e-9):.3e} candidate edges/s incl. generation)')
        return _save(args, spec, sorted_edge_path, num_sorted_edge, run_id, rank, world,
                     torch.cat([best_pairs.t().to(torch.float32), best_scores.unsqueeze(1)], 1))
    if getattr(args, "decode_precision", "fp32") == "bf16":
        raise ValueError("--decode_precision bf16: this graph does not take the half-list route of the GNN filters (it needs a "
                         "symmetric adjacency on the device); run it in fp32")
    col_lo, col_hi = rank_column_range(data.adj_t, rank, world)
    n_seen, sel_s = 0, 0.0
    all_pairs, all_scores = [], []
    top = proposals.StreamingTopK(keep) if keep else None
    if world > 1 and hasattr(model, "embeddings"):
        # the row-sharded GNN forward holds a collective: every rank must reach it, whatever its column shard yields
        with torch.no_grad():
            model.embeddings(data.x, data.adj_t)
    with torch.no_grad():
        for v_lo, v_hi, pairs, score in scored_blocks(args, model, data, ra_graph, col_lo, col_hi,
                                                      bar=top.bar if keep else None):
            n_blk = pairs.numel() if (not isinstance(pairs, torch.Tensor)) else pairs.shape[1]
            if n_blk == 0:
                continue
            if keep:
                top.push(pairs, score)          # blocks arrive in candidate (column-major) order
            elif per_node:                      # every column of the block cut to its k best (csrc/segment_topk.hip)
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                pos = per_node_positions(pairs, score, v_lo, v_hi, per_node)
                all_pairs.append(pairs[:, pos].long() if isinstance(pairs, torch.Tensor) else pairs.select(pos))
                all_scores.append(score[pos])
                torch.cuda.synchronize(device)
                sel_s += time.perf_counter() - t0
            elif not isinstance(pairs, torch.Tensor):     # candidates.ColumnBlock, possibly padded
                idx = pairs.valid()
                all_pairs.append(pairs.select(idx))
                all_scores.append(score[idx])
            else:
                all_pairs.append(pairs)
                all_scores.append(score)
            n_seen += n_blk
    dt = watch.stop(n_seen)
    if per_node:
        print(f'per-node cut: k = {per_node}, {sum(int(x.numel()) for x in all_scores)} rows kept of {n_seen} candidates seen; '
              f'selected in {sel_s:.2f} s')
    print(f'using {n_seen} edges; scored in {dt:.2f} s ({n_seen / max(dt, 1e-9):.3e} candidate edges/s incl. generation)')

    if keep:
        best_pairs, best_scores = top.result()
        best_pairs, best_scores = best_pairs.to(device), best_scores.to(device)
        if world > 1:
            # ranks hold contiguous column ranges in rank order: gather the (padded) per-rank lists -- K x 20 B each --
            # and stable-merge them in rank order
            n_mine = torch.tensor([best_scores.numel()], dtype=torch.int64, device=device)
            n_all = epd.all_gather_list(n_mine)
            pad_s = torch.full((keep,), float("-inf"), dtype=torch.float32, device=device)
            pad_p = torch.zeros((2, keep), dtype=torch.int64, device=device)
            pad_s[:best_scores.numel()] = best_scores
            pad_p[:, :best_pairs.shape[1]] = best_pairs
            gs = epd.all_gather_list(pad_s)
            gp = epd.all_gather_list(pad_p)
            cnt = [int(x.item()) for x in n_all]
            best_pairs, best_scores = proposals.merge_ranked_lists([gp[r][:, :cnt[r]] for r in range(world)],
                                                                   [gs[r][:cnt[r]] for r in range(world)], keep)
        sorted_edges = torch.cat([best_pairs.t().to(torch.float32), best_scores.unsqueeze(1)], 1)
    else:
        pairs = torch.cat(all_pairs, 1) if all_pairs else torch.zeros((2, 0), dtype=torch.int64, device=device)
        scores = torch.cat(all_scores) if all_scores else torch.zeros(0, dtype=torch.float32, device=device)
        if world > 1:
            # the full list: ranks hold contiguous column ranges in rank order, so the shards concatenated in rank order ARE
            # the single-process candidate order -- one variable-length all-gather (20 B per candidate; sized for lists that
            # fit one GPU, which is what a file of all [E,3] rows presupposes), then the same sort on every rank
            pairs = torch.stack([scan._gather_varlen(pairs[0].contiguous(), world),
                                 scan._gather_varlen(pairs[1].contiguous(), world)])
            scores = scan._gather_varlen(scores, world)
        sorted_edges = proposals.sorted_edges_tensor(pairs, scores)          # filter.py:160-161
        if per_node and keep_rows:
            sorted_edges = sorted_edges[:keep_rows]      # --keep_top on top of the per-node cut: the first K rows of that file
    return _save(args, spec, sorted_edge_path, num_sorted_edge, run_id, rank, world, sorted_edges)


def _save(args, spec, sorted_edge_path, num_sorted_edge, run_id, rank, world, sorted_edges, sharded: bool = False) -> str:
    filename = f'filtered_edges/{spec}_{sorted_edge_path}_{num_sorted_edge}_{run_id}_sorted_edges.pt'
    if sharded:
        # (every rank holds the chunk of the sorted list it ordered: rank r's rows follow rank r - 1's -- proposals.load_sorted_edges)
        import os
        if rank == 0 and os.path.exists(filename):
            os.remove(filename)                      # (a list of an earlier, unsharded run would shadow the shards)
        proposals.save_sorted_edges_shard(filename, sorted_edges, rank, world)
        print(f"rank {rank}: {sorted_edges.shape[0]} rows to {proposals.shard_path(filename, rank, world)}")
    elif rank == 0:
        print(sorted_edges)
        proposals.save_sorted_edges(filename, sorted_edges)                    # filter.py:164-165
        print("Saving to ", filename)
    if world > 1:
        torch.distributed.barrier()
    return filename


def main(argv=None):
    return run(make_parser().parse_args(argv))
