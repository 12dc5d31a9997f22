"""The per-node cut (filter.py --keep_per_node k, eps_segment_topk) restated in numpy / torch on the host: what the GPU tests
compare against.  The declared order inside a segment: score descending, then position ascending -- a STABLE descending sort."""
import numpy as np
import torch


def segment_topk_ref(colptr, score, k, counts=None):
    """Positions (int64, ascending within each segment, segments in order) of the k best entries of every segment: per segment
    ``np.argsort(-score, kind="stable")[:k]``, sorted ascending, offset by the segment's start.  (-score: -0.0 and +0.0 compare
    equal in the sort, as the two zeros tie under eps_ordered_bits; no NaN in the cases.)"""
    colptr, score = np.asarray(colptr, dtype=np.int64), np.asarray(score, dtype=np.float32)
    out = []
    for s in range(len(colptr) - 1):
        lo = int(colptr[s])
        n = int(counts[s]) if counts is not None else int(colptr[s + 1]) - lo
        best = np.argsort(-score[lo:lo + n], kind="stable")[:k]
        out.append(np.sort(best).astype(np.int64) + lo)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def segment_topk_bruteforce(colptr, score, k, counts=None):
    """The same by one lexsort over (segment, -score, position) and a rank-in-segment cut: the independent restatement the
    helper itself is tested against."""
    colptr, score = np.asarray(colptr, dtype=np.int64), np.asarray(score, dtype=np.float64)
    seg, pos = [], []
    for s in range(len(colptr) - 1):
        n = int(counts[s]) if counts is not None else int(colptr[s + 1] - colptr[s])
        seg += [s] * n
        pos += list(range(int(colptr[s]), int(colptr[s]) + n))
    seg, pos = np.asarray(seg, np.int64), np.asarray(pos, np.int64)
    if len(pos) == 0:
        return np.zeros(0, np.int64)
    order = np.lexsort((pos, -score[pos], seg))                   # last key first: segment, then score descending, then position
    seg_o, pos_o = seg[order], pos[order]
    first = np.searchsorted(seg_o, seg_o, side="left")             # where each row's segment starts in the sorted list
    keep = pos_o[np.arange(len(seg_o)) - first < k]
    return np.sort(keep)                                          # (segments follow each other in the arrays)


def first_k_rows_per_v(rows: torch.Tensor, k: int) -> torch.Tensor:
    """The file-level restatement: of a whole [E,3] file (u, v, score) in its declared order, the first k rows of every v, the
    order of the kept rows unchanged."""
    v = rows[:, 1].to(torch.int64)
    by_v = torch.sort(v, stable=True).indices                      # rows grouped by v, file order inside a group
    v_sorted = v[by_v]
    start = torch.searchsorted(v_sorted, v_sorted, right=False)    # first row of each row's group
    rank_in_v = torch.arange(v.numel()) - start
    keep = torch.zeros(v.numel(), dtype=torch.bool)
    keep[by_v[rank_in_v < k]] = True
    return rows[keep]
