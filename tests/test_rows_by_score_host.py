"""CPU: the truth module of eps_rows_by_score (tests/rows_by_score_truth.py) against small cases worked out by hand -- the bucket
edges that make the cut, liveness at the bar, and the declared row order with and without a relabelling."""
import numpy as np

import rows_by_score_truth as rt


def _f(bits: int) -> np.float32:
    return np.array([bits], np.uint32).view(np.float32)[0]


def _bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def test_bucket_edges_by_hand():
    # distances below 2^8 are their own bucket; above, a bucket keeps the top bit and the eight bits below it
    assert [rt.bucket(d) for d in (0, 1, 255, 256, 257, 511, 512)] == [0, 1, 255, 256, 257, 511, 512]
    assert rt.bucket(1 << 22) == 15 << 8 and rt.bucket_floor(15 << 8) == 1 << 22
    assert rt.bucket(0x6147AE) == (15 << 8) | 0x85 and rt.bucket_floor((15 << 8) | 0x85) == 0x614000
    assert rt.bucket((1 << 23) + 3) == 16 << 8 and rt.bucket_floor(16 << 8) == 1 << 23
    for b in (0, 1, 255, 256, 300, 4096, 6399):
        assert rt.bucket(rt.bucket_floor(b)) == b
    # the ordered pattern ascends with the value and takes -0 for +0
    xs = [-np.inf, -2.0, -1e-30, 0.0, 1e-30, 1.0, np.inf]
    assert [rt.ordered(x) for x in xs] == sorted(rt.ordered(x) for x in xs)
    assert rt.ordered(-0.0) == rt.ordered(0.0) == 0x80000000
    for x in xs:
        assert _bits(rt.unordered(rt.ordered(x))) == _bits(x)


def test_cut_and_count_by_hand():
    above = _f(0x3F800001)                                    # the float next above the bar
    vals = np.array([3.0, 1.76, 1.0, above, -np.inf, 0.5, 2.0], np.float32)
    # live: 3, 1.76, the float above the bar, 2 -- the entry AT the bar, the one below it and -inf are not
    want = {0: (-np.inf, 4), 1: (3.0, 1), 2: (2.0, 2), 3: (_f(0x3FE14000), 3), 4: (above, 4), 5: (-np.inf, 4)}
    for k2, (cut, n_sel) in want.items():
        got_cut, got_n, sel = rt.cut_and_count(vals, 1.0, k2)
        assert (_bits(got_cut), got_n) == (_bits(cut), n_sel), k2
        assert int(sel.sum()) == n_sel and not sel[[2, 4, 5]].any()
    # 1.76 sits 0x6147AE steps above 1.0: its bucket's lower edge is 0x614000 steps above (1.759765625), so a score between the two
    # is selected with it
    got_cut, got_n, _ = rt.cut_and_count(np.array([1.76, 1.7598, 1.7597], np.float32), 1.0, 1)
    assert _bits(got_cut) == 0x3FE14000 and got_n == 2
    # nothing live
    assert rt.cut_and_count(np.array([1.0, 0.0], np.float32), 1.0, 1)[:2] == (np.float32(-np.inf), 0)
    assert rt.cut_and_count(np.zeros(0, np.float32), 1.0, 3)[:2] == (np.float32(-np.inf), 0)


def test_row_order_by_hand():
    keys = np.array([(5 << 32) | 1, (3 << 32) | 2, (9 << 32) | 0], np.int64)          # v << 32 | u
    vals = np.array([2.0, 2.0, 7.0], np.float32)
    pairs, scores = rt.ordered_rows(keys, vals, 10)
    assert pairs.tolist() == [[9, 0, 5, 3, 2, 1], [0, 9, 1, 2, 3, 5]] and scores.tolist() == [7, 7, 2, 2, 2, 2]
    pairs, scores = rt.ordered_rows(keys, vals, 3)
    assert pairs.tolist() == [[9, 0, 5], [0, 9, 1]] and scores.tolist() == [7, 7, 2]
    perm = np.arange(9, -1, -1)                               # id i is the caller's 9 - i: the larger endpoint becomes the smaller
    pairs, scores = rt.ordered_rows(keys, vals, 6, perm)
    assert pairs.tolist() == [[9, 0, 8, 7, 6, 4], [0, 9, 4, 6, 7, 8]] and scores.tolist() == [7, 7, 2, 2, 2, 2]
    assert rt.ordered_rows(keys[:0], vals[:0], 4)[0].shape == (2, 0)


def test_rows_by_score_by_hand():
    keys_by_u = np.array([(1 << 32) | 5, (2 << 32) | 3, (0 << 32) | 9, (4 << 32) | 6], np.int64)      # u << 32 | v
    vals = np.array([2.0, 2.0, 7.0, 1.0], np.float32)
    cut, n_sel, pairs, scores, longest = rt.rows_by_score(keys_by_u, vals, 1.0, 2, 5)
    assert (float(cut), n_sel, longest) == (2.0, 3, 2)
    assert pairs.tolist() == [[9, 0, 5, 3, 2], [0, 9, 1, 2, 3]] and scores.tolist() == [7, 7, 2, 2, 2]
