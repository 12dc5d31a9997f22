"""CPU: the rank emulation and the host truths of tests/shard_emulation.py against cases worked out by hand, and the input
conditions that tests/test_gpu_shard_kernels.py relies on (empty score ranges, scores that sit on splitters), checked here on CPU
tensors through scan.score_splitters / score_range_counts so that the GPU tests cannot pass vacuously."""
import numpy as np
import pytest
import torch

import shard_emulation as se

NINF = float("-inf")


# ---- the all-to-all and the gathers ----------------------------------------------------------------------------------------------
def test_all_to_all_on_three_ranks_with_an_empty_piece():
    sends = [np.array([10, 11, 12, 13]), np.array([20, 21, 22]), np.array([30, 31, 99])]          # (rank 2 holds one element it does not send)
    counts = [[1, 2, 1], [0, 3, 0], [1, 0, 1]]                                                   # rank 1 sends ranks 0 and 2 nothing
    got = se.all_to_all(sends, counts)
    assert [g.tolist() for g in got] == [[10, 30], [11, 12, 20, 21, 22], [13, 31]]
    got = se.all_to_all([torch.from_numpy(s) for s in sends], counts)
    assert [g.tolist() for g in got] == [[10, 30], [11, 12, 20, 21, 22], [13, 31]]
    assert [g.tolist() for g in se.all_to_all([np.zeros(0)] * 2, [[0, 0], [0, 0]])] == [[], []]
    with pytest.raises(AssertionError):
        se.all_to_all([np.arange(2), np.arange(2)], [[1, 2], [1, 1]])


def test_exchange_runs_every_rank_twice_and_checks_the_receive_counts():
    sends = [torch.tensor([10, 11, 12, 13]), torch.tensor([20, 21, 22]), torch.tensor([30, 31])]
    counts = [[1, 2, 1], [0, 3, 0], [1, 0, 1]]
    ex = se.Exchange(3)
    seen = []

    def call(r, table=counts):
        seen.append(r)
        got = ex.all_to_all_ragged(sends[r], table[r], [table[q][r] for q in range(3)])
        return got.tolist()

    assert ex.run(call) == [[10, 30], [11, 12, 20, 21, 22], [13, 31]]
    assert seen == [0, 1, 2, 0, 1, 2]
    assert ex.serve(call) == [[10, 30], [11, 12, 20, 21, 22], [13, 31]]
    # a rank that expects something else than it is sent, and a rank that never exchanges
    with pytest.raises(AssertionError):
        ex.run(lambda r: ex.all_to_all_ragged(sends[r], counts[r], [1, 1, 1]))
    with pytest.raises(AssertionError):
        ex.run(lambda r: None)


def test_gathers_return_the_own_chunk_then_the_concatenation():
    g = se.Gathers(3)
    data = [torch.tensor([1, 2, 3]), torch.tensor([7]), torch.tensor([4, 5])]
    lens = [2, 0, 2]
    for r in range(3):
        g.start(r)
        assert g.gather_ragged(data[r], lens).tolist() == data[r][:lens[r]].tolist()
        assert g.gather_ragged_to(data[r] * 10, lens, 1).tolist() == (data[r][:lens[r]] * 10).tolist()
    g.assembled = True
    for r in range(3):
        g.start(r)
        assert g.gather_ragged(data[r], lens).tolist() == [1, 2, 4, 5]
        assert g.gather_ragged_to(data[r] * 10, lens, 1).tolist() == [10, 20, 40, 50]


# ---- the job-wide k-th -----------------------------------------------------------------------------------------------------------
def test_union_kth_by_hand():
    above = np.nextafter(np.float32(1.0), np.float32(2.0), dtype=np.float32)
    xs = [np.array([1.0, NINF, -0.0, 3.0], np.float32), np.zeros(0, np.float32), np.array([NINF, NINF], np.float32),
          np.array([0.0, 1.0, above, -2.0, 1.0], np.float32)]
    # live, descending: 3, 1 + 2^-23, 1, 1, 1, (-0, 0), -2  -- eight values; the three -inf are no values
    want = {0: NINF, 1: 3.0, 2: above, 3: 1.0, 4: 1.0, 5: 1.0, 6: 0.0, 7: 0.0, 8: -2.0, 9: NINF, 100: NINF}
    for k, w in want.items():
        assert se.same_value(se.union_kth(xs, k), w), k
    assert se.same_value(-0.0, 0.0) and not se.same_value(1.0, above)
    assert se.union_kth([], 1) == NINF and se.union_kth(xs[1:3], 1) == NINF
    assert se.union_kth([np.array([np.inf, 5.0], np.float32)], 1) == np.inf
    h = se.top_byte_hist(xs)
    # top bytes of the ordered patterns: 3.0 -> 0xC0, 1.0 and 1 + 2^-23 -> 0xBF, the zeros -> 0x80, -2.0 -> 0x3F
    assert h.sum() == 8 and (h[0xC0], h[0xBF], h[0x80], h[0x3F]) == (1, 4, 2, 1)


# ---- the range compaction --------------------------------------------------------------------------------------------------------
def test_between_by_hand():
    keys = np.array([4, -1, 9, 1 << 40, 7, 2, -1], np.int64)
    vals = np.array([1.0, 7.0, 0.25, NINF, -0.0, 7.0, NINF], np.float32)
    live = [0, 2, 3, 4, 5]

    def kept(lo, hi):
        return np.flatnonzero(se.between(keys, vals, lo, hi)).tolist()

    assert kept(None, None) == live and kept(NINF, None) == live and kept(NINF, np.inf) == live
    assert kept(None, NINF) == [] and kept(np.inf, None) == []
    assert kept(0.25, 1.0) == [2]                      # the lower end is inclusive, the upper one is not
    assert kept(0.25, 7.0) == [0, 2] and kept(1.0, None) == [0, 5] and kept(None, 0.25) == [3, 4]
    assert kept(0.0, 0.25) == [4] and kept(-0.0, 0.25) == [4]          # the zeros are one value
    assert kept(1.0, 1.0) == [] and kept(7.0, 7.0) == [] and kept(7.0, 1.0) == []
    assert kept(7.0, np.inf) == [5]                    # the dead slot with the stale 7.0 stays out
    pb = se.pair_bits(keys[live], vals[live])
    assert pb[:, 0].tolist() == [2, 4, 7, 9, 1 << 40] and pb[2, 1] == 0x80000000 and pb[4, 1] == 0xFF800000


# ---- the inputs of the ordered-rows test -----------------------------------------------------------------------------------------
def splitter_facts(vals: torch.Tensor, world: int):
    """(empty ranges, scores equal to a splitter, equal neighbouring splitters) under scan.score_splitters."""
    from eps_amd import scan
    sp = scan.score_splitters(vals, world)
    counts = scan.score_range_counts(vals, sp)
    assert sp.numel() == world - 1 and int(counts.sum()) == vals.numel() and bool((sp[:-1] >= sp[1:]).all())
    on = int((vals.unsqueeze(1) == sp.unsqueeze(0)).any(1).sum())
    return int((counts == 0).sum()), on, int((sp[:-1] == sp[1:]).sum())


def test_three_levels_at_world_8_leave_ranges_empty():
    """3 levels under 7 splitters: the splitters are 1.25, 1.25, 1.125, 1.125, 1.125, 1, 1, so the ranges [1.25, 1.25),
    [1.125, 1.125) twice, [1, 1) and (-inf, 1) are empty -- 5 of 8 -- and every score equals a splitter."""
    vals = torch.from_numpy(se.level_scores(3))
    assert sorted(set(vals.tolist())) == [1.0, 1.125, 1.25]
    empty, on, equal = splitter_facts(vals, 8)
    assert (empty, on, equal) == (5, 40_000, 4)


def test_41_levels_fill_every_range_with_scores_on_the_splitters():
    """41 levels: no range is empty at world 2, 3 or 8, and the scores of a splitter's level sit exactly on it (965, 1 905 and 6 889
    of these 40 000): the inclusive lower end and the exclusive upper end of a range both decide rows."""
    vals = torch.from_numpy(se.level_scores(41))
    assert len(set(vals.tolist())) == 41
    for world in (2, 3, 8):
        empty, on, equal = splitter_facts(vals, world)
        assert (empty, equal) == (0, 0) and 40_000 // 41 // 2 < on < 40_000, world
