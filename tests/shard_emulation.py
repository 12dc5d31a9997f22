"""The ranks of a sharded filter step as a loop in ONE process, and the host truths of the device code that only a job of several
ranks reaches (tests/test_shard_emulation_host.py holds this file on the CPU, tests/test_gpu_shard_kernels.py uses it):

  all_to_all / Exchange   the one all-to-all of scan._deal_rows, defined directly: rank q receives, in rank order, slice q of every
                          rank's send buffer.  A function that calls dist.all_to_all_ragged once runs twice per rank: the first pass
                          records what every rank sends (and stops the call there), the second hands every rank what it receives
  Gathers                 stand-ins for dist.gather_ragged / gather_ragged_to: the caller's own chunk (the test concatenates the
                          chunks in rank order itself) or, once every rank's chunk is on record, their concatenation
  union_kth               the job-wide k-th largest (eps_kth_begin / eps_kth_hist_f32 / eps_kth_pick; ops.kth_largest_dist)
  between                 the range compaction (eps_compact_between; sel_cut_kernel)

The ordered rows come from rows_by_score_truth.ordered_rows / cut_and_count."""
import numpy as np

KTH_WORDS = 260                     # int32 words of the select's state: prefix, mask, k (two words), hist[256] (csrc/topk_keys.hip)
KTH_HIST = slice(4, 260)            # ... and where its histogram lies: what the ranks sum per round


def _cat(parts):
    if isinstance(parts[0], np.ndarray):
        return np.concatenate(parts)
    import torch
    return torch.cat(parts)


def all_to_all(sends, send_counts):
    """sends[r] = rank r's send buffer, cut into pieces of send_counts[r][q] elements for rank q = 0, 1, ... (elements beyond the last
    piece are not sent) -> one receive buffer per rank: rank q gets, in rank order, piece q of every rank."""
    world = len(sends)
    assert len(send_counts) == world and all(len(c) == world for c in send_counts)
    offs = [np.concatenate([[0], np.cumsum(c)]).astype(np.int64) for c in send_counts]
    assert all(int(offs[r][-1]) <= len(sends[r]) for r in range(world)), "a rank sends more than it holds"
    return [_cat([sends[r][int(offs[r][q]):int(offs[r][q + 1])] for r in range(world)]) for q in range(world)]


class _Recorded(Exception):
    """Ends a rank's call in the recording pass of an Exchange."""


class Exchange:
    """Stand-in for dist.all_to_all_ragged under a loop over the ranks: ``run(call)`` runs ``call(rank)`` for every rank twice and
    returns the results of the second pass.  Every call must reach the all-to-all exactly once."""

    def __init__(self, world: int):
        self.world, self.rank, self.serving = world, None, False
        self.sends, self.send_counts, self.recv_counts = {}, {}, {}

    def all_to_all_ragged(self, t, send_counts, recv_counts):
        r = self.rank
        if not self.serving:
            assert r not in self.sends, "one all-to-all per call"
            self.sends[r], self.send_counts[r], self.recv_counts[r] = t, [int(x) for x in send_counts], [int(x) for x in recv_counts]
            raise _Recorded()
        assert [int(x) for x in send_counts] == self.send_counts[r] and t.shape == self.sends[r].shape and bool((t == self.sends[r]).all()), \
            "a rank sends something else the second time"
        world = self.world
        got = all_to_all([self.sends[q] for q in range(world)], [self.send_counts[q] for q in range(world)])[r]
        # what the rank expects from everybody (its column of the deal table) is what everybody sends it
        assert [int(x) for x in recv_counts] == [self.send_counts[q][r] for q in range(world)], (r, list(recv_counts))
        assert len(got) == sum(int(x) for x in recv_counts)
        self.served += 1
        return got

    def run(self, call):
        self.serving = False
        self.sends.clear(), self.send_counts.clear(), self.recv_counts.clear()
        for r in range(self.world):
            self.rank = r
            try:
                call(r)
            except _Recorded:
                continue
            raise AssertionError(f"rank {r} finished without an all-to-all")
        return self.serve(call)

    def serve(self, call):
        """One more pass over the ranks on the buffers that ``run`` recorded."""
        self.serving, out = True, []
        for r in range(self.world):
            self.rank, self.served = r, 0
            out.append(call(r))
            assert self.served == 1, f"rank {r}: {self.served} all-to-alls"
        return out


class Gathers:
    """Stand-ins for dist.gather_ragged / gather_ragged_to.  The test sets ``rank`` before it calls a rank's function.  While
    ``assembled`` is False a call returns the caller's own chunk -- its first lens[rank] elements -- and keeps it; once every rank
    has been through, ``assembled = True`` makes the i-th call of every rank return the ranks' i-th chunks in rank order."""

    def __init__(self, world: int):
        self.world, self.rank, self.assembled = world, None, False
        self.chunks = [[] for _ in range(world)]          # [rank][call] = chunk
        self.calls = [0] * world

    def start(self, rank: int):
        self.rank = rank
        self.calls[rank] = 0
        if not self.assembled:
            self.chunks[rank] = []

    def gather_ragged(self, t, lens):
        r = self.rank
        assert len(lens) == self.world and len(t) >= int(lens[r]), (r, len(t), list(lens))
        own = t[:int(lens[r])]
        i = self.calls[r]
        self.calls[r] += 1
        if not self.assembled:
            self.chunks[r].append(own)
            return own
        assert all(len(self.chunks[q][i]) == int(lens[q]) for q in range(self.world)), "the ranks disagree on the lengths"
        assert bool((own == self.chunks[r][i]).all()), "a rank contributes something else the second time"
        return _cat([self.chunks[q][i] for q in range(self.world)])

    def gather_ragged_to(self, t, lens, dst):
        assert 0 <= int(dst) < self.world
        return self.gather_ragged(t, lens)

    def install(self, monkeypatch, dist_module):
        monkeypatch.setattr(dist_module, "gather_ragged", self.gather_ragged)
        monkeypatch.setattr(dist_module, "gather_ragged_to", self.gather_ragged_to)


def union_kth(xs, k: int) -> np.float32:
    """The k-th largest, by value (-0.0 == 0.0), of the live values of every rank -- those above -inf; -inf when k == 0 or fewer
    than k values are live."""
    live = np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in xs] + [np.zeros(0, np.float32)])
    live = live[live > -np.inf]
    if k == 0 or live.size < k:
        return np.float32(-np.inf)
    return np.sort(live)[::-1][k - 1]


def same_value(a, b) -> bool:
    """Equal as float32 values: equal bits but for the two zeros (no NaN comes near these tests)."""
    return bool(np.float32(a) == np.float32(b))


def top_byte_hist(xs) -> np.ndarray:
    """int64[256]: the job-wide histogram of the select's first round -- the top byte of the order-preserving pattern of every live
    value (-0 counts as +0)."""
    live = np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in xs] + [np.zeros(0, np.float32)])
    b = (live[live > -np.inf] + np.float32(0.0)).view(np.uint32)
    o = np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)
    return np.bincount(o >> 24, minlength=256).astype(np.int64)


def between(keys, vals, lo, hi) -> np.ndarray:
    """Mask of the entries a range compaction keeps: a key (>= 0) whose score lies in [lo, hi); None: that end is open."""
    keys, vals = np.asarray(keys, np.int64), np.asarray(vals, np.float32)
    m = keys >= 0
    if lo is not None:
        m = m & (vals >= np.float32(lo))
    if hi is not None:
        m = m & (vals < np.float32(hi))
    return m


def pair_bits(keys, vals) -> np.ndarray:
    """A list of (key, score) as a sorted [n, 2] int64 array of (key, score bits): equal arrays = equal multisets."""
    keys = np.asarray(keys, np.int64).reshape(-1)
    bits = np.ascontiguousarray(np.asarray(vals, np.float32).reshape(-1)).view(np.uint32).astype(np.int64)
    o = np.lexsort((bits, keys))
    return np.stack([keys[o], bits[o]], 1)


def level_scores(levels: int, n: int = 40_000, seed: int = 11) -> np.ndarray:
    """n scores of ``levels`` tied levels 1, 1 + 1/8, ... (exact in float32), drawn evenly."""
    import torch
    return (torch.randint(0, levels, (n,), generator=torch.Generator().manual_seed(seed)).to(torch.float32) / 8 + 1).numpy()


def pair_keys(m: int, n_nodes: int, rng) -> np.ndarray:
    """m distinct pairs u < v over ids below n_nodes, as keys v << 32 | u in random order."""
    keys = np.zeros(0, np.int64)
    while keys.size < m:
        a, b = rng.integers(0, n_nodes, 2 * m + 8), rng.integers(0, n_nodes, 2 * m + 8)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        keys = np.unique(np.concatenate([keys, ((hi << 32) | lo)[lo < hi]]))
    return rng.permutation(keys)[:m]
