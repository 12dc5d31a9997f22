"""GPU: the device code that only a job of several ranks reaches, with the ranks as a loop in ONE process on one device, against the
host truths of tests/shard_emulation.py and tests/rows_by_score_truth.py -- integer and bit-exact work, so every comparison is equality:

  a. eps_compact_between and the kernel it shares with eps_compact_at_least / eps_compact_survivors (sel_cut_kernel,
     csrc/topk_select.hip): both ends of the range, the 1024-entry chunk edges, a second trip of its grid-stride loop
  b. eps_kth_begin / eps_kth_hist_f32 / eps_kth_pick (csrc/topk_keys.hip), the job-wide k-th: on the raw ABI in lockstep, one state
     per rank, and through ops.kth_largest_dist
  c. scan._ordered_rows_distributed, rank by rank: range compaction, the ordering under a relabelling, concatenation in rank order
  d. scan._deal_rows from the plan that eps_score_hist_into + eps_score_deal_plan make: the all-to-all, the ordering, the shards

No process group, no child process, no thread: eps_amd.dist's collectives are replaced by stand-ins that serve a loop over the ranks."""
import ctypes

import numpy as np
import pytest
import torch

import rows_by_score_truth as rt
import shard_emulation as se

pytestmark = pytest.mark.gpu

NINF, INF = float("-inf"), float("inf")
ABOVE_1 = np.float32(1.0 + 2.0 ** -23)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).reshape(-1).view(np.uint32)


def _f32(dev, x):
    return None if x is None else torch.tensor([x], dtype=torch.float32, device=dev)


# ---- a. the range compaction and the shared cut kernel ---------------------------------------------------------------------------
LEVELS = np.array([-2.5, -0.0, 0.0, 0.25, 1.0, ABOVE_1, 7.0], np.float32)
ENDS = [None, NINF] + [float(x) for x in LEVELS] + [INF]
END_NAMES = ["None", "-inf", "-2.5", "-0", "+0", "0.25", "1", "1+ulp", "7", "+inf"]


def _cut_list(n):
    """n slots like a survivor list's: distinct keys, some beyond 32 bits; a third dead (key -1, score -inf), one of them with a
    stale score of the highest level; one live key that scores -inf; the rest scores one of LEVELS."""
    rng = np.random.default_rng(n)
    keys = rng.permutation(n).astype(np.int64) + (np.int64(1) << 33) * (np.arange(n) % 3 == 1)
    vals = LEVELS[rng.integers(0, len(LEVELS), n)]
    dead = rng.random(n) < 1 / 3
    keys[dead], vals[dead] = -1, -np.inf
    if n >= 63:
        keys[5], vals[5] = -1, 7.0
        keys[6], vals[6] = n + 10, -np.inf
        keys[7], vals[7] = n + 11, 7.0
    return keys, vals


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 100_003))
def test_compact_between(eps, dev, n):
    """Every pair of ends (lo, hi) from None, -inf, each level and +inf -- lo == hi and lo > hi among them: the count is int64 and
    the truth's, and the stored (key, score bits) are the truth's multiset.  A wave of the kernel takes 1024 consecutive entries:
    the sizes sit on both sides of one and of four such chunks."""
    keys, vals = _cut_list(n)
    d_keys, d_vals = torch.from_numpy(keys).to(dev), torch.from_numpy(vals).to(dev)
    o = np.argsort(keys, kind="stable")                    # (live keys are distinct: a selection in key order is its multiset)
    keys_s, vals_s = keys[o], vals[o]
    d_ends = [_f32(dev, e) for e in ENDS]
    n_live = int((keys >= 0).sum())
    sizes = {}
    for i, lo in enumerate(ENDS):
        for j, hi in enumerate(ENDS):
            case = (n, END_NAMES[i], END_NAMES[j])
            out_k, out_v, n_out = eps.ops.compact_between(d_keys, d_vals, d_ends[i], d_ends[j])
            keep = se.between(keys_s, vals_s, lo, hi)
            m = int(n_out)
            assert n_out.dtype == torch.int64 and n_out.shape == (1,) and m == int(keep.sum()), case
            got_k, got_v = out_k[:m].cpu().numpy(), out_v[:m].cpu().numpy()
            g = np.argsort(got_k, kind="stable")
            assert np.array_equal(got_k[g], keys_s[keep]), case
            assert np.array_equal(_bits(got_v[g]), _bits(vals_s[keep])), case
            sizes[(i, j)] = m
    # the cases are what they are meant to be: open ends keep every live key, the one scoring -inf included; a closed lower end
    # drops it; equal ends and crossed ends keep nothing; one level alone is cut out by [level, next level)
    assert sizes[(0, 0)] == sizes[(1, 0)] == sizes[(1, 9)] == n_live
    assert all(sizes[(i, i)] == 0 for i in range(1, len(ENDS))) and sizes[(8, 4)] == 0 and sizes[(0, 1)] == 0
    if n >= 63:
        assert sizes[(2, 0)] == n_live - 1 and sizes[(0, 2)] == 1                       # the live key that scores -inf
        assert sizes[(8, 9)] == sizes[(8, 0)] == int(((keys >= 0) & (vals == 7.0)).sum()) >= 1
        assert int((keys < 0).sum()) > n // 5 and keys.max() >= 1 << 33
    if n >= 1023:
        assert sizes[(6, 7)] == int(((keys >= 0) & (vals == 1.0)).sum()) > 0          # [1, 1 + ulp): the inclusive and the exclusive end
        assert sizes[(3, 5)] == int(((keys >= 0) & (vals == 0.0)).sum()) > 0          # both zeros, from either zero
        assert sizes[(3, 5)] == sizes[(4, 5)] and sizes[(3, 4)] == 0
        assert 0 < sizes[(5, 8)] < n_live


def test_cut_kernel_second_grid_stride_trip(eps, dev):
    """The grid of sel_cut_kernel is capped at 8 workgroups per CU, four waves each, 1024 entries per wave and trip: a list of
    32768 x CUs + 1025 entries sends the first waves round again -- for a whole chunk and a chunk of one entry.  The three entries
    that launch the kernel, each against the same mask in tensor ops."""
    ops = eps.ops
    first = 32768 * ops.device_info()[0]
    n = first + 1025
    i = torch.arange(n, dtype=torch.int64, device=dev)
    keys = torch.where(i % 3 == 1, torch.full_like(i, -1), i)                           # (keys = positions: vals[key] is a key's score)
    levels = torch.tensor([0.25, 1.0, float(ABOVE_1), 7.0], dtype=torch.float32, device=dev)
    vals = levels[(i + i // 1021) % 4]
    live = keys >= 0

    def check(out_k, out_v, m, keep, what):
        assert m == int(keep.sum()), what
        # the second trip both keeps and drops, in its whole chunk and in its last entry's chunk
        assert bool(keep[first:first + 1024].any()) and bool((~keep[first:first + 1024]).any()) and bool(keep[first + 1024:].any()), what
        sk, o = torch.sort(out_k[:m])
        assert torch.equal(sk, i[keep]), what
        assert torch.equal(out_v[:m][o].view(torch.int32), vals[keep].view(torch.int32)), what

    out_k, out_v, n_out = ops.compact_at_least(keys, vals, _f32(dev, 1.0))
    check(out_k, out_v, int(n_out), live & (vals >= 1.0), "compact_at_least")
    del out_k, out_v
    out_k, out_v, n_out = ops.compact_between(keys, vals, _f32(dev, 1.0), _f32(dev, 7.0))
    assert n_out.dtype == torch.int64
    check(out_k, out_v, int(n_out), live & (vals >= 1.0) & (vals < 7.0), "compact_between")
    del out_k, out_v
    res = ops.Survivors(n, 0.0, dev)
    res.key.copy_(keys)
    res.val.copy_(vals)
    out_k, out_v = res.valid(n)
    check(out_k, out_v, out_k.numel(), live, "Survivors.valid")


# ---- b. the job-wide k-th --------------------------------------------------------------------------------------------------------
def _rank_vectors():
    rng = np.random.default_rng(23)
    lv = np.array([-np.inf, -3.5, -1.0, -0.0, 0.0, 0.25, 1.0, ABOVE_1, 7.0, np.inf], np.float32)
    return {
        "mixed": lv[rng.integers(0, len(lv), 100_003)],            # heavy ties, negatives, both zeros, +inf, dead slots, 1 and 1 + ulp
        "empty": np.zeros(0, np.float32),
        "dead": np.full(65, -np.inf, np.float32),                  # a rank whose every slot is "no value"
        "const": np.full(4097, 0.25, np.float32),                  # one constant: every wave adds its count once
        "one": np.array([ABOVE_1], np.float32),
        "normal": rng.standard_normal(63).astype(np.float32),
        "zeros": np.tile(np.array([0.0, -0.0, -1.0, 1.0], np.float32), 16),
        "last_bit": np.concatenate([np.full(32, 1.0, np.float32), np.full(32, ABOVE_1, np.float32), np.float32([np.inf])]),
    }


VECTORS = _rank_vectors()
LAYOUTS = {                      # name -> the ranks' vectors, in rank order
    "w1_mixed": ["mixed"], "w1_empty": ["empty"], "w1_dead": ["dead"], "w1_const": ["const"],
    "w2_empty_first": ["empty", "mixed"], "w2_dead_const": ["dead", "const"],
    "w3_mixed": ["mixed", "empty", "dead"], "w3_short": ["normal", "zeros", "one"],
    "w8": ["normal", "empty", "mixed", "dead", "one", "const", "zeros", "last_bit"],
}
SHIFTS = (24, 16, 8, 0)


def _layout(dev, name):
    xs = [VECTORS[v] for v in LAYOUTS[name]]
    n_live = int(sum((x > -np.inf).sum() for x in xs))
    ks = sorted({0, 1, 2, n_live // 3 + 1, n_live, n_live + 1})
    return xs, [torch.from_numpy(x).to(dev) for x in xs], n_live, ks


def test_kth_layouts_are_what_they_are_meant_to_be():
    """(no device needed, but it belongs to the cases below) world 1, 2, 3 and 8; lengths 0, 1, 63, 64, 65, 4097 and 100 003; in the
    layouts of 3 and 8 ranks a rank without slots and a rank without values; ties, both zeros, +inf and a last-bit pair in the union."""
    assert sorted({len(v) for v in LAYOUTS.values()}) == [1, 2, 3, 8]
    assert sorted({len(x) for x in VECTORS.values()}) == [0, 1, 63, 64, 65, 4097, 100_003]
    for name in ("w3_mixed", "w8"):
        xs = [VECTORS[v] for v in LAYOUTS[name]]
        assert any(x.size == 0 for x in xs) and any(x.size and (x == -np.inf).all() for x in xs)
    m = VECTORS["mixed"]
    assert (m == -np.inf).sum() > 5000 and (m == np.inf).sum() > 5000 and (_bits(m) == 0x80000000).sum() > 5000 and (_bits(m) == 0).sum() > 5000
    assert (m == 1.0).sum() > 5000 and (m == ABOVE_1).sum() > 5000 and int(_bits(ABOVE_1)[0]) - int(_bits(1.0)[0]) == 1


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_kth_rounds_in_lockstep_on_the_raw_abi(eps, dev, name):
    """One state per rank.  Per round: every rank's histogram launch, the sum of the 256 counters over the ranks written back into
    every state (what dist.all_reduce_sum_ does), every rank's pick.  After every round the ranks hold the same prefix / mask / k
    and a cleared histogram; the first round's summed histogram is the union's; the last round's result is the union's k-th."""
    ops = eps.ops
    xs, d_xs, n_live, ks = _layout(dev, name)
    world = len(xs)
    assert int(eps.load().eps_kth_largest_workspace_bytes()) == 4 * se.KTH_WORDS
    want_hist = se.top_byte_hist(xs)
    assert int(want_hist.sum()) == n_live
    for k in ks:
        states = [torch.full((se.KTH_WORDS,), -1, dtype=torch.int32, device=dev) for _ in range(world)]       # (begin clears them)
        outs = [torch.full((1,), 123.0, dtype=torch.float32, device=dev) for _ in range(world)]
        for st in states:
            ops._call("eps_kth_begin", dev, st, k)
        begun = torch.stack(states).cpu().numpy()
        assert (begun[:, [0, 1, 3]] == 0).all() and (begun[:, 2] == k).all() and not begun[:, se.KTH_HIST].any(), (name, k)
        for shift in SHIFTS:
            for x, st in zip(d_xs, states):
                ops._call("eps_kth_hist_f32", dev, x, x.numel(), st, shift)
            total = torch.stack([st[se.KTH_HIST] for st in states]).sum(0)
            if shift == 24:
                assert np.array_equal(total.cpu().numpy(), want_hist), (name, k)
            for st in states:
                st[se.KTH_HIST] = total.to(torch.int32)
            for st, out in zip(states, outs):
                ops._call("eps_kth_pick", dev, st, shift, out)
            words = torch.stack(states).cpu().numpy()
            assert (words[:, :4] == words[0, :4]).all(), (name, k, shift, words[:, :4])
            assert not words[:, se.KTH_HIST].any(), (name, k, shift)
        want = se.union_kth(xs, k)
        got = torch.cat(outs).cpu().numpy()
        assert all(se.same_value(g, want) for g in got), (name, k, got, want)
        assert (int(words[0, 0]) & 0xFFFFFFFF, int(words[0, 1])) == (rt.ordered(want), -1), (name, k)
        if k in (0, n_live + 1):
            assert want == -np.inf


class _ReduceFromOtherRanks:
    """Stand-in for dist.all_reduce_sum_ under ops.kth_largest_dist on rank r: adds the other ranks' histograms to the caller's by
    launching eps_kth_hist_f32 on their vectors into the caller's state -- which it finds 16 bytes in front of the slice it is
    handed; the round is its call count."""

    def __init__(self, ops, dev, others, state_bytes):
        self.ops, self.dev, self.others, self.state_bytes, self.calls = ops, dev, others, state_bytes, 0

    def __call__(self, t):
        assert t.dtype == torch.int32 and t.shape == (256,) and t.is_contiguous() and t.storage_offset() == 4
        assert t.untyped_storage().nbytes() == self.state_bytes
        shift = SHIFTS[self.calls]
        self.calls += 1
        state = ctypes.c_void_p(t.data_ptr() - 16)
        for x in self.others:
            self.ops._call("eps_kth_hist_f32", self.dev, x, x.numel(), state, shift)
        return t


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_kth_largest_dist_on_every_rank(eps, dev, name, monkeypatch):
    """ops.kth_largest_dist(x_r, k, world) for every rank r: the same value on all of them, the union's k-th."""
    from eps_amd import dist as epd
    ops = eps.ops
    xs, d_xs, n_live, ks = _layout(dev, name)
    world = len(xs)
    assert not epd.FORCE_COLLECTIVES
    state_bytes = int(eps.load().eps_kth_largest_workspace_bytes())
    outs = []
    for k in ks:
        for r in range(world):
            red = _ReduceFromOtherRanks(ops, dev, [x for q, x in enumerate(d_xs) if q != r], state_bytes)
            monkeypatch.setattr(epd, "all_reduce_sum_", red)
            out = ops.kth_largest_dist(d_xs[r], k, world)
            assert out.shape == (1,) and out.dtype == torch.float32 and red.calls == (4 if world > 1 else 0), (name, k, r)
            outs.append(out)
    got = torch.cat(outs).cpu().numpy().reshape(len(ks), world)
    for k, row in zip(ks, got):
        want = se.union_kth(xs, k)
        assert all(se.same_value(g, want) for g in row), (name, k, row, want)


# ---- c. the final ordering dealt by score range over gathered pairs --------------------------------------------------------------
N_NODES, N_PAIRS = 5000, 40_000
ID_BITS = (N_NODES - 1).bit_length()


def _score_set(kind, m, rng):
    if kind == "tied3":
        return se.level_scores(3, m)
    if kind == "levels41":
        return se.level_scores(41, m)
    assert kind == "distinct"
    return (1 + rng.permutation(m) / 64).astype(np.float32)


def _as_pairs(rows_k):
    return torch.stack([rows_k & 0xFFFFFFFF, rows_k >> 32]).cpu().numpy()


def _same_rows(rows_k, rows_v, want_pairs, want_scores):
    return (rows_k.numel() == want_pairs.shape[1] and np.array_equal(_as_pairs(rows_k), want_pairs)
            and np.array_equal(_bits(rows_v.cpu().numpy()), _bits(want_scores)))


@pytest.mark.parametrize("kind,world", [("tied3", 8), ("levels41", 2), ("levels41", 3), ("levels41", 8), ("distinct", 3)])
def test_ordered_rows_distributed_rank_by_rank(eps, dev, kind, world, monkeypatch):
    """Every rank holds the same selected pairs; rank r compacts score range r, orders its rows (as labelled and under a random
    relabelling) and the chunks concatenate in rank order to the declared order of all rows, scores included.  "tied3": 3 levels
    under 7 splitters -- empty ranges between equal splitters; "levels41": every splitter has scores sitting on it."""
    from eps_amd import dist as epd, scan
    rng = np.random.default_rng(world * 7 + len(kind))
    m = N_PAIRS
    keys, vals = se.pair_keys(m, N_NODES, rng), _score_set(kind, m, rng)
    t_keys, t_vals = torch.from_numpy(keys).to(dev), torch.from_numpy(vals).to(dev)
    sp = scan.score_splitters(t_vals, world).cpu().numpy()
    assert sp.shape == (world - 1,) and (sp[:-1] >= sp[1:]).all()
    ends = [(sp[r] if r < world - 1 else None, sp[r - 1] if r > 0 else None) for r in range(world)]
    counts = [int(se.between(keys, vals, lo, hi).sum()) for lo, hi in ends]
    assert sum(counts) == m
    on_splitters = int(np.isin(vals, sp).sum())
    if kind == "tied3":
        assert counts.count(0) >= 1 and int((sp[:-1] == sp[1:]).sum()) >= 1 and on_splitters == m
    elif kind == "levels41":
        assert 0 not in counts and 0 < on_splitters < m
    else:
        assert 0 not in counts and np.unique(vals).size == m
    gathers = se.Gathers(world)
    gathers.install(monkeypatch, epd)
    for perm in (None, rng.permutation(N_NODES).astype(np.int64)):
        t_perm = None if perm is None else torch.from_numpy(perm).to(dev)
        case = (kind, world, perm is not None)
        want_pairs, want_scores = rt.ordered_rows(keys, vals, 2 * m, perm)
        gathers.assembled = False
        chunks = []
        for r in range(world):
            gathers.start(r)
            rk, rv = scan._ordered_rows_distributed(t_keys, t_vals, 2 * m, ID_BITS, t_perm, r, world)
            assert rk.numel() == rv.numel() == 2 * counts[r] and gathers.calls[r] == 2, (case, r)
            chunks.append((rk, rv))
        all_k, all_v = torch.cat([c[0] for c in chunks]), torch.cat([c[1] for c in chunks])
        assert _same_rows(all_k, all_v, want_pairs, want_scores), case
        # cut at k: the concatenation's first k rows; and the function's own cut of the gathered rows, on every rank and on one
        gathers.assembled = True
        for k in (1, m, 2 * m - 5):
            first_pairs, first_scores = rt.ordered_rows(keys, vals, k, perm)
            assert first_pairs.shape == (2, k) and _same_rows(all_k[:k], all_v[:k], first_pairs, first_scores), (case, k)
            for r, rows_on in [(r, None) for r in range(world)] + [(world - 1, world - 1)]:
                gathers.start(r)
                rk, rv = scan._ordered_rows_distributed(t_keys, t_vals, k, ID_BITS, t_perm, r, world, rows_on)
                assert _same_rows(rk, rv, first_pairs, first_scores), (case, k, r, rows_on)


# ---- d. the final ordering dealt by one all-to-all of every rank's own pairs -----------------------------------------------------
DEAL_BAR = np.float32(1.75)


def _own_lists(world, n, rng):
    """Per rank its own scored pairs (disjoint over the ranks; rank r holds n // (r + 1)), every score above the bar; odd ranks score
    in tied levels of 1 / 8; one slot in twenty is dropped (key -1, score -inf)."""
    sizes = [n // (r + 1) for r in range(world)]
    pool = se.pair_keys(sum(sizes), N_NODES, rng)
    lists, at = [], 0
    for r, m in enumerate(sizes):
        keys = pool[at:at + m].copy()
        at += m
        vals = (DEAL_BAR + np.float32(2.0 ** -10) + rng.exponential(1.5, m)).astype(np.float32)
        if r % 2:
            vals = (np.floor(vals * 8) / 8 + 0.125).astype(np.float32)
        dead = rng.random(m) < 0.05
        keys[dead], vals[dead] = -1, -np.inf
        lists.append((keys, vals))
    return lists


@pytest.mark.parametrize("world", [2, 3, 8])
def test_deal_rows_from_the_real_plan(eps, dev, world, monkeypatch):
    """Every rank holds its own pairs.  The plan: eps_score_hist_into per rank into one table, eps_score_deal_plan on it; the
    selection: eps_compact_at_least at the plan's cut.  Then scan._deal_rows on every rank through the all-to-all stand-in: the
    shards in rank order (rows_on = "shards"), and the rows gathered onto every rank (rows_on = None), are the first k rows of the
    declared order of the pairs that the truth selects -- for a k that ends inside the first range, inside a middle one, and
    beyond the last row."""
    from eps_amd import dist as epd, scan
    ops = eps.ops
    rng = np.random.default_rng(100 + world)
    lists = _own_lists(world, 6000, rng)
    d_lists = [(torch.from_numpy(k).to(dev), torch.from_numpy(v).to(dev)) for k, v in lists]
    all_keys, all_vals = np.concatenate([k for k, _ in lists]), np.concatenate([v for _, v in lists])
    n_live = int((all_vals > -np.inf).sum())
    assert (all_vals[all_vals > -np.inf] > DEAL_BAR).all() and ((all_keys >= 0) == (all_vals > -np.inf)).all()
    assert 0 < n_live < all_vals.size and len({k.size for k, _ in lists}) == world
    k2 = n_live // 3
    # the plan, as _cut_from_histograms makes it
    base = torch.tensor([DEAL_BAR], dtype=torch.float32, device=dev)
    bins = ops.score_bins()
    hists = torch.zeros((world, 16 + bins), dtype=torch.int32, device=dev)
    for r, (d_k, d_v) in enumerate(d_lists):
        ops.score_hist_into(d_k, d_v, None, base, hists[r, 16:], above=base)
    cut, sp, counts, nsel = ops.score_deal_plan(hists[:, 16:], k2, base)
    c, nsel_r = counts.tolist(), nsel.tolist()
    # the truth's selection (the cut itself is held by test_deal_plan_from_gathered_histograms) and the ranges' rows
    _, n_sel, sel = rt.cut_and_count(all_vals, DEAL_BAR, k2)
    assert sum(nsel_r) == n_sel and k2 <= n_sel < n_live
    sp_h = sp.cpu().numpy()
    lens = (2 * np.bincount((all_vals[sel][:, None] < sp_h[None, :]).sum(1), minlength=world)).tolist()
    assert [2 * sum(c[r][q] for r in range(world)) for q in range(world)] == lens
    own = []
    for r, (d_k, d_v) in enumerate(d_lists):
        s_k, s_v, n_out = ops.compact_at_least(d_k, d_v, cut)
        assert int(n_out) == nsel_r[r]
        own.append((s_k[:nsel_r[r]].contiguous(), s_v[:nsel_r[r]].contiguous()))
    # k: inside the first range, inside a middle (for two ranks: the last) range, beyond all rows
    mid = min(range(1, world), key=lambda q: (lens[q] < 4, abs(q - world // 2)))
    assert lens[0] > 3 and lens[mid] >= 4 and sum(lens) == 2 * n_sel
    ks = [lens[0] - 3, sum(lens[:mid]) + lens[mid] // 2 + 1, sum(lens) + 5]
    exchange, gathers = se.Exchange(world), se.Gathers(world)
    monkeypatch.setattr(epd, "all_to_all_ragged", exchange.all_to_all_ragged)
    gathers.install(monkeypatch, epd)
    for perm in (None, rng.permutation(N_NODES).astype(np.int64)):
        t_perm = None if perm is None else torch.from_numpy(perm).to(dev)
        want_pairs, want_scores = rt.ordered_rows(all_keys[sel], all_vals[sel], 2 * n_sel, perm)
        cut_shards = 0
        for k in ks:
            case = (world, perm is not None, k)
            take = min(k, 2 * n_sel)

            def rank_call(r, rows_on):
                gathers.start(r)
                return scan._deal_rows(own[r][0], own[r][1], sp, c, k, ID_BITS, t_perm, r, world, rows_on)

            shards = exchange.run(lambda r: rank_call(r, "shards"))
            keep = [max(0, min(lens[r], k - sum(lens[:r]))) for r in range(world)]
            assert [s[0].numel() for s in shards] == keep == [s[1].numel() for s in shards], case
            cut_shards += sum(0 < keep[r] < lens[r] for r in range(world))
            assert _same_rows(torch.cat([s[0] for s in shards]), torch.cat([s[1] for s in shards]),
                              want_pairs[:, :take], want_scores[:take]), case
            assert not gathers.calls[0], "the shards stay where they were ordered"
            # gathered: a pass that records every rank's ordered chunk, then one in which every rank receives all of them
            gathers.assembled = False
            exchange.run(lambda r: rank_call(r, None))
            assert [len(gathers.chunks[r][0]) for r in range(world)] == lens, case
            gathers.assembled = True
            for rk, rv in exchange.serve(lambda r: rank_call(r, None)):
                assert _same_rows(rk, rv, want_pairs[:, :take], want_scores[:take]), case
        assert cut_shards == 2, "k is meant to end inside a shard twice"
