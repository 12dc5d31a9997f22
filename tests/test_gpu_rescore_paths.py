"""GPU parity of the two launches behind eps_rescore_runs (csrc/rescore.hip) against the kernels' own definition, computed
on the host: for a pair (u, v) the int64 sum of fixw[w] over w in N(u) & N(v), as float32(float64(sum) * 2^-40).  The sum is
order-independent, so every comparison is bit for bit.

rescore_short_kernel looks for its pairs (deg(u) <= RS_SHORT = 512) 64 at a time -- a ballot over a window of keys and a walk
over the set bits -- and rescore_runs_kernel sets and clears one LDS bitmap of N(u) per run of a long row: the key lists below
are where those two can go wrong (sparse masks, a lone short pair in lane 0 / lane 63, partial last windows, more than one
window per wave, a row of exactly 512 / 513 entries, many long runs inside one 256-pair chunk, a long row after a longer one).
The production lists are sorted by (block of v, u, v): u goes up AND down between neighbouring runs, so the lists of long runs
here do too; all the others are sorted ascending.

The second half of the file runs the same comparison where the kernel's loop over id windows of RS_BITS ids takes more than one
trip: a world of 2 RS_BITS + 77 nodes (three windows), and the small world declared as RS_BITS and as RS_BITS + 1 nodes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3000
A, B, C, D = 1000, 1010, 2000, 1500           # rows of 513, 1500, 600 (long) and exactly 512 (short) entries
HUB_LEN = {A: 513, B: 1500, C: 600, D: 512}
EMPTY = list(range(10, N, 75))                # 40 rows without entries
LENGTHS = (1, 63, 64, 65, 127, 257, 4097)
CASES = (["all_short", "all_long", "interleaved", "lane0_lane63", "empty_rows", "many_long_runs", "A_then_B", "B_then_A"]
         + [f"len_{n}" for n in LENGTHS])
SENTINEL = -7.0


def _graph(rng):
    special = set(HUB_LEN) | set(EMPTY)
    plain = np.array([i for i in range(N) if i not in special])
    src = [plain, rng.choice(plain, 9000)]                      # a ring (no plain row is empty) + random edges
    dst = [np.roll(plain, -1), rng.choice(plain, 9000)]
    for h, ln in HUB_LEN.items():                                # a hub's row is exactly the plain nodes drawn for it
        src.append(np.full(ln, h))
        dst.append(rng.choice(plain, ln, replace=False))
    s, d = np.concatenate(src), np.concatenate(dst)
    keep = s != d
    s, d = s[keep], d[keep]
    flat = np.unique(np.concatenate([s * N + d, d * N + s]))     # symmetric, unit values, rows ascending
    rows, col = flat // N, (flat % N).astype(np.int32)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=rowptr[1:])
    deg = np.diff(rowptr)
    assert all(deg[h] == ln for h, ln in HUB_LEN.items()) and (deg[EMPTY] == 0).all()
    assert deg[plain].min() >= 1 and deg[plain].max() <= 40
    return rowptr, col, deg, plain


def _keys(u, v, ascending=True):
    k = (np.asarray(u, dtype=np.int64) << 32) | np.asarray(v, dtype=np.int64)
    return np.sort(k) if ascending else k


def _key_lists(rng, deg, plain):
    long_u, short_u = np.array([A, B, C]), np.concatenate([plain, [D], EMPTY])
    any_v = lambda k: rng.integers(0, N, k)                                         # noqa: E731
    lists = {}
    # every pair short: u = the 512-entry row against longer rows (u's row is staged) and shorter ones (v's is), plain u
    # against hubs and plain v
    u = np.concatenate([np.full(40, D), rng.choice(short_u, 260)])
    v = np.concatenate([[A, B, C], any_v(37), rng.choice(long_u, 60), any_v(200)])
    lists["all_short"] = _keys(u, v)
    staged_u = deg[u] <= deg[v]
    assert staged_u.any() and (~staged_u).any()
    lists["all_long"] = _keys(rng.choice(long_u, 300), np.concatenate([any_v(280), [A, B, C, D], EMPTY[:16]]))
    # long and short runs interleaved: windows of 64 keys with a few short pairs among long ones
    u = np.concatenate([np.arange(990, 1000), np.full(50, A), [1003, 1007], np.full(50, B), np.arange(1011, 1020), np.full(20, D),
                        [1777], np.full(45, C), np.arange(2001, 2011)])
    lists["interleaved"] = _keys(u, any_v(u.size))
    # window 0: the only short pair in lane 0; window 1: the only short pair in lane 63
    lists["lane0_lane63"] = _keys(np.concatenate([[999], np.full(126, A), [1001]]),
                                  np.concatenate([[5], rng.choice(N, 126, replace=False), [6]]))
    assert deg[999] <= 512 and deg[1001] <= 512 and lists["lane0_lane63"].size == 128
    e0, e1, p = EMPTY[0], EMPTY[1], int(plain[7])
    lists["empty_rows"] = _keys([e0, p, A, e0, e0, B], [p, e0, e0, A, e1, e1])
    # one workgroup, 42 long runs of 5 pairs in 210 < 256 pairs: a bit of N(B) left in the bitmap would count for the next run
    u = np.repeat(np.tile(long_u, 14), 5)
    lists["many_long_runs"] = _keys(u, any_v(u.size), ascending=False)
    lists["A_then_B"] = _keys(np.repeat([A, B], 30), any_v(60), ascending=False)
    lists["B_then_A"] = _keys(np.repeat([B, A], 30), any_v(60), ascending=False)
    for n in LENGTHS:                                                               # partial last window; several windows a wave
        pick_long = (rng.random(n) < 0.5) & (n > 1)                                 # (the single pair is a short one)
        lists[f"len_{n}"] = _keys(np.where(pick_long, rng.choice(long_u, n), rng.choice(short_u, n)), any_v(n))
        assert lists[f"len_{n}"].size == n
    assert set(lists) == set(CASES)
    return lists


def _reference(rowptr, col, fixw, keys):
    out = np.empty(keys.size, dtype=np.float32)
    for i, k in enumerate(keys):
        u, v = int(k >> 32), int(k & 0xFFFFFFFF)
        both = np.intersect1d(col[rowptr[u]:rowptr[u + 1]], col[rowptr[v]:rowptr[v + 1]], assume_unique=True)
        out[i] = np.float32(np.float64(fixw[both].sum(dtype=np.int64)) * 2.0 ** -40)
    return out


@pytest.fixture(scope="module")
def world(dev):
    rng = np.random.default_rng(20240611)
    rowptr, col, deg, plain = _graph(rng)
    fixw = rng.integers(1, 1 << 41, N, dtype=np.int64)           # multiples of 2^-40 below 2: a row's sum stays below 2^53
    lists = _key_lists(rng, deg, plain)
    ref = {name: _reference(rowptr, col, fixw, k) for name, k in lists.items()}
    assert not ref["empty_rows"].any() and ref["all_short"].any() and ref["all_long"].any()
    t = lambda a: torch.from_numpy(a).to(dev)                                       # noqa: E731
    return {"rowptr": t(rowptr), "col": t(col), "fixw": t(fixw), "keys": {n: t(k) for n, k in lists.items()}, "ref": ref}


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("case", CASES)
def test_rescore_runs_matches_host_sums(eps, world, case):
    w = world
    got = eps.ops.rescore_runs(w["rowptr"], w["col"], w["fixw"], N, w["keys"][case])
    assert _same_bits(got, w["ref"][case])


@pytest.mark.parametrize("case", CASES)
def test_rescore_runs_dev_stops_at_device_count(eps, dev, world, case):
    """A count on the device below the list's length: the first `count` scores are the reference's, and no slot beyond them is
    written (the wrapper's own output is uninitialised memory, so the sentinel goes through the same call with an output of the
    test's)."""
    w = world
    keys = w["keys"][case]
    count = keys.numel() * 2 // 3
    n_dev = torch.tensor([count], dtype=torch.int64, device=dev)
    got = eps.ops.rescore_runs_dev(w["rowptr"], w["col"], w["fixw"], N, keys, n_dev)
    assert _same_bits(got[:count], w["ref"][case][:count])
    out = torch.full((keys.numel(),), SENTINEL, dtype=torch.float32, device=dev)
    eps.ops._call("eps_rescore_runs_dev", dev, w["rowptr"], w["col"], w["fixw"], N, keys, keys.numel(), n_dev, out)
    assert _same_bits(out[:count], w["ref"][case][:count])
    assert bool((out[count:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- several id windows
# rescore_runs_kernel walks the id space in windows of RS_BITS ids, setting and clearing the bitmap of N(u) per window.  The world
# above fits one window; the one below has n = 2 RS_BITS + 77 nodes -- three windows, almost every node isolated -- and is held to
# the same host sums, bit for bit.  Every size comes from ops.rescore_limits().
LA, LB = 10, 11                               # long rows: LA has entries in every window, LB none in the second one
WIDE_CASES = ["long_runs", "A_then_B_stale_bits", "B_then_A", "mixed_with_short", "last_window_only"]


def _wide_graph(rng, bits, short):
    n = 2 * bits + 77
    edge_ids = [bits - 1, bits, bits + 1, 2 * bits - 1, 2 * bits, n - 1]
    w0, w1, w2 = np.arange(100, 3000), np.arange(bits + 100, bits + 3000), np.arange(2 * bits + 1, n - 1)
    apart = np.arange(3000, 4000)                                                   # ids no long row holds
    rows = {LA: np.concatenate([rng.choice(w0, short // 2 + 40, replace=False), rng.choice(w1, short // 2 + 40, replace=False),
                                rng.choice(w2, 20, replace=False), edge_ids]),
            LB: np.concatenate([rng.choice(w0, short + 9, replace=False), rng.choice(w2, 20, replace=False), [bits - 1, 2 * bits, n - 1]])}
    in_a = rows[LA]
    a1 = in_a[(in_a >= bits) & (in_a < 2 * bits)]
    v_all = np.arange(5000, 5100)                                                   # rows with entries in every window, half of them LA's
    for i in v_all:
        rows[i] = np.concatenate([rng.choice(w0, 12), rng.choice(in_a[in_a < bits], 6), rng.choice(w1, 8), rng.choice(a1, 8),
                                  rng.choice(w2, 6), rng.choice(edge_ids, 2)])
    v_last = np.arange(5100, 5140)                                                  # common neighbours with LA / LB in the last window only
    for i in v_last:
        rows[i] = np.concatenate([rng.choice(apart, 20), rng.choice(w2, 10), [2 * bits] if i % 2 else [n - 1]])
    rows[5140] = np.array(edge_ids)                                                 # exactly the ids on the window edges
    rows[5141] = np.concatenate([rng.choice(w1, short, replace=False), edge_ids])                  # a third long row, as v and as u
    src = np.concatenate([np.full(len(c), r, np.int64) for r, c in rows.items()])
    flat = np.unique(src * n + np.concatenate(list(rows.values())).astype(np.int64))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat // n, minlength=n), out=rowptr[1:])
    col = (flat % n).astype(np.int32)
    deg = np.diff(rowptr)
    assert deg[LA] > short and deg[LB] > short and deg[5141] > short and deg[v_all].max() <= short
    row = lambda r: col[rowptr[r]:rowptr[r + 1]]                                     # noqa: E731
    assert set(edge_ids) <= set(row(LA).tolist()) and not ((row(LB) >= bits) & (row(LB) < 2 * bits)).any()
    assert all(((row(v) >= bits) & (row(v) < 2 * bits) & np.isin(row(v), row(LA))).any() for v in v_all)   # what a stale bit would count
    assert all((np.intersect1d(row(v), row(LA)) >= 2 * bits).all() and len(np.intersect1d(row(v), row(LA))) for v in v_last)
    return n, rowptr, col, dict(v_all=v_all, v_last=v_last, edges=5140, third=5141)


def _wide_lists(rng, g, chunk):
    v_all, v_last = g["v_all"], g["v_last"]
    every_v = np.concatenate([v_all, v_last, [g["edges"], g["third"], LA, LB]])
    lists = {"long_runs": _keys(np.repeat([LA, LB, g["third"]], len(every_v)), np.tile(every_v, 3))}
    # one 256-pair chunk: the run of LA (bits in the second window), then the run of LB (none there) on rows v that DO have entries there
    k = chunk // 2 - 8
    lists["A_then_B_stale_bits"] = _keys(np.repeat([LA, LB], k), np.tile(rng.choice(v_all, k), 2))
    assert lists["A_then_B_stale_bits"].size < chunk and LA < LB
    lists["B_then_A"] = _keys(np.repeat([LB, LA], k), np.tile(rng.choice(v_all, k), 2), ascending=False)
    u = np.concatenate([rng.choice(v_all, 150), np.full(60, LA), rng.choice(v_last, 40), np.full(60, g["third"]), [g["edges"]] * 10])
    lists["mixed_with_short"] = _keys(u, rng.choice(every_v, u.size))
    lists["last_window_only"] = _keys(np.repeat([LA, LB], len(v_last)), np.tile(v_last, 2))
    assert set(lists) == set(WIDE_CASES)
    return lists


@pytest.fixture(scope="module")
def limits(eps):
    bits, short, chunk = eps.ops.rescore_limits()
    assert short == HUB_LEN[D] and short + 1 == HUB_LEN[A]          # the small world's rows of exactly RS_SHORT / RS_SHORT + 1 entries
    return bits, short, chunk


@pytest.fixture(scope="module")
def wide_world(dev, limits):
    bits, short, chunk = limits
    rng = np.random.default_rng(20240612)
    n, rowptr, col, g = _wide_graph(rng, bits, short)
    fixw = rng.integers(1, 1 << 41, n, dtype=np.int64)
    lists = _wide_lists(rng, g, chunk)
    ref = {name: _reference(rowptr, col, fixw, k) for name, k in lists.items()}
    assert all(r.any() for r in ref.values()) and (ref["last_window_only"] > 0).all()
    t = lambda a: torch.from_numpy(a).to(dev)                                       # noqa: E731
    return {"n": n, "rowptr": t(rowptr), "col": t(col), "fixw": t(fixw), "keys": {k: t(v) for k, v in lists.items()}, "ref": ref}


@pytest.mark.parametrize("case", WIDE_CASES)
def test_rescore_runs_over_three_id_windows(eps, dev, wide_world, limits, case):
    w = wide_world
    assert w["n"] == 2 * limits[0] + 77
    keys = w["keys"][case]
    got = eps.ops.rescore_runs(w["rowptr"], w["col"], w["fixw"], w["n"], keys)
    assert _same_bits(got, w["ref"][case])
    # the device count below the list's length: the head is the reference's, nothing beyond it is written
    count = keys.numel() * 2 // 3
    n_dev = torch.tensor([count], dtype=torch.int64, device=dev)
    out = torch.full((keys.numel(),), SENTINEL, dtype=torch.float32, device=dev)
    eps.ops._call("eps_rescore_runs_dev", dev, w["rowptr"], w["col"], w["fixw"], w["n"], keys, keys.numel(), n_dev, out)
    assert _same_bits(out[:count], w["ref"][case][:count]) and bool((out[count:] == SENTINEL).all())
    assert _same_bits(eps.ops.rescore_runs_dev(w["rowptr"], w["col"], w["fixw"], w["n"], keys, n_dev)[:count], w["ref"][case][:count])


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("case", ["all_long", "interleaved", "many_long_runs", "A_then_B"])
def test_rescore_runs_at_the_window_switch(eps, dev, world, limits, case, extra):
    """The small world again as a graph of exactly RS_BITS nodes (one window) and of RS_BITS + 1 (a second window of one id): the
    nodes beyond N are isolated, the sums are the same."""
    w = world
    n = limits[0] + extra
    nnz = w["col"].numel()
    rowptr = torch.cat([w["rowptr"], torch.full((n - N,), nnz, dtype=torch.int64, device=dev)])
    fixw = torch.cat([w["fixw"], torch.ones(n - N, dtype=torch.int64, device=dev)])
    assert rowptr.numel() == n + 1 and fixw.numel() == n
    got = eps.ops.rescore_runs(rowptr, w["col"], fixw, n, w["keys"][case])
    assert _same_bits(got, w["ref"][case])
