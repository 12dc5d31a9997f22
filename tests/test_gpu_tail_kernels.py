"""GPU parity of the small kernels behind the scan (still filter.py:96-142 + :160-161 under --keep_top), each against a host model:
eps_scan_refine on hand-made walked lists (csrc/scan_heads.hip: the head term, the early exit, holes, the list's end, a full
output list, the candidate counter it hands on), eps_score_hist + eps_score_pick_compact against the bucket arithmetic restated
in numpy (csrc/tail_sort.hip: k-th bucket, threshold, the compacted set, the state left zeroed), and eps_sort_pairs_by_u against
numpy.lexsort for both outcomes of its device-side decision (csrc/topk_select.hip)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SP_FLAG = 0x80000000


# ---- eps_scan_refine --------------------------------------------------------------------------------------------------------------
def bar_units(thr, shift):
    """sp_bar_units (csrc/scan_common.h): the bar in table units."""
    thr = np.float32(thr)

    def above(a):
        return bool(np.float32(float(a) * 2.0 ** -40) > thr)
    top = 0x7fffffffffffffff
    if not above(top):
        return SP_FLAG
    if above(0):
        return 1
    lo, hi = 1, top
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if above(mid):
            hi = mid
        else:
            lo = mid + 1
    q = lo >> (40 - shift)
    return SP_FLAG if q >= SP_FLAG else (q if q else 1)


N_HUB = 256
MAX_ROWS = (0, 1, 4, 5, 9)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 300, 5000)


@pytest.fixture(scope="module")
def refine_world(eps, dev):
    """The graph, its tables and, per ``max_rows``, a pool of distinct slots (key, walked sum) with their host-model totals."""
    from eps_amd import scan, synth
    from eps_amd.heuristics import node_weight_table
    g0 = synth.rmat_graph(12, 10, 5, dev)
    g, perm = g0.degree_ordered()[:2]
    sc = scan.screen_weights(g0, g, perm, node_weight_table(g0, eps.ops.W_AA))
    n = g.n_rows
    rp, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    fx = sc.fx32.cpu().numpy().view(np.uint32).astype(np.int64)
    adj = np.zeros((n, n), dtype=bool)
    adj[np.repeat(np.arange(n), np.diff(rp)), col] = True
    hub = eps.ops.scan_hub_rows(g.rowptr, g.col, N_HUB)
    # a bar above every head term (nine rows at most), so that a walked sum can sit exactly at bar - head and one below
    units = 12 * int(fx[:N_HUB].max())
    assert units < 1 << 30
    bar = float(np.float32(units * 2.0 ** -sc.shift))
    thr32 = bar_units(bar, sc.shift)
    assert 9 * int(fx[:N_HUB].max()) < thr32 < SP_FLAG
    rng = np.random.default_rng(11)
    pools = {}
    for max_rows in MAX_ROWS:
        heads = eps.ops.scan_heads(g.rowptr, g.col, sc.fx32, N_HUB, (1 << 31) - 1, max_rows)
        hx = heads.cpu().numpy().view(np.uint32)[:, 0].astype(np.int64)
        assert hx.max() == max_rows, "no column's head is as long as max_rows"
        vs, us, kinds = [], [], []
        cols_any = rng.integers(0, n, 6000)
        for v in cols_any:
            x = hx[v]
            rows = col[rp[v]:rp[v] + x]
            u_rand = int(rng.integers(0, n))
            picks = [(u_rand, "random")]
            if x >= 2:
                # u reached through the deepest skipped row only (row 0: the LAST one probed) / through the shallowest only
                for w_only, kind in ((rows[0], "deepest"), (rows[x - 1], "shallowest")):
                    cand = np.flatnonzero(adj[w_only] & ~adj[np.setdiff1d(rows, [w_only])].any(axis=0))
                    if cand.size:
                        picks.append((int(cand[rng.integers(0, cand.size)]), kind))
            for u, kind in picks:
                vs.append(int(v)); us.append(u); kinds.append(kind)
        vs, us, kinds = np.array(vs), np.array(us), np.array(kinds)
        key = (vs.astype(np.int64) << 32) | us
        _, first = np.unique(key, return_index=True)                 # (distinct pairs: a stored slot is then known by its key)
        first = rng.permutation(first)                               # (... and neighbouring slots come from different columns)
        vs, us, kinds, key = vs[first], us[first], kinds[first], key[first]
        head = np.zeros(len(vs), np.int64)
        for j in range(max_rows):
            has = hx[vs] > j
            w = col[np.minimum(rp[vs] + j, len(col) - 1)]
            head += np.where(has & adj[np.where(has, w, 0), us], fx[np.where(has, w, 0)], 0)
        # walked sums: exactly at the bar with the head / one below / alone at the bar / alone one below / anything
        mode = rng.integers(0, 5, len(vs))
        mode[kinds != "random"] = rng.integers(0, 2, int((kinds != "random").sum()))
        s_walk = np.select([mode == 0, mode == 1, mode == 2, mode == 3],
                           [thr32 - head, thr32 - head - 1, thr32 + rng.integers(0, 1000, len(vs)), np.full(len(vs), thr32 - 1)],
                           rng.integers(0, thr32, len(vs)))
        assert s_walk.min() >= 0 and s_walk.max() < SP_FLAG
        total = s_walk + head
        passes = total >= thr32
        for kind in ("deepest", "shallowest"):
            if max_rows >= 5:
                assert (passes & (kinds == kind) & (s_walk < thr32)).sum() > 3, f"no slot passes through the {kind} row alone"
        if max_rows:
            assert (passes & (mode == 2)).sum() > 3 and (~passes & (mode == 1)).sum() > 3 and (head > 0).sum() > 50
        score = (total.astype(np.uint64).astype(np.float32) * np.float32(2.0 ** -sc.shift)).astype(np.float32)
        pools[max_rows] = dict(heads=heads, key=key, s_walk=s_walk.astype(np.uint32), passes=passes, score=score)
        assert len(key) >= 5000
    return dict(g=g, sc=sc, hub=hub, bar=bar, pools=pools)


def _walked_list(eps, dev, pool, length, bar, with_holes, rng):
    """A Survivors list of ``length`` slots made by hand, garbage behind it -> (list, expected (key, score bits) of what passes)."""
    key = pool["key"][:length].copy()
    live = np.ones(length, bool)
    if with_holes and length:
        live[rng.integers(0, length, max(1, length // 9))] = False           # single holes ...
        if length >= 129:
            live[64:128] = False                                             # ... and a whole wave's stretch
    key[~live] = -1
    s_walk = pool["s_walk"][:length].copy()
    s_walk[~live] = 0xFFFFFFFF                                               # (a hole's value word is never looked at)
    pad = 200                                                                # slots behind the list's end: pairs that WOULD pass
    walked = eps.ops.Survivors(length + pad, bar, dev, prefill=False)
    behind = pool["passes"].nonzero()[0][:pad]
    all_key = np.concatenate([key, np.resize(pool["key"][behind], pad)])
    all_val = np.concatenate([s_walk, np.resize(pool["s_walk"][behind], pad)])
    walked.key.copy_(torch.from_numpy(all_key))
    walked.val.view(torch.int32).copy_(torch.from_numpy(all_val.view(np.int32)))
    walked.rec[1] = length
    walked.rec[4] = 1234567 + length
    want = live & pool["passes"][:length]
    return walked, key[want], pool["score"][:length][want].view(np.uint32)


def _sorted_pairs(key, bits):
    o = np.lexsort((bits, key))
    return key[o], bits[o]


@pytest.mark.parametrize("max_rows", MAX_ROWS)
def test_refine_against_host_model(eps, dev, refine_world, max_rows):
    W = refine_world
    g, sc, pool = W["g"], W["sc"], W["pools"][max_rows]
    rng = np.random.default_rng(100 + max_rows)

    def refine(walked, capacity, bar):
        out = eps.ops.Survivors(capacity, bar, dev, prefill=False)
        eps.ops.scan_refine(walked, pool["heads"], W["hub"], sc.fx32, g.rowptr, g.col, g.n_rows, sc.shift, out)
        count, cand = out.counts()
        m = min(count, capacity)
        return count, cand, out.key[:m].cpu().numpy(), out.val[:m].cpu().numpy().view(np.uint32)

    for length in LENGTHS:
        for with_holes in (False, True):
            walked, want_k, want_b = _walked_list(eps, dev, pool, length, W["bar"], with_holes, rng)
            count, cand, got_k, got_b = refine(walked, length + 1, W["bar"])
            assert count == len(want_k), (max_rows, length, with_holes)
            assert cand == 1234567 + length, "the walk's candidate counter was not handed on"
            a, b = _sorted_pairs(got_k, got_b), _sorted_pairs(want_k, want_b)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (max_rows, length, with_holes)
            if length >= 300 and not with_holes:
                assert len(want_k) > length // 8, "too few slots pass for the cases below to mean anything"
                # a bar of +inf: nothing passes
                count, _, got_k, _ = refine(walked, length, float("inf"))
                assert count == 0 and got_k.size == 0
                # an output list smaller than what passes: everything is counted, `capacity` distinct members are stored
                cap = len(want_k) // 3
                count, cand, got_k, got_b = refine(walked, cap, W["bar"])
                assert count == len(want_k) and got_k.size == cap and np.unique(got_k).size == cap and cand == 1234567 + length
                where = np.searchsorted(b[0], got_k)
                assert np.array_equal(b[0][where], got_k) and np.array_equal(b[1][where], got_b)


# ---- eps_score_hist + eps_score_pick_compact ----------------------------------------------------------------------------------------
TS_MB = 8
TS_BINS = (32 - TS_MB + 1) << TS_MB


def ts_ordered(f):
    b = (np.asarray(f, np.float32) + np.float32(0.0)).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)


def ts_unordered(o):
    o = int(o)
    b = (o & 0x7fffffff) if o & 0x80000000 else (~o & 0xFFFFFFFF)
    return np.array([b], np.uint32).view(np.float32)[0]


def ts_bucket(d):
    d = np.asarray(d, np.int64)
    big = d >= 1 << TS_MB
    e = np.frexp(d.astype(np.float64))[1].astype(np.int64) - 1                   # (position of the top bit: d < 2^32 is exact in a double)
    return np.where(big, ((e - TS_MB + 1) << TS_MB) | ((d >> np.maximum(e - TS_MB, 0)) & ((1 << TS_MB) - 1)), d)


def ts_bucket_floor(b):
    if b < 1 << TS_MB:
        return b
    e1, m = b >> TS_MB, b & ((1 << TS_MB) - 1)
    return ((1 << TS_MB) | m) << (e1 - 1)


def pick_model(hist, ob, k, mode, params):
    """(kth, thr) of ts_pick_compact_kernel from the histogram."""
    suffix = np.cumsum(hist[::-1])[::-1]                              # values in buckets >= b
    kth = np.float32(-np.inf)
    if k != 0 and suffix[0] >= k:
        bstar = int(np.flatnonzero(suffix >= k).max())
        if bstar:
            kth = ts_unordered(min(ob + ts_bucket_floor(bstar), 0xFFFFFFFF))
    thr = kth
    if kth > -np.inf:
        if mode == 1:
            o = int(ts_ordered(kth))
            thr = ts_unordered(o - 2 if o == 0x80000000 else o - 1)
        elif mode == 2:
            pa, pb, pc = (np.float32(x) for x in params)
            low, rel = np.float32(kth - pa), np.float32(kth * pb)
            thr = np.float32((low if low > rel else rel) - np.float32(np.abs(kth) * pc))
    return np.float32(kth), np.float32(thr)


def _bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 511, 512, 513, 8191, 8192, 8193, 16385, 300_000])
def test_hist_pick_compact_against_numpy(eps, dev, n):
    rng = np.random.default_rng(n + 5)
    pad = 777                                                        # garbage behind the list: live, and better than everything
    vals = (rng.integers(0, 4096, n + pad) / np.float32(512.0)).astype(np.float32)        # (many ties)
    vals = np.where(rng.random(n + pad) < 0.5, vals, (rng.random(n + pad) * 8).astype(np.float32)).astype(np.float32)
    vals[rng.random(n + pad) < 0.05] = -np.inf
    vals[n:] = 100.0
    keys = (rng.permutation(n + pad).astype(np.int64) << 32) | rng.integers(0, 1 << 31, n + pad)
    keys[rng.random(n + pad) < 0.1] = -1
    keys[n:] = np.abs(keys[n:])
    base_v, above_v = np.float32(0.75), np.float32(1.5)
    t_keys, t_vals = torch.from_numpy(keys).to(dev), torch.from_numpy(vals).to(dev)
    n_dev = torch.tensor([n], dtype=torch.int64, device=dev)
    base = torch.tensor([base_v], dtype=torch.float32, device=dev)
    above = torch.tensor([above_v], dtype=torch.float32, device=dev)
    ob = int(ts_ordered(base_v))
    params = (0.25, 0.9, 1e-3)
    for use_above in (False, True):
        live = (keys[:n] >= 0) & (vals[:n] > -np.inf)
        if use_above:
            live &= vals[:n] > above_v
        o = ts_ordered(vals[:n][live])
        hist = np.bincount(ts_bucket(np.maximum(o - ob, 0)), minlength=TS_BINS)
        assert hist.size == TS_BINS
        n_live = int(live.sum())
        for k in sorted({0, 1, n // 2, n, n + 1}):
            for mode in (0, 1, 2):
                for swap in (False, True):
                    kth, thr = pick_model(hist, ob, k, mode, params)
                    keep = live & (vals[:n] >= thr)
                    order = np.argsort(keys[:n][keep])
                    want, want_b = keys[:n][keep][order], _bits(vals[:n][keep])[order]
                    rooms = [None] + ([len(want) // 2] if mode == 0 and swap and len(want) >= 4 else [])
                    for room in rooms:
                        first = None
                        for _ in range(2):       # (twice back to back: the second run starts from the state the first one left)
                            eps.ops.score_hist(t_keys, t_vals, n_dev, base, above if use_above else None)
                            ok, ov, n_out, g_kth, g_thr = eps.ops.score_pick_compact(
                                t_keys, t_vals, n_dev, base, k, above if use_above else None, mode, params, swap, room)
                            got = (int(n_out), _bits(g_kth.cpu().numpy())[0], _bits(g_thr.cpu().numpy())[0])
                            case = (n, use_above, k, mode, swap, room)
                            assert got == (len(want), _bits(kth)[0], _bits(thr)[0]), (case, got, kth, thr)
                            stored = min(len(want), ok.numel())
                            gk = ok[:stored].cpu().numpy()
                            if swap:
                                gk = ((gk.view(np.uint64) << np.uint64(32)) | (gk.view(np.uint64) >> np.uint64(32))).view(np.int64)
                            gv = _bits(ov[:stored].cpu().numpy())
                            assert np.unique(gk).size == stored and stored == (len(want) if room is None else min(room, len(want))), case
                            at = np.minimum(np.searchsorted(want, gk), max(len(want) - 1, 0))
                            assert stored == 0 or (np.array_equal(want[at], gk) and np.array_equal(want_b[at], gv)), case
                            first = first or got
                            assert got == first
    # the selection without a list to compact (the bar sample): k-th and threshold alone, and the state is left clean as well
    finite = vals[:n] > -np.inf
    hist = np.bincount(ts_bucket(np.maximum(ts_ordered(vals[:n][finite]) - ob, 0)), minlength=TS_BINS)
    kth, thr = pick_model(hist, ob, max(1, int(finite.sum()) // 3), 1, params)
    for _ in range(2):
        eps.ops.score_hist(None, t_vals, n_dev, base, None)
        _, _, _, g_kth, g_thr = eps.ops.score_pick_compact(None, t_vals, n_dev, base, max(1, int(finite.sum()) // 3), None, 1)
        assert (_bits(g_kth.cpu().numpy())[0], _bits(g_thr.cpu().numpy())[0]) == (_bits(kth)[0], _bits(thr)[0]), n


# ---- eps_sort_pairs_by_u ----------------------------------------------------------------------------------------------------------
def _by_u_model(keys, id_bits, shift):
    """(expected order, whether the blocked order is the one kept): SEL_BLOCK_MIN_RUN = 64 pairs per run of equal (v block, u)."""
    v, u = keys >> 32, keys & 0xFFFFFFFF
    o = np.lexsort((v, u, v >> shift))
    bv, bu = (v >> shift)[o], u[o]
    runs = 1 + int(((bv[1:] != bv[:-1]) | (bu[1:] != bu[:-1])).sum())
    blocked = runs * 64 <= len(keys)
    if not blocked:
        o = np.lexsort((v, u))
    return (u[o] << 32) | v[o], blocked


def _pairs(rng, n, id_bits, n_u):
    """n distinct pairs u < v with u among the first n_u ids."""
    u = rng.integers(0, n_u, 3 * n + 50)
    v = rng.integers(n_u, 1 << id_bits, 3 * n + 50)
    key = np.unique((v.astype(np.int64) << 32) | u)
    assert key.size >= n
    return rng.permutation(key)[:n]


@pytest.mark.parametrize("n,n_u,want_blocked", [(1, 8, False), (255, 8, False), (256, 8, False), (257, 8, False),
                                                (100_000, 8, True), (100_000, 1 << 13, False), (20_000, 2, True)])
def test_sort_pairs_by_u_against_lexsort(eps, dev, n, n_u, want_blocked):
    id_bits, shift = 14, 10
    keys = _pairs(np.random.default_rng(n + n_u), n, id_bits, n_u)
    want, blocked = _by_u_model(keys, id_bits, shift)
    assert blocked == want_blocked, "the list does not test the decision it was made for"
    got = eps.ops.sort_pairs_by_u(torch.from_numpy(keys).to(dev), id_bits, shift).cpu().numpy()
    assert np.array_equal(got, want)
    # (without blocks: the (u, v) order whatever the runs are)
    v, u = keys >> 32, keys & 0xFFFFFFFF
    o = np.lexsort((v, u))
    got = eps.ops.sort_pairs_by_u(torch.from_numpy(keys).to(dev), id_bits, 0).cpu().numpy()
    assert np.array_equal(got, (u[o] << 32) | v[o])
