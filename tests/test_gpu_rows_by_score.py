"""GPU: eps_rows_by_score (csrc/rows_by_score.hip) -- the cut, the selection and the K rows of a step from ONE score sort of the
re-scored pairs.  The entry alone on synthetic lists, against the numpy truth (tests/rows_by_score_truth.py), against
eps_score_hist + eps_score_pick_compact (the cut and the count it replaces) and against eps_select_topk_rows_pairs (the rows it
replaces), bit for bit; then scan_topk with the default tail against TAIL_SORT = "library"."""
import numpy as np
import pytest
import torch

import rows_by_score_truth as rt

pytestmark = pytest.mark.gpu

L, W = 1024, 1024            # the longest run the kernel orders / sorted pairs per workgroup (test_limits holds them to the library)
BAR = np.float32(1.75)
ABOVE = np.nextafter(BAR, np.float32(np.inf), dtype=np.float32)


def _bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


def _state_is_clean(eps, dev):
    torch.cuda.synchronize()
    return int(eps.ops.tail_state(dev).abs().sum().item()) == 0


def test_limits(eps):
    assert eps.ops.rows_by_score_limits() == (L, W) and L >= 1024


def _runs(*lengths, top=900.0):
    """A descending score profile: one run of equal scores per length, levels 0.5 apart (exact in float32) from ``top`` down."""
    return np.concatenate([np.full(g, top - 0.5 * i, np.float32) for i, g in enumerate(lengths)]) if lengths else np.zeros(0, np.float32)


def _distinct(n, rng):
    return (BAR + np.float32(0.01) + rng.permutation(n).astype(np.float32) / np.float32(64.0)).astype(np.float32)


def _eighths(n, rng):
    return (np.floor((BAR + 0.2 + 6 * rng.random(n)) * 8) / 8).astype(np.float32)


def _profiles(rng):
    """name -> scores of a list (any order: the entry sorts them).  Sorted positions are what the profile says, so a run's place
    relative to the windows of W sorted pairs is chosen here."""
    p = {}
    for n in (0, 1, 2, 63, 64, 65, W - 1, W, W + 1):
        p[f"distinct_{n}"] = _distinct(n, rng)
        p[f"eighths_{n}"] = _eighths(n, rng)
    p["eighths_3000"] = _eighths(3000, rng)                                       # many short runs over three windows
    p["straddle"] = _runs(*([1] * (W - 5)), 10, *([1] * 300))                    # a run over sorted positions W - 5 .. W + 5
    p["starts_on_last"] = _runs(*([1] * (W - 1)), 5, *([1] * 200), 3)            # a run that starts on a window's last entry
    p["two_windows"] = _runs(*([1] * 7), W, *([1] * (W - 7 - 2)), 4, 1)          # a run of W pairs from position 7, then one over 2 W - 2 ..
    p["run_L"] = _runs(3, L, 2)                                                   # exactly L: ordered in the kernel
    p["run_L_plus_1"] = _runs(3, L + 1, 2)                                        # L + 1: no attempt, the flag
    p["run_L_from_last"] = _runs(*([1] * (W - 1)), L, 2)                          # the furthest a run reaches beyond its window: L - 1
    p["run_L_plus_1_from_last"] = _runs(*([1] * (W - 1)), L + 1, 2)
    p["equal_L"] = np.full(L, 3.25, np.float32)
    p["equal_L_plus_1"] = np.full(L + 1, 3.25, np.float32)
    p["equal_2500"] = np.full(2500, 3.25, np.float32)
    bar_mix = _eighths(700, rng)
    bar_mix[rng.random(700) < 0.2] = BAR                                           # at the bar: not live
    bar_mix[rng.random(700) < 0.2] = ABOVE                                         # one float above it: live, one run
    bar_mix[rng.random(700) < 0.1] = -np.inf
    bar_mix[rng.random(700) < 0.1] = BAR - np.float32(0.5)
    p["bar_mix"] = bar_mix
    p["one_dead"] = np.concatenate([_distinct(99, rng), np.float32([-np.inf])])
    p["nothing_live"] = np.concatenate([np.full(40, BAR, np.float32), np.float32([-np.inf, 0.0, -3.0])])
    return p


def _pairs(n, n_ids, rng):
    """n distinct pairs u < v over ids below n_ids, as keys u << 32 | v in random order."""
    keys = np.zeros(0, np.int64)
    while keys.size < n:
        a, b = rng.integers(0, n_ids, 2 * n + 8), rng.integers(0, n_ids, 2 * n + 8)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        keys = np.unique(np.concatenate([keys, ((lo << 32) | hi)[lo < hi]]))
    return rng.permutation(keys)[:n]


N_IDS = 3000
LABELS = {
    # name -> (id_bits, perm over the N_IDS ids or None)
    "as_labelled_20": (20, lambda rng: None),
    "flipped_20": (20, lambda rng: np.arange(N_IDS - 1, -1, -1, dtype=np.int64)),                 # the larger endpoint becomes the smaller
    "random_20": (20, lambda rng: rng.permutation(1 << 20)[:N_IDS].astype(np.int64)),
    "random_32": (32, lambda rng: rng.permutation(np.unique(rng.integers(0, 1 << 31, 2 * N_IDS)))[:N_IDS].astype(np.int64)),
}


def _check(eps, dev, name, vals, labels, rng):
    ops = eps.ops
    id_bits, make_perm = LABELS[labels]
    perm = make_perm(rng)
    n = vals.size
    keys = _pairs(n, N_IDS, rng)
    vals = vals[rng.permutation(n)]
    t_keys, t_vals = torch.from_numpy(keys).to(dev), torch.from_numpy(vals).to(dev)
    t_perm = None if perm is None else torch.from_numpy(perm).to(dev)
    bar = torch.tensor([BAR], dtype=torch.float32, device=dev)
    n_live = int(((vals > BAR) & (vals > -np.inf)).sum())
    desc = np.sort(vals)[::-1]
    for k2 in sorted({0, 1, max(1, n_live // 3), n_live, n_live + 1}):            # (n_live + 1: fewer than k2 live entries, the cut is -inf)
        cut, n_sel, _, _, longest = rt.rows_by_score(keys, vals, BAR, k2, 0)
        # a K inside a run: one row past the first row of the run that holds the middle selected pair
        inside = [2 * int(np.flatnonzero(desc == desc[n_sel // 2])[0]) + 1] if n_sel else []
        for k in sorted({1, 2, 7, max(1, 2 * n_sel - 1), max(1, 2 * n_sel), 2 * n_sel + 5, *inside}):
            case = (name, labels, k2, k)
            _, _, want_pairs, want_scores, _ = rt.rows_by_score(keys, vals, BAR, k2, k, perm)
            pairs, scores, s_keys, s_vals, g_n, g_cut, flag = ops.rows_by_score(t_keys, t_vals, bar, k2, k, id_bits, t_perm)
            # the cut and the count: the truth, and the histogram selection on the same list
            assert (int(g_n), _bits(g_cut.cpu().numpy())[0]) == (n_sel, _bits(cut)[0]), case
            ops.score_hist(t_keys, t_vals, None, bar, above=bar)
            h_k, h_v, h_n, h_cut, _ = ops.score_pick_compact(t_keys, t_vals, None, bar, k2, above=bar, swap_halves=True)
            assert int(h_n) == n_sel and _bits(h_cut.cpu().numpy())[0] == _bits(g_cut.cpu().numpy())[0], case
            # the sorted list: descending, and its first n_sel entries are the selection (as v << 32 | u)
            sv = s_vals.cpu().numpy()
            assert n < 2 or bool((sv[:-1] >= sv[1:]).all()), case
            got_sel = torch.sort(s_keys[:n_sel]).values
            assert torch.equal(got_sel, torch.sort(h_k[:n_sel]).values), case
            assert np.array_equal(np.sort(_bits(sv[:n_sel])), np.sort(_bits(h_v[:n_sel].cpu().numpy()))), case
            # the rows: the library ordering of that selection == the truth, always; the entry's own rows unless the flag is set
            take = min(k, 2 * n_sel)
            lib_pairs, lib_scores = ops.select_rows_pairs(s_keys[:n_sel].contiguous(), s_vals[:n_sel].contiguous(), k, id_bits, t_perm)
            assert lib_pairs.shape == (2, take) and np.array_equal(lib_pairs.cpu().numpy(), want_pairs), case
            assert np.array_equal(_bits(lib_scores.cpu().numpy()), _bits(want_scores)), case
            assert int(flag) == int(longest > L), (case, longest)
            if longest <= L:
                assert torch.equal(pairs[:, :take], lib_pairs) and torch.equal(scores[:take].view(torch.int32), lib_scores.view(torch.int32)), case
    assert _state_is_clean(eps, dev)


_RNG = np.random.default_rng(11)
PROFILES = _profiles(_RNG)


@pytest.mark.parametrize("name", sorted(PROFILES))
def test_entry_on_synthetic_lists(eps, dev, name):
    """Every profile as labelled (id_bits 20); the ones with runs also under a relabelling that flips which endpoint is the larger,
    under a random one, and with ids up to 2^31 (id_bits 32: the ids are compared as whole words)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    _check(eps, dev, name, PROFILES[name], "as_labelled_20", rng)
    if name in ("eighths_65", "eighths_3000", "straddle", "starts_on_last", "run_L", "run_L_plus_1", "run_L_from_last", "bar_mix",
                f"distinct_{W + 1}", "equal_2500"):
        for labels in ("flipped_20", "random_20", "random_32"):
            _check(eps, dev, name, PROFILES[name], labels, rng)


# ---- the step --------------------------------------------------------------------------------------------------------------------
def _step(scan, g, wt, k, relabel, tail, monkeypatch):
    monkeypatch.setattr(scan, "TAIL_SORT", tail)
    st = {}
    pairs, scores = scan.scan_topk(g, wt, k, relabel=relabel, stats=st)
    return pairs, scores, st


@pytest.mark.parametrize("kind", ["aa", "ra", "cn"])
def test_scan_topk_default_tail_equals_library_tail(eps, dev, kind, monkeypatch):
    """scan_topk with the default tail (TAIL_SORT = "score") == the library tail: the same rows, scores and status counts, as
    labelled and under hubs-first labels with skipped heads.  ``rows_path``: common neighbours are a Screen.exact list, which the
    score sort leaves to the library ordering; Adamic-Adar and resource allocation are asserted to take the score sort: their
    scores are float32 sums of 1 / ln d (1 / d) over the common neighbours, and among the best 100 000 pairs of this graph -- hub
    pairs with tens of common neighbours of assorted degrees -- equal sums are rare: the longest run of equal scores among the
    returned rows is 3 pairs for Adamic-Adar and 504 for resource allocation at K = 200 001, 1 pair at K = 5000, against a limit
    of 1024.  The run length is asserted next to the path, so a failure says which of the two broke."""
    from eps_amd import scan, synth
    from eps_amd.heuristics import node_weight_table
    assert scan.TAIL_SORT == "score" and scan.TAIL_DEVICE
    g = synth.rmat_graph(15, 14, 7, dev)
    wt = (torch.ones(g.n_rows, dtype=torch.float32, device=dev) if kind == "cn" else
          node_weight_table(g, {"aa": eps.ops.W_AA, "ra": eps.ops.W_RA}[kind]))
    monkeypatch.setattr(scan, "SMALL_SET", 0)
    monkeypatch.setattr(scan, "RELABEL_MIN_NODES", 0)
    monkeypatch.setattr(scan, "HEAD_MIN_PATHS", 0)
    for relabel in (False, True):
        for k in (1, 5000, 200_001):
            # (the tail without the device selections first, as test_gpu_tail.py does: a graph object's FIRST scan runs with a narrower
            #  hub table than its later ones and touches a different number of candidates, whatever the tail)
            monkeypatch.setattr(scan, "TAIL_DEVICE", False)
            rp, rs, _ = _step(scan, g, wt, k, relabel, "library", monkeypatch)
            monkeypatch.setattr(scan, "TAIL_DEVICE", True)
            pairs, scores, st = _step(scan, g, wt, k, relabel, "score", monkeypatch)
            lp, ls, lst = _step(scan, g, wt, k, relabel, "library", monkeypatch)
            case = (kind, relabel, k)
            assert torch.equal(pairs, lp) and torch.equal(scores.view(torch.int32), ls.view(torch.int32)), case
            assert torch.equal(pairs, rp) and torch.equal(scores.view(torch.int32), rs.view(torch.int32)), case
            for key in ("survivors", "launches", "touched", "survivor_slots", "candidates", "rescored"):
                assert st[key] == lst[key], (case, key)
            longest = int(torch.unique_consecutive(scores, return_counts=True)[1].max()) // 2
            print(kind, relabel, k, "rows_path", st["rows_path"], "longest run of equal scores", longest, "pairs")
            assert lst["rows_path"] == "library"
            if kind == "cn":
                assert st["rows_path"] == "library", case
            else:
                assert longest <= L and st["rows_path"] == "score", (case, longest)
    assert _state_is_clean(eps, dev)


def test_scan_topk_falls_back_on_a_heavily_tied_list(eps, dev, monkeypatch):
    """A complete bipartite block of 128 + 128 fresh nodes next to a small R-MAT graph: every pair inside either side has the same 128
    common neighbours of degree 128, so 16 256 pairs share the Adamic-Adar score 128 / ln 128 = 26.4 -- one run, far longer than the
    kernel orders, high enough to be among the 10 000 best pairs.  The flag is set, the rows come from the library ordering and
    equal the library tail's."""
    from eps_amd import scan, synth
    from eps_amd.graph import CSRGraph
    from eps_amd.heuristics import node_weight_table
    base = synth.rmat_graph(12, 8, 2, "cpu")
    n = base.n_rows
    row = torch.repeat_interleave(torch.arange(n), base.rowptr[1:] - base.rowptr[:-1])
    a, b = torch.meshgrid(torch.arange(n, n + 128), torch.arange(n + 128, n + 256), indexing="ij")
    ei = torch.cat([torch.stack([row, base.col.long()]), torch.stack([a.reshape(-1), b.reshape(-1)]),
                    torch.stack([b.reshape(-1), a.reshape(-1)])], 1)
    g = CSRGraph.from_edge_index(ei, None, (n + 256, n + 256)).to(dev)
    wt = node_weight_table(g, eps.ops.W_AA)
    monkeypatch.setattr(scan, "SMALL_SET", 0)
    k = 20_000
    monkeypatch.setattr(scan, "TAIL_DEVICE", False)               # (a graph object's first scan touches a different number of candidates)
    rp, rs, _ = _step(scan, g, wt, k, False, "library", monkeypatch)
    monkeypatch.setattr(scan, "TAIL_DEVICE", True)
    pairs, scores, st = _step(scan, g, wt, k, False, "score", monkeypatch)
    lp, ls, lst = _step(scan, g, wt, k, False, "library", monkeypatch)
    tied = int(torch.unique_consecutive(scores, return_counts=True)[1].max()) // 2
    print("rows_path", st["rows_path"], "longest run among the rows", tied, "pairs; bar", st["bar"])
    assert st["bar"] is not None, "the step is meant to run the device tail (under a bar)"
    assert tied > L and st["rows_path"] == "library" and lst["rows_path"] == "library"
    assert pairs.shape == (2, k) and torch.equal(pairs, lp) and torch.equal(scores.view(torch.int32), ls.view(torch.int32))
    assert torch.equal(pairs, rp) and torch.equal(scores.view(torch.int32), rs.view(torch.int32))
    for key in ("survivors", "launches", "touched", "survivor_slots"):
        assert st[key] == lst[key], key
    assert _state_is_clean(eps, dev)
