"""The stored-value (weighted) scoring path at values whose float32 products ROUND, against tests/weighted_truth.py (plain numpy,
held to a triple loop by tests/test_weighted_truth_host.py).  The suite's other weighted graphs carry small integers, whose
products are exact, so none of the following had met a rounding before:

  * eps_expand_fill, eps_rescore_weighted and scan_topk return float32 of the int64 sum of the 2^-40 fixed-point terms
    fl(fl(A[u,w] A[v,w]) node_w[w]) -- bit for bit the truth's;
  * the piece kernel's screening score s (csrc/scan_pieces.hip, HV flavour) is an upper bound of the exact score -- it keeps a pair
    only when s exceeds the bar, so a screening score below the exact one would lose a pair silently;
  * Screen.lower_bound(s) stays below the exact score (the pre-filter in front of the re-scoring rests on it);
  * candidates.fused_score_bound is an upper bound of every score; ops.pair_scores stays within the rounding of its float32 sum.

Cases: weighted_truth.cases() -- two graphs (an R-MAT of 2048 nodes with hub rows of several hundred entries, an Erdos-Renyi graph
of 300 nodes whose rows all fit one wave) x five value families x four node-weight tables, without the combinations the scan
refuses (weighted_truth.REMOVED says why).  Every test prints what it measured as one line that starts with "WV".

What was measured on an MI355X stands in the docstrings of the tests below."""
import numpy as np
import pytest
import torch

import weighted_truth as W

pytestmark = pytest.mark.gpu

CASES = W.cases()
_WORLD = {}


class Case:
    """One (graph, family, table): the host truth and the same arrays on the device."""

    def __init__(self, eps, oracle, dev, name, family, table):
        from eps_amd import synth
        if "graphs" not in _WORLD:
            _WORLD["graphs"] = W.graphs(synth)
            _WORLD["paths"], _WORLD["dev"] = {}, {}
        h = _WORLD["graphs"][(name, family)]
        if name not in _WORLD["paths"]:
            _WORLD["paths"][name] = W.paths(h.rowptr, h.col)
        if (name, family) not in _WORLD["dev"]:
            _WORLD["dev"][(name, family)] = eps.CSRGraph(torch.from_numpy(h.rowptr).to(dev), torch.from_numpy(h.col.astype(np.int32)).to(dev),
                                                       torch.from_numpy(h.val).to(dev), h.n, h.n)
        self.h, self.g = h, _WORLD["dev"][(name, family)]
        self.w = W.node_table(oracle, h, table)
        self.wt = torch.from_numpy(self.w).to(dev)
        self.t = W.Truth(h, self.w, _WORLD["paths"][name])
        self.tag = f"{name} {family} {table}"
        self.dev = dev
        self._launch = {}

    def keys_dev(self, keys):
        return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int64)).to(self.dev)

    def launch(self, bar=None):
        """ONE launch of the piece kernel over the graph as it is, without a bar or under ``bar`` (cached):
        (Screen, keys, s float32 tensor, candidates counted)."""
        from eps_amd import scan
        if bar not in self._launch:
            g = self.g
            sc = scan.screen_weights(g, g, None, self.wt)
            assert sc.usable and scan.screen_variant(g) is not None
            capacity = scan._capacity(2 * scan.total_half_paths(g), scan._PIECE_SLACK)
            res = scan._launch(g, None, scan.column_order(g), float("-inf") if bar is None else bar, capacity, screen=sc)
            assert int(res.status) == 0
            slots, n_cand = res.counts()
            keys, s32 = res.valid(slots)
            self._launch[bar] = (sc, keys.cpu().numpy(), s32, n_cand)
        return self._launch[bar]

    def bar(self):
        """The truth's 500th best score."""
        return float(np.sort(self.t.scores)[::-1][499])


@pytest.fixture
def case(eps, oracle, dev, request):
    key = request.param
    if key not in _WORLD:
        _WORLD[key] = Case(eps, oracle, dev, *key)
    return _WORLD[key]


def _ids(c):
    return "-".join(c)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


per_case = pytest.mark.parametrize("case", CASES, indirect=True, ids=_ids)


def test_every_case_is_usable(eps, oracle, dev):
    """scan.scan_usable takes every case of the table (a combination it refuses is removed in the helper, with the reason)."""
    from eps_amd import scan
    for key in CASES:
        if key not in _WORLD:
            _WORLD[key] = Case(eps, oracle, dev, *key)
        c = _WORLD[key]
        assert scan.values_symmetric(c.g) and scan.scan_usable(c.g, c.wt), c.tag
    assert len(CASES) == 26


# ------------------------------------------------------------------------------------------------- a. the fused expansion
@per_case
def test_expand_candidates_is_the_truth(eps, case):
    g, t = case.g, case.t
    _, cu, cv, _, sc = eps.ops.expand_candidates(g.rowptr, g.col, g.val, case.wt, g.n_rows, 0, g.n_rows, want_cn=False)
    cu, cv, sc = cu.cpu().numpy().astype(np.int64), cv.cpu().numpy().astype(np.int64), sc.cpu().numpy()
    assert len(cu) == 2 * len(t.keys)
    for half in (cu < cv, cu > cv):
        lo, hi, s = np.minimum(cu, cv)[half], np.maximum(cu, cv)[half], sc[half]
        key = (hi << 32) | lo
        o = np.argsort(key, kind="stable")
        assert np.array_equal(key[o], t.keys), "the candidate set differs from the truth's"
        assert np.array_equal(_bits(s[o]), _bits(t.scores)), ("scores differ in bits", int((_bits(s[o]) != _bits(t.scores)).sum()))


# ------------------------------------------------------------------------------------------------- b. the weighted re-scoring
@per_case
def test_rescore_weighted_is_the_truth(eps, dev, case):
    g, t, h = case.g, case.t, case.h
    rng = np.random.default_rng(11)

    def rescore(keys):
        return eps.ops.rescore_weighted(g.rowptr, g.col, g.val, case.wt, g.n_rows, case.keys_dev(keys)).cpu().numpy()

    # all candidates in shuffled order, and with u and v swapped in the key (the term is symmetric)
    p = rng.permutation(len(t.keys))
    assert np.array_equal(_bits(rescore(t.keys[p])), _bits(t.scores[p]))
    assert np.array_equal(_bits(rescore((t.u[p] << 32) | t.v[p])), _bits(t.scores[p]))
    # lists that are no multiple of the four waves of a workgroup
    for m in (1, 3, 5):
        assert np.array_equal(_bits(rescore(t.keys[p[:m]])), _bits(t.scores[p[:m]])), m
    # more pairs than 4 waves x 8 workgroups per CU: the grid-stride loop
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus == eps.ops.device_info()[0]
    reps = -(-(4 * 8 * cus + 1) // len(t.keys))
    many = np.tile(p, reps)
    assert len(many) > 4 * 8 * cus
    if reps > 1:
        assert np.array_equal(_bits(rescore(t.keys[many])), _bits(t.scores[many]))
    # pairs that are no candidates: no common neighbour (score 0.0 exactly), u == v, two hub rows, two rows of equal length
    n, deg = h.n, h.degree()
    a, b = rng.integers(0, n, 4000), rng.integers(0, n, 4000)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    apart = (lo != hi) & ~W.is_edge(h.rowptr, h.col, lo, hi) & ~np.isin((hi << 32) | lo, t.keys)
    lo, hi = lo[apart], hi[apart]
    assert len(lo) > 100
    got = rescore(np.concatenate([(hi << 32) | lo, (lo << 32) | hi]))
    assert np.array_equal(_bits(got), np.zeros(2 * len(lo), np.int32)), "a pair without a common neighbour does not score +0.0"
    by_deg = np.argsort(-deg, kind="stable")
    same = np.flatnonzero(deg[t.u] == deg[t.v])
    assert len(same) and deg[t.u[same]].max() > 1
    e = same[np.argmax(deg[t.u[same]])]
    odd = [(int(x), int(x)) for x in (by_deg[0], by_deg[1], by_deg[n // 2], by_deg[-1])]
    odd += [(int(by_deg[i]), int(by_deg[j])) for i in range(4) for j in range(4) if i != j]          # (hub rows: > 64 entries on rmat11)
    odd += [(int(t.u[e]), int(t.v[e])), (int(t.v[e]), int(t.u[e]))]
    if h.n > 1000:
        assert deg[by_deg[3]] > 64
    want = np.array([W.pair_exact(h.rowptr, h.col, h.val, case.w, u, v) for u, v in odd], np.float32)
    got = rescore(np.array([(u << 32) | v for u, v in odd], np.int64))
    assert np.array_equal(_bits(got), _bits(want)), (odd, got, want)
    assert (want[:2] > 0).all()


# ------------------------------------------------------------------------------------------------- c. no silent loss
@per_case
def test_screening_score_is_an_upper_bound(eps, case):
    """One launch without a bar reports every candidate once, and -- in float64 -- exact <= s (1 + 2^-23) for each of them (2^-23:
    the float32 rounding of s, half an ulp, with room: the margin of the unit-valued test in test_gpu_scan_tables.py).

    Largest exact / s seen on an MI355X, per family over both graphs and all tables: ints 0.999999191, mantissa 0.999999223,
    wide 0.999999259, tiny 0.999996527, big_scores 0.999999198 -- the 2^-20 inflation of the row factor, less three roundings."""
    t = case.t
    sc, keys, s32, n_cand = case.launch()
    assert len(np.unique(keys)) == len(keys), "a pair reported twice"
    assert n_cand == len(t.keys)
    o = np.argsort(keys)
    assert np.array_equal(keys[o], t.keys), "the survivors of a launch without a bar are not the candidate set"
    s = s32.double().cpu().numpy()[o]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(s > 0, t.exact64 / s, 0.0)
    print("WV up", case.tag, "shift", sc.shift, "pairs", len(keys), "max exact/s %.9f" % ratio.max(),
          "top s units %.4g" % (s.max() * 2.0 ** sc.shift))
    up = t.exact64 <= s * (1 + 2.0 ** -23)
    assert up.all(), ("a screening score below the exact one", int((~up).sum()))


@per_case
def test_no_pair_above_a_bar_is_lost(eps, case):
    """The same launch under a bar, the truth's 500th best score: every pair whose exact score exceeds the bar is among the
    survivors, and every survivor's screening score is an upper bound of its exact score there too."""
    t, bar = case.t, case.bar()
    sc, bk, bs, n_cand = case.launch(bar)
    bs = bs.cpu().numpy()
    assert n_cand == len(t.keys) and len(np.unique(bk)) == len(bk)
    must = t.keys[t.scores > np.float32(bar)]
    assert 0 < len(must) <= 499
    assert np.isin(must, bk).all(), ("a pair above the bar was lost", int((~np.isin(must, bk)).sum()))
    assert (t.exact64[t.at(bk)] <= bs.astype(np.float64) * (1 + 2.0 ** -23)).all()
    print("WV bar", case.tag, "bar %.6g" % bar, "above it", len(must), "survivors", len(bk))


@per_case
def test_every_survivor_exceeds_the_bar(eps, case):
    """Every survivor of the launch under the bar has s > bar: the launches over stored values round the bar UP to a whole
    screening unit (sp_bar_units, csrc/scan_common.h).  With the bar rounded down, as the unit-valued launches and eps_scan_refine
    take it, er300-tiny-ones reported one pair of 509 at s = 1529 units under a bar of 1529.018 (measured on an MI355X)."""
    bar = case.bar()
    sc, bk, bs, _ = case.launch(bar)
    bs = bs.cpu().numpy()
    at_or_below = bs <= np.float32(bar)
    print("WV strict", case.tag, "shift", sc.shift, "bar units %.3f" % (bar * 2.0 ** sc.shift), "survivors", len(bk), "with s <= bar", int(at_or_below.sum()),
          "lowest s units %.1f" % (float(bs.min()) * 2.0 ** sc.shift if len(bs) else 0.0))
    assert not at_or_below.any(), ("a survivor that does not exceed the bar", int(at_or_below.sum()))


# ------------------------------------------------------------------------------------------------- d. the bound under the bar
@per_case
def test_lower_bound_stays_below_the_exact_score(eps, case):
    """Screen.lower_bound(s) (1 - 2^-22) <= exact for every candidate of the launch above (2^-22: the rounding of s plus the two
    float32 operations of the bound's own arithmetic, as in the unit-valued test).

    Smallest exact / lower_bound seen on an MI355X, per family over both graphs and all tables: ints 1.000012602, mantissa
    1.000007713, wide 1.000016218, tiny 1.004562587, big_scores 1.000002983.  Before lower_params allowed for the relative
    inflation of the screening terms (2^12 units on top of 4 per path) the 300-node graph -- rows of at most 30 entries, so only 120
    units were subtracted -- failed in 12 of its 15 cases, the integer-valued control among them: ints 0.999999403, mantissa
    0.999999236, wide 0.999999489, big_scores 0.999999168 (tiny held at 1.000304831: its sums use 19 bits of the word)."""
    from eps_amd import scan
    t = case.t
    sc, keys, s32, _ = case.launch()
    o = np.argsort(keys)
    low = sc.lower_bound(s32, scan.max_degree(case.g)).double().cpu().numpy()[o]
    a, b = sc.lower_params(scan.max_degree(case.g))
    pos = low > 0
    tightest = float((t.exact64[pos] / low[pos]).min()) if pos.any() else float("inf")
    print("WV down", case.tag, "shift", sc.shift, "a units %.1f" % (a * 2.0 ** sc.shift), "b", b, "bounds above 0", int(pos.sum()),
          "min exact/low %.9f" % tightest)
    down = low * (1 - 2.0 ** -22) <= t.exact64
    assert down.all(), ("lower_bound above the exact score", int((~down).sum()), tightest)
    assert b == 0.0 or 0.0 < b < 1.0


# ------------------------------------------------------------------------------------------------- e. scan_topk
@per_case
def test_scan_topk_is_the_truth(eps, case, monkeypatch):
    """scan_topk returns DIRECTED rows (each pair both ways round): against the truth's pairs, each taken twice."""
    from eps_amd import scan
    g, t = case.g, case.t
    dkeys = np.concatenate([(t.u << 32) | t.v, (t.v << 32) | t.u])               # (u << 32 | v of a directed row (u, v))
    dscore = np.concatenate([t.scores, t.scores])
    best = np.sort(dscore)[::-1]
    small_set = scan.SMALL_SET
    for patched in (small_set, 0):
        monkeypatch.setattr(scan, "SMALL_SET", patched)
        for k in (1, 500, len(dkeys)):
            st = {}
            pairs, scores = scan.scan_topk(g, case.wt, k, stats=st)
            pairs, scores = pairs.cpu().numpy(), scores.cpu().numpy()
            assert st["candidates"] == len(dkeys), (patched, k)
            assert pairs.shape == (2, k) and np.array_equal(_bits(scores), _bits(best[:k])), (case.tag, patched, k)
            rows = (pairs[0] << 32) | pairs[1]
            assert len(np.unique(rows)) == k
            kth = best[k - 1]
            assert np.array_equal(np.sort(rows[scores > kth]), np.sort(dkeys[dscore > kth])), (patched, k)
            assert np.isin(rows[scores == kth], dkeys[dscore == kth]).all(), (patched, k)


# ------------------------------------------------------------------------------------------------- f. the score bound
@per_case
def test_fused_score_bound(eps, case):
    from eps_amd import candidates
    bound = candidates.fused_score_bound(case.g, case.wt)
    formula = W.bound_formula(case.h, case.w)
    print("WV bound", case.tag, "bound / formula - 1 = %.3e" % (bound / formula - 1), "formula / best score %.3f" % (formula / case.t.real.max()))
    assert bound >= case.t.real.max()
    assert bound >= formula * (1 - 2.0 ** -22)
    assert bound <= 2 * formula


# ------------------------------------------------------------------------------------------------- g. the pair kernel
@per_case
@pytest.mark.parametrize("grouped", (False, True))
def test_pair_scores_with_stored_values(eps, oracle, case, grouped):
    """ops.pair_scores sums float32 terms a_u (a_v w) -- two roundings each, 2^-24 relative apiece -- in float32: the p terms of a
    pair are positive, so whatever the order of the additions the sum is within (2 + (p - 1)) 2^-24 < (p + 2) 2^-23 of the real one."""
    g, t, h = case.g, case.t, case.h
    u = torch.from_numpy(t.u.astype(np.int32)).to(case.dev)
    v = torch.from_numpy(t.v.astype(np.int32)).to(case.dev)               # (the truth's keys ascend: sorted by v)
    count, _, ws = eps.ops.pair_scores(g.rowptr, g.col, g.val, case.wt, g.n_rows, u, v, grouped=grouped)
    cnt_o, ws_o = oracle.pair_scores_f64(h.rowptr, h.col.astype(np.int32), h.val, case.w.astype(np.float64), t.u, t.v)
    assert np.array_equal(count.cpu().numpy(), t.counts) and np.array_equal(cnt_o, t.counts)
    assert np.allclose(ws_o, t.real, rtol=1e-13, atol=0)
    err = np.abs(ws.double().cpu().numpy() - ws_o)
    allowed = (t.counts + 2) * 2.0 ** -23 * t.real
    zero = allowed == 0
    assert (err[zero] == 0).all()
    worst = float((err[~zero] / allowed[~zero]).max())
    print("WV pair", case.tag, "grouped", grouped, "max error / allowed %.4f" % worst)
    assert worst <= 1.0
