"""CPU: the zone rule of the main scan launch -- eps_amd.scan.lean_columns / zone_order (torch) and its restatement in plain loops
(tests/scan_split_truth.py) against lists worked out by hand: the row bound on both sides, every record kind in first, middle and
last place, the unit-bitmap bound met exactly and missed by one path, a light column, empty and one-column zones, and the order
inside every zone."""
import numpy as np
import torch

import scan_split_truth as st

K00, K01, K10, K11 = 0, 1, 2, 3


def _plan(columns):
    """rows [N], pptr [N + 1], recs [P, 4] of columns given as (rows, [(kind, paths), ...])."""
    rows = [r for r, _ in columns]
    pptr, recs = [0], []
    for _, pieces in columns:
        for kind, paths in pieces:
            recs.append([paths | (kind << 30), 0, 0, 0])
        pptr.append(len(recs))
    return np.array(rows, np.int64), np.array(pptr, np.int64), np.array(recs, np.int64).reshape(-1, 4)


def _both(columns):
    from eps_amd import scan
    rows, pptr, recs = _plan(columns)
    truth = st.lean_ok(rows, pptr, recs)
    got = scan.lean_columns(torch.from_numpy(rows), torch.from_numpy(pptr), torch.from_numpy(recs)).numpy()
    assert np.array_equal(got, truth), (got, truth)
    return truth.tolist()


def test_constants_agree_with_the_host_module():
    from eps_amd import scan
    assert (scan.LEAN_ROWS, scan.LEAN_UNITS) == (st.ROWS, st.UBITS) == (256, 8192)


def test_row_bound():
    assert _both([(256, [(K11, 10)]), (257, [(K11, 10)]), (1, [(K10, 1)]), (0, [])]) == [True, False, True, True]


def test_record_kinds_in_every_place():
    good = (K01, K10, K11)
    cases, want = [], []
    for place in range(3):
        for kind in (K00, K01, K10, K11):
            pieces = [(good[(place + i) % 3], 100 + i) for i in range(3)]
            pieces[place] = (kind, 50)
            cases.append((12, pieces))
            want.append(kind != K00)
    assert _both(cases) == want
    # one record alone, of each kind
    assert _both([(5, [(k, 7)]) for k in (K00, K01, K10, K11)]) == [False, True, True, True]


def test_unit_bitmap_bound_exact_and_one_over():
    for rows in (1, 7, 256):
        edge = 4 * st.UBITS - 3 * rows
        assert _both([(rows, [(K01, edge)]), (rows, [(K01, edge + 1)]), (rows, [(K11, 5), (K10, edge), (K01, 9)]),
                      (rows, [(K11, 5), (K10, 9), (K01, edge + 1)])]) == [True, False, True, False]


def _order(columns, light, lean):
    from eps_amd import scan
    order, lean_from, light_from = scan.zone_order(torch.tensor(light, dtype=torch.bool), torch.tensor(lean, dtype=torch.bool))
    got = [columns[i] for i in order.tolist()]
    want = st.zones(columns, light, lean)
    assert (got, lean_from, light_from) == want, ((got, lean_from, light_from), want)
    return want


def test_zones_keep_their_order_and_light_wins():
    cols = [40, 41, 42, 43, 44, 45, 46, 47]
    light = [False, True, False, False, True, False, False, True]
    lean = [True, True, False, True, False, False, True, True]          # (41 and 47 are light AND admissible: light wins)
    assert _order(cols, light, lean) == ([42, 45, 40, 43, 46, 41, 44, 47], 2, 5)


def test_empty_and_one_column_zones():
    assert _order([7, 8, 9], [False] * 3, [False] * 3) == ([7, 8, 9], 3, 3)           # general only
    assert _order([7, 8, 9], [False] * 3, [True] * 3) == ([7, 8, 9], 0, 3)            # lean only
    assert _order([7, 8, 9], [True] * 3, [True] * 3) == ([7, 8, 9], 0, 0)             # light only
    assert _order([7, 8, 9], [False, False, True], [False, True, False]) == ([7, 8, 9], 1, 2)      # one of each
    assert _order([7, 8, 9], [True, False, False], [False, False, True]) == ([8, 9, 7], 1, 2)
    assert _order([7], [False], [True]) == ([7], 0, 1)
    assert _order([], [], []) == ([], 0, 0)


def test_light_split_views():
    """LightSplit's views are the zones of its list; no lean zone given: lean_from = light_from, an empty lean view."""
    from eps_amd import scan
    cols = torch.arange(10, dtype=torch.int32)
    s = scan.LightSplit(cols, cols, 7, 3)
    assert s.main.tolist() == [0, 1, 2] and s.lean.tolist() == [3, 4, 5, 6] and (s.lean_from, s.light_from) == (3, 7)
    s = scan.LightSplit(cols, cols, 7)
    assert s.main.tolist() == list(range(7)) and s.lean.numel() == 0 and s.lean_from == 7
    s = scan.LightSplit(cols, cols, 10)
    assert s.main is cols and s.lean.numel() == 0


def test_a_zone_backstop_repeats_the_launch_without_zones():
    """scan._Retry.verdict: the backstop bit of a launch WITH zones repeats the same launch without them (it does not count twice);
    without zones the bit stays what it was, a full hash table; the sketch set is looked at first."""
    import pytest
    from eps_amd import ops, scan
    bits = lambda x: int(np.float32(x).view(np.int32))                    # noqa: E731
    row = lambda status: scan.StepStatus(100, 5000, 60, bits(1.0), status, bits(float("-inf")), 0, bits(0.5))      # noqa: E731
    args = dict(capacity=1000, walked_cap=100, head_budget=None, shift=None, screened=True, k2=50, bar_set=True)
    state = scan._Retry(launches=2, wanted=400, head_list=2, use_heads=True, sketch=True)
    assert state.zones
    v = state.verdict([row(2 | 16)], zoned=True, **args)
    assert (v.action, v.launches) == ("zones off", 1)
    assert state.apply(v, 1000, 1) == "keep" and not state.zones and state.sketch
    with pytest.raises(ops._lib.EpsError, match="full hash table"):
        state.verdict([row(2 | 16)], zoned=False, **args)
    with pytest.raises(ops._lib.EpsError, match="full hash table"):
        state.verdict([row(2 | 16)], **args)
    with pytest.raises(ops._lib.EpsError, match="full hash table"):
        state.verdict([row(32)], zoned=True, **args)
    assert state.verdict([row(8 | 2)], zoned=True, **args).action == "sketch off"
    assert state.verdict([row(16)], zoned=True, **args).action == "done"
