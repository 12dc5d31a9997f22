"""rescore_runs_kernel (csrc/rescore.hip) at the edges of its trip: a half wave takes 256 entries of a row N(v) per trip as two
16-byte loads a lane, reads the eight bitmap words of a lane unconditionally, loads the weights of the hits through a buffer
descriptor, and takes (first entry, length) of every row of a 256-pair chunk from LDS words written once per chunk.  Truth as in
test_gpu_rescore_paths.py: numpy int64 sums of fixw over N(u) & N(v), float32(float64(sum) * 2^-40), compared bit for bit
(the sums stay below 2^53, asserted: the float64 is exact).

The graph is built by hand (a CSR with ascending rows; the kernel reads nothing else), unit values:
  * rows N(v) of 0, 1, 3, 4, 5, 127, 128, 129, 255, 256, 257, 511, 512, 513 and 1025 entries -- around the 4 entries of a load, the 128
    of a half wave's load, the 256 of a trip and the 512 of the short-row threshold -- once WITH node 0 in them and once WITHOUT.
    Every long row N(u) but one holds node 0.  A lane past the end of a row reads zeros from the descriptor over col[], which is
    id 0: in the set WITHOUT node 0 such a lane would count a neighbour that is not there, were the row's end not part of the hit.
  * the last row of col[] (the end of the descriptor's range) with lengths = 1, 2, 3 mod 4: three graphs that differ in that row;
  * rows that start at every residue mod 4 of the entry index (asserted on the graph);
  * a row that is a subset of N(u), one that shares nothing with it, one with ~1000 common neighbours;
  * weights with bits on both sides of bit 32 of the 2^-40 fixed point (3.000000001-like values, two just under 2^11), so that
    the 64-bit adds carry across the word boundary.
The key lists put half-wave partners of very different length side by side (a wave scores pairs s + 2w and s + 2w + 1 of a run),
runs of 1, 2, 31, 32, 33 and odd numbers of pairs, runs inside a chunk, across a chunk edge, ending on one, a run of exactly one
chunk, and a run of a lighter u directly behind a run of a heavier one in the same chunk (a descriptor or a bitmap bit left over
would show).  Both entries run every list, eps_rescore_runs_dev with a count below the list's length and a sentinel behind it.

The same lists run on the small world declared as RS_BITS and RS_BITS + 1 nodes and on its monotone relabelling into an id space
of 2 RS_BITS + 77 nodes (three id windows, rows with entries on both sides of the first window edge and in the last window): the
kernel has one instantiation for an id space of one window and one for a wider space.  Sizes come from ops.rescore_limits()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4200
LENGTHS = (0, 1, 3, 4, 5, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)
U1, U2, U3 = 3000, 3001, 3002                 # long rows: 1300 and 700 entries with node 0, 2000 entries without
V_WITH, V_WITHOUT = 3100, 3200                # + index into LENGTHS: rows N(v) with / without node 0
V_SUB, V_DIS, V_BIG = 3300, 3301, 3302        # subset of N(U1); disjoint from N(U1); ~1000 common neighbours with N(U3)
TAIL = N - 1                                  # the last row of col[]
TAIL_LENGTHS = (5, 130, 1027)                 # = 1, 2, 3 mod 4
FAR = np.arange(4130, 4161)                   # neighbour ids that the wide relabelling puts into the last window
SENTINEL = -7.0
LISTS = ["lengths_with_0", "lengths_without_0", "partners", "run_sizes", "chunk_edges", "special_rows", "tail"]


def _rows(rng, tail_len):
    pool = np.concatenate([np.arange(1, 3000), FAR])
    pick = lambda k, src=pool: np.sort(rng.choice(src, k, replace=False))          # noqa: E731
    rows = {U1: np.concatenate([[0], pick(1299)]), U2: np.concatenate([[0], pick(699)]), U3: pick(2000)}
    for k, ln in enumerate(LENGTHS):
        if ln:
            rows[V_WITH + k] = np.concatenate([[0], pick(ln - 1)])
        rows[V_WITHOUT + k] = pick(ln)
    rows[V_SUB] = pick(400, rows[U1])
    rows[V_DIS] = pick(300, np.setdiff1d(pool, rows[U1]))
    rows[V_BIG] = np.sort(np.concatenate([pick(1000, rows[U3]), pick(25, np.setdiff1d(pool, rows[U3]))]))
    rows[TAIL] = pick(tail_len)
    return rows


def _csr(rows, n):
    deg = np.zeros(n, dtype=np.int64)
    for r, c in rows.items():
        deg[r] = len(c)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.concatenate([rows[r] for r in sorted(rows)]).astype(np.int32)
    assert col.size == rowptr[-1] and all((np.diff(c) > 0).all() for c in rows.values() if len(c) > 1)
    return rowptr, col


def _keys(u, v):
    return (np.asarray(u, dtype=np.int64) << 32) | np.asarray(v, dtype=np.int64)


def _runs(*runs):
    """[(u, [v, ...]), ...] -> keys, the runs in the order given (the kernel needs runs of equal u, not an ascending list)."""
    return np.concatenate([_keys(np.full(len(v), u), v) for u, v in runs])


def _lists(rng, rows, chunk):
    with_0 = [V_WITH + k for k, ln in enumerate(LENGTHS) if ln]
    without_0 = [V_WITHOUT + k for k in range(len(LENGTHS))]
    wo = {ln: V_WITHOUT + k for k, ln in enumerate(LENGTHS)}
    any_v = np.array(with_0 + without_0 + [V_SUB, V_DIS, V_BIG, TAIL, U1, U2, U3])
    draw = lambda k: rng.choice(any_v, k).tolist()                                   # noqa: E731
    lists = {
        "lengths_with_0": _runs((U1, with_0), (U2, with_0), (U3, with_0)),
        "lengths_without_0": _runs((U1, without_0), (U2, without_0), (U3, without_0)),
        # pairs 2j and 2j + 1 of a run share a wave: 1 entry next to 1025, 0 next to 513, both ways round, and an odd run
        "partners": _runs((U1, [wo[1], wo[1025], wo[0], wo[513], wo[1025], wo[1], wo[513], wo[0]]),
                          (U2, [wo[1025], wo[0], wo[3], wo[257], wo[1]])),
        "run_sizes": _runs((U1, draw(1)), (U2, draw(2)), (U1, draw(31)), (U2, draw(32)), (U1, draw(33)), (U3, draw(7))),
        # inside chunk 0; across the edge at 256; ending on the edge at 512; exactly chunk 2; then, inside chunk 3, the run of
        # U2 (700 entries) behind the run of U3 (2000), on rows full of N(U3): V_BIG, U3 itself
        "chunk_edges": _runs((U1, draw(100)), (U2, draw(200)), (U3, draw(2 * chunk - 300)), (U1, draw(chunk)),
                             (U3, draw(40)), (U2, [V_BIG, U3, V_BIG] + draw(30)), (U1, draw(9))),
        "special_rows": _runs((U1, [V_SUB, V_DIS, V_BIG]), (U3, [V_BIG, V_SUB, V_DIS, U3]), (V_WITH + 5, [U1, V_BIG]),
                              (U2, [V_DIS, V_SUB])),
        "tail": _runs((U1, [TAIL]), (U2, [TAIL, wo[1025]]), (U3, [wo[513], TAIL, TAIL])),
    }
    assert lists["chunk_edges"].size == 3 * chunk + 40 + 33 + 9 and set(lists) == set(LISTS)
    return lists


def _reference(rowptr, col, fixw, keys):
    out = np.empty(keys.size, dtype=np.float32)
    top = 0
    for i, k in enumerate(keys):
        u, v = int(k >> 32), int(k & 0xFFFFFFFF)
        both = np.intersect1d(col[rowptr[u]:rowptr[u + 1]], col[rowptr[v]:rowptr[v + 1]], assume_unique=True)
        s = int(fixw[both].sum(dtype=np.int64))
        top = max(top, s)
        out[i] = np.float32(np.float64(s) * 2.0 ** -40)
    assert top < 1 << 53, "an int64 sum of these weights is not exact in float64"
    return out


def _weights(rng):
    """2^-40 fixed point: values in [1, 3.1) with random low bits (3.000000001 among them), two just under 2^11."""
    fixw = rng.integers(1 << 40, int(3.1 * 2 ** 40), N, dtype=np.int64)
    fixw[1:6] = int(round(3.000000001 * 2 ** 40))
    fixw[0] = (1 << 51) - 12345                       # node 0, the one a lane past a row's end would count
    fixw[7] = (1 << 51) - 1
    assert ((fixw >> 32) > 0).all() and ((fixw & 0xFFFFFFFF) > 0).all()
    return fixw


@pytest.fixture(scope="module")
def limits(eps):
    bits, short, chunk = eps.ops.rescore_limits()
    assert short == 512 and chunk == 256, "LENGTHS and the lists are laid around these"
    return bits, short, chunk


@pytest.fixture(scope="module")
def worlds(dev, limits):
    """One small world per tail length: the graph, the weights, every list with its host sums (computed once)."""
    bits, short, chunk = limits
    t = lambda a: torch.from_numpy(a).to(dev)                                       # noqa: E731
    out = {}
    for tail_len in TAIL_LENGTHS:
        rng = np.random.default_rng(20241021)
        rows = _rows(rng, tail_len)
        rowptr, col = _csr(rows, N)
        fixw = _weights(rng)
        lists = _lists(rng, rows, chunk)
        if tail_len != TAIL_LENGTHS[0]:
            lists = {"tail": lists["tail"]}
        deg = np.diff(rowptr)
        assert deg[U1] > short and deg[U2] > short and deg[U3] > short and rowptr[TAIL + 1] == col.size and deg[TAIL] == tail_len
        assert 0 in rows[U1] and 0 in rows[U2] and 0 not in rows[U3] and 0 not in rows[TAIL]
        assert all(0 not in rows[V_WITHOUT + k] for k in range(len(LENGTHS)))
        v_rows = [r for r in rows if V_WITH <= r < V_WITHOUT + len(LENGTHS) and deg[r]]
        assert {int(rowptr[r]) % 4 for r in v_rows} == {0, 1, 2, 3}, "a row start at every residue mod 4"
        ref = {name: _reference(rowptr, col, fixw, k) for name, k in lists.items()}
        out[tail_len] = {"rowptr": rowptr, "col": col, "fixw": fixw, "lists": lists, "ref": ref,
                         "d_rowptr": t(rowptr), "d_col": t(col), "d_fixw": t(fixw), "d_keys": {n: t(k) for n, k in lists.items()}}
    w = out[TAIL_LENGTHS[0]]
    ref = w["ref"]
    k_sub = w["lists"]["special_rows"]
    assert ref["special_rows"][1] == 0.0 and ref["special_rows"][0] > 0.0 and (k_sub[0] & 0xFFFFFFFF) == V_SUB
    assert ref["lengths_without_0"][0] == 0.0 and ref["lengths_with_0"][0] > 0.0     # the empty row; the row that is just {0}
    # carries across bit 32: ~1000 common neighbours of weights with bits on both sides of it
    u3_big = int(w["fixw"][np.intersect1d(w["col"][w["rowptr"][U3]:w["rowptr"][U3 + 1]],
                                          w["col"][w["rowptr"][V_BIG]:w["rowptr"][V_BIG + 1]])].sum())
    assert u3_big >> 32 > 1000 and np.float32(np.float64(u3_big) * 2.0 ** -40) == ref["special_rows"][3]
    return out


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def _check_both_entries(eps, dev, rowptr, col, fixw, n, keys, want):
    assert _same_bits(eps.ops.rescore_runs(rowptr, col, fixw, n, keys), want)
    # the device count below the list's length: the head is the reference's, nothing beyond it is written
    count = keys.numel() * 2 // 3
    n_dev = torch.tensor([count], dtype=torch.int64, device=dev)
    assert _same_bits(eps.ops.rescore_runs_dev(rowptr, col, fixw, n, keys, n_dev)[:count], want[:count])
    out = torch.full((keys.numel(),), SENTINEL, dtype=torch.float32, device=dev)
    eps.ops._call("eps_rescore_runs_dev", dev, rowptr, col, fixw, n, keys, keys.numel(), n_dev, out)
    assert _same_bits(out[:count], want[:count]) and bool((out[count:] == SENTINEL).all())


@pytest.mark.parametrize("name", LISTS)
def test_trip_edges_match_host_sums(eps, dev, worlds, name):
    w = worlds[TAIL_LENGTHS[0]]
    _check_both_entries(eps, dev, w["d_rowptr"], w["d_col"], w["d_fixw"], N, w["d_keys"][name], w["ref"][name])


@pytest.mark.parametrize("tail_len", TAIL_LENGTHS[1:])
def test_last_row_of_col_at_every_length_mod_4(eps, dev, worlds, tail_len):
    """The row that ends where the descriptor over col[] ends: its last load reads 1, 2 or 3 entries and zeros behind them."""
    w = worlds[tail_len]
    _check_both_entries(eps, dev, w["d_rowptr"], w["d_col"], w["d_fixw"], N, w["d_keys"]["tail"], w["ref"]["tail"])


@pytest.mark.parametrize("extra", [0, 1])
def test_trip_edges_at_the_window_switch(eps, dev, worlds, limits, extra):
    """The small world as a graph of exactly RS_BITS nodes (one window: the instantiation without window arithmetic) and of
    RS_BITS + 1 (the windowed one, its second window holding one isolated id): the sums are the same."""
    w = worlds[TAIL_LENGTHS[0]]
    n = limits[0] + extra
    rowptr = torch.cat([w["d_rowptr"], torch.full((n - N,), w["col"].size, dtype=torch.int64, device=dev)])
    fixw = torch.cat([w["d_fixw"], torch.ones(n - N, dtype=torch.int64, device=dev)])
    for name in LISTS:
        _check_both_entries(eps, dev, rowptr, w["d_col"], fixw, n, w["d_keys"][name], w["ref"][name])


@pytest.fixture(scope="module")
def wide_world(dev, worlds, limits):
    """The small world relabelled monotonically (rows stay ascending, node 0 stays node 0) into 2 RS_BITS + 77 ids: ids below 2100
    stay, 2100 .. 4129 start three ids below the first window edge, 4130 and up start at the second edge."""
    bits = limits[0]
    n = 2 * bits + 77
    w = worlds[TAIL_LENGTHS[0]]
    old = np.arange(N, dtype=np.int64)
    new = np.where(old < 2100, old, np.where(old < 4130, bits - 3 + (old - 2100), 2 * bits + (old - 4130)))
    assert (np.diff(new) > 0).all() and new[0] == 0 and new[-1] < n
    deg = np.zeros(n, dtype=np.int64)
    deg[new] = np.diff(w["rowptr"])
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = new[w["col"]].astype(np.int32)                     # (rows keep their order in col[]: the relabelling is monotone)
    fixw = np.ones(n, dtype=np.int64)
    fixw[new] = w["fixw"]
    row_u1 = col[rowptr[new[U1]]:rowptr[new[U1] + 1]]
    assert (row_u1 < bits).any() and ((row_u1 >= bits) & (row_u1 < 2 * bits)).any() and (row_u1 >= 2 * bits).any()
    t = lambda a: torch.from_numpy(a).to(dev)                                       # noqa: E731
    keys = {name: t((new[k >> 32] << 32) | new[k & 0xFFFFFFFF]) for name, k in w["lists"].items()}
    return {"n": n, "rowptr": t(rowptr), "col": t(col), "fixw": t(fixw), "keys": keys}


@pytest.mark.parametrize("name", LISTS)
def test_trip_edges_over_three_id_windows(eps, dev, worlds, wide_world, name):
    ww = wide_world
    _check_both_entries(eps, dev, ww["rowptr"], ww["col"], ww["fixw"], ww["n"], ww["keys"][name], worlds[TAIL_LENGTHS[0]]["ref"][name])
