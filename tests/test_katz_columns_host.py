"""CPU: the argument checks of the Katz column kernel's entry points (csrc/katz_columns.hip) -- they return before any HIP
call --, its workspace size, its limits, and the filter's work estimate against a SciPy count."""
import ctypes
import os

import numpy as np
import scipy.sparse as ssp
import torch

from conftest import GOLDEN

COEFFS = (0.05, 0.005, 0.000125)
FAKE = ctypes.c_void_p(0x1000)          # never dereferenced: every call below must stop at its argument checks


def _call(lib, graph=None, n=10, v_lo=0, v_hi=10, colptr=FAKE, cand_u=FAKE, n_cand=5, coeffs=COEFFS, max_support=10, chunk=0,
          ws=None, ws_bytes=0, out=FAKE):
    graph = [FAKE] * 7 if graph is None else graph
    return lib.eps_katz_column_scores(*graph, n, v_lo, v_hi, colptr, cand_u, n_cand, *coeffs, max_support, chunk, ws, ws_bytes, out,
                                      None)


def test_column_scores_refuse_bad_arguments_before_any_launch(eps):
    lib = eps.load()
    assert _call(lib, graph=[None] * 7, colptr=None, cand_u=None) == -1 and b"null" in lib.eps_last_error()
    assert _call(lib, colptr=None) == -1 and b"null" in lib.eps_last_error()
    assert _call(lib, cand_u=None) == -1 and b"null" in lib.eps_last_error()
    assert _call(lib, out=None) == -1 and b"null" in lib.eps_last_error()
    assert _call(lib, n=-1, v_hi=0) == -1 and b"negative" in lib.eps_last_error()
    assert _call(lib, n_cand=-5) == -1 and b"negative" in lib.eps_last_error()
    assert _call(lib, v_lo=7, v_hi=3) == -1 and b"columns" in lib.eps_last_error()
    assert _call(lib, v_lo=-1) == -1 and b"columns" in lib.eps_last_error()
    assert _call(lib, v_hi=11) == -1 and b"columns" in lib.eps_last_error()
    assert _call(lib, v_lo=4, v_hi=4) == -1 and b"empty block" in lib.eps_last_error()
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(3):
            c = list(COEFFS)
            c[k] = bad
            assert _call(lib, coeffs=c) == -1 and b"non-finite" in lib.eps_last_error()
    assert _call(lib, chunk=-1) == -1 and b"chunk" in lib.eps_last_error()
    assert _call(lib, chunk=(1 << 20) + 1) == -1 and b"chunk" in lib.eps_last_error()
    # values on one side only
    g = [FAKE] * 7
    g[2] = None
    assert _call(lib, graph=g) == -1 and b"unit-valued" in lib.eps_last_error()
    # a support beyond the LDS table needs the workspace, at its full size
    cap = ctypes.c_int32(0)
    chunk = ctypes.c_int32(0)
    assert lib.eps_katz_columns_limits(ctypes.byref(cap), ctypes.byref(chunk)) == 0
    big = cap.value + 1
    need = lib.eps_katz_columns_workspace_bytes(big)
    assert need > 0
    assert _call(lib, n=2 * big, v_hi=10, max_support=big) == -1 and b"workspace" in lib.eps_last_error()
    assert _call(lib, n=2 * big, v_hi=10, max_support=big, ws=FAKE, ws_bytes=need - 1) == -1 and b"workspace" in lib.eps_last_error()


def test_empty_block_is_a_no_op(eps):
    lib = eps.load()
    assert _call(lib, graph=[None] * 7, colptr=None, cand_u=None, n_cand=0, out=None) == 0
    assert _call(lib, graph=[None] * 7, n=0, v_lo=0, v_hi=0, colptr=None, cand_u=None, n_cand=0, out=None, max_support=0) == 0
    assert _call(lib, v_lo=4, v_hi=4, n_cand=0) == 0


def test_limits_and_workspace_size(eps):
    lib = eps.load()
    assert lib.eps_katz_columns_limits(None, None) == -1
    cap, chunk = eps.ops.katz_columns_limits()
    assert cap >= 4267 and chunk >= 64 and chunk % 64 == 0          # (the ddi-sized graph's columns keep their table in LDS)
    # the default work unit: the smallest for short lists, never smaller for longer ones, a power-of-two multiple of it
    sizes = [-1, 0, 1, chunk, 222_834, 1 << 21, (1 << 22) - 1, 1 << 22, 1 << 23, 16_020_530, 50_398_780, 1 << 40]
    units = [eps.ops.katz_columns_chunk(s) for s in sizes]
    assert units[:5] == [chunk] * 5 and all(a <= b for a, b in zip(units, units[1:]))
    assert all(u % chunk == 0 and (u // chunk) & (u // chunk - 1) == 0 and u <= 1 << 20 for u in units) and units[-1] > chunk
    ws = lib.eps_katz_columns_workspace_bytes
    assert ws(0) == 0 and ws(-3) == 0 and ws(cap) == 0 and ws(cap + 1) > 0
    sizes = [0, 1, 63, 64, 65, cap - 1, cap, cap + 1, 2 * cap, 10_000, 65_536, 65_537, 235_868, 576_289, 1 << 24, 1 << 30, 1 << 31,
             1 << 40]
    got = [ws(s) for s in sizes]
    assert all(a <= b for a, b in zip(got, got[1:])), got
    # every workgroup's table has two slots per possible key, 12 bytes each
    assert ws(cap + 1) >= 12 * 2 * (cap + 1) and ws(235_868) >= 12 * 2 * 235_868


def test_work_estimate_matches_a_scipy_count(eps):
    """sum over the 2-hop non-edges (u, v) of deg(u) -- the table lookups of a whole filter run -- and its bound from the
    two-hop path counts, on the golden graph."""
    from eps_amd import candidates, heuristics
    d = np.load(os.path.join(GOLDEN, "pairs_er500.npz"))
    n = d["rowptr"].size - 1
    A = ssp.csr_matrix((np.ones(d["col"].size), d["col"], d["rowptr"]), shape=(n, n))
    A2 = (A @ A).tocoo()
    keep = (A2.row != A2.col) & (np.asarray(A[A2.row, A2.col]).ravel() == 0)
    u = A2.row[keep]
    deg = np.diff(A.indptr)
    truth = int(deg[u].sum())
    assert truth > 0
    g = eps.CSRGraph.from_scipy(A.astype(np.float32))
    assert heuristics.katz_column_steps(g, torch.from_numpy(u.astype(np.int32))) == truth
    assert heuristics.katz_column_steps(g, candidates.all_candidates(g)[0]) == truth
    assert heuristics.katz_column_steps(g, torch.zeros(0, dtype=torch.int32)) == 0
    # the bound counts deg(u) for every two-path out of u, capped at N - 1 ends
    paths = np.asarray(A @ deg).ravel()
    bound = int((deg * np.minimum(paths, n - 1)).sum())
    assert heuristics.katz_steps_bound(g) == bound >= truth
