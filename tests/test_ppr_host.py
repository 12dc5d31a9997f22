"""CPU: the fixed-point personalized-PageRank push without a GPU -- the numpy truth (tests/ppr_truth.py) against the
Andersen-Chung-Lang bound on the symmetric golden graphs, the host-side pieces (ppr_parameters, ppr_queries, the factory, the
parsers) and the library's argument errors.  On the parent of this change the names do not exist."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import ppr_truth as pt

MAX_ROUNDS = 1024


def _symmetric(rowptr, col):
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    a = set(zip(rows.tolist(), col.tolist()))
    return all((c, r) in a for r, c in a)


def _check_bound(name, eps, sources=None):
    """Mass conserved exactly (asserted inside the truth); 0 <= pi - p < eps' d + pushes 2^-48 + 1e-12 at every node.  The
    1e-12 covers the dense float64 solve: n <= 1024 and the 1-norm condition number of I - (1 - alpha) P is at most
    (2 - alpha) / alpha.  The left side gets none: it is never negative on these graphs (unreached nodes solve to exact zeros)."""
    rowptr, col, _ = pt.golden_graph(name)
    assert _symmetric(rowptr, col)
    a16, thr = pt.parameters(0.15, eps)
    deg = np.diff(rowptr).astype(np.float64)
    pi = pt.exact_ppr(rowptr, col, a16 / 65536.0)
    eps_eff = thr * 2.0 ** -48
    bars = pt.thresholds(np.diff(rowptr), thr)
    worst, most_rounds = 0.0, 0
    for s in (range(len(rowptr) - 1) if sources is None else sources):
        p, r, rounds, pushes, steps, capped = pt.push(rowptr, col, s, a16, thr, MAX_ROUNDS, bars)
        assert capped == 0 and int(p.sum()) + int(r.sum()) == pt.ONE
        gap = pi[s] - p.astype(np.float64) * 2.0 ** -48
        assert gap.min() >= 0.0, (name, eps, s, gap.min())
        assert np.all(gap < eps_eff * deg + pushes * 2.0 ** -48 + 1e-12), (name, eps, s)
        live = deg > 0
        if live.any():
            worst = max(worst, float((gap[live] / (eps_eff * deg[live])).max()))
        most_rounds = max(most_rounds, rounds)
    return worst, most_rounds


@pytest.mark.parametrize("name", pt.SYMMETRIC_GOLDEN)
def test_truth_meets_the_push_bound_from_every_source(name):
    worst, rounds = _check_bound(name, 1e-4)
    assert worst < 1.0 + 1e-6 and rounds <= MAX_ROUNDS


@pytest.mark.parametrize("eps", [1e-3, 1e-6])
@pytest.mark.parametrize("name", pt.SYMMETRIC_GOLDEN)
def test_truth_meets_the_push_bound_at_other_thresholds(name, eps):
    n = len(pt.golden_graph(name)[0]) - 1
    sources = sorted(set(np.random.default_rng(7).integers(0, n, 48).tolist()))
    _check_bound(name, eps, sources)


def test_truth_conventions():
    """An isolated source keeps everything; max_rounds stops the loop and says so; a saturated threshold never pushes."""
    rowptr, col, _ = pt.golden_graph("isolated_deg1")
    deg = np.diff(rowptr)
    a16, thr = pt.parameters(0.15, 1e-4)
    s = int(np.flatnonzero(deg == 0)[0])
    p, r, rounds, pushes, steps, capped = pt.push(rowptr, col, s, a16, thr, MAX_ROUNDS)
    assert p[s] == pt.ONE and r.sum() == 0 and (rounds, pushes, steps, capped) == (0, 0, 0, 0)
    rowptr, col, _ = pt.golden_graph("path30")
    p3 = pt.push(rowptr, col, 0, a16, thr, 3)
    full = pt.push(rowptr, col, 0, a16, thr, MAX_ROUNDS)
    assert p3[2] == 3 and p3[5] == 1 and full[2] > 3 and full[5] == 0
    assert pt.thresholds(np.array([0, 1, 1 << 20]), 1 << 47).tolist() == [pt.ONE + 1, 1 << 47, pt.ONE + 1]


def test_ppr_parameters(eps):
    from eps_amd import heuristics
    assert heuristics.ppr_parameters() == heuristics.ppr_parameters(heuristics.PPR_ALPHA, heuristics.PPR_EPS) == pt.parameters(0.15, 1e-4)
    assert heuristics.ppr_parameters(0.15, 1e-4) == (9830, 28147497672)
    assert heuristics.ppr_parameters(0.5, 1.0) == (32768, 1 << 48)
    assert heuristics.ppr_parameters(1 / 65536, 2.0 ** -47) == (1, 2)
    for alpha in (0.0, 1e-6, 0.51, 1.0, float("nan")):
        with pytest.raises(eps.EpsError, match="a16"):
            heuristics.ppr_parameters(alpha, 1e-4)
    for e in (0.0, -1e-4, 1.5, float("inf")):
        with pytest.raises(eps.EpsError, match="eps"):
            heuristics.ppr_parameters(0.15, e)
    # the refusal rule: thr * (65536 - a16) < 65536.  a16 = 32768: thr = 1 is refused, thr = 2 passes
    with pytest.raises(eps.EpsError, match="share"):
        heuristics.ppr_parameters(0.5, 2.0 ** -48)
    assert heuristics.ppr_parameters(0.5, 2.0 ** -47) == (32768, 2)
    with pytest.raises(eps.EpsError, match="share"):
        heuristics.ppr_parameters(0.15, 2.0 ** -48)            # 1 * 55706 < 65536
    assert heuristics.ppr_parameters(0.15, 2.0 ** -47) == (9830, 2)
    assert heuristics.PPR_MAX_ROUNDS == 1024


def test_ppr_queries_round_trip(eps):
    from eps_amd import heuristics
    src = torch.tensor([5, 2, 5, 9, 2, 5, 7, 2, 5], dtype=torch.int64)      # duplicates (5 -> 1 twice), a self pair, 7 and 9 with one query
    dst = torch.tensor([1, 2, 3, 4, 0, 1, 7, 8, 6], dtype=torch.int64)
    sources, qptr, qnode, back = heuristics.ppr_queries(src, dst)
    assert sources.dtype == torch.int32 and qptr.dtype == torch.int64 and qnode.dtype == torch.int32
    assert sources.tolist() == [2, 5, 7, 9] and qptr.tolist() == [0, 3, 7, 8, 9]
    assert qnode.tolist() == [2, 0, 8, 1, 3, 1, 6, 7, 4]                       # request order inside a source
    owner = torch.repeat_interleave(sources.long(), qptr[1:] - qptr[:-1])
    assert torch.equal(owner[back], src) and torch.equal(qnode.long()[back], dst)
    assert sorted(back.tolist()) == list(range(9))
    e = heuristics.ppr_queries(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert e[0].numel() == 0 and e[1].tolist() == [0] and e[2].numel() == 0 and e[3].numel() == 0
    with pytest.raises(eps.EpsError):
        heuristics.ppr_queries(src, dst[:3])


def _args(dataset, model, **kw):
    base = dict(dataset=dataset, model=model, num_layers=None, hidden_channels=None, dropout=None, batch_size=None, lr=None,
                epochs=None, use_feature=None, use_learnable_embedding=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_build_model_takes_ppr(eps):
    from eps_amd import heuristics, models
    assert "ppr" in models._MODELS and "ppr" in models._HEURISTICS
    for dataset in ("ddi", "collab", "ppa"):
        args = models.default_model_configs(_args(dataset, "ppr"))
        assert args.use_feature is False and args.use_learnable_embedding is False
        m = models.build_model(args, argparse.Namespace(num_nodes=12, x=torch.zeros(12, 4)), "cpu")
        assert isinstance(m, models.CommonNeighborsPredictor) and m.type == "ppr"
        assert sum(p.numel() for p in m.parameters()) == 0
        assert (m.ppr_alpha, m.ppr_eps) == (heuristics.PPR_ALPHA, heuristics.PPR_EPS) == (0.15, 1e-4)
    m = models.build_model(models.default_model_configs(_args("ddi", "ppr", ppr_alpha=0.5, ppr_eps=1e-6)),
                           argparse.Namespace(num_nodes=12, x=None), "cpu")
    assert (m.ppr_alpha, m.ppr_eps) == (0.5, 1e-6)
    with pytest.raises(eps.EpsError, match="a16"):
        models.build_model(models.default_model_configs(_args("ddi", "ppr", ppr_alpha=0.9)), argparse.Namespace(num_nodes=12, x=None), "cpu")
    for refused in ("sage2", "ensemble_gcn_sage"):                          # (their refusal keeps its wording)
        with pytest.raises(NotImplementedError, match="outside the accelerated path"):
            models.build_model(models.default_model_configs(_args("ddi", refused)), argparse.Namespace(num_nodes=12, x=None), "cpu")


def test_parsers_take_the_flags(eps):
    from eps_amd import filter_stage, rank_stage
    a = filter_stage.make_parser().parse_args(["--dataset", "ddi", "--model", "ppr", "--checkpoint", "ddi_ppr||0|0.pt"])
    assert (a.ppr_alpha, a.ppr_eps) == (0.15, 1e-4)
    a = filter_stage.make_parser().parse_args(["--dataset", "ddi", "--model", "ppr", "--checkpoint", "x", "--ppr_alpha", "0.25",
                                               "--ppr_eps", "1e-5"])
    assert (a.ppr_alpha, a.ppr_eps) == (0.25, 1e-5)
    r = rank_stage.make_parser().parse_args(["--dataset", "collab", "--model", "ppr"])
    assert (r.ppr_alpha, r.ppr_eps) == (0.15, 1e-4)
    r = rank_stage.make_parser().parse_args(["--dataset", "collab", "--model", "ppr", "--ppr_alpha", "0.2", "--ppr_eps", "1e-3"])
    assert (r.ppr_alpha, r.ppr_eps) == (0.2, 1e-3)
    # never the threshold scan, never the bf16 screen
    assert filter_stage.fused_node_weights(argparse.Namespace(model="ppr"), None, None) is None
    with pytest.raises(ValueError, match="no MLP decode"):
        filter_stage.check_decode_args(argparse.Namespace(model="ppr", decode_precision="bf16", decode_guard=None, keep_top=10))


def test_ops_refuse_cpu_tensors_and_bad_tables(eps):
    z64, z32 = torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(eps.EpsError, match="CPU tensor"):
        eps.ops.ppr_push(z64, z32, 1, z32, z64, z32, 9830, 1 << 20, 8)
    with pytest.raises(eps.EpsError, match="table"):
        eps.ops.ppr_push(z64, z32, 1, z32, z64, z32, 9830, 1 << 20, 8, table="lds")
    assert eps.ops.ppr_touched_bound(10 ** 9, 9830, 28147497672) == 2 * (1 << 48) * 65536 // (28147497672 * 9830) + 2
    assert eps.ops.ppr_touched_bound(500, 9830, 28147497672) == 500
    assert eps.ops.ppr_touched_bound(10 ** 9, 1, 2) == 10 ** 9                   # (no useful bound: the table takes every node)


def test_limits_and_argument_errors_without_gpu(eps):
    """EINVAL before any HIP call: a null pointer, a16 out of range, thr too small, max_rounds < 1, a workspace too small."""
    lib = eps.load()
    lds_nodes, big_row, per_cu, ws0 = eps.ops.ppr_push_limits(0)
    assert lds_nodes >= 64 and big_row >= 64 and per_cu >= 1 and ws0 == 0
    small, big = eps.ops.ppr_push_limits(lds_nodes + 1)[3], eps.ops.ppr_push_limits(100 * lds_nodes)[3]
    assert 0 < small < big and small % 8 == 0
    assert lib.eps_ppr_push_limits(0, None, None, None, None) == -1 and b"null" in lib.eps_last_error()

    buf = (ctypes.c_int64 * 64)()                      # (stands for every array: nothing is read before the checks are through)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(a16=9830, thr=28147497672, max_rounds=8, n_nodes=4, ptr=p, force=0, table_nodes=0, ws=None, ws_bytes=0, mass=p):
        return lib.eps_ppr_push(ptr, p, n_nodes, p, 1, p, p, a16, thr, max_rounds, force, table_nodes, ws, ws_bytes, mass, p, p, p, p,
                                None, p, None)

    assert call(ptr=None) == -1 and b"null" in lib.eps_last_error()
    assert call(mass=None) == -1 and b"null" in lib.eps_last_error()
    for a16 in (0, -3, 32769, 65536):
        assert call(a16=a16) == -1 and b"a16" in lib.eps_last_error()
    assert call(thr=0) == -1 and b"thr" in lib.eps_last_error()
    assert call(thr=(1 << 48) + 1) == -1 and b"thr" in lib.eps_last_error()
    assert call(a16=32768, thr=1) == -1 and b"too small" in lib.eps_last_error()
    assert call(a16=9830, thr=1) == -1 and b"too small" in lib.eps_last_error()
    assert call(max_rounds=0) == -1 and b"max_rounds" in lib.eps_last_error()
    # a graph beyond the LDS table, or a forced global table, needs one workgroup's region
    n = lds_nodes + 1
    need = eps.ops.ppr_push_limits(n)[3]
    assert call(n_nodes=n, table_nodes=n, ws=None, ws_bytes=0) == -1 and b"workspace" in lib.eps_last_error()
    assert call(n_nodes=n, table_nodes=n, ws=p, ws_bytes=need - 8) == -1 and b"workspace" in lib.eps_last_error()
    assert call(n_nodes=4, force=1, table_nodes=4, ws=p, ws_bytes=8) == -1 and b"workspace" in lib.eps_last_error()
    assert call(n_nodes=n, table_nodes=0, ws=p, ws_bytes=need) == -1 and b"table_nodes" in lib.eps_last_error()
    assert call(n_nodes=-1) == -1 and call(n_nodes=1 << 31) == -1
