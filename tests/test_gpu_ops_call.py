"""GPU: the one call path of ops.py -- a wrong-dtype tensor is refused before any launch, a failed call is reported under the
symbol that was called, and the timing bracket records the same event names as before it was folded into that path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 64


@pytest.fixture(scope="module")
def small(eps, dev):
    """A 64-node random symmetric graph (no self loops) and a few well-typed operands of <= 256 entries."""
    from eps_amd.graph import CSRGraph
    gen = torch.Generator().manual_seed(5)
    a = torch.rand(N, N, generator=gen) < 0.1
    a = (a | a.t()) & ~torch.eye(N, dtype=torch.bool)
    r, c = a.nonzero(as_tuple=True)
    g = CSRGraph.from_edge_index(torch.stack([r, c]), None, (N, N)).to(dev)
    i32, i64, f32 = (dict(dtype=t, device=dev) for t in (torch.int32, torch.int64, torch.float32))
    nnz = g.col.numel()
    return dict(g=g, nnz=nnz, i32=i32, i64=i64, f32=f32,
                keys=torch.arange(200, **i64), vals=torch.rand(200, generator=gen).to(dev), base=torch.zeros(1, **f32),
                count=torch.tensor([200], **i64), x=torch.rand(N, 8, generator=gen).to(dev))


def _wrong(t):
    """The same values in the other width (int32 <-> int64, float32 <-> float64): what a caller's slip looks like."""
    return t.to({torch.int32: torch.int64, torch.int64: torch.int32, torch.float32: torch.float64, torch.int16: torch.int32}[t.dtype])


def _screen_args(s):
    g, i32 = s["g"], s["i32"]
    m = 32
    return dict(rowptr=g.rowptr, col=g.col, revpos=torch.zeros(s["nnz"], **i32), fx32=torch.ones(N, **i32),
                cuts=torch.zeros((N, m), dtype=torch.int16, device=g.device), bounds=torch.zeros(m + 1, **i32), n_nodes=N,
                columns=torch.arange(N, **i32), shift=0, out=None, status=torch.zeros(1, **i32))


CASES = {
    # wrapper that gained a check -> (name the refusal must carry, call with ONE tensor of the wrong dtype)
    "gcn_norm": ("col", lambda o, s: o.gcn_norm(s["g"].rowptr, _wrong(s["g"].col), None)),
    "unpack_keys": ("keys", lambda o, s: o.unpack_keys(_wrong(s["keys"]))),
    "row_window_splits": ("rowptr", lambda o, s: o.row_window_splits(_wrong(s["g"].rowptr), s["g"].col, 32, 2)),
    "scan_plan_rewalk": ("pptr", lambda o, s: o.scan_plan_rewalk((torch.zeros(N + 1, **s["i64"]), torch.zeros((1, 4), **s["i32"])), 2)),
    "scan_plan_rewalk_records": ("plan", lambda o, s: o.scan_plan_rewalk((torch.zeros(N + 1, **s["i32"]),
                                                                          torch.zeros((1, 4), **s["i64"])), 2)),
    "rescore_runs_dev": ("col", lambda o, s: o.rescore_runs_dev(s["g"].rowptr, _wrong(s["g"].col), torch.ones(N, **s["i64"]), N,
                                                                 s["keys"], s["count"])),
    "rescore_runs_dev_count": ("n_dev", lambda o, s: o.rescore_runs_dev(s["g"].rowptr, s["g"].col, torch.ones(N, **s["i64"]), N,
                                                                       s["keys"], _wrong(s["count"]))),
    "score_pick_compact": ("vals", lambda o, s: o.score_pick_compact(s["keys"], _wrong(s["vals"]), None, s["base"], 10)),
    "score_pick_compact_keys": ("keys", lambda o, s: o.score_pick_compact(_wrong(s["keys"]), s["vals"], None, s["base"], 10)),
    "score_pick_compact_count": ("n_dev", lambda o, s: o.score_pick_compact(s["keys"], s["vals"], _wrong(s["count"]), s["base"], 10)),
    "score_hist_count": ("n_dev", lambda o, s: o.score_hist(s["keys"], s["vals"], _wrong(s["count"]), s["base"])),
    "score_hist_into_count": ("n_dev", lambda o, s: o.score_hist_into(s["keys"], s["vals"], _wrong(s["count"]), s["base"],
                                                                      torch.zeros(o.score_bins(), **s["i32"]))),
    "radix_sort_by_u_count": ("n_dev", lambda o, s: o.radix_sort_by_u(s["keys"], _wrong(s["count"]))),
    "radix_sort_rows_count": ("m_dev", lambda o, s: o.radix_sort_rows(s["keys"], s["vals"], _wrong(s["count"]), 50)),
    "scan_screen_rowrec": ("rowrec", lambda o, s: o.scan_screen(**_screen_args(s), rowrec=torch.zeros((N, 32), **s["i64"]))),
    "scan_screen_colrec": ("colrec", lambda o, s: o.scan_screen(**_screen_args(s), colrec=torch.zeros((N, 8), **s["i64"]))),
    "scan_screen_pack": ("pack", lambda o, s: o.scan_screen(**_screen_args(s), pack=torch.zeros((s["nnz"], 8), **s["i64"]))),
    "spmm_csr_out": ("out", lambda o, s: o.spmm_csr(s["g"].rowptr, s["g"].col, None, s["x"], out=_wrong(torch.empty_like(s["x"])))),
    "gemm_out": ("out", lambda o, s: o.gemm(s["x"], s["x"], out=torch.empty((N, N), dtype=torch.float64, device=s["x"].device))),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_wrong_dtype_is_refused(eps, small, case):
    """Every wrapper that passed a pointer unchecked before: one tensor of the wrong dtype raises EpsError naming it.  The check
    sits in front of every allocation and launch of the wrapper (``out=None`` of scan_screen would fail first otherwise)."""
    name, call = CASES[case]
    with pytest.raises(eps.EpsError, match=rf"^{name}: expected torch\."):
        call(eps.ops, small)


def test_a_failed_call_names_the_symbol_that_was_called(eps, small, dev):
    """The library refuses a bad mode / a negative size on the host (rc = -1, nothing launched): the EpsError's label is the
    exported symbol the call went to -- the float64 flavours used to report under their float32 siblings' names."""
    sums = torch.ones(8, dtype=torch.float64, device=dev)
    with pytest.raises(eps.EpsError, match=r"^eps_node_weights_f64 failed \(rc=-1\)"):
        eps.ops.node_weights(sums, 7, f64=True)
    with pytest.raises(eps.EpsError, match=r"^eps_node_weights_f64 failed \(rc=-1\)"):
        eps.ops._call("eps_node_weights_f64", dev, sums, -1, eps.ops.W_AA, torch.empty_like(sums))
    with pytest.raises(eps.EpsError, match=r"^eps_node_weights failed \(rc=-1\)"):
        eps.ops.node_weights(sums.float(), 7)


# what one scan_topk of the estimate -> scan -> verify path records on test_gpu_scan.py's smallest graph with every call bracketed
# (EVENT_NAMES = None), taken from the commit before the brackets were folded into ops._call
EVENTS_UNFILTERED = {"scan_piece_kernel", "select_compact", "sort_pairs_by_u", "rescore_runs", "select_rows"}
SCAN_EVENTS = {"scan_piece_kernel", "filter_scan_kernel"}


def _recorded(eps, dev, names):
    from eps_amd import scan, synth
    from eps_amd.heuristics import node_weight_table
    ops = eps.ops
    g = synth.rmat_graph(12, 12, 3, "cpu").to(dev)
    wt = node_weight_table(g, ops.W_AA)
    ops.KERNEL_EVENTS, ops.EVENT_NAMES = [], names
    try:
        scan.scan_topk(g, wt, 20000)
        events = ops.KERNEL_EVENTS
    finally:
        ops.KERNEL_EVENTS, ops.EVENT_NAMES = None, None
    torch.cuda.synchronize(dev)
    for name, start, end, size in events:                # the tuples keep their form: two recorded events and a work size
        assert isinstance(name, str) and isinstance(size, int) and start.elapsed_time(end) >= 0.0
    return [e[0] for e in events]


def test_event_names_unfiltered(eps, dev, monkeypatch):
    from eps_amd import scan
    monkeypatch.setattr(scan, "SMALL_SET", 0)             # the piece kernel under a bar, as on a graph of production size
    names = _recorded(eps, dev, None)
    assert "scan_piece_kernel" in names
    assert set(names) == EVENTS_UNFILTERED


def test_event_names_filtered(eps, dev, monkeypatch):
    """EVENT_NAMES = (): bench.py's timed region -- the scan launches are recorded all the same, nothing else is."""
    from eps_amd import scan
    monkeypatch.setattr(scan, "SMALL_SET", 0)
    names = _recorded(eps, dev, ())
    assert names and set(names) <= SCAN_EVENTS
