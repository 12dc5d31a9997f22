"""Thin torch-tensor wrappers over the C ABI (include/eps_abi.h).  Every function requires its
tensors on a HIP device and launches on torch's current stream; nothing here computes on the
CPU.  Every launch goes through ``_call``; host-only queries (workspace sizes, table geometry) are plain calls."""
from __future__ import annotations

import ctypes
import struct
from typing import Optional, Sequence, Tuple

import torch

from . import _lib

W_AA, W_RA = 0, 1

KERNEL_EVENTS = None      # a list while bench.py times kernels: (kernel name, start event, end event, work size) per launch
EVENT_NAMES = None        # None: every library call is bracketed while KERNEL_EVENTS is a list; a collection of names: only those (the
                          # scan launches always are) -- bench.py's timed region carries the dominant kernel's events alone
_SCAN_EVENTS = ("scan_piece_kernel", "filter_scan_kernel")

_SCRATCH = {}


def _scratch(name, dev, n_words: int, alloc, zero: bool = False) -> torch.Tensor:
    """The grow-only int64 buffer ``name`` of a device, at least ``n_words`` long; when it has to grow it is replaced by one of
    ``alloc`` words (an int, or a callable that gives it), the old buffer let go BEFORE the larger one is allocated.
    Stream-ordered like any other tensor on the current stream, so one buffer must not serve launches on several streams at once."""
    key = (name, dev.type, dev.index)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < n_words:
        _SCRATCH.pop(key, None)
        buf = None
        make = torch.zeros if zero else torch.empty
        buf = _SCRATCH[key] = make(alloc() if callable(alloc) else alloc, dtype=torch.int64, device=dev)
    return buf


def _ptr(t: Optional[torch.Tensor]):
    """Device pointer for the C ABI.  An EMPTY tensor has no storage (data_ptr() == 0), which the ABI would take for a
    missing argument: it gets the address of a small per-device dummy instead (nothing is read through it: the sizes say 0)."""
    if t is None:
        return None
    if t.numel() == 0 and t.is_cuda:
        return ctypes.c_void_p(_scratch("empty", t.device, 8, 8, zero=True).data_ptr())
    return ctypes.c_void_p(t.data_ptr())


def _call(name: str, dev: torch.device, *args, timed=None) -> None:
    """The one way into the library for everything that launches: ``name`` is the exported symbol, resolved on the loaded library
    and reported in the EpsError of a failed call; tensors among ``args`` go as their device pointers (``_ptr``), everything else
    (ints, floats, None, ctypes values, raw device addresses) as it is; the current stream of ``dev`` is appended.
    ``timed`` = (event name, work size): HIP events around the call on its stream while bench.py collects KERNEL_EVENTS."""
    fn = getattr(_lib.load(), name)
    args = [_ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ev = None
        if timed is not None and KERNEL_EVENTS is not None and (
                EVENT_NAMES is None or timed[0] in EVENT_NAMES or timed[0] in _SCAN_EVENTS):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(stream)
        _lib.check(fn(*args, ctypes.c_void_p(stream.cuda_stream)), name)
        if ev is not None:
            ev[1].record(stream)
            KERNEL_EVENTS.append((timed[0], ev[0], ev[1], int(timed[1])))


def _need_gpu(*tensors: Optional[torch.Tensor], row_strided=()) -> torch.device:
    """All tensors on one HIP device and contiguous; those listed in ``row_strided`` may be 2-D views
    with unit column stride and an arbitrary row stride (passed to the ABI as the leading dimension)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.EpsError("edge-proposal-sets_amd ops run on the MI355X only: got a CPU tensor "
                                "(there is no CPU fallback; move inputs to 'cuda')")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise _lib.EpsError(f"tensors on different devices: {dev} vs {t.device}")
        if any(t is r for r in row_strided):
            if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
                raise _lib.EpsError("2-D operand must have unit column stride")
        elif not t.is_contiguous():
            raise _lib.EpsError("non-contiguous tensor passed to the C ABI")
    if dev is None:
        raise _lib.EpsError("no tensor given")
    return dev


_I16, _I32, _I64, _F32, _F64 = torch.int16, torch.int32, torch.int64, torch.float32, torch.float64


def _chk(dtype: torch.dtype, **named) -> None:
    """``_chk(_I32, u=u, v=v)``: every named tensor has that dtype (None, and a device count given as a raw address, pass)."""
    for name, t in named.items():
        if isinstance(t, torch.Tensor) and t.dtype != dtype:
            raise _lib.EpsError(f"{name}: expected {dtype}, got {t.dtype}")


def _csr(rowptr, col, val=None, sfx: str = "") -> None:
    """The dtypes of a CSR triple: rowptr int64, col int32, val float32 (or None)."""
    _chk(_I64, **{"rowptr" + sfx: rowptr}); _chk(_I32, **{"col" + sfx: col}); _chk(_F32, **{"val" + sfx: val})


def _chk_2d(who: str, **named) -> None:
    """Every named tensor is a matrix (None passes).  Called BEFORE ``_need_gpu``, whose own refusal of a row-strided operand
    that is not 2-D does not say which operand it was."""
    for name, t in named.items():
        if t is not None and t.dim() != 2:
            raise _lib.EpsError(f"{who}: {name} must be 2-D, got {tuple(t.shape)}")


def _chk_len(who: str, name: str, t: Optional[torch.Tensor], n: int, what: str) -> None:
    """A vector operand holds exactly ``n`` entries (None passes): the kernels read ``n`` of them unchecked."""
    if t is not None and t.numel() != n:
        raise _lib.EpsError(f"{who}: {name} holds {t.numel()} entries, not {n} ({what})")


def _chk_out(who: str, out: Optional[torch.Tensor], rows: int, cols: int) -> None:
    """A caller's ``out`` has the result's shape (None passes): the kernels write rows x cols through its row stride."""
    if out is not None and tuple(out.shape) != (rows, cols):
        raise _lib.EpsError(f"{who}: out must be [{rows}, {cols}], got {tuple(out.shape)}")


def device_info() -> Tuple[int, str]:
    lib = _lib.load()
    n = ctypes.c_int(0)
    buf = ctypes.create_string_buffer(256)
    _lib.check(lib.eps_device_info(ctypes.byref(n), buf, 256), "eps_device_info")
    return n.value, buf.value.decode()


def col_sums(rowptr, col, val, n_cols: int, f64: bool = False) -> torch.Tensor:
    """Column sums, accumulated in float64 on the device; returned as float32 (rounded once) or, ``f64=True``, as is."""
    dev = _need_gpu(rowptr, col, val)
    _csr(rowptr, col, val)
    if col.numel() == 0:                        # a graph without entries (its col[] has no storage to point at)
        return torch.zeros(n_cols, dtype=_F64 if f64 else _F32, device=dev)
    wide = torch.empty(n_cols, dtype=_F64, device=dev)
    out = None if f64 else torch.empty(n_cols, dtype=_F32, device=dev)
    _call("eps_col_sums", dev, rowptr, col, val, rowptr.numel() - 1, n_cols, wide, out)
    return wide if f64 else out


def node_weights(colsum: torch.Tensor, mode: int, f64: bool = False) -> torch.Tensor:
    """1/log(colsum) (AA) or 1/colsum (RA), inf -> 0: float32 from float32 sums, or float64 from float64 sums."""
    dev = _need_gpu(colsum)
    _chk(_F64 if f64 else _F32, colsum=colsum)
    out = torch.empty(colsum.numel(), dtype=_F64 if f64 else _F32, device=dev)
    _call("eps_node_weights_f64" if f64 else "eps_node_weights", dev, colsum, colsum.numel(), mode, out)
    return out


GROUPED_MIN_RUN = 256  # mean pairs per run of equal v above which the column-run kernel is used


def v_runs_are_long(v: torch.Tensor) -> bool:
    """True when ``v`` (the reference's column-major candidate order) has runs long enough for the
    column-run kernel to pay: one elementwise pass + a reduction on the device."""
    n = v.numel()
    if n < 4 * GROUPED_MIN_RUN:
        return False
    n_runs = int((v[1:] != v[:-1]).sum().item()) + 1
    return n >= n_runs * GROUPED_MIN_RUN


def pair_scores(rowptr, col, val, node_w, n_nodes: int, u, v, want_count=True, want_cn=True, want_wsum=None,
                grouped=None):
    """-> (count int32[E] | None, cn float32[E] | None, wsum float32/float64[E] | None).
    node_w float64 selects the float64-accumulate kernel (cn is then not produced).
    ``grouped``: True -> column-run kernel (pair list sorted by v), False -> generic kernel, None -> decide
    from the run statistics of ``v``.  Results are identical either way."""
    dev = _need_gpu(rowptr, col, val, node_w, u, v)
    _csr(rowptr, col, val); _chk(_I32, u=u, v=v)
    if u.numel() != v.numel():
        raise _lib.EpsError("u and v differ in length")
    if want_wsum is None:
        want_wsum = node_w is not None
    n = u.numel()
    if grouped is None:
        grouped = v_runs_are_long(v)
    count = torch.empty(n, dtype=_I32, device=dev) if want_count else None
    if node_w is not None and node_w.dtype == _F64:
        ws = torch.empty(n, dtype=_F64, device=dev) if want_wsum else None
        _call("eps_pair_scores_grouped_f64" if grouped else "eps_pair_scores_f64", dev, rowptr, col, val, node_w, n_nodes, u, v,
              n, count, ws)
        return count, None, ws
    _chk(_F32, node_w=node_w)
    cn = torch.empty(n, dtype=_F32, device=dev) if want_cn else None
    ws = torch.empty(n, dtype=_F32, device=dev) if want_wsum else None
    _call("eps_pair_scores_grouped" if grouped else "eps_pair_scores", dev, rowptr, col, val, node_w, n_nodes, u, v, n, count, cn,
          ws)
    return count, cn, ws


def two_path_counts(rowptr, col) -> torch.Tensor:
    """paths[x] = sum over the entries w of row x of the length of row w: the two-paths out of every node (int64)."""
    dev = _need_gpu(rowptr, col)
    _csr(rowptr, col)
    n = rowptr.numel() - 1
    if n < 0:
        raise _lib.EpsError("rowptr must hold at least one entry")
    out = torch.empty(n, dtype=_I64, device=dev)
    _call("eps_two_path_counts", dev, rowptr, col, n, out)
    return out


KATZ_CHUNK = 1 << 20   # pairs per eps_katz_pair_scores call (its workspace is ~132 bytes per pair)


def katz_pair_scores(rowptr, col, val, rowptr_t, col_t, val_t, paths_out, paths_in, n_nodes: int, u, v,
                     coeffs: Sequence[float]) -> torch.Tensor:
    """-> float32[E]: c1*A[u,v] + c2*(A^2)[u,v] + c3*(A^3)[u,v] (float64 accumulate, one rounding).  ``(rowptr_t,
    col_t, val_t)`` is A's transpose (A's own tensors when A is symmetric); ``paths_out`` / ``paths_in`` are
    ``two_path_counts`` of A and of A^T."""
    dev = _need_gpu(rowptr, col, val, rowptr_t, col_t, val_t, paths_out, paths_in, u, v)
    _csr(rowptr, col, val); _csr(rowptr_t, col_t, val_t, "_t")
    _chk(_I64, paths_out=paths_out, paths_in=paths_in); _chk(_I32, u=u, v=v)
    if u.numel() != v.numel():
        raise _lib.EpsError("u and v differ in length")
    if rowptr.numel() != n_nodes + 1 or rowptr_t.numel() != n_nodes + 1:
        raise _lib.EpsError(f"katz_pair_scores: A and A^T must both be [{n_nodes},{n_nodes}]")
    if paths_out.numel() != n_nodes or paths_in.numel() != n_nodes:
        raise _lib.EpsError(f"katz_pair_scores: two-path counts must hold {n_nodes} entries")
    c = [float(x) for x in coeffs]
    if len(c) != 3:
        raise _lib.EpsError(f"katz_pair_scores: expected three coefficients, got {len(c)}")
    n = u.numel()
    out = torch.empty(n, dtype=_F32, device=dev)
    if n == 0:
        return out
    ws = torch.empty((int(_lib.load().eps_katz_workspace_bytes(min(n, KATZ_CHUNK))) + 7) // 8, dtype=_I64, device=dev)
    for s in range(0, n, KATZ_CHUNK):
        e = min(n, s + KATZ_CHUNK)
        _call("eps_katz_pair_scores", dev, rowptr, col, val, rowptr_t, col_t, val_t, paths_out, paths_in, n_nodes, u[s:e], v[s:e],
              e - s, c[0], c[1], c[2], ws, out[s:e])
    return out


def katz_columns_limits() -> Tuple[int, int]:
    """(largest support bound min(paths_in[v], N) whose y2 table stays in LDS, smallest default number of candidates per work
    unit -- ``katz_columns_chunk`` gives a list's own) of eps_katz_column_scores (host-only query)."""
    cap, chunk = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.load().eps_katz_columns_limits(ctypes.byref(cap), ctypes.byref(chunk)), "eps_katz_columns_limits")
    return cap.value, chunk.value


def katz_columns_chunk(n_cand: int) -> int:
    """Candidates per work unit eps_katz_column_scores takes by default for a list of ``n_cand`` candidates (host-only query)."""
    return int(_lib.load().eps_katz_columns_chunk(int(n_cand)))


def katz_column_scores(rowptr, col, val, rowptr_t, col_t, val_t, paths_in, n_nodes: int, v_lo: int, v_hi: int, colptr, cand_u,
                       coeffs: Sequence[float], chunk: int = 0) -> torch.Tensor:
    """-> float32[E]: c1*A[u,v] + c2*(A^2)[u,v] + c3*(A^3)[u,v] of the column-major candidates of columns [v_lo, v_hi)
    (``colptr`` int64[v_hi - v_lo + 1], ``cand_u`` int32[E]; any u of the graph may be listed), with (A^2)[:, v] built once per
    column (csrc/katz_columns.hip; float64 accumulate, one rounding).  ``(rowptr_t, col_t, val_t)`` is A's transpose (A's own
    tensors when A is symmetric), ``paths_in`` = ``two_path_counts`` of A^T.  ``chunk``: candidates per work unit (0: the
    kernel's default; the scores do not depend on it).  Node ids and the column pointers' ends are checked
    here, on the host, before anything is launched."""
    dev = _need_gpu(rowptr, col, val, rowptr_t, col_t, val_t, paths_in, colptr, cand_u)
    _csr(rowptr, col, val); _csr(rowptr_t, col_t, val_t, "_t")
    _chk(_I64, paths_in=paths_in, colptr=colptr); _chk(_I32, cand_u=cand_u)
    v_lo, v_hi, n_nodes = int(v_lo), int(v_hi), int(n_nodes)
    if rowptr.numel() != n_nodes + 1 or rowptr_t.numel() != n_nodes + 1 or paths_in.numel() != n_nodes:
        raise _lib.EpsError(f"katz_column_scores: A, A^T and the two-path counts must all describe {n_nodes} nodes")
    if not 0 <= v_lo <= v_hi <= n_nodes:
        raise _lib.EpsError(f"katz_column_scores: columns [{v_lo}, {v_hi}) outside [0, {n_nodes}]")
    if colptr.numel() != v_hi - v_lo + 1:
        raise _lib.EpsError(f"katz_column_scores: colptr must hold {v_hi - v_lo + 1} entries, got {colptr.numel()}")
    if (val is None) != (val_t is None):
        raise _lib.EpsError("katz_column_scores: A and A^T must both carry values or both be unit-valued")
    c = [float(x) for x in coeffs]
    if len(c) != 3:
        raise _lib.EpsError(f"katz_column_scores: expected three coefficients, got {len(c)}")
    n = cand_u.numel()
    out = torch.empty(n, dtype=_F32, device=dev)
    if n == 0:
        return out
    # one host read: the ids' range, the column pointers' ends and order, the largest support bound of the block
    lo, hi = torch.aminmax(cand_u)
    facts = torch.stack([lo.to(_I64), hi.to(_I64), colptr[0], colptr[-1], (colptr[1:] - colptr[:-1]).min(),
                         paths_in[v_lo:v_hi].max()]).tolist()
    if facts[0] < 0 or facts[1] >= n_nodes:
        raise _lib.EpsError(f"katz_column_scores: node ids must lie in [0, {n_nodes}), got [{facts[0]}, {facts[1]}]")
    if facts[2] != 0 or facts[3] != n or facts[4] < 0:
        raise _lib.EpsError(f"katz_column_scores: colptr must ascend from 0 to {n} (the candidates), got {facts[2]} .. {facts[3]}")
    max_support = min(int(facts[5]), n_nodes)
    ws_bytes = int(_lib.load().eps_katz_columns_workspace_bytes(max_support))
    ws = _scratch("katz_columns", dev, (ws_bytes + 7) // 8, (ws_bytes + 7) // 8) if ws_bytes else None
    _call("eps_katz_column_scores", dev, rowptr, col, val, rowptr_t, col_t, val_t, paths_in, n_nodes, v_lo, v_hi, colptr, cand_u,
          n, c[0], c[1], c[2], max_support, int(chunk), ws, ws_bytes, out, timed=("katz_columns_kernel", n))
    return out


def expand_max_nodes() -> int:
    return int(_lib.load().eps_expand_max_nodes())


def _expand_scratch(dev, n_bytes: int) -> torch.Tensor:
    """int64 scratch of the fill kernel (status word + per-workgroup path buckets): one grow-only buffer per device,
    reused by every block of a filter run (a fresh multi-GB allocation per block costs more than the kernel saves)."""
    n_words = (n_bytes + 7) // 8
    return _scratch("expand", dev, n_words, int(n_words * 1.25) + 1024)


def _scan_scratch(dev, max_degree: int) -> torch.Tensor:
    """Scratch of eps_filter_scan (1 GiB of bucket records on 256 CUs + max_degree weights per workgroup), at its exact size."""
    need = (int(_lib.load().eps_filter_scan_workspace_bytes(int(max_degree))) + 7) // 8
    return _scratch("scan", dev, need, need)


def _aligned_ws(dev, n_bytes: int):
    """(tensor, 256-byte aligned pointer, bytes from there) of the grow-only scratch of the sorts and selections."""
    need = (int(n_bytes) + 7) // 8 + 32
    ws = _scratch("select", dev, need, int(need * 1.25))
    off = (-ws.data_ptr()) % 256
    return ws, ctypes.c_void_p(ws.data_ptr() + off), ws.numel() * 8 - off


def max_column_paths(rowptr: torch.Tensor, col: torch.Tensor, v_lo: int, v_hi: int) -> int:
    """max over the columns v of [v_lo, v_hi) of sum_{w in N(v)} deg(w): the two-hop paths of the heaviest column, which
    sizes the per-workgroup buckets of the fused expansion."""
    if v_hi <= v_lo:
        return 0
    deg = rowptr[1:] - rowptr[:-1]
    lo, hi = int(rowptr[v_lo].item()), int(rowptr[v_hi].item())
    if hi == lo:
        return 0
    dsum = torch.cumsum(deg[col[lo:hi].long()], 0)
    ends = rowptr[v_lo + 1:v_hi + 1] - lo                      # exclusive end of every column's slice
    upto = torch.where(ends > 0, dsum[(ends - 1).clamp(min=0)], torch.zeros_like(ends))
    per_col = upto - torch.cat([upto.new_zeros(1), upto[:-1]])
    return int(per_col.max().item())


class ExpandResult(tuple):
    """(colptr, cand_u, cand_v, cn, score) of ``expand_candidates``; ``.pairs`` is the int32 [2,E] buffer cand_u and
    cand_v are rows of (None without cand_v), so the (u; v) list exists without a copy; ``.counts`` is set in the
    upper-bound layout (see ``expand_candidates``)."""
    pairs = None
    counts = None
    survivors = None
    status = None


_EXPAND_WS_LIMIT = 96 << 30       # bytes of bucket scratch we are willing to hold on a 288 GB device


def expand_workspace_fits(max_paths: int) -> bool:
    """Whether the bucket scratch for columns of up to ``max_paths`` two-hop paths stays within the budget."""
    return int(_lib.load().eps_expand_workspace_bytes(int(max_paths))) <= _EXPAND_WS_LIMIT


def expand_unit(rowptr, col, node_w, n_nodes: int, v_lo: int, v_hi: int, max_degree: int, splits=None, want_score=True,
                want_v=True, col_order=None, revpos=None, colptr_ub=None, total_ub=None):
    """The candidate list of columns [v_lo, v_hi) of a graph WITHOUT stored values, on the threshold scan's structure
    (eps_expand_unit_count / eps_expand_unit_fill, csrc/filter_scan.hip): same tuple and same bits as
    ``expand_candidates(rowptr, col, None, node_w, ...)`` with ``want_cn=False`` -- (colptr, cand_u, cand_v | None, None,
    score | None) -- at about half the time.  ``node_w`` None with ``want_score``: all-ones weights (the score is the
    common-neighbour count).  ``max_degree`` / ``splits``: the per-graph figures ``filter_scan`` takes.  ``revpos``
    (``reverse_positions``; symmetric pattern) selects the HALF list: column v holds its candidates u < v only.

    ``colptr_ub`` (int64[n_cols + 1] on the device: an exclusive prefix of upper bounds of the columns' candidate counts,
    ``candidates.segment_bounds``) + ``total_ub`` (its last entry as a Python int) select the ONE-PASS list
    (eps_expand_unit_list): no counting launch, no host read before the launch; column v fills the front of its segment, the rest
    of the segment is NOT written, ``.counts`` (int64[n_cols]) holds the real counts and there is no cand_v."""
    dev = _need_gpu(rowptr, col, node_w, col_order, splits, revpos, colptr_ub)
    _csr(rowptr, col); _chk(_F32, node_w=node_w); _chk(_I32, col_order=col_order, splits=splits, revpos=revpos)
    _chk(_I64, colptr_ub=colptr_ub)
    n_cols = v_hi - v_lo
    if colptr_ub is not None and (total_ub is None or want_v or colptr_ub.numel() != n_cols + 1):
        raise ValueError("expand_unit: the one-pass list takes colptr_ub[n_cols + 1] + total_ub and writes no cand_v")
    if col_order is not None and col_order.numel() != n_cols:
        raise ValueError("col_order must have one entry per column of the range")
    ws = _scan_scratch(dev, int(max_degree))
    counts = torch.zeros(n_cols, dtype=_I64, device=dev)

    def fixw():
        if not want_score:
            return None
        return fixed_weights(node_w if node_w is not None else torch.ones(n_nodes, dtype=_F32, device=dev))

    graph = (n_nodes, col.numel(), int(max_degree), v_lo, v_hi, col_order)
    if colptr_ub is not None:
        cand_u = torch.empty(int(total_ub), dtype=_I32, device=dev)
        score = torch.empty(int(total_ub), dtype=_F32, device=dev) if want_score else None
        status = torch.zeros(1, dtype=_I32, device=dev)       # (the call clears it itself; an empty range makes no call)
        fw = fixw()
        if n_cols > 0:
            _call("eps_expand_unit_list", dev, rowptr, col, revpos, fw, splits, *graph, colptr_ub, counts, cand_u, score, status,
                  ws, ws.numel() * 8)
        out = ExpandResult((colptr_ub, cand_u, None, None, score))
        out.counts = counts
        out.status = status           # (device word: bit 1 = a bound was too small, bit 2 = a sum left the fixed-point range)
        return out
    colptr = torch.zeros(n_cols + 1, dtype=_I64, device=dev)
    if n_cols:
        _call("eps_expand_unit_count", dev, rowptr, col, revpos, splits, *graph, counts, ws, ws.numel() * 8)
    torch.cumsum(counts, 0, out=colptr[1:])
    total = int(colptr[-1].item())
    pairs = torch.empty((2 if want_v else 1, total), dtype=_I32, device=dev)
    score = torch.empty(total, dtype=_F32, device=dev) if want_score else None
    if total:
        fw = fixw()
        status = torch.zeros(1, dtype=_I32, device=dev)
        _call("eps_expand_unit_fill", dev, rowptr, col, revpos, fw, splits, *graph, colptr, None, pairs[0],
              pairs[1] if want_v else None, score, status, ws, ws.numel() * 8)
        st = int(status.item())
        if st:
            raise _lib.EpsError("expand_unit: " + ("a column outgrew its segment; " if st & 2 else "")
                                + ("a score left the fixed-point range (|sum| >= 2**23): use the pair kernels" if st & 4 else ""))
    out = ExpandResult((colptr, pairs[0], pairs[1] if want_v else None, None, score))
    out.pairs = pairs if want_v else None
    return out


def expand_candidates(rowptr, col, val, node_w, n_nodes: int, v_lo: int, v_hi: int, want_cn=True, want_score=True,
                      want_v=True, col_order=None, max_paths=None, colptr_ub=None, total_ub=None, cut=None, tile_ranks=0,
                      signed=False):
    """Fused 2-hop expansion of columns [v_lo, v_hi) of a SYMMETRIC adjacency (filter.py:96-109 + scoring).
    -> (colptr int64[n_cols+1], cand_u int32[E], cand_v int32[E] | None, cn int32[E] | None, score float32[E] | None);
    candidates are column-major, u ascending inside a column (the reference's order).  ``col_order`` (int32
    permutation of range(v_hi - v_lo), optional) is the order the columns are handed to the workgroups; the results
    do not depend on it.  ``max_paths`` (optional) is an upper bound of the two-hop paths of any column of the range
    (``max_column_paths``; callers that expand many blocks of one graph pass the cached figure).

    ``colptr_ub`` (int64[n_cols+1] on the device) + ``total_ub`` (its last entry, as a Python int) select the
    UPPER-BOUND layout: no counting pass and no host synchronisation before the launch; column v's candidates fill
    the front of [colptr_ub[v], colptr_ub[v+1]) and the rest of the segment is padded (cand_u -1, score -inf, cn 0).
    The result then carries ``.counts`` (int64[n_cols], real candidates per column) and E == total_ub.

    ``tile_ranks`` (0 = default): candidate ranks per LDS summation pass (eps_expand_fill_tiled); results do not depend on it.

    ``cut=(threshold, capacity)``: the kernel also reports the candidates whose score exceeds ``threshold`` (the
    streaming top-K's current K-th score) -- the result carries ``.survivors`` = (positions int64 ascending, scores) or
    None when more than ``capacity`` qualified.  With a cut, ``want_score=False`` skips the score array altogether.

    ``signed``: the terms may be negative (edge cosines, eps_expand_fill_signed): the kernel does not flag negative sums;
    the caller must have checked the range (candidates.fused_scores_fit)."""
    dev = _need_gpu(rowptr, col, val, node_w, col_order, colptr_ub)
    _csr(rowptr, col, val); _chk(_F32, node_w=node_w); _chk(_I32, col_order=col_order); _chk(_I64, colptr_ub=colptr_ub)
    lib = _lib.load()
    n_cols = v_hi - v_lo
    if col_order is not None and col_order.numel() != n_cols:
        raise ValueError("col_order must have one entry per column of the range")
    if colptr_ub is not None and (colptr_ub.numel() != n_cols + 1 or total_ub is None):
        raise ValueError("colptr_ub needs n_cols + 1 entries and total_ub")
    counts = torch.empty(n_cols, dtype=_I64, device=dev)
    if colptr_ub is None:
        colptr = torch.zeros(n_cols + 1, dtype=_I64, device=dev)
        _call("eps_expand_count", dev, rowptr, col, n_nodes, v_lo, v_hi, col_order, counts)
        torch.cumsum(counts, 0, out=colptr[1:])
        total = int(colptr[-1].item())
    else:
        colptr, total = colptr_ub, int(total_ub)
    pairs = torch.empty((2 if want_v else 1, total), dtype=_I32, device=dev)
    cand_u = pairs[0]
    cand_v = pairs[1] if want_v else None
    cn = torch.empty(total, dtype=_I32, device=dev) if want_cn else None
    score = torch.empty(total, dtype=_F32, device=dev) if want_score else None
    cut_rec = cut_pos = cut_val = None
    if cut is not None and total:
        thr, cap = float(cut[0]), int(cut[1])
        cut_pos = torch.empty(cap, dtype=_I64, device=dev)
        cut_val = torch.empty(cap, dtype=_F32, device=dev)
        head = struct.unpack("<q", struct.pack("<fI", thr, cap))[0]          # eps_score_cut: threshold, capacity
        cut_rec = torch.tensor([head, 0, cut_pos.data_ptr(), cut_val.data_ptr()], dtype=_I64, device=dev)
    scored = want_cn or want_score or cut_rec is not None
    if total:
        if max_paths is None:
            max_paths = max_column_paths(rowptr, col, v_lo, v_hi) if scored else 0
        ws_bytes = int(lib.eps_expand_workspace_bytes(int(max_paths) if scored else 0))
        if ws_bytes > _EXPAND_WS_LIMIT:
            raise _lib.EpsError(f"expand_candidates: a column with {max_paths} two-hop paths needs {ws_bytes >> 30} GiB "
                                "of bucket scratch; score such graphs with the pair kernels")
        ws = _expand_scratch(dev, ws_bytes)
        _call("eps_expand_fill_signed" if signed else "eps_expand_fill_tiled", dev, rowptr, col, val, node_w, n_nodes, v_lo, v_hi,
              col_order, colptr, counts if colptr_ub is not None else None, cand_u, cand_v, cn, score, cut_rec, ws, ws_bytes,
              int(tile_ranks))
        if cut_rec is not None:                      # one read-back for the status word and the survivor count
            both = torch.stack([ws[0], cut_rec[1]]).tolist()
            status, n_cut = both[0] & 0xFFFFFFFF, both[1] & 0xFFFFFFFF
        else:
            status, n_cut = int(ws[0].item()) & 0xFFFFFFFF, 0
        if status:
            raise _lib.EpsError("expand_candidates: " + ("a column had more two-hop paths than max_paths allows; " if status & 1 else "")
                                + ("a column had more candidates than its colptr_ub segment; " if status & 2 else "")
                                + ("a score left the fixed-point range (|sum| >= 2**23): use the pair kernels" if status & 4 else ""))
    out = ExpandResult((colptr, cand_u, cand_v, cn, score))
    out.pairs = pairs if want_v else None
    out.counts = counts if colptr_ub is not None else None
    if cut_rec is not None and n_cut <= cut_pos.numel():
        order = torch.argsort(cut_pos[:n_cut])                     # arrival order -> candidate order
        out.survivors = (cut_pos[:n_cut][order], cut_val[:n_cut][order])
    elif cut is not None and not total:
        out.survivors = (torch.zeros(0, dtype=_I64, device=dev), torch.zeros(0, dtype=_F32, device=dev))
    return out


# ------------------------------------------------------------------ threshold scan of the whole candidate set
def filter_scan_max_nodes() -> int:
    return int(_lib.load().eps_filter_scan_max_nodes())


def reverse_positions(rowptr: torch.Tensor, col: torch.Tensor, with_stats: bool = False):
    """int32[nnz]: for entry e of row v with w = col[e], the number of entries of row w below v (per-graph table).
    ``with_stats``: -> (revpos, half_paths int64[N] = its row sums, asymmetric int32[1] device flag) from the same pass."""
    dev = _need_gpu(rowptr, col)
    _csr(rowptr, col)
    n = rowptr.numel() - 1
    out = torch.empty(col.numel(), dtype=_I32, device=dev)
    hp = torch.zeros(n, dtype=_I64, device=dev) if with_stats else None
    flag = torch.zeros(1, dtype=_I32, device=dev) if with_stats else None
    _call("eps_reverse_positions", dev, rowptr, col, n, out, hp, flag)
    return (out, hp, flag) if with_stats else out


REVPOS_SORT_MIN = 1 << 62      # stored entries from which the reverse positions come out of a sort instead of searches: never by default --
                               # measured 3.56 vs 3.37 ms on the ppa-like graph (profiles/r06/revpos_sorted.txt)


def reverse_positions_symmetric(rowptr: torch.Tensor, col: torch.Tensor):
    """(revpos, half_paths, asymmetric flag) as ``reverse_positions(with_stats=True)`` for a SYMMETRIC pattern, with one search
    per unordered stored pair (eps_reverse_positions_symmetric); the flag comes back 1 on any other pattern and revpos is then
    not usable."""
    dev = _need_gpu(rowptr, col)
    _csr(rowptr, col)
    n, nnz = rowptr.numel() - 1, col.numel()
    out = torch.empty(nnz, dtype=_I32, device=dev)
    hp = torch.empty(n, dtype=_I64, device=dev)
    # one small buffer for everything the caller reads back: [asymmetric flag (low word), max degree, max half paths, their sum]
    # (zeros: the library clears the flag as the 32-bit word it is -- the high half of info[0] is nobody's)
    info = torch.zeros(4, dtype=_I64, device=dev)
    if nnz >= REVPOS_SORT_MIN:
        # (r06: no search at all -- the mirror entries come out of a stable sort of the entry indices by column id)
        _keep, wsp, wsb = _aligned_ws(dev, _lib.load().eps_reverse_positions_sorted_workspace_bytes(n, nnz))
        _call("eps_reverse_positions_sorted", dev, rowptr, col, n, nnz, max(1, int(n - 1).bit_length()), out, hp, info.data_ptr(),
              info.data_ptr() + 8, wsp, wsb)
    else:
        _call("eps_reverse_positions_symmetric", dev, rowptr, col, n, nnz, out, hp, info.data_ptr(), info.data_ptr() + 8)
    return out, hp, info


def node_order(rowptr: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None, relabel: bool = False):
    """Nodes by descending key (the degrees when ``rowptr`` is given, else ``keys`` int64 >= 0), ties by ascending id
    (eps_node_order: a stable radix sort of the library).  -> order int32[n]; with ``relabel`` -> (perm int64[n], inv int32[n],
    new_rowptr int64[n + 1]): what ``relabel_graph`` needs for the copy under that order."""
    src = rowptr if rowptr is not None else keys
    dev = _need_gpu(src)
    _chk(_I64, **{"rowptr / keys": src})
    n = src.numel() - 1 if rowptr is not None else src.numel()
    order = perm = inv = new_rp = None
    if relabel:
        perm = torch.empty(n, dtype=_I64, device=dev)
        inv = torch.empty(n, dtype=_I32, device=dev)
        new_rp = torch.empty(n + 1, dtype=_I64, device=dev)
    else:
        order = torch.empty(n, dtype=_I32, device=dev)
    _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_node_order_workspace_bytes(n))
    _call("eps_node_order", dev, rowptr, keys if rowptr is None else None, n, order, perm, inv, new_rp, wsp, wsb)
    return (perm, inv, new_rp) if relabel else order


def relabel_graph(rowptr, col, val, perm: torch.Tensor, inv32: torch.Tensor, new_rowptr: torch.Tensor):
    """(col, val) of the copy of a coalesced CSR graph under a node permutation: row i = row perm[i] with ids through inv32,
    sorted inside the row (eps_relabel_graph: gather + segmented radix sort)."""
    dev = _need_gpu(rowptr, col, val, perm, inv32, new_rowptr)
    _csr(rowptr, col, val); _chk(_I64, perm=perm, new_rowptr=new_rowptr); _chk(_I32, inv=inv32)
    n, nnz = rowptr.numel() - 1, col.numel()
    out_c = torch.empty(nnz, dtype=_I32, device=dev)
    out_v = None if val is None else torch.empty(nnz, dtype=_F32, device=dev)
    if nnz:
        _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_relabel_graph_workspace_bytes(n, nnz, int(val is not None)))
        _call("eps_relabel_graph", dev, rowptr, col, val, perm, inv32, new_rowptr, n, nnz, max(1, int(n - 1).bit_length()), out_c,
              out_v, wsp, wsb)
    return out_c, out_v


def csr_merge(rowptr, col, val, n: int, xkeys: torch.Tensor, want_val: bool):
    """(new_rowptr, new_col, new_val | None) of a coalesced square CSR graph [n, n] plus the batch ``xkeys`` -- int64, SORTED
    ascending, each ``row << 32 | col``, both orientations put in by the caller, duplicates allowed (eps_csr_merge_count /
    _fill: a merge per row, nothing the size of the graph is sorted).  ``want_val``: values are ``val`` (None = ones) + how
    often the batch names the pair; otherwise the pattern alone.  A key outside [0, n) or an unsorted batch raises EpsError
    (checked on the device, read with the new entry count: one host read per call).  An empty batch returns the arrays it
    was given."""
    dev = _need_gpu(rowptr, col, val, xkeys)
    _csr(rowptr, col, val); _chk(_I64, xkeys=xkeys)
    n, m = int(n), int(xkeys.numel())
    if rowptr.numel() != n + 1:
        raise _lib.EpsError(f"csr_merge: rowptr holds {rowptr.numel()} entries for n={n}")
    if m == 0:
        return rowptr, col, (val if want_val else None)
    new_deg = torch.empty(n, dtype=_I64, device=dev)
    xrank = torch.empty(m + 1, dtype=_I32, device=dev)
    status = torch.empty(1, dtype=_I32, device=dev)                  # (the call clears it)
    _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_csr_merge_workspace_bytes(m))
    _call("eps_csr_merge_count", dev, rowptr, col, n, xkeys, m, new_deg, xrank, status, wsp, wsb)
    new_rowptr = torch.zeros(n + 1, dtype=_I64, device=dev)
    torch.cumsum(new_deg, 0, out=new_rowptr[1:])
    st, nnz = torch.stack([status[0].to(_I64), new_rowptr[-1]]).tolist()
    if st:
        raise _lib.EpsError("csr_merge: " + (f"an edge names a node outside [0, {n}); " if st & 1 else "")
                            + ("xkeys is not sorted ascending" if st & 2 else ""))
    new_col = torch.empty(nnz, dtype=_I32, device=dev)
    new_val = torch.empty(nnz, dtype=_F32, device=dev) if want_val else None
    _call("eps_csr_merge_fill", dev, rowptr, col, val if want_val else None, n, xkeys, m, xrank, new_rowptr, nnz, new_col, new_val)
    return new_rowptr, new_col, new_val


def score_bound(rowptr, col, val, node_w, n_rows: int, n_cols: int) -> torch.Tensor:
    """1-element float64 DEVICE tensor: max over the rows of sum |A[v,w]| |node_w[w]| max_u |A[u,w]| (eps_score_bound)."""
    dev = _need_gpu(rowptr, col, val, node_w)
    _csr(rowptr, col, val); _chk(_F32, node_w=node_w)
    out = torch.empty(1, dtype=_F64, device=dev)
    ws = torch.empty(n_cols, dtype=_I32, device=dev) if val is not None else None
    _call("eps_score_bound", dev, rowptr, col, val, node_w, int(n_rows), int(n_cols), col.numel(), out, ws)
    return out


def filter_scan_windows(n_nodes: int):
    """(ids per window, number of windows) eps_filter_scan uses for an id space of ``n_nodes``."""
    w, k = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().eps_filter_scan_windows(int(n_nodes), ctypes.byref(w), ctypes.byref(k)), "eps_filter_scan_windows")
    return int(w.value), int(k.value)


def row_window_splits(rowptr: torch.Tensor, col: torch.Tensor, win_ids: int, n_win: int) -> Optional[torch.Tensor]:
    """int32[(n_win - 1) * N]: entries of every row below each window boundary (None for a single window)."""
    if n_win <= 1:
        return None
    dev = _need_gpu(rowptr, col)
    _csr(rowptr, col)
    n = rowptr.numel() - 1
    out = torch.empty((n_win - 1) * n, dtype=_I32, device=dev)
    _call("eps_row_window_splits", dev, rowptr, col, n, int(win_ids), int(n_win), out)
    return out


def fixed_weights(node_w: torch.Tensor) -> torch.Tensor:
    """int64[N]: round(node_w * 2**40), the per-node weights in the scan kernel's fixed point."""
    dev = _need_gpu(node_w)
    _chk(_F32, node_w=node_w)
    out = torch.empty(node_w.numel(), dtype=_I64, device=dev)
    _call("eps_fixed_weights", dev, node_w, node_w.numel(), out)
    return out


SURVIVOR_SLOTS_MAX = (1 << 32) - (1 << 20)   # slots are 32-bit positions handed out in chunks: keep a chunk's worth of head-room


_PINNED = {"buf": None, "i": 0}


def _pinned_words(words) -> torch.Tensor:
    """A pinned int64 host tensor holding ``words`` (<= 8), from a ring of 256 slots -- the source of an asynchronous host-to-device
    copy must stay untouched until the stream has run it; 256 copies ahead of the device do not happen in this library."""
    if _PINNED["buf"] is None:
        _PINNED["buf"] = torch.empty((256, 8), dtype=_I64).pin_memory()
    _PINNED["i"] = (_PINNED["i"] + 1) % 256
    slot = _PINNED["buf"][_PINNED["i"]]
    n = len(words)
    slot[:n] = torch.tensor(words, dtype=_I64)
    return slot[:n]


class Survivors:
    """Device-resident eps_survivors record + its key / val arrays.  ``threshold`` may be a Python float or a 0-dim /
    1-element float32 DEVICE tensor (copied on the stream: no host round trip)."""

    def __init__(self, capacity: int, threshold, device, scores_only: bool = False, both: bool = False, prefill: bool = True):
        """``scores_only``: the caller will read the scores alone (the bar estimate): untouched slots are then recognisable
        in ``val`` (-inf) instead of in ``key`` (-1), so no compaction pass is needed before a k-th-largest query.
        ``both``: both fills (key -1 AND val -inf): the list can go through a k-th-largest query as it is and be compacted
        afterwards (scan_topk's selection).
        ``prefill=False`` (eps_scan_screen only): no fill at all -- that kernel marks the unused slots of its reservations
        (key -1, val -inf) itself, and the list's readers stop at the slot counter (``count_ptr``): a step saves two passes
        over a list that is sized for the worst case."""
        self.capacity = int(capacity)
        if not 0 < self.capacity <= SURVIVOR_SLOTS_MAX:
            raise _lib.EpsError(f"Survivors: capacity {capacity} outside (0, {SURVIVOR_SLOTS_MAX}]")
        self.scores_only = bool(scores_only) and not both
        self.prefilled = bool(prefill)
        if not prefill:
            self.key = torch.empty(self.capacity, dtype=_I64, device=device)
            self.val = torch.empty(self.capacity, dtype=_F32, device=device)
        elif both:
            self.key = torch.full((self.capacity,), -1, dtype=_I64, device=device)
            self.val = torch.full((self.capacity,), float("-inf"), dtype=_F32, device=device)
        elif scores_only:
            self.key = torch.empty(self.capacity, dtype=_I64, device=device)
            self.val = torch.full((self.capacity,), float("-inf"), dtype=_F32, device=device)
        else:
            self.key = torch.full((self.capacity,), -1, dtype=_I64, device=device)
            self.val = torch.empty(self.capacity, dtype=_F32, device=device)
        thr_host = float(threshold) if not isinstance(threshold, torch.Tensor) else 0.0
        head = struct.unpack("<q", struct.pack("<fI", thr_host, self.capacity))[0]
        # (the 40-byte record goes up through a pinned staging slot, asynchronously on the stream: torch.tensor(..., device=) is a
        #  blocking copy, and a filter step builds three of these between its launches)
        self.rec = torch.empty(5, dtype=_I64, device=device)
        self.rec.copy_(_pinned_words([head, 0, self.key.data_ptr(), self.val.data_ptr(), 0]), non_blocking=True)
        if isinstance(threshold, torch.Tensor):
            self.rec.view(_F32)[0:1].copy_(threshold.reshape(1).to(_F32))

    @property
    def count_ptr(self) -> int:
        """Device address of the slot counter (uint64): how many slots the launches have handed out so far."""
        return self.rec.data_ptr() + 8

    def counts(self):
        """(slots handed out, unordered candidates scored) -- one device read-back."""
        c = self.rec[[1, 4]].tolist()
        return int(c[0]), int(c[1])                          # (the slot counter is 64-bit: it cannot wrap under the capacity)

    def scores(self, slots: int) -> torch.Tensor:
        """The first ``slots`` score slots as they are: survivors' scores, -inf in untouched slots (``scores_only``)."""
        assert self.scores_only
        return self.val[:min(int(slots), self.capacity)]

    def valid(self, slots: int):
        """(keys, scores) of the survivors among the first ``slots`` slots (unordered): eps_compact_survivors + one host
        read of the count."""
        assert not self.scores_only
        n = min(int(slots), self.capacity)
        dev = self.key.device
        out_k = torch.empty(n, dtype=_I64, device=dev)
        out_v = torch.empty(n, dtype=_F32, device=dev)
        n_out = torch.zeros(1, dtype=_I64, device=dev)
        _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_select_topk_cut_workspace_bytes())
        _call("eps_compact_survivors", dev, self.key, self.val, n, out_k, out_v, n_out, wsp, wsb)
        m = int(n_out.item())
        return out_k[:m], out_v[:m]


def filter_scan(rowptr, col, revpos, fixw, n_nodes: int, columns: torch.Tensor, out: Survivors, max_degree: int,
                splits: Optional[torch.Tensor] = None) -> None:
    """Launch eps_filter_scan over ``columns`` (int32 ids, hand-out order); survivors accumulate in ``out``.
    ``max_degree``: the longest row of the graph (sizes a scratch table); ``splits``: ``row_window_splits`` of the graph
    when ``filter_scan_windows`` reports more than one id window."""
    dev = _need_gpu(rowptr, col, revpos, fixw, columns, splits)
    _csr(rowptr, col); _chk(_I32, revpos=revpos, columns=columns, splits=splits); _chk(_I64, fixw=fixw)
    if revpos.numel() != col.numel() or fixw.numel() != n_nodes:
        raise _lib.EpsError("filter_scan: revpos / fixw do not match the graph")
    ws = _scan_scratch(dev, max_degree)
    _call("eps_filter_scan", dev, rowptr, col, revpos, fixw, splits, n_nodes, col.numel(), int(max_degree), columns,
          columns.numel(), out.rec, ws, ws.numel() * 8, timed=("filter_scan_kernel", columns.numel()))


# ------------------------------------------------------------------ one-pass threshold scan (csrc/scan_pieces.hip, scan_tables.hip, rescore.hip)
def scan_windows() -> int:
    return int(_lib.load().eps_scan_windows())


def scan_cuts(rowptr: torch.Tensor, col: torch.Tensor, bounds: torch.Tensor) -> torch.Tensor:
    """uint16 table [N, M] (stored as int16 bits): entries of every row below each id-window boundary (per-graph table)."""
    dev = _need_gpu(rowptr, col, bounds)
    _csr(rowptr, col); _chk(_I32, bounds=bounds)
    m = scan_windows()
    if bounds.numel() != m + 1:
        raise _lib.EpsError(f"scan_cuts: bounds must hold {m + 1} boundaries")
    n = rowptr.numel() - 1
    out = torch.empty((n, m), dtype=_I16, device=dev)
    _call("eps_scan_cuts", dev, rowptr, col, n, bounds, out)
    return out


def scan_window_paths(rowptr, col, revpos, cuts, heads: Optional[torch.Tensor] = None, columns: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint32 table [N, M] (int32 bits): two-hop half paths of every column per id window (per-graph table of the scan).
    ``heads`` (``scan_heads``): the paths of the rows a column still walks.
    ``columns`` (int32 ids; without heads): only these rows are computed, the rest of the table stays uninitialised
    (eps_scan_window_paths_columns: the bar sample of a graph whose whole-graph table has not been needed yet)."""
    dev = _need_gpu(rowptr, col, revpos, cuts, heads, columns)
    _csr(rowptr, col); _chk(_I32, revpos=revpos, columns=columns); _chk(_I16, cuts=cuts)
    n = rowptr.numel() - 1
    _chk_heads(heads, n)
    out = torch.empty((n, scan_windows()), dtype=_I32, device=dev)
    if columns is None:
        _call("eps_scan_window_paths", dev, rowptr, col, revpos, cuts, n, heads, out)
        return out
    if heads is not None:
        raise _lib.EpsError("scan_window_paths: a column subset comes without a head table")
    _call("eps_scan_window_paths_columns", dev, rowptr, col, revpos, cuts, n, columns, columns.numel(), out)
    return out


def _chk_heads(heads: Optional[torch.Tensor], n_nodes: int) -> None:
    _chk(_I32, heads=heads)
    if heads is not None and tuple(heads.shape) != (n_nodes, 2):
        raise _lib.EpsError("heads: expected the int32 [N, 2] table of scan_heads")


HUB_MAX = 16384           # hub rows a graph's bitmap table holds (eps_scan_hub_rows; the library takes up to 65536).  Main launch on the
                          # ppa-like graph with 4096 / 8192 / 16384 / 32768 rows: 11.27 / 10.40 / 10.00 / 9.87 ms (72 KB per row)


SCAN_MAX_NNZ = 1 << 30         # eps_scan_screen's limit; the row records keep rowptr's LOW word and their call takes no nnz: checked here


def scan_row_records(cuts: torch.Tensor, rowptr: torch.Tensor, fx32: torch.Tensor, nnz: Optional[int] = None) -> torch.Tensor:
    """int32-bits [N, 32]: per node ONE 128-byte line -- its 32 cuts, its first entry, its screening weight (eps_scan_row_records):
    what eps_scan_screen gathers per walked row, out of one table instead of three.  Per (graph, weight table).  ``nnz``: the
    graph's stored entries where the caller has them at hand (col.numel(): no device read) -- the records hold the low 32 bits of
    rowptr and serve a kernel that refuses nnz >= 2^30, so such a graph is refused here, before any launch."""
    if nnz is not None and int(nnz) >= SCAN_MAX_NNZ:
        raise _lib.EpsError(f"scan_row_records: the records keep 32-bit entry positions for eps_scan_screen (nnz < 2^30), got {int(nnz)} entries")
    dev = _need_gpu(cuts, rowptr, fx32)
    _chk(_I16, cuts=cuts); _chk(_I64, rowptr=rowptr); _chk(_I32, fx32=fx32)
    n = fx32.numel()
    if cuts.shape[0] != n or rowptr.numel() != n + 1:
        raise _lib.EpsError("scan_row_records: cuts / rowptr / fx32 do not match")
    buf = torch.empty(n * 32 + 32, dtype=_I32, device=dev)           # (128-byte aligned start inside the allocation)
    off = (-buf.data_ptr() % 128) // 4
    out = buf[off:off + n * 32].view(n, 32)
    _call("eps_scan_row_records", dev, cuts, rowptr, fx32, n, out)
    return out


def scan_column_pack(rowptr, col, revpos, rowrec: torch.Tensor, plan) -> torch.Tensor:
    """int32 [nnz, 8]: the per-column pack of eps_scan_screen's main launch (eps_scan_column_pack): per stored entry, in CSR order,
    what a column's set-up gathers for that neighbour -- id, first entry, weight, reverse position and the cuts of the column's
    first nine pieces in the neighbour's row.  Built from ``plan`` = (pptr, records) and the row records ``rowrec``."""
    pptr, recs = plan
    dev = _need_gpu(rowptr, col, revpos, rowrec, pptr, recs)
    _csr(rowptr, col); _chk(_I32, revpos=revpos, rowrec=rowrec, pptr=pptr, plan=recs)
    n_nodes = rowptr.numel() - 1
    if pptr.numel() != n_nodes + 1 or revpos.numel() != col.numel() or rowrec.numel() != n_nodes * 32:
        raise _lib.EpsError("scan_column_pack: the tables do not match the graph")
    pack = torch.empty((max(col.numel(), 1), 8), dtype=_I32, device=dev)
    _call("eps_scan_column_pack", dev, rowptr, col, revpos, rowrec, pptr, recs, n_nodes, pack)
    return pack


def scan_heads(rowptr, col, fx32: torch.Tensor, n_hub: int, budget: int, max_rows: int = 65535) -> torch.Tensor:
    """int32-bits [N, 2] (x_v, T_v): per column the longest prefix of its row with ids < ``n_hub`` whose screening weights sum
    to T_v <= ``budget`` (table units) -- the rows eps_scan_screen does not walk under a bar (eps_scan_heads)."""
    dev = _need_gpu(rowptr, col, fx32)
    _csr(rowptr, col); _chk(_I32, fx32=fx32)
    n = rowptr.numel() - 1
    if fx32.numel() != n or not 0 <= int(budget) < 1 << 31:
        raise _lib.EpsError("scan_heads: fx32 does not match the graph, or budget outside [0, 2^31)")
    out = torch.empty((n, 2), dtype=_I32, device=dev)
    _call("eps_scan_heads", dev, rowptr, col, fx32, n, int(n_hub), int(budget), int(max_rows), out)
    return out


def scan_hub_row_words(n_nodes: int) -> int:
    return int(_lib.load().eps_scan_hub_row_words(int(n_nodes)))


def scan_hub_rows(rowptr, col, n_hub: int) -> torch.Tensor:
    """int32-bits [n_hub, words]: bit x of row w = "x is a neighbour of hub w" -- the adjacency rows of the first ``n_hub`` ids as
    bitmaps over the id space (eps_scan_hub_rows; per-graph table)."""
    dev = _need_gpu(rowptr, col)
    _csr(rowptr, col)
    n = rowptr.numel() - 1
    out = torch.empty((max(int(n_hub), 1), scan_hub_row_words(n)), dtype=_I32, device=dev)[:int(n_hub)]
    _call("eps_scan_hub_rows", dev, rowptr, col, n, int(n_hub), out)
    return out


def scan_refine(walked: "Survivors", heads, hubrows, fx32, rowptr, col, n_nodes: int, shift: int, out: "Survivors") -> None:
    """Complete the walked sums of a launch with skipped heads (eps_scan_refine): every valid slot of ``walked`` gets its pair's
    exact head term added; sums at or above ``out``'s bar are appended to ``out`` (compact, scores in 2^-shift units x 2^-shift), and ``out`` takes over
    the walk's candidate counter (``rec[4]``)."""
    dev = _need_gpu(heads, hubrows, fx32, rowptr, col)
    _chk_heads(heads, n_nodes); _chk(_I32, hubrows=hubrows, fx32=fx32); _csr(rowptr, col)
    if hubrows.dim() != 2 or hubrows.shape[1] != scan_hub_row_words(n_nodes) or fx32.numel() != n_nodes:
        raise _lib.EpsError("scan_refine: hubrows / fx32 do not match the graph")
    _call("eps_scan_refine", dev, walked.rec, heads, hubrows, hubrows.shape[0], fx32, rowptr, col, n_nodes, int(shift), out.rec,
          timed=("scan_refine", walked.capacity))


def scan_screen_weights(fixw: torch.Tensor, shift: int):
    """(fx32 int32-bits[N], bad int32[1]): the scan's fixed-point weights rounded UP to 2^-shift (at least 1)."""
    dev = _need_gpu(fixw)
    _chk(_I64, fixw=fixw)
    out = torch.empty(fixw.numel(), dtype=_I32, device=dev)
    bad = torch.empty(1, dtype=_I32, device=dev)
    _call("eps_scan_screen_weights", dev, fixw, fixw.numel(), int(shift), out, bad)
    return out, bad


RESCORE_MAX_NNZ = 1 << 30      # eps_rescore_runs[_dev] address col[] with 32-bit byte offsets and take no nnz to check: checked here


def _chk_rescore_nnz(who: str, col: torch.Tensor) -> None:
    if col.numel() >= RESCORE_MAX_NNZ:
        raise _lib.EpsError(f"{who}: col[] is addressed with 32-bit byte offsets (nnz < 2^30), got {col.numel()} entries")


def rescore_runs(rowptr, col, fixw: torch.Tensor, n_nodes: int, keys_by_u: torch.Tensor) -> torch.Tensor:
    """float32 exact scores of the pairs ``keys_by_u`` = (u << 32) | v, sorted ascending (eps_rescore_runs; unit values).
    A graph of 2^30 stored entries or more is refused (the kernel's 32-bit byte offsets into col[])."""
    dev = _need_gpu(rowptr, col, fixw, keys_by_u)
    _csr(rowptr, col); _chk(_I64, fixw=fixw, keys=keys_by_u)
    _chk_rescore_nnz("rescore_runs", col)
    out = torch.empty(keys_by_u.numel(), dtype=_F32, device=dev)
    _call("eps_rescore_runs", dev, rowptr, col, fixw, n_nodes, keys_by_u, keys_by_u.numel(), out,
          timed=("rescore_runs", keys_by_u.numel()))
    return out


def rescore_weighted(rowptr, col, val, node_w: torch.Tensor, n_nodes: int, keys: torch.Tensor) -> torch.Tensor:
    """float32 exact scores of the pairs ``keys`` = (a << 32) | b on an adjacency with stored values (eps_rescore_weighted)."""
    dev = _need_gpu(rowptr, col, val, node_w, keys)
    _csr(rowptr, col, val); _chk(_F32, node_w=node_w); _chk(_I64, keys=keys)
    out = torch.empty(keys.numel(), dtype=_F32, device=dev)
    _call("eps_rescore_weighted", dev, rowptr, col, val, node_w, n_nodes, keys, keys.numel(), out)
    return out


def scan_plan_rewalk(plan, variant: int):
    """(paths walked again in hash-partitioned passes, all paths) of a plan table (eps_scan_plan_rewalk) -- two Python ints."""
    pptr, recs = plan
    dev = _need_gpu(pptr, recs)
    _chk(_I32, pptr=pptr, plan=recs)
    out = torch.empty(2, dtype=_I64, device=dev)
    _call("eps_scan_plan_rewalk", dev, recs, int(pptr[-1].item()), int(variant), out)
    re, total = out.tolist()
    return re, total


def scan_bounds(rowptr, n_nodes: int) -> torch.Tensor:
    """int32 [M + 1]: the id windows of equal stored-entry mass eps_scan_cuts / eps_scan_screen work on (eps_scan_bounds)."""
    dev = _need_gpu(rowptr)
    _chk(_I64, rowptr=rowptr)
    out = torch.empty(scan_windows() + 1, dtype=_I32, device=dev)
    _call("eps_scan_bounds", dev, rowptr, n_nodes, out)
    return out


def scan_row_sums(rowptr, col, fx32: torch.Tensor, bounds: torch.Tensor, n_nodes: int):
    """(ssum int32-bits [N], smax int32-bits [M + 1], min_fx int32-bits [1]): every row's sum of screening weights (clamped to
    2^31 - 1), its suffix maxima at the window boundaries, and the smallest screening weight of a node with two neighbours or
    more (-1 = none) -- eps_scan_row_sums."""
    dev = _need_gpu(rowptr, col, fx32, bounds)
    _csr(rowptr, col); _chk(_I32, fx32=fx32, bounds=bounds)
    m = scan_windows()
    buf = torch.empty(n_nodes + 2 * m + 2, dtype=_I32, device=dev)       # ssum | smax | min_fx | workspace
    ssum, smax, min_fx, ws = buf[:n_nodes], buf[n_nodes:n_nodes + m + 1], buf[n_nodes + m + 1:n_nodes + m + 2], buf[n_nodes + m + 2:]
    _call("eps_scan_row_sums", dev, rowptr, col, fx32, bounds, n_nodes, ssum, smax, min_fx, ws)
    return ssum, smax, min_fx


SCAN_WIDE = 1 << 24        # eps_scan_plan / eps_scan_screen `variant` word, bit 24: packed pieces of single-round columns hold 2^(bits + 1) paths (sketch launches)
SCAN_SKETCH = 1 << 16      # eps_scan_screen's `variant` word, bit 16: packed pieces of single-round columns run as sketch pieces (r06)


def scan_variant_word(variant: int, dmax: Optional[int] = None) -> int:
    """The ``variant`` argument of eps_scan_plan / eps_scan_screen: geometry in the low byte, (dmax + 1) << 8 above it when the
    caller limits the low weight bits a packed / 16-bit direct piece may drop (include/eps_abi.h)."""
    return int(variant) | ((min(int(dmax), 254) + 1) << 8 if dmax is not None else 0)


def scan_plan(rowptr, cuts, wpaths, ssum, smax, bounds, n_nodes: int, shift: int, variant: int, with_d: bool = False,
              heads: Optional[torch.Tensor] = None):
    """(pptr int32-bits [N + 1], records int32 [P, 4]): eps_scan_screen's per-graph plan table (eps_scan_plan, two passes).
    ``with_d``: also the device word that holds the largest number of weight bits a packed / 16-bit direct piece drops.
    ``heads``: the head table ``wpaths`` was built with (a column's sum bound then leaves its skipped head out)."""
    dev = _need_gpu(rowptr, cuts, wpaths, ssum, smax, bounds, heads)
    _chk_heads(heads, n_nodes)
    _chk(_I64, rowptr=rowptr); _chk(_I16, cuts=cuts); _chk(_I32, wpaths=wpaths, ssum=ssum, smax=smax, bounds=bounds)
    tables = (rowptr, cuts, wpaths, ssum, smax, heads, bounds, n_nodes, int(shift), int(variant))
    counts = torch.empty(n_nodes, dtype=_I32, device=dev)
    _call("eps_scan_plan", dev, *tables, counts, None, None, None)
    pptr = torch.zeros(n_nodes + 1, dtype=_I32, device=dev)
    if n_nodes:
        torch.cumsum(counts, 0, dtype=_I32, out=pptr[1:])
    n_rec = int(pptr[-1].item()) if n_nodes else 0
    recs = torch.empty((max(n_rec, 1), 4), dtype=_I32, device=dev)
    d_used = torch.zeros(1, dtype=_I32, device=dev) if with_d else None
    _call("eps_scan_plan", dev, *tables, None, pptr, recs, d_used)
    return (pptr, recs, d_used) if with_d else (pptr, recs)


SCAN_VARIANT = 2          # default workgroup / table geometry of eps_scan_screen (include/eps_abi.h); scan.screen_variant picks per graph


def scan_screen(rowptr, col, revpos, fx32, cuts, bounds, n_nodes: int, columns: torch.Tensor, shift: int, out: "Survivors",
                status: torch.Tensor, variant: Optional[int] = None, val: Optional[torch.Tensor] = None,
                node_w: Optional[torch.Tensor] = None, wpaths: Optional[torch.Tensor] = None,
                ssum: Optional[torch.Tensor] = None, smax: Optional[torch.Tensor] = None, plan=None,
                heads: Optional[torch.Tensor] = None, batch_from: Optional[int] = None, rowrec: Optional[torch.Tensor] = None,
                colrec: Optional[torch.Tensor] = None, pack: Optional[torch.Tensor] = None, light_from: Optional[int] = None,
                lean_from: Optional[int] = None, lean_batch_from: Optional[int] = None) -> None:
    """Launch eps_scan_screen over ``columns``; survivors (screening scores) accumulate in ``out``.  ``val`` / ``node_w``
    (float32 stored values / node weights): the weighted flavour (eps_scan_screen_weighted; ``fx32`` unused).
    ``ssum`` / ``smax`` (int32-bits [N] / [M + 1]; unit-valued graphs): per-node sums of fx32 over the row and their
    suffix maxima at the window boundaries -- they let pieces keep key and sum in one table word (include/eps_abi.h).
    ``plan`` = (pptr, records) from ``scan_plan`` built with the same wpaths / ssum / smax / shift / variant.
    ``heads`` (``scan_heads``; with the wpaths / plan built for it): the launch skips every column's head and ``out.val`` holds
    the walked sums as raw bits -- ``scan_refine`` turns that list into the one a launch without heads reports.
    ``batch_from``: ``columns[batch_from:]`` are handed out eight per draw (light columns at the end of a heaviest-first list).
    ``rowrec`` (``scan_row_records``): per node one 128-byte line with its cuts, first entry and weight.
    ``colrec`` (int32 [len(columns), 8]; ``scan.column_records``): the columns' headers in hand-out order.
    ``pack`` (``scan_column_pack``; main launch only): the per-column pack built from this plan table and these row records.
    ``light_from`` (``scan.light_split``; main launch with sketch pieces only): ``columns[light_from:]`` are single sketch pieces of
    at most 64 rows and 2048 paths + known edges and take the lean kernel of
    csrc/scan_light.hip, one column per wave.
    ``lean_from`` (``scan.light_split``; under the same conditions): ``columns[lean_from:light_from]`` are single-round columns of direct
    and sketch pieces and take the piece kernel's LEAN body in a launch of their own; ``lean_batch_from`` counts within that zone as
    ``batch_from`` does within ``columns[:lean_from]``.  None: no lean zone."""
    pptr, recs = plan if plan is not None else (None, None)
    dev = _need_gpu(rowptr, col, revpos, fx32, cuts, bounds, columns, status, val, node_w, wpaths, ssum, smax, pptr, recs, heads,
                    rowrec, colrec, pack)
    _chk_heads(heads, n_nodes)
    if heads is not None and (pptr is None or val is not None):
        raise _lib.EpsError("scan_screen: a head table comes with the plan table built for it (unit-valued graphs)")
    _chk(_I32, pptr=pptr, plan=recs)
    if pptr is not None and (val is not None or wpaths is None or pptr.numel() != n_nodes + 1):
        raise _lib.EpsError("scan_screen: the plan table does not match the graph (unit-valued graphs with wpaths only)")
    _chk(_I32, wpaths=wpaths, ssum=ssum, smax=smax)
    if (ssum is None) != (smax is None) or (ssum is not None and (ssum.numel() != n_nodes or smax.numel() != scan_windows() + 1)):
        raise _lib.EpsError("scan_screen: ssum / smax do not match the graph")
    if wpaths is not None and tuple(wpaths.shape) != (n_nodes, scan_windows()):
        raise _lib.EpsError("scan_screen: wpaths does not match the graph")
    _csr(rowptr, col, val); _chk(_F32, node_w=node_w); _chk(_I16, cuts=cuts)
    _chk(_I32, revpos=revpos, fx32=fx32, bounds=bounds, columns=columns, status=status, rowrec=rowrec, colrec=colrec, pack=pack)
    if revpos.numel() != col.numel() or cuts.shape[0] != n_nodes or (val is None and fx32.numel() != n_nodes):
        raise _lib.EpsError("scan_screen: revpos / fx32 / cuts do not match the graph")
    if val is not None and (val.numel() != col.numel() or node_w is None or node_w.numel() != n_nodes):
        raise _lib.EpsError("scan_screen: val / node_w do not match the graph")
    variant = SCAN_VARIANT if variant is None else int(variant)
    timed = ("scan_piece_kernel", columns.numel())
    if val is None:
        _call("eps_scan_screen", dev, rowptr, col, revpos, fx32, cuts, wpaths, ssum, smax, pptr, recs, heads, rowrec, pack,
              bounds, n_nodes, col.numel(), columns, colrec, columns.numel(), -1 if batch_from is None else int(batch_from),
              -1 if lean_from is None else int(lean_from), -1 if lean_batch_from is None else int(lean_batch_from),
              -1 if light_from is None else int(light_from), int(shift), variant, out.rec, status, timed=timed)
    else:
        _call("eps_scan_screen_weighted", dev, rowptr, col, val, revpos, node_w, cuts, wpaths, bounds, n_nodes, col.numel(),
              columns, columns.numel(), int(shift), variant, out.rec, status, timed=timed)


def spmm_csr(rowptr, col, val, x: torch.Tensor, bias=None, relu=False, mean=False, out=None) -> torch.Tensor:
    _chk_2d("spmm_csr", x=x, out=out)
    dev = _need_gpu(rowptr, col, val, x, bias, out, row_strided=(x, out))
    _csr(rowptr, col, val); _chk(_F32, x=x, bias=bias, out=out)
    n_rows = rowptr.numel() - 1
    f = x.shape[1]
    _chk_len("spmm_csr", "val", val, col.numel(), "one value per stored entry of col")
    _chk_len("spmm_csr", "bias", bias, f, "one per column of x")
    _chk_out("spmm_csr", out, n_rows, f)
    if out is None:
        out = torch.empty((n_rows, f), dtype=_F32, device=dev)
    _call("eps_spmm_csr", dev, rowptr, col, val, n_rows, x, x.stride(0), f, bias, int(relu), int(mean), out, out.stride(0))
    return out


GAT_MAX_HEADS = 8        # csrc/gat_attend.hip: GA_MAX_HEADS
GAT_SLOPE = 0.2          # the LeakyReLU slope of the published layer


def _gat_tables(who: str, n: int, heads: int, z, s_src, s_dst) -> int:
    """The shared operand checks of the two attention calls -> the row stride of the score tables."""
    f = int(z.shape[1])
    if not 1 <= heads <= GAT_MAX_HEADS or f < 4 or f % (4 * heads):
        raise _lib.EpsError(f"{who}: width {f} with {heads} heads is outside the kernel's domain (1 <= heads <= {GAT_MAX_HEADS}, "
                            f"width a multiple of 4 * heads)")
    if z.shape[0] != n:
        raise _lib.EpsError(f"{who}: z must have one row per node ({n}), got {tuple(z.shape)}")
    for name, s in (("s_src", s_src), ("s_dst", s_dst)):
        if tuple(s.shape) != (n, heads):
            raise _lib.EpsError(f"{who}: {name} must be [{n}, {heads}], got {tuple(s.shape)}")
    lds = s_src.stride(0) if n > 1 else max(heads, s_src.stride(0))
    if n > 1 and s_dst.stride(0) != lds:
        raise _lib.EpsError(f"{who}: s_src and s_dst must share one row stride ({s_src.stride(0)} vs {s_dst.stride(0)})")
    return lds


def _ld16(who: str, name: str, t: torch.Tensor) -> int:
    """The row stride of a float4-read operand: 16-byte aligned rows."""
    ld = t.stride(0) if t.shape[0] > 1 else max(int(t.shape[1]), t.stride(0))
    if ld % 4 or t.data_ptr() % 16:
        raise _lib.EpsError(f"{who}: {name} needs 16-byte aligned rows (row stride {ld} floats, address % 16 = {t.data_ptr() % 16})")
    return ld


def gat_aggregate(rowptr, col, z: torch.Tensor, s_src: torch.Tensor, s_dst: torch.Tensor, heads: int, row0: int = 0,
                  slope: float = GAT_SLOPE, bias=None, relu=False, out=None, want_lse=False):
    """The attention aggregate of GATConv (eps_gat_aggregate): rows [row0, row0 + len(rowptr) - 1) of
    out[i,h,:] = sum_{j in N(i) + {i}} softmax_j(LeakyReLU(s_src[j,h] + s_dst[i,h])) z[j,h,:] (+ bias, ReLU).  ``rowptr``: the row
    block's slice of the graph's (absolute offsets into ``col``); ``z`` float32 [N, heads * C] (a row stride of its own is fine);
    ``s_src`` / ``s_dst`` float32 [N, heads] (two column blocks of one table are fine).  The column ids are the caller's to check
    (< N): the kernel gathers unchecked.  -> out [rows, heads * C], or (out, lse [rows, heads]) with ``want_lse``."""
    _chk_2d("gat_aggregate", z=z, s_src=s_src, s_dst=s_dst, out=out)
    dev = _need_gpu(rowptr, col, z, s_src, s_dst, bias, out, row_strided=(z, s_src, s_dst, out))
    _csr(rowptr, col); _chk(_F32, z=z, s_src=s_src, s_dst=s_dst, bias=bias, out=out)
    n, f, heads, row0 = int(z.shape[0]), int(z.shape[1]), int(heads), int(row0)
    n_rows = rowptr.numel() - 1
    lds = _gat_tables("gat_aggregate", n, heads, z, s_src, s_dst)
    if n_rows < 0 or row0 < 0 or row0 + n_rows > n:
        raise _lib.EpsError(f"gat_aggregate: rows [{row0}, {row0 + n_rows}) are outside the {n} nodes of z")
    _chk_len("gat_aggregate", "bias", bias, f, "one per column of z")
    _chk_out("gat_aggregate", out, n_rows, f)
    if out is None:
        out = torch.empty((n_rows, f), dtype=_F32, device=dev)
    lse = torch.empty((n_rows, heads), dtype=_F32, device=dev) if want_lse else None
    _call("eps_gat_aggregate", dev, rowptr, col, row0, n_rows, n, z, _ld16("gat_aggregate", "z", z), heads, f, s_src, s_dst, lds,
          ctypes.c_float(slope), bias, int(relu), out, _ld16("gat_aggregate", "out", out), lse)
    return (out, lse) if want_lse else out


def gat_aggregate_backward(rowptr, col, z: torch.Tensor, s_src: torch.Tensor, s_dst: torch.Tensor, heads: int, lse: torch.Tensor,
                           out_nobias: torch.Tensor, gout: torch.Tensor, slope: float = GAT_SLOPE):
    """The backward of ``gat_aggregate`` over the whole graph (eps_gat_aggregate_backward), whose pattern must be symmetric (the
    caller's to check: the sums over the rows that attend to j are taken over row j).  ``lse`` and ``out_nobias``: what the
    forward returned without bias and ReLU; ``gout``: the gradient of that output.  -> (gz [N, heads * C], g_s_src [N, heads],
    g_s_dst [N, heads]); the same bits on every call."""
    _chk_2d("gat_aggregate_backward", z=z, s_src=s_src, s_dst=s_dst, lse=lse, out_nobias=out_nobias, gout=gout)
    dev = _need_gpu(rowptr, col, z, s_src, s_dst, lse, out_nobias, gout, row_strided=(z, s_src, s_dst, out_nobias, gout))
    _csr(rowptr, col); _chk(_F32, z=z, s_src=s_src, s_dst=s_dst, lse=lse, out_nobias=out_nobias, gout=gout)
    n, f, heads = int(z.shape[0]), int(z.shape[1]), int(heads)
    who = "gat_aggregate_backward"
    lds = _gat_tables(who, n, heads, z, s_src, s_dst)
    if rowptr.numel() != n + 1:
        raise _lib.EpsError(f"{who}: rowptr holds {rowptr.numel()} offsets, not {n + 1} (the whole graph, one row per row of z)")
    if tuple(lse.shape) != (n, heads):
        raise _lib.EpsError(f"{who}: lse must be [{n}, {heads}], got {tuple(lse.shape)}")
    for name, t in (("out_nobias", out_nobias), ("gout", gout)):
        if tuple(t.shape) != (n, f):
            raise _lib.EpsError(f"{who}: {name} must be [{n}, {f}], got {tuple(t.shape)}")
    gz = torch.empty((n, f), dtype=_F32, device=dev)
    gs, gd, dwork = (torch.empty((n, heads), dtype=_F32, device=dev) for _ in range(3))
    _call("eps_gat_aggregate_backward", dev, rowptr, col, n, z, _ld16(who, "z", z), heads, f, s_src, s_dst, lds, ctypes.c_float(slope),
          lse, out_nobias, _ld16(who, "out_nobias", out_nobias), gout, _ld16(who, "gout", gout), gz, f, gs, gd, dwork)
    return gz, gs, gd


COS_ROW_FLOATS = 32      # xhat rows padded to a multiple of 128 bytes (whole cache lines per gathered row)


def cos_node_features(rowptr, col, val, x: torch.Tensor, want_norm: bool = False):
    """xhat = normalise(x + (A @ x) / (rowsum(A) + 1e-6)), each row divided by max(||row||_2, 1e-8) (eps_cos_node_features).
    ``x``: float32 [N, F] (any F >= 1; a row stride of its own is fine).  -> float32 [N, F] view of an [N, ldh] buffer whose
    rows are 128-byte aligned and whose pad columns are zero (what ``edge_cosines`` reads).  ``want_norm``: -> (xhat, nrm)
    with nrm float32 [N] = max(||x'||_2, 1e-8), what the backward needs (eps_cos_node_features_nrm; the same xhat)."""
    dev = _need_gpu(rowptr, col, val, x, row_strided=(x,))
    _csr(rowptr, col, val); _chk(_F32, x=x)
    n = rowptr.numel() - 1
    if x.dim() != 2 or x.shape[0] != n:
        raise _lib.EpsError(f"cos_node_features: x must be [{n}, F], got {tuple(x.shape)}")
    f = int(x.shape[1])
    if f < 1:
        raise _lib.EpsError("cos_node_features: x needs at least one feature column")
    if val is not None and val.numel() != col.numel():
        raise _lib.EpsError("cos_node_features: val and col differ in length")
    ldh = (f + COS_ROW_FLOATS - 1) // COS_ROW_FLOATS * COS_ROW_FLOATS
    buf = torch.empty((n, ldh), dtype=_F32, device=dev)
    ldx = x.stride(0) if n > 1 else max(f, x.stride(0))
    if want_norm:
        nrm = torch.empty(n, dtype=_F32, device=dev)
        _call("eps_cos_node_features_nrm", dev, rowptr, col, val, n, x, ldx, f, buf, ldh, nrm)
        return buf[:, :f], nrm
    _call("eps_cos_node_features", dev, rowptr, col, val, n, x, ldx, f, buf, ldh)
    return buf[:, :f]


def edge_cosines(rowptr, col, xhat: torch.Tensor, revpos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """c[e] = xhat[row(e)] . xhat[col(e)] for every stored entry -> float32[nnz] (eps_edge_cosines).  ``xhat``: the output of
    ``cos_node_features``.  ``revpos`` (scan.reverse_positions of a SYMMETRIC pattern) computes each undirected entry once."""
    dev = _need_gpu(rowptr, col, xhat, revpos, row_strided=(xhat,))
    _csr(rowptr, col); _chk(_F32, xhat=xhat); _chk(_I32, revpos=revpos)
    n = rowptr.numel() - 1
    if xhat.dim() != 2 or xhat.shape[0] != n:
        raise _lib.EpsError(f"edge_cosines: xhat must be [{n}, F], got {tuple(xhat.shape)}")
    if revpos is not None and revpos.numel() != col.numel():
        raise _lib.EpsError("edge_cosines: revpos and col differ in length")
    f = int(xhat.shape[1])
    ldh = xhat.stride(0) if n > 1 else max(f, xhat.stride(0))
    if f < 1 or ldh % 4 or xhat.data_ptr() % 16:
        raise _lib.EpsError("edge_cosines: xhat needs 16-byte aligned rows of at least one column (cos_node_features output)")
    out = torch.empty(col.numel(), dtype=_F32, device=dev)
    _call("eps_edge_cosines", dev, rowptr, col, n, xhat, ldh, f, revpos, out)
    return out


def pair_cn_backward(rowptr, col, c: torch.Tensor, u, v, g: torch.Tensor) -> torch.Tensor:
    """gc float32[nnz]: the gradient of L w.r.t. the edge cosines ``c`` given g[p] = dL/draw_p of the edge-valued
    common-neighbour sums raw_p = sum_w c[(u_p, w)] c[(v_p, w)] (eps_pair_cn_backward).  Order-independent: the same inputs --
    in any order of the pair list -- give the same bits."""
    dev = _need_gpu(rowptr, col, c, u, v, g)
    _csr(rowptr, col); _chk(_F32, c=c, g=g); _chk(_I32, u=u, v=v)
    if c.numel() != col.numel():
        raise _lib.EpsError("pair_cn_backward: c and col differ in length")
    if u.numel() != v.numel() or g.numel() != u.numel():
        raise _lib.EpsError("pair_cn_backward: u, v and g differ in length")
    n, nnz = rowptr.numel() - 1, col.numel()
    gc = torch.empty(nnz, dtype=_F32, device=dev)
    if nnz == 0:
        return gc
    ws_bytes = int(_lib.load().eps_pair_cn_backward_workspace_bytes(nnz))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=_I64, device=dev)
    _call("eps_pair_cn_backward", dev, rowptr, col, c, n, nnz, u, v, g, u.numel(), gc, ws, ws_bytes)
    return gc


def cos_features_backward(rowptr, col, val, xhat: torch.Tensor, nrm: torch.Tensor, revpos: torch.Tensor, gc: torch.Tensor,
                          want_scaled: bool = False):
    """gxp float32 [N, F]: the gradient w.r.t. the smoothed features x' given ``gc`` = dL/dc per stored entry
    (eps_cos_features_backward): through c[e] = xhat_row(e) . xhat_col(e) and xhat = x' / max(||x'||, 1e-8).  ``xhat``,
    ``nrm``: ``cos_node_features(..., want_norm=True)``; ``revpos``: scan.reverse_positions of the SYMMETRIC pattern.
    ``want_scaled``: -> (gxp, gxp / (rowsum(A) + 1e-6)), the second being what the smoothing's backward multiplies by A.
    Both are views of buffers with 128-byte aligned rows and zero pad columns."""
    dev = _need_gpu(rowptr, col, val, xhat, nrm, revpos, gc, row_strided=(xhat,))
    _csr(rowptr, col, val); _chk(_F32, xhat=xhat, nrm=nrm, gc=gc); _chk(_I32, revpos=revpos)
    n = rowptr.numel() - 1
    if xhat.dim() != 2 or xhat.shape[0] != n or nrm.numel() != n:
        raise _lib.EpsError(f"cos_features_backward: xhat must be [{n}, F] and nrm [{n}], got {tuple(xhat.shape)} and {tuple(nrm.shape)}")
    if revpos is None or revpos.numel() != col.numel() or gc.numel() != col.numel():
        raise _lib.EpsError("cos_features_backward: revpos, gc and col differ in length")
    if val is not None and val.numel() != col.numel():
        raise _lib.EpsError("cos_features_backward: val and col differ in length")
    f = int(xhat.shape[1])
    ldh = xhat.stride(0) if n > 1 else max(f, xhat.stride(0))
    if f < 1 or ldh % 4 or xhat.data_ptr() % 16:
        raise _lib.EpsError("cos_features_backward: xhat needs 16-byte aligned rows of at least one column (cos_node_features output)")
    ldg = (f + COS_ROW_FLOATS - 1) // COS_ROW_FLOATS * COS_ROW_FLOATS
    gxp = torch.empty((n, ldg), dtype=_F32, device=dev)
    gxs = torch.empty((n, ldg), dtype=_F32, device=dev) if want_scaled else None
    _call("eps_cos_features_backward", dev, rowptr, col, val, n, xhat, ldh, f, nrm, revpos, gc, gxp, gxs, ldg)
    return (gxp[:, :f], gxs[:, :f]) if want_scaled else gxp[:, :f]


def gcn_norm(rowptr, col, val) -> torch.Tensor:
    dev = _need_gpu(rowptr, col, val)
    _csr(rowptr, col, val)
    _chk_len("gcn_norm", "val", val, col.numel(), "one value per stored entry of col")
    n_rows = rowptr.numel() - 1
    dis = torch.empty(n_rows, dtype=_F32, device=dev)
    out = torch.empty(col.numel(), dtype=_F32, device=dev)
    _call("eps_gcn_norm", dev, rowptr, col, val, n_rows, dis, out)
    return out


def gemm(a: torch.Tensor, b_nk: torch.Tensor, bias=None, relu=False, out=None, accumulate=False, lower_only=False) -> torch.Tensor:
    """C = act(a @ b_nk.T + bias (+ C)); b_nk is [N,K] (torch.nn.Linear layout).  ``lower_only``: the product is symmetric and
    only its 128 x 128 tiles on and below the diagonal are computed (the rest of ``out`` is left as it is)."""
    _chk_2d("gemm", a=a, b=b_nk, out=out)
    dev = _need_gpu(a, b_nk, bias, out, row_strided=(a, b_nk, out))
    _chk(_F32, a=a, b=b_nk, bias=bias, out=out)
    m, k = a.shape
    n = b_nk.shape[0]
    if b_nk.shape[1] != k:
        raise _lib.EpsError(f"gemm: inner dims differ ({k} vs {b_nk.shape[1]})")
    _chk_len("gemm", "bias", bias, n, "one per row of b")
    _chk_out("gemm", out, m, n)
    if out is None:
        if accumulate:
            raise _lib.EpsError("gemm: accumulate needs out")
        out = torch.empty((m, n), dtype=_F32, device=dev)
    _call("eps_gemm_f32", dev, a, a.stride(0), b_nk, b_nk.stride(0), bias, int(relu) | (2 if lower_only else 0), int(accumulate), out,
          out.stride(0), m, n, k)
    return out


def dense_adjacency(rowptr, col, n_nodes: int, pad_to: int = 128) -> torch.Tensor:
    """float32 [Np, Np] (Np = n_nodes rounded up to ``pad_to``): 1.0 at every stored entry, 0 elsewhere (eps_dense_adjacency)."""
    dev = _need_gpu(rowptr, col)
    _csr(rowptr, col)
    np_ = (int(n_nodes) + pad_to - 1) // pad_to * pad_to
    a = torch.empty((max(np_, 1), max(np_, 1)), dtype=_F32, device=dev)[:np_, :np_]
    _call("eps_dense_adjacency", dev, rowptr, col, int(n_nodes), np_, np_, a)
    return a


def dense_cn_candidates(rowptr, col, n_nodes: int, directed: bool = False, check_symmetric: bool = False, as_rows: bool = False):
    """(keys int64 (v << 32) | u, counts float32) of the 2-hop non-edges of a DENSE unit-valued symmetric graph, column-major (v
    ascending, then u), with their common-neighbour counts: A A^T on the f32 MFMA + a masked read (csrc/dense_cn.hip).  Default:
    every unordered pair once (u < v; lower tiles of the product only); ``directed``: both orientations -- the reference's
    candidate list (filter.py:96-109) in its own order.  ``check_symmetric``: None comes back when A != A^T (a transposed
    compare of the dense matrix: the check costs no table).  ``as_rows``: (rows float32 [E, 3] = (u, v, count), counts) instead
    of keys -- the proposal file's rows written by the kernel itself.  One host read (the list's length; with the check, one more)."""
    dev = _need_gpu(rowptr, col)
    a = dense_adjacency(rowptr, col, n_nodes)
    if check_symmetric and not bool(torch.equal(a, a.t())):
        return None
    c = torch.empty_like(a)
    gemm(a, a, out=c, lower_only=True)               # (symmetric: half the tiles ...
    if directed:                                     #  ... and a transposed copy for the readers of whole rows)
        _call("eps_dense_mirror_lower", dev, c, n_nodes, c.stride(0))
    counts = torch.empty(n_nodes + 1, dtype=_I64, device=dev)
    counts[n_nodes:] = 0
    half = 0 if directed else 1
    _call("eps_dense_candidates", dev, a, c, n_nodes, a.stride(0), half, counts, None, None, None, None)
    colptr = torch.zeros(n_nodes + 1, dtype=_I64, device=dev)
    torch.cumsum(counts[:n_nodes], 0, out=colptr[1:])
    total = int(colptr[-1].item())
    keys = torch.empty((total, 3), dtype=_F32, device=dev) if as_rows else torch.empty(total, dtype=_I64, device=dev)
    vals = torch.empty(total, dtype=_F32, device=dev)
    if total:
        _call("eps_dense_candidates", dev, a, c, n_nodes, a.stride(0), half, None, colptr, None if as_rows else keys, vals,
              keys if as_rows else None)
    return keys, vals


def mlp_decode(h: torch.Tensor, u, v, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
               apply_sigmoid=True) -> torch.Tensor:
    dev = _need_gpu(h, u, v, *weights, *biases)
    _chk(_F32, h=h); _chk(_I32, u=u, v=v)
    _chk_2d("mlp_decode", h=h)
    if u.numel() != v.numel():
        raise _lib.EpsError(f"mlp_decode: u and v differ in length ({u.numel()} vs {v.numel()})")
    hd = h.shape[1]
    L = _decode_layers("mlp_decode", hd, weights, biases)
    n = u.numel()
    out = torch.empty(n, dtype=_F32, device=dev)
    wp = (ctypes.c_void_p * L)(*[w.data_ptr() for w in weights])
    bp = (ctypes.c_void_p * L)(*[b.data_ptr() for b in biases])
    _call("eps_mlp_decode", dev, h, h.shape[0], hd, u, v, n, wp, bp, L, int(apply_sigmoid), out)
    return out


TRAIN_MIN_HIDDEN, TRAIN_MAX_HIDDEN = 32, 256     # csrc/mlp_decode_train.hip: hdim % 4 == 0, 32 <= hdim <= 256, 2 <= layers <= 8


def mask_words(hdim: int) -> int:
    return (int(hdim) + 31) // 32


def pack_mask(mask: torch.Tensor) -> torch.Tensor:
    """bool [..., H] -> int32 [..., ceil(H / 32)]: bit c & 31 of word c // 32 is mask[..., c] (the layout of the ``keep`` /
    ``taken`` masks of eps_mlp_decode_train; the bits past H are zero).  Plain torch ops on the mask's device."""
    hd = mask.shape[-1]
    nw = mask_words(hd)
    m = mask.to(torch.int64)
    if nw * 32 != hd:
        m = torch.nn.functional.pad(m, (0, nw * 32 - hd))
    m = m.reshape(*mask.shape[:-1], nw, 32)
    words = (m << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(-1)
    return (words - ((words >> 31) << 32)).to(torch.int32)          # (uint32 bit patterns held as int32)


def unpack_mask(words: torch.Tensor, hdim: int) -> torch.Tensor:
    """The inverse of ``pack_mask``: int32 [..., ceil(H / 32)] -> bool [..., H]."""
    bits = (words.to(torch.int64)[..., None] >> torch.arange(32, dtype=torch.int64, device=words.device)) & 1
    return bits.reshape(*words.shape[:-1], -1)[..., :hdim].bool()


def _decode_layers(who: str, hd: int, weights, biases):
    L = len(weights)
    if len(biases) != L:
        raise _lib.EpsError(f"{who}: one bias per weight")
    for i, (w, b) in enumerate(zip(weights, biases)):
        _chk(_F32, **{f"w{i}": w, f"b{i}": b})
        exp = (1 if i == L - 1 else hd, hd)
        if tuple(w.shape) != exp:
            raise _lib.EpsError(f"{who}: layer {i} weight {tuple(w.shape)} != {exp} "
                                f"(hidden width must equal the embedding width, last layer out=1)")
        if b.numel() != exp[0]:
            raise _lib.EpsError(f"{who}: layer {i} bias holds {b.numel()} entries, not {exp[0]}")
    return L


def _chk_keep(who: str, keep, L: int, n: int, hd: int) -> None:
    _chk(_I32, keep=keep)
    if keep is not None and tuple(keep.shape) != (L - 1, n, mask_words(hd)):
        raise _lib.EpsError(f"{who}: keep must be int32 {(L - 1, n, mask_words(hd))} (pack_mask), got {tuple(keep.shape)}")


def mlp_decode_train(h: torch.Tensor, u, v, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
                     keep: Optional[torch.Tensor] = None, keep_scale: float = 1.0, apply_sigmoid=True, want_taken=False):
    """The training forward of the decode (eps_mlp_decode_train): ``mlp_decode`` with dropout given as bit masks.  ``keep``:
    int32 [L - 1, E, ceil(H / 32)] (``pack_mask``; None = no dropout); a kept unit is multiplied by ``keep_scale`` after the ReLU.
    -> scores float32 [E], or (scores, taken) with ``want_taken``: the same layout, set where a ReLU output was > 0."""
    dev = _need_gpu(h, u, v, keep, *weights, *biases)
    _chk(_F32, h=h); _chk(_I32, u=u, v=v)
    if h.dim() != 2:
        raise _lib.EpsError("mlp_decode_train: h must be [N, H]")
    hd = h.shape[1]
    L = _decode_layers("mlp_decode_train", hd, weights, biases)
    n = u.numel()
    if v.numel() != n:
        raise _lib.EpsError("u and v differ in length")
    _chk_keep("mlp_decode_train", keep, L, n, hd)
    out = torch.empty(n, dtype=_F32, device=dev)
    taken = torch.zeros((max(L - 1, 0), n, mask_words(hd)), dtype=_I32, device=dev) if want_taken else None
    wp = (ctypes.c_void_p * max(L, 1))(*[w.data_ptr() for w in weights])
    bp = (ctypes.c_void_p * max(L, 1))(*[b.data_ptr() for b in biases])
    _call("eps_mlp_decode_train", dev, h, h.shape[0], hd, u, v, n, wp, bp, L, keep, float(keep_scale), int(apply_sigmoid), out, taken)
    return (out, taken) if want_taken else out


def mlp_decode_backward(h: torch.Tensor, u, v, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
                        grad_out: torch.Tensor, keep: Optional[torch.Tensor] = None, keep_scale: float = 1.0, apply_sigmoid=True,
                        want_h=True, want_params=True):
    """The gradients of ``mlp_decode_train`` (eps_mlp_decode_backward) given ``grad_out`` = dL/d(scores) float32 [E] ->
    (grad_h [N, H] | None, [grad_w[l]] | None, [grad_b[l]] | None).  The same inputs give the same bits on every call: no
    atomics; grad_h sums each node's incidences in the order of a stable sort of cat(u, v), done here."""
    dev = _need_gpu(h, u, v, keep, grad_out, *weights, *biases)
    _chk(_F32, h=h, grad_out=grad_out); _chk(_I32, u=u, v=v)
    if h.dim() != 2:
        raise _lib.EpsError("mlp_decode_backward: h must be [N, H]")
    n_nodes, hd = h.shape
    L = _decode_layers("mlp_decode_backward", hd, weights, biases)
    n = u.numel()
    if v.numel() != n or grad_out.numel() != n:
        raise _lib.EpsError("mlp_decode_backward: u, v and grad_out differ in length")
    _chk_keep("mlp_decode_backward", keep, L, n, hd)
    wts = [w.t().contiguous() for w in weights[:-1]]
    gw = [torch.empty_like(w) for w in weights] if want_params else None
    gb = [torch.empty_like(b) for b in biases] if want_params else None
    gh = torch.empty_like(h) if want_h else None
    order = ptr = None
    if want_h and n:
        ids = torch.cat([u, v]).to(_I64)
        order = torch.sort(ids, stable=True).indices.to(_I32)
        ptr = torch.zeros(n_nodes + 1, dtype=_I64, device=dev)
        torch.cumsum(torch.bincount(ids, minlength=n_nodes)[:n_nodes], 0, out=ptr[1:])
    ws_bytes = int(_lib.load().eps_mlp_decode_backward_workspace_bytes(n, hd, L))
    ws = torch.empty((ws_bytes + 7) // 8 + 2, dtype=_I64, device=dev)
    arr = lambda ts, k: (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() for t in ts])   # noqa: E731
    _call("eps_mlp_decode_backward", dev, h, n_nodes, hd, u, v, n, arr(weights, L), arr(wts, L - 1), arr(biases, L), L, keep,
          float(keep_scale), int(apply_sigmoid), grad_out, order, ptr, arr(gw, L) if want_params else None,
          arr(gb, L) if want_params else None, gh, ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 16), ws_bytes)
    return gh, gw, gb


def _bn_decode_args(who: str, h, u, v, weights, biases):
    """The shared checks of the BatchNorm decode calls -> (n_nodes, hd, n_pairs).  The domain itself (two layers, the width,
    at least two pairs) is the library's to refuse: EPS_EINVAL names the value."""
    _chk(_F32, h=h); _chk(_I32, u=u, v=v)
    if h.dim() != 2:
        raise _lib.EpsError(f"{who}: h must be [N, H]")
    n_nodes, hd = h.shape
    _decode_layers(who, hd, weights, biases)
    if v.numel() != u.numel():
        raise _lib.EpsError(f"{who}: u and v differ in length")
    return n_nodes, hd, u.numel()


def _bn_workspace(n: int, hd: int, L: int, dev):
    """(tensor that owns it, 16-byte aligned address, bytes) of eps_mlp_decode_bn_workspace_bytes (0 outside the domain)."""
    ws_bytes = int(_lib.load().eps_mlp_decode_bn_workspace_bytes(n, hd, L))
    ws = torch.empty((ws_bytes + 7) // 8 + 2, dtype=_I64, device=dev)
    return ws, ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 16), ws_bytes


def mlp_decode_bn_stats(h: torch.Tensor, u, v, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor]):
    """The batch statistics of a two-layer BatchNorm decoder's hidden pre-activation z = (h[u] * h[v]) W0^T + b0
    (eps_mlp_decode_bn_stats) -> (mean, var) float32 [H], var the BIASED variance over the E >= 2 edges.  ``weights`` /
    ``biases``: the layers as they are, [W0, w1] / [b0, b1].  The same inputs give the same bits."""
    dev = _need_gpu(h, u, v, *weights, *biases)
    who = "mlp_decode_bn_stats"
    n_nodes, hd, n = _bn_decode_args(who, h, u, v, weights, biases)
    L = len(weights)
    mean, var = torch.empty(hd, dtype=_F32, device=dev), torch.empty(hd, dtype=_F32, device=dev)
    ws, ws_ptr, ws_bytes = _bn_workspace(n, hd, L, dev)
    arr = lambda ts: (ctypes.c_void_p * max(L, 1))(*[t.data_ptr() for t in ts])   # noqa: E731
    _call("eps_mlp_decode_bn_stats", dev, h, n_nodes, hd, u, v, n, arr(weights), arr(biases), L, mean, var, ws_ptr, ws_bytes)
    return mean, var


def mlp_decode_bn_backward(h: torch.Tensor, u, v, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
                           folded_w: torch.Tensor, folded_b: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor,
                           var: torch.Tensor, eps: float, grad_out: torch.Tensor, keep: Optional[torch.Tensor] = None,
                           keep_scale: float = 1.0, want_h=True):
    """The gradients of the BatchNorm decode (eps_mlp_decode_bn_backward) given ``grad_out`` = dL/d(logits) float32 [E] ->
    (grad_h [N, H] | None, [grad_W0, grad_w1], [grad_b0 (exact zeros), grad_b1], grad_gamma, grad_beta).  ``folded_w`` /
    ``folded_b``: the folded hidden layer the forward ran on (``mlp_decode_train``); ``mean`` / ``var``: ``mlp_decode_bn_stats``.
    The same inputs give the same bits; grad_h sums each node's incidences in the order of a stable sort of cat(u, v)."""
    dev = _need_gpu(h, u, v, keep, grad_out, folded_w, folded_b, gamma, mean, var, *weights, *biases)
    who = "mlp_decode_bn_backward"
    n_nodes, hd, n = _bn_decode_args(who, h, u, v, weights, biases)
    L = len(weights)
    _chk(_F32, grad_out=grad_out, folded_w=folded_w, folded_b=folded_b, gamma=gamma, mean=mean, var=var)
    if grad_out.numel() != n:
        raise _lib.EpsError(f"{who}: u, v and grad_out differ in length")
    if tuple(folded_w.shape) != (hd, hd) or any(t.numel() != hd for t in (folded_b, gamma, mean, var)):
        raise _lib.EpsError(f"{who}: the folded layer must be [{hd}, {hd}] / [{hd}], gamma, mean and var [{hd}]")
    _chk_keep(who, keep, L, n, hd)
    wts = [w.t().contiguous() for w in weights[:-1]]
    gw, gb = [torch.empty_like(w) for w in weights], [torch.empty_like(b) for b in biases]
    ggamma, gbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    gh = torch.empty_like(h) if want_h else None
    order = ptr = None
    if want_h and n:
        ids = torch.cat([u, v]).to(_I64)
        order = torch.sort(ids, stable=True).indices.to(_I32)
        ptr = torch.zeros(n_nodes + 1, dtype=_I64, device=dev)
        torch.cumsum(torch.bincount(ids, minlength=n_nodes)[:n_nodes], 0, out=ptr[1:])
    ws, ws_ptr, ws_bytes = _bn_workspace(n, hd, L, dev)
    arr = lambda ts, k: (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() for t in ts])   # noqa: E731
    _call("eps_mlp_decode_bn_backward", dev, h, n_nodes, hd, u, v, n, arr(weights, L), arr(wts, L - 1), arr(biases, L), L,
          arr([folded_w], 1), arr([folded_b], 1), gamma, mean, var, float(eps), keep, float(keep_scale), grad_out, order, ptr,
          arr(gw, L), arr(gb, L), ggamma, gbeta, gh, ws_ptr, ws_bytes)
    return gh, gw, gb, ggamma, gbeta


SIGNATURES = _lib.SIGNATURES      # name -> (restype, argtypes) of every export: the table tests/test_abi.py holds to the header
BF16_MAX_HIDDEN = 256             # csrc/mlp_decode_bf16.hip: hdim % 16 == 0 && hdim <= 256, 2 <= layers


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """The bfloat16 bit patterns of a float32 tensor (int16 storage, same shape), rounded to nearest even as torch's
    ``.to(torch.bfloat16)`` rounds (eps_f32_to_bf16)."""
    dev = _need_gpu(x)
    _chk(_F32, x=x)
    out = torch.empty(x.shape, dtype=_I16, device=dev)
    _call("eps_f32_to_bf16", dev, x, x.numel(), out)
    return out


def mlp_decode_bf16(h: torch.Tensor, u, v, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
                    apply_sigmoid=True) -> torch.Tensor:
    """``mlp_decode`` on the bf16 matrix cores (eps_mlp_decode_bf16): ``h`` [N, H] and the hidden ``weights`` [H, H] are bf16
    bit patterns (int16, from ``to_bf16``); the last weight [1, H] and every bias are float32.  -> float32 [E]."""
    dev = _need_gpu(h, u, v, *weights, *biases)
    _chk(_I16, h=h); _chk(_I32, u=u, v=v)
    L = len(weights)
    if h.dim() != 2 or len(biases) != L:
        raise _lib.EpsError("mlp_decode_bf16: h must be [N, H], with one bias per weight")
    hd = h.shape[1]
    for i, (w, b) in enumerate(zip(weights, biases)):
        _chk(_I16 if i < L - 1 else _F32, **{f"w{i}": w}); _chk(_F32, **{f"b{i}": b})
        exp = (1 if i == L - 1 else hd, hd)
        if tuple(w.shape) != exp:
            raise _lib.EpsError(f"mlp_decode_bf16: layer {i} weight {tuple(w.shape)} != {exp} "
                                f"(hidden width must equal the embedding width, last layer out=1)")
        if b.numel() != exp[0]:
            raise _lib.EpsError(f"mlp_decode_bf16: layer {i} bias holds {b.numel()} entries, not {exp[0]}")
    n = u.numel()
    if v.numel() != n:
        raise _lib.EpsError("u and v differ in length")
    out = torch.empty(n, dtype=_F32, device=dev)
    wp = (ctypes.c_void_p * max(L, 1))(*[w.data_ptr() for w in weights])
    bp = (ctypes.c_void_p * max(L, 1))(*[b.data_ptr() for b in biases])
    _call("eps_mlp_decode_bf16", dev, h, h.shape[0], hd, u, v, n, wp, bp, L, int(apply_sigmoid), out)
    return out


def kth_largest(x: torch.Tensor, k: int) -> torch.Tensor:
    """The k-th largest value of a float32 device vector (1-element device tensor; no host round trip): radix select."""
    dev = _need_gpu(x)
    _chk(_F32, x=x)
    out = torch.empty(1, dtype=_F32, device=dev)
    ws = torch.empty((int(_lib.load().eps_kth_largest_workspace_bytes()) + 7) // 8, dtype=_I64, device=dev)
    _call("eps_kth_largest_f32", dev, x, x.numel(), int(k), out, ws)
    return out


SEGMENT_TOPK_WAVE_MAX = 256    # csrc/segment_topk.hip SEG_WAVE_MAX: segments up to this long are one wave's work (keys in registers)
SEGMENT_TOPK_LDS_MAX = 8192    # ... SEG_LDS_MAX: up to this long one workgroup's with the keys in LDS; longer ones are streamed
                               # (eps_segment_topk_class_max(0 / 1) answers the same: tests/test_per_node_host.py holds the two together)


def segment_topk(colptr: torch.Tensor, score: torch.Tensor, k: int, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Positions (int64, into ``score``) of the ``k`` best entries of every segment of ``score`` -- segment s is
    [colptr[s], colptr[s + 1]), or [colptr[s], colptr[s] + counts[s]) in the padded layout of a ``ColumnBlock`` -- in the
    declared order: score descending (``ordered_bits``), then position ascending.  A segment with at most ``k`` entries keeps
    all of them.  The positions are ascending within each segment and the segments follow each other, so the result as a
    whole is ascending: candidate order (eps_segment_topk; one host read, the size of the result)."""
    dev = _need_gpu(colptr, score, counts)
    _chk(_I64, colptr=colptr, counts=counts); _chk(_F32, score=score)
    k = int(k)
    if colptr.dim() != 1 or colptr.numel() < 1 or score.dim() != 1:
        raise _lib.EpsError(f"segment_topk: colptr [n_seg + 1] and score [E] are vectors (got {tuple(colptr.shape)}, {tuple(score.shape)})")
    n_seg = colptr.numel() - 1
    if counts is not None and counts.shape != (n_seg,):
        raise _lib.EpsError(f"segment_topk: counts holds {tuple(counts.shape)} entries for {n_seg} segments")
    if k < 1:                      # (the library refuses it too; no tensor work for a call that cannot run)
        raise _lib.EpsError(f"segment_topk: k={k} must lie in [1, 2^31)")
    lens = (colptr[1:] - colptr[:-1]) if counts is None else counts
    outptr = torch.zeros(n_seg + 1, dtype=_I64, device=dev)
    torch.cumsum(torch.clamp(lens, min=0, max=k), 0, out=outptr[1:])
    order = torch.argsort(lens, descending=True, stable=True).to(_I32)       # heaviest first, like candidates.heaviest_first
    if n_seg:
        # (one host read: the result's size, and that every segment lies inside the score array)
        total, lo, hi = torch.stack([outptr[-1], colptr[:-1].min(), (colptr[:-1] + torch.clamp(lens, min=0)).max()]).tolist()
        if lo < 0 or hi > score.numel():
            raise _lib.EpsError(f"segment_topk: segments span [{lo}, {hi}) of a score array of {score.numel()} entries")
    else:
        total = 0
    out = torch.empty(total, dtype=_I64, device=dev)
    _call("eps_segment_topk", dev, colptr, counts, score, n_seg, k, outptr, order, out)
    return out


LOCAL_INDEX = {"salton": 0, "jaccard": 1, "sorensen": 2, "hpi": 3, "hdi": 4, "lhn": 5, "pa": 6}     # csrc/local_index.hip: name -> code


def _local_index_code(index) -> int:
    if isinstance(index, str):
        if index not in LOCAL_INDEX:
            raise _lib.EpsError(f"local index '{index}': one of {', '.join(LOCAL_INDEX)}")
        return LOCAL_INDEX[index]
    return int(index)          # (the library refuses a code outside the table)


def local_index_pairs(rowptr, n_nodes: int, u, v, cn, index) -> torch.Tensor:
    """-> float32[E]: the local index ``index`` (a name of ``LOCAL_INDEX`` or its code) of the pairs (u[p], v[p]) whose numbers
    of common stored neighbours are ``cn`` (int32: the ``count`` of ``pair_scores``); degrees are rowptr differences, float64
    arithmetic, one rounding (eps_local_index_pairs).  Any pair may be listed; an id outside the graph scores NaN."""
    dev = _need_gpu(rowptr, u, v, cn)
    _chk(_I64, rowptr=rowptr); _chk(_I32, u=u, v=v, cn=cn)
    n_nodes = int(n_nodes)
    if rowptr.numel() != n_nodes + 1:
        raise _lib.EpsError(f"local_index_pairs: rowptr must hold {n_nodes + 1} entries, got {rowptr.numel()}")
    if u.numel() != v.numel() or u.numel() != cn.numel():
        raise _lib.EpsError("local_index_pairs: u, v and cn differ in length")
    out = torch.empty(u.numel(), dtype=_F32, device=dev)
    _call("eps_local_index_pairs", dev, rowptr, n_nodes, u, v, cn, u.numel(), _local_index_code(index), out,
          timed=("local_index_pairs_kernel", u.numel()))
    return out


def local_index_columns(rowptr, n_nodes: int, v_lo: int, v_hi: int, colptr, cand_u, cn, index, counts=None, bar=None,
                        capacity: int = 0, out: Optional[torch.Tensor] = None, check: bool = True, stats: Optional[dict] = None):
    """The local index ``index`` of a column-major candidate block (eps_local_index_columns): slot p of ``cand_u`` (int32) is the
    pair (cand_u[p], v_lo + s) for the segment s = [colptr[s], colptr[s + 1]) that holds p -- with ``counts`` (int64 per
    column) only [colptr[s], colptr[s] + counts[s]): the padded layout, whose other slots are neither read nor written.  ``cn``:
    the common-neighbour counts per slot, int32 (``expand_candidates`` want_cn) or float32 holding the integer (the unit-weight
    score of ``expand_unit``; n_nodes < 2^24).

    ``bar`` None -> float32 scores per slot (into ``out`` when given; padding slots keep what they held).
    ``bar`` (a float, or a 1-element float32 device tensor) -> ``(positions int64 ascending, scores)`` of the slots whose score
    EXCEEDS it, or None when more than ``capacity`` do (score the block in full then); ``out`` is filled as well when given.
    ``stats`` (a dict) receives ``n_surv``, the true number of such slots, either way.

    ``check``: the ids of the live slots and the ends and order of ``colptr`` (and ``counts`` within the segments) are verified
    here, on the host, before the launch (one read).  ``check=False`` is for lists that have just come out of the expansion
    kernels: the kernel itself scores NaN for an id outside the graph and reads no slot beyond the list."""
    dev = _need_gpu(rowptr, colptr, cand_u, cn, counts, out, bar if isinstance(bar, torch.Tensor) else None)
    _chk(_I64, rowptr=rowptr, colptr=colptr, counts=counts); _chk(_I32, cand_u=cand_u); _chk(_F32, out=out)
    if cn.dtype not in (_I32, _F32):
        raise _lib.EpsError(f"local_index_columns: cn is int32 or float32, got {cn.dtype}")
    v_lo, v_hi, n_nodes, capacity = int(v_lo), int(v_hi), int(n_nodes), int(capacity)
    n_cols, n = v_hi - v_lo, cand_u.numel()
    if rowptr.numel() != n_nodes + 1:
        raise _lib.EpsError(f"local_index_columns: rowptr must hold {n_nodes + 1} entries, got {rowptr.numel()}")
    if not 0 <= v_lo <= v_hi <= n_nodes:
        raise _lib.EpsError(f"local_index_columns: columns [{v_lo}, {v_hi}) outside [0, {n_nodes}]")
    if colptr.numel() != n_cols + 1 or (counts is not None and counts.numel() != n_cols):
        raise _lib.EpsError(f"local_index_columns: colptr must hold {n_cols + 1} entries (counts {n_cols}), got {colptr.numel()}"
                            + ("" if counts is None else f" ({counts.numel()})"))
    if cn.numel() != n or (out is not None and out.numel() != n):
        raise _lib.EpsError(f"local_index_columns: cn / out must hold one entry per slot of cand_u ({n})")
    if check and n:
        width = colptr[1:] - colptr[:-1]
        facts = [colptr[0], colptr[-1], width.min()]
        if counts is None:
            lo, hi = torch.aminmax(cand_u)
        else:
            facts += [counts.min(), (width - counts).min()]
            pos = torch.arange(n, dtype=_I64, device=dev)
            seg = torch.searchsorted(colptr[1:].contiguous(), pos, right=True).clamp_(max=n_cols - 1)
            live = cand_u[(pos - colptr[seg]) < counts[seg]]
            lo, hi = torch.aminmax(live) if live.numel() else (cand_u.new_zeros(()), cand_u.new_zeros(()))
        facts = torch.stack([x.to(_I64) for x in facts + [lo, hi]]).tolist()
        if facts[0] != 0 or facts[1] != n or facts[2] < 0:
            raise _lib.EpsError(f"local_index_columns: colptr must ascend from 0 to {n} (the slots), got {facts[0]} .. {facts[1]}")
        if counts is not None and (facts[3] < 0 or facts[4] < 0):
            raise _lib.EpsError("local_index_columns: counts must lie within the segments of colptr")
        if facts[-2] < 0 or facts[-1] >= n_nodes:
            raise _lib.EpsError(f"local_index_columns: node ids must lie in [0, {n_nodes}), got [{facts[-2]}, {facts[-1]}]")
    code = _local_index_code(index)
    cn_i, cn_f = (cn, None) if cn.dtype == _I32 else (None, cn)
    if bar is None:
        score = out if out is not None else torch.empty(n, dtype=_F32, device=dev)
        _call("eps_local_index_columns", dev, rowptr, n_nodes, v_lo, v_hi, colptr, counts, cand_u, n, cn_i, cn_f, code, score,
              None, 0, None, None, None, None, 0, timed=("local_index_columns_kernel", n))
        return score
    if not isinstance(bar, torch.Tensor):
        bar = torch.tensor([float(bar)], dtype=_F32, device=dev)
    _chk(_F32, bar=bar)
    if bar.numel() != 1 or capacity < 0:
        raise _lib.EpsError(f"local_index_columns: bar is one float32 and capacity >= 0, got {bar.numel()} entries, capacity {capacity}")
    pos = torch.empty(capacity, dtype=_I64, device=dev)
    val = torch.empty(capacity, dtype=_F32, device=dev)
    n_surv = torch.zeros(1, dtype=_I64, device=dev)
    ws_bytes = int(_lib.load().eps_local_index_columns_workspace_bytes(n))
    ws = _scratch("local_index", dev, (ws_bytes + 7) // 8, (ws_bytes + 7) // 8) if ws_bytes else None
    _call("eps_local_index_columns", dev, rowptr, n_nodes, v_lo, v_hi, colptr, counts, cand_u, n, cn_i, cn_f, code, out,
          bar, capacity, pos, val, n_surv, ws, ws_bytes,
          timed=("local_index_columns_kernel", n))
    m = int(n_surv.item())
    if stats is not None:
        stats["n_surv"] = m
    return None if m > capacity else (pos[:m], val[:m])


def pair_cn_list_limits() -> Tuple[int, int]:
    """(long-row entries staged in LDS per pass, ratio long / short from which a longer row is searched in place) of the
    common-neighbour list kernel: the sizes at which it changes its path (host-only query)."""
    cap, ratio = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.load().eps_pair_cn_list_limits(ctypes.byref(cap), ctypes.byref(ratio)), "eps_pair_cn_list_limits")
    return cap.value, ratio.value


def _limits(name: str, k: int) -> Tuple[int, ...]:
    out = [ctypes.c_int32(0) for _ in range(k)]
    _lib.check(getattr(_lib.load(), name)(*[ctypes.byref(x) for x in out]), name)
    return tuple(x.value for x in out)


def pair_scores_limits() -> Tuple[int, int, int, int, int, int]:
    """(PI_SMALL, PI_CAP, PI_QCAP, PI_INPLACE_RATIO, PI_TICKET, PI_CLS_STRIDE) of the generic pair-score kernel: the sizes at
    which it changes its path (include/eps_abi.h; host-only query)."""
    return _limits("eps_pair_scores_limits", 6)


def pair_scores_grouped_limits() -> Tuple[int, int, int, int]:
    """(PG_CHUNK, PG_QCAP, the exact bitmap's bits, PG_RING) of the column-run pair-score kernel (host-only query)."""
    return _limits("eps_pair_scores_grouped_limits", 4)


def rescore_limits() -> Tuple[int, int, int]:
    """(RS_BITS, RS_SHORT, RS_CHUNK) of eps_rescore_runs: ids per bitmap window, the longest short row, pairs per chunk
    (host-only query)."""
    return _limits("eps_rescore_limits", 3)


def _cn_list_args(who: str, rowptr, col, n_nodes: int, u, v, check: bool) -> torch.device:
    dev = _need_gpu(rowptr, col, u, v)
    _csr(rowptr, col); _chk(_I32, u=u, v=v)
    if rowptr.numel() != n_nodes + 1:
        raise _lib.EpsError(f"{who}: rowptr must hold {n_nodes + 1} entries, got {rowptr.numel()}")
    if u.dim() != 1 or u.shape != v.shape:
        raise _lib.EpsError(f"{who}: u and v are two vectors of one length, got {tuple(u.shape)} and {tuple(v.shape)}")
    if check and u.numel():
        lo, hi = torch.stack([torch.minimum(u.min(), v.min()), torch.maximum(u.max(), v.max())]).tolist()
        if lo < 0 or hi >= n_nodes:
            raise _lib.EpsError(f"{who}: node ids must lie in [0, {n_nodes}), got [{lo}, {hi}]")
    return dev


def pair_cn_list_count(rowptr, col, n_nodes: int, u, v, check: bool = True) -> torch.Tensor:
    """-> int32[B]: |N(u_b) & N(v_b)| on the stored pattern (eps_pair_cn_list_count): the counts ``pair_cn_list_fill``'s pointers
    are the prefix of.  ``check=False``: a pair with an id outside the graph counts 0 (the kernel reads nothing for it)."""
    n_nodes = int(n_nodes)
    dev = _cn_list_args("pair_cn_list_count", rowptr, col, n_nodes, u, v, check)
    count = torch.empty(u.numel(), dtype=_I32, device=dev)
    if u.numel():
        _call("eps_pair_cn_list_count", dev, rowptr, col, n_nodes, u, v, u.numel(), count, timed=("pair_cn_list_kernel<count>", u.numel()))
    return count


def pair_cn_list_fill(rowptr, col, n_nodes: int, u, v, ptr: torch.Tensor, out_w: torch.Tensor, check: bool = True) -> torch.Tensor:
    """Writes the common neighbours of pair b, ascending, to out_w[ptr[b] : ptr[b + 1]] (eps_pair_cn_list_fill) and returns
    ``out_w``.  ``ptr`` (int64[B + 1]) is the exclusive prefix of ``pair_cn_list_count`` of the same pairs; with any other ``ptr``
    nothing is stored at or past ptr[b + 1] or ptr[B], and the call raises EpsError (one read of the status word)."""
    n_nodes = int(n_nodes)
    dev = _cn_list_args("pair_cn_list_fill", rowptr, col, n_nodes, u, v, check)
    _need_gpu(rowptr, ptr, out_w)
    _chk(_I64, ptr=ptr); _chk(_I32, out_w=out_w)
    if ptr.numel() != u.numel() + 1:
        raise _lib.EpsError(f"pair_cn_list_fill: ptr must hold {u.numel() + 1} entries, got {ptr.numel()}")
    if u.numel() == 0:
        return out_w
    m = int(ptr[-1].item())
    if not 0 <= m <= out_w.numel() or m >= 1 << 31:
        raise _lib.EpsError(f"pair_cn_list_fill: ptr ends at {m}: out_w holds {out_w.numel()} entries and a list fewer than 2^31")
    status = torch.empty(1, dtype=_I32, device=dev)
    _call("eps_pair_cn_list_fill", dev, rowptr, col, n_nodes, u, v, u.numel(), ptr, out_w, status, timed=("pair_cn_list_kernel<fill>", u.numel()))
    if int(status.item()) != 0:
        raise _lib.EpsError("pair_cn_list_fill: a segment of ptr is not as long as its pair's list of common neighbours (ptr is not "
                            "the prefix of pair_cn_list_count of these pairs on this graph); nothing was stored outside the segments")
    return out_w


def pair_cn_list(rowptr, col, n_nodes: int, u, v, check: bool = True, count: Optional[torch.Tensor] = None):
    """-> (ptr int64[B + 1], w int32[M]): the common STORED neighbours of every pair (u[b], v[b]) as CSR rows, w ascending per
    pair -- so the lists of (u, v) and (v, u) are equal; stored values are ignored, u == v lists the whole row.  Count, prefix,
    fill: two launches of one kernel and one read of M (which must stay below 2^31).  ``check``: the ids are verified on the host
    first; ``check=False`` gives a pair with an id outside the graph an empty segment.  ``count``: the counts of exactly these
    pairs when the caller has them already.  B == 0 and M == 0 launch nothing that dereferences a list."""
    n_nodes = int(n_nodes)
    if count is None:
        count = pair_cn_list_count(rowptr, col, n_nodes, u, v, check)
    else:
        _cn_list_args("pair_cn_list", rowptr, col, n_nodes, u, v, check)
        _chk(_I32, count=count)
        if count.shape != u.shape:
            raise _lib.EpsError("pair_cn_list: one count per pair")
    dev = count.device
    ptr = torch.zeros(u.numel() + 1, dtype=_I64, device=dev)
    if u.numel():
        torch.cumsum(count, 0, dtype=_I64, out=ptr[1:])
    m = int(ptr[-1].item()) if u.numel() else 0
    if m >= 1 << 31:
        raise _lib.EpsError(f"pair_cn_list: {m} common neighbours in one list; a list holds fewer than 2^31 (split the pairs)")
    w = torch.empty(m, dtype=_I32, device=dev)
    if m:
        pair_cn_list_fill(rowptr, col, n_nodes, u, v, ptr, w, check=False)
    return ptr, w


def cn_list_transpose(ptr: torch.Tensor, w: torch.Tensor, n_nodes: int, check: bool = True):
    """-> (tptr int64[n_nodes + 1], tb int32[M]): the incidence of ``pair_cn_list`` by node -- the pairs that list w are
    tb[tptr[w] : tptr[w + 1]], ascending in b (eps_cn_list_transpose: a stable radix sort, no atomics: a function of the input
    alone).  ``check``: ptr ascends from 0 to M and every w lies in [0, n_nodes) (one read)."""
    dev = _need_gpu(ptr, w)
    _chk(_I64, ptr=ptr); _chk(_I32, w=w)
    n_nodes, m, n_pairs = int(n_nodes), w.numel(), ptr.numel() - 1
    if n_pairs < 0 or n_nodes < 0 or m >= 1 << 31:
        raise _lib.EpsError(f"cn_list_transpose: ptr holds B + 1 entries, n_nodes >= 0 and M < 2^31 (got {ptr.numel()}, {n_nodes}, {m})")
    if check and m:
        facts = torch.stack([ptr[0], ptr[-1], (ptr[1:] - ptr[:-1]).min(), w.min().to(_I64), w.max().to(_I64)]).tolist()
        if facts[0] != 0 or facts[1] != m or facts[2] < 0:
            raise _lib.EpsError(f"cn_list_transpose: ptr must ascend from 0 to {m} (the entries of w), got {facts[0]} .. {facts[1]}")
        if facts[3] < 0 or facts[4] >= n_nodes:
            raise _lib.EpsError(f"cn_list_transpose: w must lie in [0, {n_nodes}), got [{facts[3]}, {facts[4]}]")
    elif check and n_pairs >= 0 and ptr.numel() and int(ptr[-1].item()) != 0:
        raise _lib.EpsError("cn_list_transpose: ptr names entries but w is empty")
    tptr = torch.empty(n_nodes + 1, dtype=_I64, device=dev)
    tb = torch.empty(m, dtype=_I32, device=dev)
    ws, ws_ptr, ws_bytes = _aligned_ws(dev, int(_lib.load().eps_cn_list_transpose_workspace_bytes(m, n_nodes))) if m else (None, None, 0)
    _call("eps_cn_list_transpose", dev, ptr, w, m, n_pairs, n_nodes, tptr, tb, ws_ptr, ws_bytes, timed=("cn_list_transpose", m))
    return tptr, tb


LOCAL_COMMUNITY_INDEX = {"car": 0, "cpa": 1, "caa": 2, "cra": 3, "cjc": 4}     # csrc/local_community.hip: name -> code


def _local_community_code(index) -> int:
    if isinstance(index, str):
        if index not in LOCAL_COMMUNITY_INDEX:
            raise _lib.EpsError(f"local-community index '{index}': one of {', '.join(LOCAL_COMMUNITY_INDEX)}")
        return LOCAL_COMMUNITY_INDEX[index]
    return int(index)          # (the library refuses a code outside the table)


def local_community_limits() -> Tuple[int, int, int]:
    """(list length up to which the ordered pairs of a list are dealt over the lanes, list entries staged in LDS per pass, ratio
    row / staged entries from which a row is searched in place) of the local-community degree kernel: the sizes at which it
    changes its path (host-only query)."""
    short, cap, ratio = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.load().eps_local_community_limits(ctypes.byref(short), ctypes.byref(cap), ctypes.byref(ratio)),
               "eps_local_community_limits")
    return short.value, cap.value, ratio.value


def _list_args(who: str, ptr, w, **same_length) -> int:
    """The checks every consumer of a (ptr, w) list makes before a launch: ptr holds B + 1 entries, M < 2^31, and the arrays
    named in ``same_length`` hold one entry per entry of w.  -> B."""
    _chk(_I64, ptr=ptr); _chk(_I32, w=w)
    if ptr.dim() != 1 or ptr.numel() < 1 or w.dim() != 1:
        raise _lib.EpsError(f"{who}: ptr holds B + 1 entries and w is a vector, got {tuple(ptr.shape)} and {tuple(w.shape)}")
    if w.numel() >= 1 << 31:
        raise _lib.EpsError(f"{who}: {w.numel()} entries in one list; a list holds fewer than 2^31 (split the pairs)")
    for name, t in same_length.items():
        _chk_len(who, name, t, w.numel(), "one per entry of w")
    return ptr.numel() - 1


def local_community_degrees(rowptr, col, n_nodes: int, ptr, w, check: bool = True, out: Optional[torch.Tensor] = None,
                            stats: Optional[dict] = None) -> torch.Tensor:
    """-> int32[M]: gamma[i] = the number of stored entries of row w[i] that occur in the segment of ``ptr`` holding i, other than
    w[i] itself (eps_local_community_degrees) -- for the lists of ``pair_cn_list`` the local-community degree of every common
    neighbour; any strictly ascending segments of node ids are taken.  A segment that does not ascend, or holds an id outside
    the graph, gets zeros (nothing is read for it) and raises EpsError -- with ``stats`` (a dict) given its ``status`` is stored
    there instead.  ``check``: ptr ascends from 0 to M, verified on the host first (one read); ``check=False`` is for lists that
    have just come out of the list kernel.  ``out``: an int32[M] tensor to write into."""
    n_nodes = int(n_nodes)
    _csr(rowptr, col); _chk(_I32, out=out)              # (dtypes and lengths first: they are refused the same on any device)
    n_pairs = _list_args("local_community_degrees", ptr, w, out=out)
    if rowptr.numel() != n_nodes + 1:
        raise _lib.EpsError(f"local_community_degrees: rowptr must hold {n_nodes + 1} entries, got {rowptr.numel()}")
    dev = _need_gpu(rowptr, col, ptr, w, out)
    m = w.numel()
    if check:
        facts = torch.stack([ptr[0], ptr[-1], (ptr[1:] - ptr[:-1]).min() if n_pairs else ptr[0] * 0]).tolist()
        if facts[0] != 0 or facts[1] != m or facts[2] < 0:
            raise _lib.EpsError(f"local_community_degrees: ptr must ascend from 0 to {m} (the entries of w), got {facts[0]} .. {facts[1]}")
    gamma = out if out is not None else torch.empty(m, dtype=_I32, device=dev)
    if n_pairs == 0 or m == 0:
        if stats is not None:
            stats["status"] = 0
        return gamma
    status = torch.empty(1, dtype=_I32, device=dev)
    _call("eps_local_community_degrees", dev, rowptr, col, n_nodes, ptr, w, n_pairs, gamma, status,
          timed=("local_community_degrees_kernel", m))
    if stats is not None:
        stats["status"] = int(status.item())
    elif check and int(status.item()) != 0:
        raise _lib.EpsError("local_community_degrees: a segment does not ascend strictly or holds an id outside the graph (its "
                            "entries got 0; nothing was read for them)")
    return gamma


def local_community_scores(rowptr, n_nodes: int, u, v, ptr, w, gamma, index, check: bool = True) -> torch.Tensor:
    """-> float32[B]: the local-community index ``index`` (a name of ``LOCAL_COMMUNITY_INDEX`` or its code) of the pairs
    (u[b], v[b]) whose common neighbours are w[ptr[b] : ptr[b + 1]] with the degrees ``gamma`` of ``local_community_degrees``
    (eps_local_community_scores): float64 on the integers, the sums in a fixed association of the list positions, one rounding.
    ``w`` and ``gamma`` both None: nothing is listed, ``ptr`` is the prefix of the counts alone and every pair gets its closed
    form without links among its common neighbours (what the pairs with fewer than two have).  An id outside the graph scores
    NaN.  ``check``: ptr ends at M, the entries of w, verified on the host first (one read; the kernel reads no entry at or
    past ptr[B]); ``check=False`` is for lists that have just come out of the list kernel."""
    n_nodes = int(n_nodes)
    _chk(_I64, rowptr=rowptr, ptr=ptr); _chk(_I32, u=u, v=v, w=w, gamma=gamma)
    if (w is None) != (gamma is None):
        raise _lib.EpsError("local_community_scores: w and gamma come together (both None: closed forms)")
    if rowptr.numel() != n_nodes + 1:
        raise _lib.EpsError(f"local_community_scores: rowptr must hold {n_nodes + 1} entries, got {rowptr.numel()}")
    if u.dim() != 1 or u.shape != v.shape:
        raise _lib.EpsError(f"local_community_scores: u and v are two vectors of one length, got {tuple(u.shape)} and {tuple(v.shape)}")
    if ptr.numel() != u.numel() + 1:
        raise _lib.EpsError(f"local_community_scores: ptr must hold {u.numel() + 1} entries, got {ptr.numel()}")
    if w is not None:
        _list_args("local_community_scores", ptr, w, gamma=gamma)
        if check and int(ptr[-1].item()) != w.numel():
            raise _lib.EpsError(f"local_community_scores: ptr must end at {w.numel()} (the entries of w), got {int(ptr[-1].item())}")
    code = _local_community_code(index)
    dev = _need_gpu(rowptr, u, v, ptr, w, gamma)
    out = torch.empty(u.numel(), dtype=_F32, device=dev)
    if u.numel():
        _call("eps_local_community_scores", dev, rowptr, n_nodes, u, v, ptr, w, gamma, u.numel(), code, out,
              timed=("local_community_scores_kernel", u.numel()))
    return out


SKETCH_REGS, SKETCH_WORDS = 256, 128     # csrc/sketch.hip: HyperLogLog registers (bytes) and MinHash words (uint32) per sketch
_U8, _U32 = torch.uint8, torch.uint32


def sketch_limits() -> Tuple[int, int]:
    """(row length above which ``sketch_propagate`` reduces a row piecewise on several waves, pairs per wave of
    ``sketch_pair_stats``): the sizes at which the sketch kernels change their path (host-only query)."""
    chunk, ppw = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.load().eps_sketch_limits(ctypes.byref(chunk), ctypes.byref(ppw)), "eps_sketch_limits")
    return chunk.value, ppw.value


def sketch_own(first_id: int, n: int, device):
    """-> (hll uint8 [n, 256], mh uint32 [n, 128]): the own sketches of the ids first_id .. first_id + n - 1 (eps_sketch_own)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.EpsError("edge-proposal-sets_amd ops run on the MI355X only: sketch_own got a CPU device (there is no CPU fallback)")
    first_id, n = int(first_id), int(n)
    if n < 0 or first_id < 0 or first_id + n > 1 << 31:
        raise _lib.EpsError(f"sketch_own: ids must lie in [0, 2^31), got [{first_id}, {first_id + n})")
    hll = torch.empty((n, SKETCH_REGS), dtype=_U8, device=dev)
    mh = torch.empty((n, SKETCH_WORDS), dtype=_U32, device=dev)
    if n:
        _call("eps_sketch_own", hll.device, first_id, n, hll, mh, timed=("sketch_own_kernel", n))
    return hll, mh


def _sketch_tables(who: str, hll, mh, lead: Tuple[int, ...]) -> None:
    _chk(_U8, hll=hll); _chk(_U32, mh=mh)
    if tuple(hll.shape) != (*lead, SKETCH_REGS) or tuple(mh.shape) != (*lead, SKETCH_WORDS):
        raise _lib.EpsError(f"{who}: hll must be {[*lead, SKETCH_REGS]} and mh {[*lead, SKETCH_WORDS]}, got {list(hll.shape)} and {list(mh.shape)}")


def sketch_propagate(rowptr, col, n: int, hll_in, mh_in, keep_own: bool, check: bool = True, out=None):
    """-> (hll uint8 [n, 256], mh uint32 [n, 128]): out[v] = the union of in[w] over the stored entries w of row v of the square
    graph (byte-wise max of the registers, word-wise min of the words), with ``keep_own`` also of in[v] (eps_sketch_propagate).
    ``check``: every entry of col lies in [0, n) (one read); ``check=False``: an entry outside is skipped by the kernel.
    ``out``: (hll, mh) tensors of the result's shapes to write into (slices of a [K, n, .] table); they must not be the inputs."""
    n = int(n)
    dev = _need_gpu(rowptr, col, hll_in, mh_in, *(out or ()))
    _csr(rowptr, col)
    _sketch_tables("sketch_propagate", hll_in, mh_in, (n,))
    if rowptr.numel() != n + 1:
        raise _lib.EpsError(f"sketch_propagate: rowptr must hold {n + 1} entries, got {rowptr.numel()}")
    nnz = col.numel()
    if check and nnz:
        lo, hi, end = torch.stack([col.min().to(_I64), col.max().to(_I64), rowptr[-1]]).tolist()
        if lo < 0 or hi >= n or end != nnz:
            raise _lib.EpsError(f"sketch_propagate: col must hold rowptr[-1] = {end} entries in [0, {n}), got {nnz} in [{lo}, {hi}]")
    if out is not None:
        hll, mh = out
        _sketch_tables("sketch_propagate (out)", hll, mh, (n,))
    else:
        hll = torch.empty((n, SKETCH_REGS), dtype=_U8, device=dev)
        mh = torch.empty((n, SKETCH_WORDS), dtype=_U32, device=dev)
    if n == 0:
        return hll, mh
    ws_bytes = int(_lib.load().eps_sketch_propagate_workspace_bytes(nnz))
    ws = torch.empty(ws_bytes + 256, dtype=_U8, device=dev) if nnz else None
    ws_ptr = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256) if nnz else None
    _call("eps_sketch_propagate", dev, rowptr, col, n, nnz, hll_in, mh_in, hll, mh, 1 if keep_own else 0, ws_ptr, ws_bytes,
          timed=("sketch_propagate", nnz))
    return hll, mh


def sketch_pair_stats(hll, mh, n: int, u, v, check: bool = True):
    """-> (S int64, Z int32, match int32), each [B, K, K]: for hll uint8 [K, n, 256] and mh uint32 [K, n, 128] (hop k at index
    k - 1) and M = the byte-wise max of hll[i][u_b] and hll[j][v_b]: S = the sum of 2^(33 - M_r), Z = the registers with M_r == 0,
    match = the equal words of mh[i][u_b] and mh[j][v_b] (eps_sketch_pair_stats: one packed int64 per slot, unpacked here).
    ``check``: the ids are verified on the host first; ``check=False`` gives a pair with an id outside [0, n) -1 in every slot of
    all three."""
    n = int(n)
    dev = _need_gpu(hll, mh, u, v)
    _chk(_I32, u=u, v=v)
    if hll.dim() != 3 or hll.shape[0] not in (1, 2):
        raise _lib.EpsError(f"sketch_pair_stats: hll must be [K, n, {SKETCH_REGS}] with K 1 or 2, got {list(hll.shape)}")
    k = int(hll.shape[0])
    _sketch_tables("sketch_pair_stats", hll, mh, (k, n))
    if u.dim() != 1 or u.shape != v.shape:
        raise _lib.EpsError(f"sketch_pair_stats: u and v are two vectors of one length, got {tuple(u.shape)} and {tuple(v.shape)}")
    b = u.numel()
    if check and b:
        lo, hi = torch.stack([torch.minimum(u.min(), v.min()), torch.maximum(u.max(), v.max())]).tolist()
        if lo < 0 or hi >= n:
            raise _lib.EpsError(f"sketch_pair_stats: node ids must lie in [0, {n}), got [{lo}, {hi}]")
    stat = torch.empty((b, k, k), dtype=_I64, device=dev)
    if b:
        _call("eps_sketch_pair_stats", dev, hll, mh, k, n, u, v, b, stat, timed=("sketch_pair_stats_kernel", b))
    bad = stat < 0
    s = torch.where(bad, stat, stat & ((1 << 42) - 1))
    z = torch.where(bad, stat, (stat >> 42) & 511).to(_I32)
    match = torch.where(bad, stat, (stat >> 51) & 255).to(_I32)
    return s, z, match


PPR_ONE = 1 << 48                 # csrc/ppr_push.hip: the mass of a source, in units of 2^-48
PPR_WS_BUDGET = 16 << 30          # global tables: fewer workgroups rather than more than this much workspace (one region per
                                  # workgroup of the launch, also for the workgroups whose sources all stay in LDS: at eps = 1e-4 a
                                  # region is 15 MB and two workgroups per CU take 7.5 GB; at 1e-5 on the ppa-like graph 59 MB each)
PPR_MAX_TABLE_NODES = 1 << 30
_PPR_CUS = {}                     # device -> its number of CUs (the launch takes two workgroups per CU)


def ppr_push_limits(table_nodes: int = 0) -> Tuple[int, int, int, int]:
    """(keys the LDS table of eps_ppr_push takes, row length above which the whole workgroup walks a row, workgroups per CU,
    workspace bytes per workgroup of a global table of ``table_nodes`` keys -- 0 for 0) (host-only query)."""
    cap, big, per_cu, ws = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.check(_lib.load().eps_ppr_push_limits(int(table_nodes), ctypes.byref(cap), ctypes.byref(big), ctypes.byref(per_cu),
                                               ctypes.byref(ws)), "eps_ppr_push_limits")
    return cap.value, big.value, per_cu.value, ws.value


def ppr_touched_bound(n_nodes: int, alpha16: int, thr: int) -> int:
    """min(n_nodes, a bound on the nodes one source touches): every push of u keeps at least thr * d(u) * a16 / 65536 - 1 units
    in p, the kept units sum to at most 2^48, so once thr * a16 >= 2 * 65536 the pushed entries sum to at most
    2 * 2^48 * 65536 / (thr * a16), and a source touches at most one node more.  Below that the bound is n_nodes."""
    n_nodes, alpha16, thr = int(n_nodes), int(alpha16), int(thr)
    if thr * alpha16 < 2 * 65536:
        return n_nodes
    return min(n_nodes, 2 * PPR_ONE * 65536 // (thr * alpha16) + 2)


def ppr_push(rowptr, col, n_nodes: int, sources, qptr, qnode, alpha16: int, thr: int, max_rounds: int, table: str = 'auto',
             check: bool = True, stats: Optional[dict] = None):
    """-> (mass int64[Q], rounds int32[S], pushes int64[S], steps int64[S], capped int32[S]): the fixed-point personalized
    PageRank push of include/eps_abi.h (csrc/ppr_push.hip) from every node of ``sources`` (int32[S]) on the pattern of the square
    CSR, read at the query nodes ``qnode[qptr[i] : qptr[i + 1]]`` (int32) of source i.  alpha = alpha16 / 65536, thr =
    ceil(eps * 2^48).  ``table='global'`` skips the LDS attempt (same bits).  ``check``: the ids, the pointers' ends and order
    are verified on the host first (one read); without it a source or an entry outside the graph is reported after the launch.
    A global table that filled up raises: nothing is lost silently.  ``stats``: a dict that receives ``global_sources``, the
    number of sources whose table left LDS."""
    if table not in ('auto', 'global'):
        raise _lib.EpsError(f"ppr_push: table must be 'auto' or 'global', got {table!r}")
    dev = _need_gpu(rowptr, col, sources, qptr, qnode)
    _csr(rowptr, col); _chk(_I32, sources=sources, qnode=qnode); _chk(_I64, qptr=qptr)
    n_nodes, alpha16, thr, max_rounds = int(n_nodes), int(alpha16), int(thr), int(max_rounds)
    if rowptr.numel() != n_nodes + 1:
        raise _lib.EpsError(f"ppr_push: rowptr must hold {n_nodes + 1} entries, got {rowptr.numel()}")
    ns, nq = sources.numel(), qnode.numel()
    if sources.dim() != 1 or qptr.numel() != ns + 1:
        raise _lib.EpsError(f"ppr_push: qptr must hold {ns + 1} entries (one more than the sources), got {qptr.numel()}")
    if check and ns:
        z = torch.zeros((), dtype=_I64, device=dev)
        facts = torch.stack([sources.min().to(_I64), sources.max().to(_I64), qptr[0], qptr[-1], (qptr[1:] - qptr[:-1]).min(),
                             qnode.min().to(_I64) if nq else z, qnode.max().to(_I64) if nq else z,
                             col.min().to(_I64) if col.numel() else z, col.max().to(_I64) if col.numel() else z,
                             rowptr[0], rowptr[-1], (rowptr[1:] - rowptr[:-1]).min() if n_nodes else z]).tolist()
        if facts[0] < 0 or facts[1] >= n_nodes:
            raise _lib.EpsError(f"ppr_push: sources must lie in [0, {n_nodes}), got [{facts[0]}, {facts[1]}]")
        if facts[2] != 0 or facts[3] != nq or facts[4] < 0:
            raise _lib.EpsError(f"ppr_push: qptr must ascend from 0 to {nq} (the query nodes), got {facts[2]} .. {facts[3]}")
        if facts[5] < 0 or facts[6] >= n_nodes:
            raise _lib.EpsError(f"ppr_push: query nodes must lie in [0, {n_nodes}), got [{facts[5]}, {facts[6]}]")
        if facts[7] < 0 or facts[8] >= n_nodes or facts[9] != 0 or facts[10] != col.numel() or facts[11] < 0:
            raise _lib.EpsError(f"ppr_push: not a square CSR of {n_nodes} nodes (entries in [{facts[7]}, {facts[8]}], rowptr "
                                f"{facts[9]} .. {facts[10]} for {col.numel()} entries)")
    mass = torch.empty(nq, dtype=_I64, device=dev)
    rounds = torch.empty(ns, dtype=_I32, device=dev)
    pushes, steps = torch.empty(ns, dtype=_I64, device=dev), torch.empty(ns, dtype=_I64, device=dev)
    capped, used = torch.empty(ns, dtype=_I32, device=dev), torch.empty(ns, dtype=_I32, device=dev)
    status = torch.zeros(1, dtype=_I32, device=dev)
    lds_nodes, _, per_cu, _ = ppr_push_limits(0)
    ws, ws_bytes, table_nodes = None, 0, 0
    if table == 'global' or n_nodes > lds_nodes:
        table_nodes = max(1, min(ppr_touched_bound(n_nodes, alpha16, thr), PPR_MAX_TABLE_NODES))
        per_group = ppr_push_limits(table_nodes)[3]
        if dev not in _PPR_CUS:
            with torch.cuda.device(dev):
                _PPR_CUS[dev] = device_info()[0]
        groups = max(1, min(per_cu * _PPR_CUS[dev], max(ns, 1), PPR_WS_BUDGET // per_group))
        ws_bytes = groups * per_group
        ws = _scratch("ppr_push", dev, ws_bytes // 8, ws_bytes // 8)
    _call("eps_ppr_push", dev, rowptr, col, n_nodes, sources, ns, qptr, qnode, alpha16, thr, max_rounds, 1 if table == 'global' else 0,
          table_nodes, ws, ws_bytes, mass, rounds, pushes, steps, capped, used, status, timed=("ppr_push_kernel", ns))
    if ns:
        st, n_global = torch.stack([status[0].to(_I64), (used == 1).sum()]).tolist()
        if st:
            raise _lib.EpsError(f"ppr_push: status {st}"
                                + (f": a table of {table_nodes} keys filled up" if st & 1 else "")
                                + (": a source left LDS without a workspace" if st & 2 else "")
                                + (": a source outside the graph" if st & 4 else "")
                                + (": an entry of col outside the graph" if st & 8 else ""))
        if stats is not None:
            stats["global_sources"] = stats.get("global_sources", 0) + int(n_global)
    return mass, rounds, pushes, steps, capped


def kth_largest_dist(x: torch.Tensor, k: int, world: int = 1) -> torch.Tensor:
    """The k-th largest value of the UNION of every rank's float32 device vector ``x`` (lengths may differ, 0 allowed) as a
    1-element device tensor, identical on all ranks; -inf when the union holds fewer than k values.  Radix select in four
    rounds; per round one all-reduce of the 256-bin histogram (1 KiB) -- no host round trip.  ``world`` == 1: no collective."""
    from . import dist as epd
    dev = _need_gpu(x)
    _chk(_F32, x=x)
    state = torch.empty(int(_lib.load().eps_kth_largest_workspace_bytes()) // 4, dtype=_I32, device=dev)
    out = torch.empty(1, dtype=_F32, device=dev)
    _call("eps_kth_begin", dev, state, int(k))
    for shift in (24, 16, 8, 0):
        _call("eps_kth_hist_f32", dev, x, x.numel(), state, shift)
        if world > 1 or epd.FORCE_COLLECTIVES:
            epd.all_reduce_sum_(state[4:260])
        _call("eps_kth_pick", dev, state, shift, out)
    return out


def select_compact(keys: Optional[torch.Tensor], vals: torch.Tensor, k: int, count_ptr: Optional[int] = None, mode: int = 0,
                   params=(0.0, 0.0, 0.0), compact: bool = True, room: Optional[int] = None):
    """Radix select + threshold + compaction of a list on ONE device in one launch (eps_select_compact; the sharded job-wide
    select is ``kth_largest_dist``).  -> (out_keys, out_vals, n_out, kth, thr): the entries with key >= 0 and score >= thr
    compacted to the front of fresh arrays (None, None, None without ``compact``), their number, the k-th largest score and
    the threshold derived from it -- all DEVICE tensors, no host read.  ``count_ptr``: device address of a uint64 that bounds the
    list (``Survivors.count_ptr``).  ``mode`` / ``params``: 0 thr = kth; 1 the largest float below kth; 2 max(kth - a, kth * b) -
    |kth| * c with params (a, b, c).  ``room``: entries the output arrays hold (default: the list's length) -- n_out may come
    back LARGER: the entries beyond ``room`` were counted, not stored (a list sized for the worst case need not be mirrored by
    outputs of that size; the caller repeats the call with more room in the rare case)."""
    dev = _need_gpu(keys, vals)
    _chk(_I64, keys=keys); _chk(_F32, vals=vals)
    n = vals.numel()
    words = (int(_lib.load().eps_select_compact_workspace_bytes()) + 7) // 8
    # (one state per call, from the caching allocator: stream-ordered -- the block is handed out again only behind this launch on
    #  this stream, whatever other streams or however many calls are pending; r04's ring of 16 per device was neither)
    state = torch.empty(words, dtype=_I64, device=dev)
    kth = torch.empty(2, dtype=_F32, device=dev)
    out_k = out_v = n_out = None
    if compact:
        if keys is None:
            raise _lib.EpsError("select_compact: the compaction needs keys")
        room = n if room is None else max(1, min(int(room), n))
        out_k = torch.empty(room, dtype=_I64, device=dev)
        out_v = torch.empty(room, dtype=_F32, device=dev)
        n_out = torch.empty(1, dtype=_I64, device=dev)
    _call("eps_select_compact", dev, keys, vals, n, count_ptr, int(k), int(mode), float(params[0]), float(params[1]),
          float(params[2]), kth.data_ptr(), kth.data_ptr() + 4, out_k, out_v, 0 if room is None else int(room), n_out, state,
          timed=("select_compact", n))
    return out_k, out_v, n_out, kth[0:1], kth[1:2]


def _compact(name: str, keys: torch.Tensor, vals: torch.Tensor, *cuts):
    """Body of compact_at_least / compact_between: the entries the library's ``name`` keeps under ``cuts``, in fresh arrays."""
    dev = _need_gpu(keys, vals, *cuts)
    _chk(_I64, keys=keys); _chk(_F32, vals=vals)
    n = keys.numel()
    out_k = torch.empty(n, dtype=_I64, device=dev)
    out_v = torch.empty(n, dtype=_F32, device=dev)
    n_out = torch.empty(1, dtype=_I64, device=dev)
    _call(name, dev, keys, vals, n, *cuts, out_k, out_v, n_out)
    return out_k, out_v, n_out


def compact_at_least(keys: torch.Tensor, vals: torch.Tensor, cut: Optional[torch.Tensor]):
    """(keys, vals, n) -- the survivors (key >= 0) with score >= ``cut`` (1-element float32 DEVICE tensor; None: all of them)
    compacted to the front of fresh arrays, ``n`` a 1-element int64 device tensor (no host read)."""
    _chk(_F32, cut=cut)
    return _compact("eps_compact_at_least", keys, vals, cut)


def compact_between(keys: torch.Tensor, vals: torch.Tensor, lo: Optional[torch.Tensor], hi: Optional[torch.Tensor]):
    """(keys, vals, n) -- the entries (key >= 0) with lo <= score < hi (1-element float32 DEVICE tensors; None: open end)
    compacted to the front of fresh arrays, ``n`` a 1-element int64 device tensor (no host read)."""
    _chk(_F32, lo=lo, hi=hi)
    return _compact("eps_compact_between", keys, vals, lo, hi)


def sort_pairs_by_u(keys: torch.Tensor, id_bits: int = 32, v_block_shift: int = 0) -> torch.Tensor:
    """Survivor keys v << 32 | u (u < v, any order) -> u << 32 | v sorted by (u, v), what ``rescore_runs`` wants: two stable
    radix sorts over the id bits (eps_sort_pairs_by_u)."""
    dev = _need_gpu(keys)
    _chk(_I64, keys=keys)
    n = keys.numel()
    out = torch.empty(n, dtype=_I64, device=dev)
    if n:
        _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_sort_pairs_by_u_workspace_bytes(n))
        _call("eps_sort_pairs_by_u", dev, keys, n, int(id_bits), int(v_block_shift), out, wsp, wsb, timed=("sort_pairs_by_u", n))
    return out


def _topk_rows(sel_keys, sel_vals, m: int, k: int, id_bits: int, perm, as_pairs: bool = False):
    """Body of select_rows / select_rows_pairs / select_topk: the first min(k, 2 m) directed rows of the first ``m`` selected
    pairs, as keys [take] or, ``as_pairs``, as the (u; v) tensor [2, take] -- and their scores."""
    dev = _need_gpu(sel_keys, sel_vals, perm)
    _chk(_I64, sel_keys=sel_keys, perm=perm); _chk(_F32, sel_vals=sel_vals)
    k = int(k)
    take = min(k, 2 * m)
    rows = torch.empty((2, take) if as_pairs else take, dtype=_I64, device=dev)
    out_v = torch.empty(take, dtype=_F32, device=dev)
    if take:
        _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_select_topk_rows_workspace_bytes(m))
        head = (sel_keys, sel_vals, m, k, int(id_bits))
        if as_pairs:
            _call("eps_select_topk_rows_pairs", dev, *head, perm, rows, take, out_v, wsp, wsb, timed=("select_rows", m))
        elif perm is None:
            _call("eps_select_topk_rows", dev, *head, rows, out_v, wsp, wsb)
        else:
            _call("eps_select_topk_rows_relabelled", dev, *head, perm, rows, out_v, wsp, wsb)
    return rows, out_v


def select_rows(sel_keys: torch.Tensor, sel_vals: torch.Tensor, k: int, id_bits: int = 32,
                perm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The first min(k, 2 m) DIRECTED rows, in the declared order, of m selected unordered pairs (every pair at or above the
    job-wide cut): mirror + stable radix sorts (eps_select_topk_rows).  No host read: m is the arrays' length.
    ``perm`` (int64 [n_nodes]): the pairs are in the labels of a relabelled graph whose id i is the caller's perm[i]; the rows
    come out -- and are ordered -- in the caller's labels."""
    return _topk_rows(sel_keys, sel_vals, sel_keys.numel(), k, id_bits, perm)


def select_rows_pairs(sel_keys: torch.Tensor, sel_vals: torch.Tensor, k: int, id_bits: int = 32,
                      perm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``select_rows`` with the rows written as the proposal tensor itself: (pairs int64 [2, min(k, 2 m)] as (u; v), scores)
    (eps_select_topk_rows_pairs) -- no tensor ops over the K rows afterwards."""
    return _topk_rows(sel_keys, sel_vals, sel_keys.numel(), k, id_bits, perm, as_pairs=True)


def rows_by_score_limits() -> Tuple[int, int]:
    """(longest run of equal scores ``rows_by_score`` orders itself, sorted pairs per workgroup of its expansion)."""
    lib = _lib.load()
    return int(lib.eps_rows_by_score_max_run()), int(lib.eps_rows_by_score_window())


def rows_by_score(keys_by_u: torch.Tensor, vals: torch.Tensor, bar: torch.Tensor, k2: int, k: int, id_bits: int = 32,
                  perm: Optional[torch.Tensor] = None):
    """The end of a one-rank step from ONE score sort of the re-scored pairs (eps_rows_by_score): ``keys_by_u`` / ``vals`` as
    ``rescore_runs`` leaves them (u << 32 | v, any order), ``bar`` a 1-element float32 device tensor.  -> (pairs int64 [2, cap] as
    (u; v), scores float32 [cap], sorted_keys, sorted_vals, n_sel, cut, flag) with cap = min(k, 2 len), all device tensors, no host
    read: cut / n_sel are what ``score_hist`` + ``score_pick_compact`` give with above = base = bar and k = k2; the first n_sel
    sorted pairs (v << 32 | u, score descending) are that selection; the first min(k, 2 n_sel) columns of ``pairs`` / ``scores`` are
    its rows in the declared order -- unless ``flag`` (int64[1]) is 1: a run of equal scores was longer than
    ``rows_by_score_limits()[0]`` and the rows are void (``select_rows_pairs`` on the selection orders them)."""
    dev = _need_gpu(keys_by_u, vals, bar, perm)
    _chk(_I64, keys_by_u=keys_by_u, perm=perm); _chk(_F32, vals=vals, bar=bar)
    n, k = keys_by_u.numel(), int(k)
    _chk_len("rows_by_score", "vals", vals, n, "one score per pair")
    cap = min(k, 2 * n)
    pairs = torch.empty((2, cap), dtype=_I64, device=dev)
    scores = torch.empty(cap, dtype=_F32, device=dev)
    sorted_k = torch.empty(n, dtype=_I64, device=dev)
    sorted_v = torch.empty(n, dtype=_F32, device=dev)
    cut = torch.empty(1, dtype=_F32, device=dev)
    words = torch.empty(2, dtype=_I64, device=dev)               # n_sel, flag
    _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_rows_by_score_workspace_bytes(n))
    _call("eps_rows_by_score", dev, keys_by_u, vals, n, bar, int(k2), k, int(id_bits), perm, sorted_k, sorted_v, cut, words.data_ptr(),
          words.data_ptr() + 8, pairs, cap, scores, wsp, wsb, timed=("select_rows", n))
    return pairs, scores, sorted_k, sorted_v, words[0:1], cut, words[1:2]


def select_topk(keys: torch.Tensor, vals: torch.Tensor, k: int, id_bits: int = 32) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best DIRECTED rows (score descending, key ascending) of a list of unordered survivors of ``filter_scan``
    (key = v << 32 | u, u < v; no -1 slots): (keys int64, scores float32), sorted.  eps_select_topk_cut (radix select of the
    cut + compaction) -> one host read of the count -> eps_select_topk_rows (mirror + stable radix sorts).  ``id_bits``:
    every node id is below 2**id_bits (fewer sort passes)."""
    dev = _need_gpu(keys, vals)
    _chk(_I64, keys=keys); _chk(_F32, vals=vals)
    n, k = keys.numel(), int(k)
    if vals.numel() != n:
        raise _lib.EpsError("select_topk: keys and vals differ in length")
    sel_k = torch.empty(n, dtype=_I64, device=dev)
    sel_v = torch.empty(n, dtype=_F32, device=dev)
    n_sel = torch.zeros(1, dtype=_I64, device=dev)
    _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_select_topk_cut_workspace_bytes())
    _call("eps_select_topk_cut", dev, keys, vals, n, k, sel_k, sel_v, n_sel, wsp, wsb)
    return _topk_rows(sel_k, sel_v, int(n_sel.item()), k, id_bits, None)


# ---- the tail of the filter step with device-side sizes (csrc/tail_sort.hip, r06) ------------------------------------------------
def tail_state(dev) -> torch.Tensor:
    """The state block of the tail kernels for (device, current stream): zeroed ONCE here -- the kernels that consume it leave it
    zeroed, so a step issues no memset for it."""
    return _scratch(("tail", torch.cuda.current_stream(dev).cuda_stream), dev, 1,
                    lambda: (int(_lib.load().eps_tail_state_bytes()) + 7) // 8 + 32, zero=True)


def _tail_addr(dev):
    st = tail_state(dev)
    return ctypes.c_void_p(st.data_ptr() + (-st.data_ptr()) % 256)


def tail_state_reset(dev) -> None:
    """Zero the state again (after a failed call that may have left a histogram or a hand-over counter half way)."""
    tail_state(dev).zero_()


# (a device count argument -- ``n_dev`` / ``m_dev`` below -- is None, a raw device address (Survivors.count_ptr) or a 1-element
#  int64 tensor)
def score_hist(keys: Optional[torch.Tensor], vals: torch.Tensor, n_dev, base: torch.Tensor, above: Optional[torch.Tensor] = None) -> None:
    """Add the histogram of the list's live scores (buckets of their distance to ``base``, a 1-element float32 device tensor) to
    the tail state (eps_score_hist).  ``n_dev``: device count that bounds the list (None: its length)."""
    dev = _need_gpu(keys, vals, base, above)
    _chk(_I64, keys=keys, n_dev=n_dev); _chk(_F32, vals=vals, base=base, above=above)
    _call("eps_score_hist", dev, keys, vals, vals.numel(), n_dev, base, above, _tail_addr(dev),
          timed=("select_compact", vals.numel()))


def score_pick_compact(keys: Optional[torch.Tensor], vals: torch.Tensor, n_dev, base: torch.Tensor, k: int, above: Optional[torch.Tensor] = None,
                       mode: int = 0, params=(0.0, 0.0, 0.0), swap_halves: bool = False, room: Optional[int] = None,
                       want_vals: bool = True):
    """The selection behind ``score_hist`` (eps_score_pick_compact): -> (out_keys, out_vals, n_out, kth, thr), all device tensors.
    ``kth`` is the lower edge of the bucket that holds the k-th best live value (<= the exact k-th, by at most 2^-8 of its distance
    to ``base``), ``thr`` derived from it as in ``select_compact``; the live entries with value >= thr are compacted into arrays
    of ``room`` entries (more are counted in n_out, not stored); ``swap_halves`` exchanges the key halves on the way."""
    dev = _need_gpu(keys, vals, base, above)
    _chk(_I64, keys=keys, n_dev=n_dev); _chk(_F32, vals=vals, base=base, above=above)
    n = vals.numel()
    kth = torch.empty(2, dtype=_F32, device=dev)
    out_k = out_v = n_out = None
    if keys is not None:
        room = max(1, n if room is None else min(int(room), max(n, 1)))
        out_k = torch.empty(room, dtype=_I64, device=dev)
        out_v = torch.empty(room, dtype=_F32, device=dev) if want_vals else None
        n_out = torch.empty(1, dtype=_I64, device=dev)
    _call("eps_score_pick_compact", dev, keys, vals, n, n_dev, base, above, int(k), int(mode), float(params[0]), float(params[1]),
          float(params[2]), int(bool(swap_halves)), kth.data_ptr(), kth.data_ptr() + 4, out_k, out_v,
          0 if out_k is None else int(room), n_out, _tail_addr(dev), timed=("select_compact", n))
    return out_k, out_v, n_out, kth[0:1], kth[1:2]


def score_bins() -> int:
    return int(_lib.load().eps_score_bins())


def score_hist_into(keys: Optional[torch.Tensor], vals: torch.Tensor, n_dev, base: torch.Tensor, hist: torch.Tensor,
                    above: Optional[torch.Tensor] = None) -> None:
    """``score_hist`` into an int32 array of the caller's (``score_bins()`` words, zeroed by the caller): the histogram a rank of a
    sharded step sends to the others (eps_score_hist_into)."""
    dev = _need_gpu(keys, vals, base, above, hist)
    _chk(_I64, keys=keys, n_dev=n_dev); _chk(_F32, vals=vals, base=base, above=above); _chk(_I32, hist=hist)
    if hist.numel() < score_bins() or not hist.is_contiguous():
        raise _lib.EpsError("score_hist_into: hist must hold score_bins() contiguous words")
    _call("eps_score_hist_into", dev, keys, vals, vals.numel(), n_dev, base, above, hist)


def score_deal_plan(hists: torch.Tensor, k: int, base: torch.Tensor):
    """(cut float32[1], splitters float32[world - 1], counts int64[world, world], nsel int64[world]) from the ranks' gathered score
    histograms ``hists`` (int32 [world, >= score_bins()], row-contiguous): eps_score_deal_plan -- device tensors, no host read."""
    dev = _need_gpu(hists, base, row_strided=(hists,))
    _chk(_I32, hists=hists); _chk(_F32, base=base)
    if hists.dim() != 2 or hists.stride(1) != 1 or hists.shape[1] < score_bins():
        raise _lib.EpsError("score_deal_plan: hists must be [world, >= score_bins()] with unit column stride")
    world = hists.shape[0]
    cut = torch.empty(1, dtype=_F32, device=dev)
    sp = torch.empty(max(world - 1, 1), dtype=_F32, device=dev)
    counts = torch.empty((world, world), dtype=_I64, device=dev)
    nsel = torch.empty(world, dtype=_I64, device=dev)
    _call("eps_score_deal_plan", dev, hists, hists.stride(0), world, int(k), base, cut, sp, counts, nsel)
    return cut, sp[:world - 1], counts, nsel


def radix_sort_by_u(keys: torch.Tensor, n_dev, id_bits: int = 32, v_block_shift: int = 0) -> torch.Tensor:
    """``sort_pairs_by_u`` in one cooperative launch with the list's length read on the device (eps_radix_sort_by_u): the first
    min(*n_dev, len(keys)) keys v << 32 | u -> u << 32 | v in the order eps_rescore_runs wants; the rest of the output is undefined."""
    dev = _need_gpu(keys)
    _chk(_I64, keys=keys, n_dev=n_dev)
    n = keys.numel()
    out = torch.empty(n, dtype=_I64, device=dev)
    if n:
        _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_radix_sort_workspace_bytes(n))
        _call("eps_radix_sort_by_u", dev, keys, n, n_dev, int(id_bits), int(v_block_shift), out, wsp, wsb, _tail_addr(dev),
              timed=("sort_pairs_by_u", n))
    return out


def radix_sort_rows(sel_keys: torch.Tensor, sel_vals: torch.Tensor, m_dev, k: int, id_bits: int = 32, perm: Optional[torch.Tensor] = None):
    """``select_rows`` in one cooperative launch with the number of selected pairs read on the device (eps_radix_sort_rows):
    -> (pairs int64 [2, cap] as (u; v), scores float32 [cap], n_rows 1-element int64 device tensor) with cap = min(k, 2 len);
    the first n_rows = min(k, 2 m) columns are the rows of the declared order, the rest undefined."""
    dev = _need_gpu(sel_keys, sel_vals, perm)
    _chk(_I64, sel_keys=sel_keys, perm=perm, m_dev=m_dev); _chk(_F32, sel_vals=sel_vals)
    m_max, k = sel_keys.numel(), int(k)
    cap = min(k, 2 * m_max)
    pairs = torch.empty((2, cap), dtype=_I64, device=dev)
    scores = torch.empty(cap, dtype=_F32, device=dev)
    n_rows = torch.zeros(1, dtype=_I64, device=dev) if cap == 0 else torch.empty(1, dtype=_I64, device=dev)
    if cap:
        _, wsp, wsb = _aligned_ws(dev, _lib.load().eps_radix_sort_workspace_bytes(2 * m_max))
        _call("eps_radix_sort_rows", dev, sel_keys, sel_vals, m_max, m_dev, k, int(id_bits), perm, pairs, cap, scores, n_rows, wsp, wsb,
              _tail_addr(dev), timed=("select_rows", m_max))
    return pairs, scores, n_rows


def rescore_runs_dev(rowptr, col, fixw: torch.Tensor, n_nodes: int, keys_by_u: torch.Tensor, n_dev: torch.Tensor) -> torch.Tensor:
    """``rescore_runs`` over the first min(*n_dev, len) keys (eps_rescore_runs_dev); the other outputs are undefined."""
    dev = _need_gpu(rowptr, col, fixw, keys_by_u, n_dev)
    _csr(rowptr, col); _chk(_I64, keys_by_u=keys_by_u, fixw=fixw, n_dev=n_dev)
    _chk_rescore_nnz("rescore_runs_dev", col)
    out = torch.empty(keys_by_u.numel(), dtype=_F32, device=dev)
    if keys_by_u.numel():
        _call("eps_rescore_runs_dev", dev, rowptr, col, fixw, int(n_nodes), keys_by_u, keys_by_u.numel(), n_dev, out,
              timed=("rescore_runs", keys_by_u.numel()))
    return out


def pack_keys(score: torch.Tensor, ids: Optional[torch.Tensor] = None, id_base: int = 0) -> torch.Tensor:
    dev = _need_gpu(score, ids)
    _chk(_F32, score=score); _chk(_I64, ids=ids)
    # the key holds the id in its low 32 bits: an id the kernel would truncate aliases another candidate's key
    if ids is not None and ids.numel():
        lo, hi = torch.aminmax(ids)
        if int(lo) < 0 or int(hi) >= 1 << 32:
            raise _lib.EpsError(f"pack_keys: ids must lie in [0, 2**32), got [{int(lo)}, {int(hi)}] "
                                "(use shard-relative ids and merge_ranked_lists for longer candidate lists)")
    elif ids is None and (id_base < 0 or id_base + score.numel() > 1 << 32):
        raise _lib.EpsError("pack_keys: id_base + n exceeds the 32-bit id field of the key")
    keys = torch.empty(score.numel(), dtype=_I64, device=dev)  # bit pattern of the uint64 key
    _call("eps_pack_keys", dev, score, ids, id_base, score.numel(), keys)
    return keys


def unpack_keys(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    dev = _need_gpu(keys)
    _chk(_I64, keys=keys)
    n = keys.numel()
    score = torch.empty(n, dtype=_F32, device=dev)
    ids = torch.empty(n, dtype=_I64, device=dev)
    _call("eps_unpack_keys", dev, keys, n, score, ids)
    return score, ids
