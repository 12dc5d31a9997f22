#!/usr/bin/env python3
"""Headline benchmark: candidate edges scored per second on a ppa-like graph (BASELINE.json configs[2]:
"ogbl-ppa Adamic-Adar scoring of full non-edge candidate set, 1xMI355X").

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

A plain run does what the headline figure needs and nothing else: it builds the graph and its per-graph tables, runs the W
warm-up steps and the K timed steps, writes --dump-outputs, and prints the result line (metric, value, unit, ms_per_step,
higher_is_better, dtype, the configuration).  --full adds everything else described below: the roofline, the step
breakdown, prep / cold / sustained / weak figures, the secondary legs and the CPU baseline (about a minute more on 1 GPU).
The warm-up and timed steps are the same in both modes, so `value` and `ms_per_step` compare across them.

--dump-outputs DIR writes the rows the last timed step returned (scan.scan_topk's pairs and scores) as DIR/pairs.npy and
DIR/scores.npy; the graph is seeded, so two builds run with the same arguments can be compared output for output.

Workload (synthetic, seeded; no dataset / network exists on either box)
  graph : S3 "ppa-like" -- N = 576,289 nodes, ~21.2 M undirected edges (nnz ~42.5 M, avg degree ~74), R-MAT skew,
          unit weights; replicated on every GPU (0.35 GB + 0.7 GB of per-graph tables).
  step  : the PRODUCTION filter pass over the FULL candidate set of that graph -- what
          `filter.py --dataset ppa --model adamic_ogb --keep_top 4000000` runs between loading the graph and writing
          the proposal file: every 2-hop non-edge (filter.py:96-109; 12.7 G directed candidates) is scored by
          Adamic-Adar (adamic_utils.py:13-25) and the 4,000,000 best rows under the declared order (filter.py:160-161)
          come out, on the device.  One step = scan.scan_topk: bar estimate from a column sample (one small launch of the
          scan kernel + a select), ONE eps_scan_screen launch over all columns (csrc/scan_pieces.hip: every candidate's
          sum is formed in an LDS table as a 15 / 31-bit SCREENING upper bound), exact 2^-40 fixed-point re-scoring of
          the survivors that can reach the top-K (eps_rescore_runs), verification, selection and ordering of the K rows.
  value : directed candidates scored per second, whole job (the kernel's own candidate count, both orientations of
          each pair; each unordered pair is computed once -- the score is symmetric).
  N > 1 : "strong" (default): the columns of ONE graph are dealt round-robin over the ranks in heaviest-first order; every
          rank scans, re-scores and selects its own share, ONE all-reduce (the bar) + one job-wide radix select (the cut) +
          one all-gather of the selected pairs are the collectives, and the final ordering is dealt over the ranks by score
          range -- the north-star target ("sharded candidate set").  "weak" (--scaling weak): every rank runs the full
          single-GPU workload on its own replica (per-GPU work fixed).
Reported next to it with --full: the roofline of the dominant kernel (scan_piece_kernel<256,false,true>; HIP events on its stream), what
the step spends outside it (`serial_ms`; for N > 1 `replicated_ms`: everything that does not shrink with N), a sustained run
of >= 5 s, secondary legs for the other hot-path kernels (pair intersection, SpMM, GEMM, decode) and one leg per BASELINE
config (bench_configs.py) with their SURVEY 8(d) rooflines, and the reference's CPU path (SciPy mirror of adamic_utils.AA)
timed on a bounded sample of the same candidates -- one thread like the reference, and split over all host cores.
A rank that fails still prints ONE JSON line (with "error") and exits non-zero.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEEP_TOP = 4_000_000       # README.md:11-17 / submit_job.py:207-213: the published ppa recipe keeps 4 M proposals
HBM_PEAK_GBPS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable by a float4 copy)
MFMA_F32_PEAK_TF = 157.3   # fp32-input MFMA, dense
CPU_SAMPLE = 4_000_000     # candidate pairs timed through the single-thread SciPy mirror (~10-20 s)
PAIR_LEG = 1 << 25
DUMP_MAX_BYTES = 64_000_000  # --dump-outputs: all files together; a larger output is written as a seeded sample of its rows
DUMP_SEED = 0


def _events(torch, n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def _timed_loop(torch, fn, reps, warmup=2, batch=1):
    """Mean HIP-event milliseconds of one ``fn`` launch on the current stream; ``batch`` > 1 brackets that many
    back-to-back launches per event pair (sub-millisecond kernels: as a layer runs them, no host gap in between)."""
    for _ in range(warmup):
        fn()
    evs = _events(torch, reps)
    s = torch.cuda.current_stream()
    for a, b in evs:
        a.record(s)
        for _ in range(batch):
            fn()
        b.record(s)
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in evs) / reps / batch


def dump_outputs(path, pairs, scores, n_nodes):
    """--dump-outputs: what a caller of scan.scan_topk receives from the last timed step -- pairs [2, K] (u; v) and scores [K] --
    as ``path``/pairs.npy and ``path``/scores.npy.  Node ids are written as float32 when every id of the graph is exact in it
    (N <= 2^24; decided by the graph, not by the data, so two builds write the same dtype), else float64; scores stay float32.
    When the whole exceeds DUMP_MAX_BYTES the same DUMP_SEED-seeded sample of rows (ascending) is taken from both arrays."""
    import numpy as np
    id_dtype = np.float32 if n_nodes <= (1 << 24) else np.float64
    p = pairs.cpu().numpy().astype(id_dtype)
    s = scores.cpu().numpy().astype(np.float32)
    rows = s.shape[0]
    row_bytes = 2 * p.itemsize + s.itemsize
    sampled = None
    budget = DUMP_MAX_BYTES - 2 * 4096                           # (the two .npy headers)
    if rows * row_bytes > budget:
        sampled = budget // row_bytes
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(rows, sampled, replace=False))
        p, s = p[:, idx], s[idx]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "pairs.npy"), np.ascontiguousarray(p))
    np.save(os.path.join(path, "scores.npy"), s)
    return {"dir": path, "rows": rows, "sampled_rows": sampled, "seed": DUMP_SEED if sampled else None,
            "arrays": {"pairs": [list(p.shape), str(p.dtype)], "scores": [list(s.shape), str(s.dtype)]}}


# ------------------------------------------------------------------------------------------------ secondary legs
def leg_pair_kernel(torch, g, w, ops, candidates):
    """Column-run intersection kernel (eval-style explicit pair lists in candidate order): 2^25 candidate pairs."""
    n = g.n_rows
    out, have, v = [], 0, 0
    while have < PAIR_LEG and v < n:
        blk = candidates.expand_block(g, v, min(v + 256, n), long_pairs=False)[0]
        out.append(blk)
        have += blk.shape[1]
        v += 256
    pairs = torch.cat(out, 1)[:, :PAIR_LEG]
    u, vv = pairs[0].contiguous(), pairs[1].contiguous()
    res = {}

    def step():
        res["r"] = ops.pair_scores(g.rowptr, g.col, g.val, w, n, u, vv, want_count=True, want_cn=False, grouped=True)
    ms = _timed_loop(torch, step, 10)
    count = res["r"][0]
    deg = g.degree()
    du, dv = int(deg[u.long()].sum()), int(deg[vv.long()].sum())
    cn = int(count.sum())
    e = u.numel()
    runs = int((vv[1:] != vv[:-1]).sum()) + 1
    dv_runs = int(deg[torch.unique_consecutive(vv).long()].sum())
    alg8d = 4 * (du + dv) + 4 * cn + 48 * e                     # both rows charged to every pair
    comp = 4 * du + 4 * dv_runs + 4 * cn + 16 * e + 32 * runs   # row u per pair, row v once per run, pair ids + outputs
    return {"kernel": "pair_scores_grouped_kernel<false,true,float,true>", "pairs": e, "kernel_ms": ms,
            "pairs_per_s": e / ms * 1e3, "bound": "hbm",
            "compulsory": {"bytes": comp, "GBps": comp / ms / 1e6, "frac": comp / ms / 1e6 / HBM_PEAK_GBPS,
                           "unit": "row u per pair (4 d_u) + row v once per run of equal v + 4 CN + ids/outputs"},
            "algorithmic_8d": {"bytes": alg8d, "GBps": alg8d / ms / 1e6,
                               "note": "SURVEY 8(d) unit 4(d_u+d_v)+4CN+48 charges row v to every pair; the kernel reads "
                                       "it once per run, so this figure may exceed the HBM peak and is NOT a roofline fraction"},
            "mean_du": du / e, "mean_dv": dv / e, "mean_cn": cn / e}


def leg_gnn(torch, g, ops):
    """configs[3] kernels on the ppa-like graph: GCN-normalised SpMM (F=256), the layer GEMM, the fused decode."""
    dev = g.device
    n, f = g.n_rows, 256
    gen = torch.Generator(device=dev).manual_seed(11)
    gn = g.gcn_normalized()
    x = torch.randn(n, f, generator=gen, device=dev)
    bias = torch.randn(f, generator=gen, device=dev)
    y = torch.empty_like(x)
    ms = _timed_loop(torch, lambda: ops.spmm_csr(gn.rowptr, gn.col, gn.val, x, bias=bias, relu=True, out=y), 10)
    nnz = gn.nnz()
    comp = nnz * 8 + (n + 1) * 8 + 2 * n * f * 4
    gather = nnz * f * 4 + nnz * 8 + n * f * 4
    spmm = {"kernel": "spmm_csr_kernel", "nnz": nnz, "F": f, "kernel_ms": ms, "bound": "hbm",
            "compulsory": {"bytes": comp, "GBps": comp / ms / 1e6, "frac": comp / ms / 1e6 / HBM_PEAK_GBPS},
            "gather_model": {"bytes": gather, "GBps": gather / ms / 1e6, "frac": gather / ms / 1e6 / HBM_PEAK_GBPS,
                             "note": "one 1-KiB row of X per stored entry: what a permuted graph costs without reuse"}}
    go, perm, _ = gn.degree_ordered()                                      # what LinkGNN.embeddings runs on: hubs first
    xo = x[perm].contiguous()
    ms_o = _timed_loop(torch, lambda: ops.spmm_csr(go.rowptr, go.col, go.val, xo, bias=bias, relu=True, out=y), 10)
    spmm["hubs_first_relabelling"] = {"kernel_ms": ms_o, "gather_model_GBps": gather / ms_o / 1e6,
                                      "note": "same kernel on the degree-ordered graph (graph.degree_ordered): the hubs' rows of "
                                              "X sit together and stay cache-resident; above the HBM peak on the gather model "
                                              "means gathers served by L2 / Infinity Cache"}
    k = 316                                                               # 58 features + 256-d embedding, padded to x4
    a = torch.randn(n, k, generator=gen, device=dev)
    wt = torch.randn(f, k, generator=gen, device=dev)
    ms_iso = _timed_loop(torch, lambda: ops.gemm(a, wt, bias=bias, relu=True, out=y), 20, warmup=5)
    ms = _timed_loop(torch, lambda: ops.gemm(a, wt, bias=bias, relu=True, out=y), 6, warmup=5, batch=10)
    fl = 2.0 * n * f * k
    gemm = {"kernel": "gemm_f32_kernel", "shape": [n, f, k], "kernel_ms": ms, "bound": "mfma", "TFLOPs": fl / ms / 1e9,
            "frac": fl / ms / 1e9 / MFMA_F32_PEAK_TF,
            "how": "10 launches back to back per event pair (the layer loop's cadence); isolated launches, each bracketed by its "
                   "own events: kernel_ms_isolated",
            "kernel_ms_isolated": ms_iso, "TFLOPs_isolated": fl / ms_iso / 1e9}
    ne = 1 << 22
    u = torch.randint(0, n, (ne,), generator=gen, device=dev, dtype=torch.int32)
    v = torch.randint(0, n, (ne,), generator=gen, device=dev, dtype=torch.int32)
    ws = [torch.randn(f, f, generator=gen, device=dev) * 0.06, torch.randn(f, f, generator=gen, device=dev) * 0.06,
          torch.randn(1, f, generator=gen, device=dev) * 0.06]
    bs = [torch.randn(f, generator=gen, device=dev) * 0.1, torch.randn(f, generator=gen, device=dev) * 0.1,
          torch.randn(1, generator=gen, device=dev)]
    ms = _timed_loop(torch, lambda: ops.mlp_decode(x, u, v, ws, bs), 10)
    fl = float(ne) * (f + 2 * f * f * 2 + 2 * f)
    dec = {"kernel": "mlp_decode_kernel", "edges": ne, "H": f, "L": 3, "kernel_ms": ms, "bound": "mfma",
           "edges_per_s": ne / ms * 1e3, "TFLOPs": fl / ms / 1e9, "frac": fl / ms / 1e9 / MFMA_F32_PEAK_TF}
    return {"spmm": spmm, "gemm": gemm, "decode": dec}


# ------------------------------------------------------------------------------------------------ CPU baseline
def _cpu_worker(args):
    """One process of the all-cores leg: its slice of the sample through the SciPy mirror of adamic_utils.AA."""
    path, lo, hi = args
    import numpy as np
    import scipy.sparse as ssp
    d = np.load(path)
    n = len(d["rowptr"]) - 1
    A = ssp.csr_matrix((np.ones(len(d["col"]), np.float32), d["col"], d["rowptr"]), shape=(n, n))
    pu, pv = d["pu"][lo:hi], d["pv"][lo:hi]
    with np.errstate(divide="ignore"):
        mult = 1 / np.log(A.sum(0))
        mult[np.isinf(mult)] = 0
        A_ = A.multiply(mult).tocsr()
    t0 = time.perf_counter()
    for s in range(0, len(pu), 2000):
        np.array(np.sum(A[pu[s:s + 2000]].multiply(A_[pv[s:s + 2000]]), 1)).flatten()
    return time.perf_counter() - t0, hi - lo


def cpu_baseline(torch, g, w, ops, candidates, keep_pairs, keep_scores):
    """Reference CPU path on the host cores: the SciPy mirror of adamic_utils.AA (bit-exact to the imported reference,
    tests/test_oracle_golden.py) on a bounded sample of the step's candidate set -- the candidates of every 512-th
    column, thinned to CPU_SAMPLE pairs -- single thread like the reference (SciPy sparse ops + a 0-worker DataLoader),
    then the same mirror split over all host cores (one process each).  The GPU scores of the sample are checked
    against it, and so are the scores of a slice of the step's own output rows."""
    import numpy as np
    from oracle import eps_oracle as orc
    A = g.to_scipy()
    n = g.n_rows
    cols = list(range(137, n, 512))
    blocks = [candidates.expand_block(g, c, c + 1, w, want_score=True, long_pairs=False) for c in cols]
    pairs = torch.cat([b[0] for b in blocks], 1)
    gpu_sc = torch.cat([b[2] for b in blocks])
    stride = max(1, pairs.shape[1] // CPU_SAMPLE)
    pairs, gpu_sc = pairs[:, ::stride][:, :CPU_SAMPLE], gpu_sc[::stride][:CPU_SAMPLE]
    pu, pv = pairs[0].cpu().numpy().astype(np.int64), pairs[1].cpu().numpy().astype(np.int64)
    with np.errstate(divide="ignore"):
        mult = 1 / np.log(A.sum(0))
        mult[np.isinf(mult)] = 0
        A_ = A.multiply(mult).tocsr()
        t0 = time.perf_counter()
        scores = []
        for s in range(0, len(pu), 2000):  # adamic_utils.py:18-24, batch_size 2000
            scores.append(np.array(np.sum(A[pu[s:s + 2000]].multiply(A_[pv[s:s + 2000]]), 1)).flatten())
        dt = time.perf_counter() - t0
        ref = np.concatenate(scores).astype(np.float32)
        # the step's own output: the first and last 20,000 of the K rows it selected
        sel = torch.cat([torch.arange(0, 20000), torch.arange(keep_scores.numel() - 20000, keep_scores.numel())])
        ku, kv = keep_pairs[0][sel].cpu().numpy(), keep_pairs[1][sel].cpu().numpy()
        kref = np.array(np.sum(A[ku].multiply(A_[kv]), 1)).flatten().astype(np.float32)

    def rel(a, b):
        den = np.maximum(np.abs(a), np.abs(b))
        den[den == 0] = 1
        return float((np.abs(a - b) / den).max())
    rel_sample = rel(ref, gpu_sc.cpu().numpy())
    rel_topk = rel(kref, keep_scores[sel].cpu().numpy())
    # the scalar C port on one core, a second CPU data point
    rp, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    wo = orc.node_weights(orc.col_sums(rp, col, None, n), orc.W_AA)
    t1 = time.perf_counter()
    orc.pair_scores(rp, col, None, wo, pu, pv)
    dt_c = time.perf_counter() - t1
    # all host cores: the SciPy mirror itself, the sample split over one process per core
    import multiprocessing as mp
    import tempfile
    n_proc = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    n_proc = max(1, min(n_proc, 64))
    tmp = os.path.join(tempfile.gettempdir(), f"eps_bench_cpu_{os.getpid()}.npz")
    np.savez(tmp, rowptr=rp, col=col, pu=pu, pv=pv)
    cuts = np.linspace(0, len(pu), n_proc + 1).astype(np.int64)
    try:
        with mp.get_context("spawn").Pool(n_proc) as pool:       # spawn: never fork a process that holds a HIP context
            res = pool.map(_cpu_worker, [(tmp, int(cuts[i]), int(cuts[i + 1])) for i in range(n_proc)])
    finally:
        os.remove(tmp)
    slowest = max(r[0] for r in res)
    hits = hits_at_100_parity(torch, g, orc)
    return {"value": len(pu) / dt, "unit": "edges/s", "cores": 1, "kind": "port",
            "sample": f"{len(pu)} candidate pairs (the 2-hop non-edges of every 512-th column, every {stride}-th of them), "
                      f"SciPy mirror of adamic_utils.AA batch 2000, per-batch loop only (weight prologue excluded); host has "
                      f"{os.cpu_count()} cores, 1 used",
            "c_port_value": len(pu) / dt_c,
            "all_cores": {"value": len(pu) / slowest, "unit": "edges/s", "cores": n_proc,
                          "what": "the same SciPy mirror, the sample split over one process per host core; rate = pairs / "
                                  "slowest worker's loop time"},
            "gpu_vs_sample_max_rel_err": rel_sample, "gpu_topk_rows_vs_mirror_max_rel_err": rel_topk,
            "hits_at_100": hits}


def hits_at_100_parity(torch, g, orc):
    """Hits@100 (the second half of BASELINE's metric) on a held-out split: 2 % of the undirected edges are removed from
    the graph (the positives), negatives are uniform random non-adjacent pairs, both scored by AA on the REMAINING
    graph -- by the engine and by the reference's CPU expression; Hits@K per ogb's rule (strict >)."""
    import numpy as np
    import eps_amd
    from eps_amd.evaluate import Evaluator
    from eps_amd.graph import CSRGraph
    dev = g.device
    gen = torch.Generator(device=dev).manual_seed(7)
    row, col, _ = g.coo()
    up = row < col
    er, ec = row[up], col[up]
    held = torch.rand(er.numel(), generator=gen, device=dev) < 0.02
    pos = torch.stack([er[held], ec[held]])[:, :200_000]
    keep = torch.stack([er[~held], ec[~held]])
    gt = CSRGraph.from_edge_index(keep, None, sparse_sizes=(g.n_rows, g.n_rows)).to_symmetric()
    neg = torch.randint(0, g.n_rows, (2, 200_000), generator=gen, device=dev)
    gp, _ = eps_amd.AA(gt, pos)
    gn, _ = eps_amd.AA(gt, neg)
    A = gt.to_scipy()
    with np.errstate(divide="ignore"):
        mult = 1 / np.log(A.sum(0))
        mult[np.isinf(mult)] = 0
        A_ = A.multiply(mult).tocsr()
        cp = np.array(np.sum(A[pos[0].cpu().numpy()].multiply(A_[pos[1].cpu().numpy()]), 1)).flatten().astype(np.float32)
        cn = np.array(np.sum(A[neg[0].cpu().numpy()].multiply(A_[neg[1].cpu().numpy()]), 1)).flatten().astype(np.float32)
    ev = Evaluator("ogbl-ppa")
    ev.K = 100
    h_gpu = ev.eval({"y_pred_pos": gp, "y_pred_neg": gn})["hits@100"]
    h_cpu = orc.hits_at_k(cp, cn, 100)
    return {"K": 100, "gpu": h_gpu, "cpu_reference_mirror": h_cpu, "identical": bool(h_gpu == h_cpu),
            "split": f"{pos.shape[1]} held-out edges (2 % of the graph's, removed before scoring) vs {neg.shape[1]} uniform "
                     "random pairs, AA on the remaining graph (seed 7)"}


class _ClockSampler:
    """Best-effort shader-clock samples while a loop runs: `rocm-smi --showclocks --json` as a CHILD process every 0.5 s from a
    thread (never an exec of this process; returns None when the tool is missing or prints something else)."""

    def __init__(self, enabled=True):
        import threading
        self.enabled = enabled
        self.samples, self._stop = [], threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _once(self):
        import re
        import subprocess
        try:
            out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=5).stdout
            card = next(iter(json.loads(out).values()))
            for k, v in card.items():
                if "sclk" in k.lower():
                    m = re.search(r"(\d+)\s*Mhz", str(v), re.I)
                    if m:
                        return int(m.group(1))
        except Exception:      # noqa: BLE001
            return None
        return None

    def _run(self):
        while not self._stop.is_set():
            v = self._once()
            if v:
                self.samples.append(v)
            self._stop.wait(0.5)

    def __enter__(self):
        if self.enabled:
            self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        if self.enabled:
            self._t.join(timeout=10)
        return False


# ------------------------------------------------------------------------------------------------ main
def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scaling", choices=["weak", "strong"], default=None,
                    help="N > 1: 'strong' (default) shards the columns of ONE graph over the ranks; 'weak' = one replica of the "
                         "whole job per rank")
    ap.add_argument("--keep_top", type=int, default=KEEP_TOP)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything besides the headline: roofline, step "
                         "breakdown, prep / cold / sustained / weak figures, secondary legs, CPU baseline")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline leg")
    ap.add_argument("--no-legs", action="store_true", help="with --full: skip the secondary kernel legs")
    ap.add_argument("--no-config-legs", action="store_true",
                    help="with --full: skip the per-config end-to-end legs (bench_configs.py)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (tests on a 1-GPU box: gloo)")
    ap.add_argument("--one-device", action="store_true", help="every rank on cuda:0 (tests on a 1-GPU box, with --backend gloo)")
    ap.add_argument("--sustain", type=float, default=5.0, help="with --full: seconds of the extra sustained loop (0: skip)")
    ap.add_argument("--nodes", type=int, default=576_289, help="graph size (tests use a small one)")
    ap.add_argument("--edges", type=int, default=21_231_931)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the rows the last timed step returned as DIR/pairs.npy and DIR/scores.npy")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


def launch_ranks(args) -> int:
    """`python bench.py --gpus N` from a plain shell: start N fresh rank processes through torch.distributed.run and pass their
    output through.  Decided BEFORE anything touches a GPU: this parent never initialises HIP (it does not even import
    torch), it only waits for the child and exits with its code -- no exec of a process that holds a device."""
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC: what RCCL needs on this host driver
    return subprocess.call(cmd, env=env)


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args))
    try:
        run(args)
    except SystemExit:
        raise
    except BaseException as exc:       # noqa: BLE001  a failing rank still leaves ONE parseable line, then a non-zero exit
        import traceback
        tb = traceback.format_exc()
        sys.stderr.write(tb)
        my_rank = int(os.environ.get("RANK", "0"))
        text = json.dumps({"metric": "candidate edges scored/sec on ogbl-ppa (ppa-like synthetic)", "value": None, "unit": "edges/s",
                           "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
                           "error": f"{type(exc).__name__}: {exc}", "rank": my_rank,
                           "traceback_tail": tb.strip().splitlines()[-6:]})
        # ONE line on the job's stdout: rank 0 reports at once; any other rank first gives rank 0 (and lower ranks) the time to do
        # so and to bring the launcher down on everybody -- when all ranks fail alike (a bad argument) only rank 0's line appears,
        # when rank 0 is healthy the failing rank's does.  The line goes out in a single write (line + newline: `print` makes two,
        # and two ranks writing at once produced `{...}{...}` on one line in the r05 suite).
        if my_rank:
            time.sleep(1.0 + 0.25 * my_rank)
        sys.stdout.write(text + "\n")
        sys.stdout.flush()
        # (no re-exec, no clean-up collectives: the other ranks are torn down by the launcher when this one exits non-zero)
        os._exit(1)


def run(args):

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
    # what each rank SEES of the job -- world size and rank as the process group reports them, its HIP device, the device's bus
    # id -- gathered onto rank 0 and printed with the line: a scaling record then checks itself (N distinct devices, one
    # backend, every rank part of the same group), which matters for the first run of this path on RCCL
    props = torch.cuda.get_device_properties(dev)
    me = {"rank": dist.get_rank() if world > 1 else 0, "world": dist.get_world_size() if world > 1 else 1, "env_rank": rank,
          "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "device_index": dev.index, "device": torch.cuda.get_device_name(dev),
          "pci_bus_id": getattr(props, "pci_bus_id", None), "uuid": str(getattr(props, "uuid", "")) or None,
          "backend": dist.get_backend() if world > 1 else None, "visible_devices": torch.cuda.device_count(),
          "ipc_mode_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}
    ranks_seen = [me]
    if world > 1:
        ranks_seen = [None] * world
        dist.all_gather_object(ranks_seen, me)

    import eps_amd  # noqa: F401
    from eps_amd import candidates, ops, scan, synth
    from eps_amd.graph import CSRGraph
    from eps_amd.heuristics import node_weight_table

    def sync():
        torch.cuda.synchronize(dev)

    g = synth.ppa_like(seed=3, device=dev, n_nodes=args.nodes, n_undirected=args.edges)
    w = node_weight_table(g, ops.W_AA)
    strong = world > 1 and args.scaling != "weak"
    srank, sworld = (rank, world) if strong else (0, 1)
    sync()

    # per-graph tables of a graph that is scanned repeatedly, built once like the graph itself: the hubs-first relabelled copy
    # the scan runs on, its revpos / half paths / column order / fixed-point weights / window + plan tables / sample
    def build_tables(graph, weights):
        gs_, perm_ = scan.scan_graph(graph, build=True)
        scan.column_order(gs_)
        scan._scan_weights(graph, gs_, perm_, weights)
        if scan.one_pass_available(gs_):
            scan.screen_tables(gs_)
            scan.window_paths(gs_)
        scan.screen_weights(graph, gs_, perm_, weights)          # screening weights, sum bounds, plan table
        scan.shard_columns(gs_, srank, sworld)
        scan.sample_columns(gs_, scan.sample_stride(args.keep_top), srank, sworld)
        paths = scan.total_half_paths(gs_)
        candidates.fused_scores_fit(graph, weights)
        sync()
        return paths

    half_paths_total = build_tables(g, w)

    def barrier():
        if world > 1:
            dist.barrier()
        sync()

    stats = {}
    out = {}

    def step():
        out["r"] = scan.scan_topk(g, w, args.keep_top, srank, sworld, stats=stats, rows_on=0 if sworld > 1 else None)

    for _ in range(args.warmup):
        step()
    # the timed region: HIP events around the scan launches only (the dominant kernel: `roofline.kernel_ms`), on their stream.
    # A plain run records them too and reads none of them: the timed steps are the same with and without --full.
    # The interpreter's cyclic collector is off inside the timed loops, as in `timeit`: a generation-2 pass of this process
    # (torch + the graph objects) stops the host for 30-45 ms, which lands in one step out of a hundred and moved the 100-step
    # average by 0.3-0.4 ms from run to run (tools/r05_loop_probe.py: median step 14.21 ms with and without it)
    import gc
    gc.collect()
    gc.disable()
    ops.KERNEL_EVENTS, ops.EVENT_NAMES = [], ()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    dt = time.perf_counter() - t0
    events, ops.KERNEL_EVENTS, ops.EVENT_NAMES = ops.KERNEL_EVENTS, None, None
    dumped = None
    if args.dump_outputs and rank == 0:                         # (strong scaling: the rows are gathered on rank 0, rows_on=0)
        dumped = dump_outputs(args.dump_outputs, out["r"][0], out["r"][1], g.n_rows)
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    n_cand = stats["candidates"]                   # directed candidates of the graph (kernel-counted)
    job_cand = n_cand if strong or world == 1 else n_cand * world
    bar = None if stats["bar"] is None else float(stats["bar"])
    ms_step = dt / args.steps * 1e3

    line = None
    if rank == 0:
        n_cu, dev_name = ops.device_info()
        line = {
            "metric": "candidate edges scored/sec on ogbl-ppa (ppa-like synthetic): Adamic-Adar over the FULL 2-hop non-edge "
                      "candidate set + top-4M selection",
            "value": job_cand * args.steps / dt,
            "unit": "edges/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ranks": ranks_seen,
            "distinct_devices": len({(r["device_index"], r["pci_bus_id"], r["uuid"]) for r in ranks_seen}),
            "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": "int64", "data": "synthetic",
            "value_unordered_pairs_per_s": job_cand / 2 * args.steps / dt,
            "full": args.full,
            "dump_outputs": dumped,
            "config": {"workload": "configs[2] ppa-like S3, full candidate set: N=%d, nnz=%d, %d directed 2-hop non-edge "
                                   "candidates per graph, filter.py --model adamic_ogb --keep_top %d (scan.scan_topk)"
                                   % (g.n_rows, g.nnz(), n_cand, args.keep_top),
                       "candidates_per_step_all_ranks": job_cand, "two_hop_half_paths": half_paths_total,
                       "arithmetic": "screening: u32 sums of weights rounded up to 2^-shift; reported scores: exact 2^-40 fixed-point "
                                     "sums (float64 of multiples of 2^-40: order-independent), rounded to f32",
                       "keep_top": args.keep_top, "bar": bar, "survivors": stats["survivors"],
                       "launches_per_step": stats["launches"], "graph_replicated": True, "device": dev_name, "n_cu": n_cu,
                       "notes": {"value": "DIRECTED candidates (both rows of the proposal file carry the score); each unordered "
                                          "pair is computed once: value_unordered_pairs_per_s.  'Scored' means: every candidate's sum "
                                          "over its common neighbours is accumulated -- SCREENED with >= upper bounds at 15 / 31 bits "
                                          "(weights rounded up to 2^-shift) -- and the survivors that can reach the top-K get their "
                                          "EXACT 2^-40 fixed-point score (eps_rescore_runs); r05: under the bar a column's heaviest hub "
                                          "rows are not walked at all -- their weights (at most half the bar per column) enter every "
                                          "pair of the column as a BOUND, and the slots that pass get the exact head term from the hub "
                                          "row bitmaps (eps_scan_refine) -- so a candidate reached through hub rows only is bounded, "
                                          "never touched (roofline.skipped_heads); r06: in the sparse tail of the id space a piece of a column keeps NO keys -- its paths add "
                                          "into two hashed half tables and a candidate's sum is bounded by the smaller of its two slots (a count-min sketch: an "
                                          "upper bound too; ids that reach the bar are reported from a second look at the paths and re-scored exactly); the K rows are identical to the exact "
                                          "scan's (eps_filter_scan: tests, profiles/r03/two_kernels_same_list.txt).  The literal "
                                          "filter.py:113-165 -- every candidate's exact score written out -- is the leg "
                                          "full_list_every_candidate_scored (--full)",
                                 "data": "synthetic stand-in (seeded R-MAT of ogbl-ppa's size): no dataset exists on the build or the GPU "
                                         "box, so Hits@100 parity is shown on a held-out split of the stand-in (--full: cpu_baseline.hits_at_100) "
                                         "and the published 53.24 (README.md:11-17) is reachable only through the $EPS_DATA_ROOT/ppa.pt "
                                         "hook (--full: legs.real_ppa)",
                                 "gc": "the interpreter's cyclic garbage collector is off inside the timed loop and, with --full, the sustained one (gc.collect() "
                                       "before, re-enabled after), as `timeit` does: a generation-2 pass stops this process's host thread "
                                       "for 30-45 ms, one step in a hundred or so (tools/r05_loop_probe.py)",
                                 "full": "false: a plain run -- set-up, warm-up, the timed steps, --dump-outputs and this line; true: "
                                         "--full, everything else the benchmark measures and checks measured after the timed steps"}},
        }

    def finish():
        if rank == 0:
            print(json.dumps(line), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()

    if not args.full:
        gc.enable()
        finish()
        return

    # --full from here on: everything else the benchmark measures and checks, after the timed steps and with their outputs dumped
    # where the rest of a step goes (`step_breakdown_ms`, `sharded_ms_per_rank`): a second, short loop with events around EVERY
    # library call -- some forty event records per step, which cost the host 0.4 ms a step when they sat in the timed region
    bd_steps = max(1, min(args.steps, 20))
    ops.KERNEL_EVENTS = []
    for _ in range(bd_steps):
        step()
    barrier()
    bd_events, ops.KERNEL_EVENTS = ops.KERNEL_EVENTS, None
    # what the FIRST scan of a fresh graph object costs: hubs-first copy and every per-graph table included.  Measured after the
    # timed loop, i.e. with the process's code objects loaded and its allocator warm (a fresh process adds ~1 GiB of first-time
    # hipMalloc and ~10 ms per torch operator it is the first to use: 0.1-0.25 s box to box -- profiles/r03/cold_scan.txt)
    # prep_ms: the same tables for another fresh graph object, without a scan (what a graph that is scanned repeatedly pays once)
    g_prep, w_prep = CSRGraph(g.rowptr, g.col, None, g.n_rows, g.n_cols), w.clone()
    sync()
    tp = time.perf_counter()
    build_tables(g_prep, w_prep)
    prep_ms = (time.perf_counter() - tp) * 1e3
    del g_prep, w_prep
    cold_ms = None
    if world == 1:
        g_cold = CSRGraph(g.rowptr, g.col, None, g.n_rows, g.n_cols)
        w_cold = w.clone()
        candidates.fused_scores_fit(g_cold, w_cold)
        sync()
        tc = time.perf_counter()
        scan.scan_topk(g_cold, w_cold, args.keep_top, relabel=True)
        sync()
        cold_ms = (time.perf_counter() - tc) * 1e3
        del g_cold, w_cold
    half = g.n_rows // (2 * sworld)
    scans = [e for e in events if e[0] in ("scan_piece_kernel", "filter_scan_kernel")]
    kernel_name = sorted({name for name, a, b, ncol in scans if ncol > half})
    kernel_name = kernel_name[0] if len(kernel_name) == 1 else "+".join(kernel_name)
    main_ms = [a.elapsed_time(b) for name, a, b, ncol in scans if ncol > half]
    samp_ms = [a.elapsed_time(b) for name, a, b, ncol in scans if ncol <= half]
    kern_ms = sum(main_ms) / max(1, len(main_ms))
    samp = sum(samp_ms) / max(1, len(samp_ms))
    # what a rank does on ITS share (shrinks with N): both scan launches, the local selects, the sort + exact re-scoring of its survivors
    per_step = {}
    for name, a, b, _ in bd_events:
        per_step[name] = per_step.get(name, 0.0) + a.elapsed_time(b) / bd_steps
    sharded_ms = sum(per_step.values())
    per_rank = [[kern_ms, samp, sharded_ms]]
    if world > 1:
        from eps_amd import dist as epd
        per_rank = torch.stack(epd.all_gather_list(torch.tensor([kern_ms, samp, sharded_ms], device=dev, dtype=torch.float64))).tolist()

    # N > 1, strong: the weak figure (every rank the whole job on its own replica) as a secondary key, from a short loop
    weak_value = None
    if strong:
        def wstep():
            scan.scan_topk(g, w, args.keep_top, 0, 1)
        wsteps = max(1, min(args.steps, 5))
        wstep()
        barrier()
        t0 = time.perf_counter()
        for _ in range(wsteps):
            wstep()
        barrier()
        tw = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        dist.all_reduce(tw, op=dist.ReduceOp.MAX)
        weak_value = n_cand * world * wsteps / tw.item()

    # the same step over >= `--sustain` seconds (the timed region above is 20 steps = 0.5 s in a driver run): clocks settle, the
    # figure is what a long job sees
    sustained = None
    if args.sustain <= 0:
        gc.enable()
    if args.sustain > 0:
        est = max(dt / args.steps, 1e-4)
        n_sus = max(args.steps, int(args.sustain / est) + 1)
        barrier()
        with _ClockSampler(enabled=rank == 0) as clk:           # (one sampler per job: rank 0's)
            t0 = time.perf_counter()
            for _ in range(n_sus):
                step()
            barrier()
            ts = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([ts], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ts = tt.item()
        gc.enable()
        sustained = {"steps": n_sus, "seconds": ts, "ms_per_step": ts / n_sus * 1e3, "value": job_cand * n_sus / ts,
                     "sclk_mhz_mean": (sum(clk.samples) / len(clk.samples)) if clk.samples else None,
                     "sclk_mhz_min": min(clk.samples) if clk.samples else None, "sclk_samples": len(clk.samples)}

    if rank == 0:
        # dominant kernel: the scan's main launch (eps_scan_screen, or eps_filter_scan where the piece kernel does not apply).
        # Algorithmic bytes per launch: every two-hop half path read once (4 B), the per-(v,w) descriptors
        # (col 4 + revpos 4 + rowptr 8 + weight 8), rowptr of the columns, and the survivors (12 B each); the per-rank
        # share under strong scaling.  The same unit for both kernels, so the fractions compare.
        # r05, skipped heads: a column does not walk its heaviest hub rows under the bar, so the launch reads the WALKED half paths
        # and rows only, and writes the slots that pass at bar - T_v (the walked list) -- that is what `achieved` counts.  The r02-r04
        # unit (every half path of the graph) stays next to it as `all_paths_unit`, so the rounds compare.
        all_bytes = (4 * half_paths_total + 24 * g.nnz() + 16 * g.n_rows) // sworld + 12 * (stats["survivors"] // 2 // sworld)
        heads_info = None
        abytes = all_bytes
        if stats.get("heads"):
            gs_, perm_ = scan.scan_graph(g)
            ht = scan.screen_weights(g, gs_, perm_, w).head_cur
            if ht is not None:
                walked_paths = int(ht.wpaths.to(torch.int64).bitwise_and(0xFFFFFFFF).sum())
                skipped_rows = int(ht.heads[:, 0].to(torch.int64).sum())
                slots = int(stats.get("walked_slots") or 0)
                abytes = (4 * walked_paths + 24 * (g.nnz() - skipped_rows) + 16 * g.n_rows) // sworld + 12 * (slots // sworld)
                heads_info = {"budget_share_of_bar": None if not bar else stats["head_budget"] / bar, "budget": stats["head_budget"],
                              "walked_half_paths": walked_paths, "walked_share": walked_paths / max(1, half_paths_total),
                              "rows_skipped": skipped_rows, "walked_list_slots_all_ranks": slots,
                              "pieces": int(ht.plan[1].shape[0]), "hub_rows": int(scan.hub_rows(gs_).shape[0]),
                              # (counted where a piece keeps keys: direct and hashed pieces; the sketch pieces of the tail do not count theirs)
                              "candidates_touched_by_the_walk": stats.get("touched"), "sketch_pieces": bool(stats.get("sketch")),
                              "plan_for_sketch_launches": bool(ht.wide)}
        kmax = max(r[0] for r in per_rank)
        achieved = abytes / (kmax * 1e-3) / 1e9
        pmc = {}
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tpath):
            pmc = json.load(open(tpath)).get(f"{kernel_name}/ppa_like/{g.n_rows}") or {}
            if not isinstance(pmc, dict):
                pmc = {"traffic": pmc}
        line.update({
            # (the two figures next to the steady-state step that the driver's stored tail used to cut off)
            "cold_ms_per_step": cold_ms,
            "sustained_ms_per_step": None if sustained is None else sustained["ms_per_step"],
            "weak_value": weak_value,
            "prep_ms": prep_ms,
            "kernel_ms_per_rank": [r[0] for r in per_rank], "sample_ms_per_rank": [r[1] for r in per_rank],
            "serial_ms": ms_step - kmax - max(r[1] for r in per_rank),
            "sharded_ms_per_rank": [r[2] for r in per_rank],
            "replicated_ms": ms_step - max(r[2] for r in per_rank),
            "step_breakdown_ms": per_step,
            "sustained": sustained,
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS, "hbm_frac": achieved / HBM_PEAK_GBPS, "traffic": pmc.get("traffic"),
                         "binds": pmc.get("binds"),
                         "kernel": kernel_name, "kernel_ms": kmax, "launches_timed": len(main_ms),
                         "sample_launch_ms": samp,
                         "algorithmic_bytes_per_launch": abytes,
                         # (`frac` counts the bytes the launch WALKS -- pruning lowers it while the launch gets faster; the same kernel
                         #  time against the r02-r04 unit, the one VERDICT r04's target was written in, rides at the top level too)
                         "frac_r04_unit": all_bytes / (kmax * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                         "all_paths_unit": {"bytes_per_launch": all_bytes, "GBps": all_bytes / (kmax * 1e-3) / 1e9,
                                            "frac": all_bytes / (kmax * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                                            "note": "the r02-r04 unit: 4 B x EVERY two-hop half path of the graph (walked or not) + "
                                                    "24 B x nnz + 16 B x N + 12 B x survivors, over the same kernel time"},
                         "skipped_heads": heads_info,
                         "issue": pmc.get("issue"),
                         "note": "`bound`: the unit of achieved / peak (bytes against the HBM peak, as the contract's vocabulary has "
                                 "it); `binds`: what limits the launch according to the counters.  Compulsory bytes: 4 B per "
                                 "two-hop half path + 24 B per stored entry + survivors; `traffic` = fabric bytes per launch "
                                 "(2 x FETCH_SIZE + WRITE_SIZE) and `issue` = VALU / LDS occupancy of the same launch, from the "
                                 "rocprofv3 PMC passes committed under profiles/ (profiles/traffic.json)"},
        })
        line["config"]["notes"].update({
            "replicated_ms": "ms_per_step minus the slowest rank's sharded work (both scan launches, its local "
                             "selects, the sort and exact re-scoring of its survivors -- HIP events, step_breakdown_ms, taken in a "
                             "second loop of <= 20 steps right after the timed region, which itself carries events around "
                             "the scan launches only): "
                             "collectives, host reads, the gathered selection and this rank's range of the final "
                             "ordering -- what does not shrink with N",
            "sustained": "the same step repeated for >= --sustain seconds after the timed region; sclk: shader-clock "
                         "samples a child process takes during the loop (_ClockSampler; null when none could be read)",
            "prep_ms": "hubs-first relabelled copy + revpos / half paths / column order / fixed-point "
                       "weights / window tables / sum bounds / plan table / sample, built once per graph, "
                       "OUTSIDE the timed region (timed on a fresh graph object after the loop: allocator warm)",
            "cold_ms_per_step": "first scan of a FRESH graph object incl. relabelling and every per-graph table, "
                                "measured after the timed loop (code objects loaded, allocator warm); a "
                                "one-shot filter.py process pays its first-time hipMalloc and code-object "
                                "loads on top: profiles/r03/cold_scan.txt",
            "serial_ms": "ms_per_step - slowest rank's main kernel - its sample launch: bar, selection, "
                         "collectives, host"})
    if rank == 0 and world == 1 and not args.no_legs:
        line["legs"] = {"pair_intersection": leg_pair_kernel(torch, g, w, ops, candidates)}
        line["legs"].update(leg_gnn(torch, g, ops))
        if not args.no_config_legs:
            import bench_configs
            torch.cuda.empty_cache()
            line["legs"].update(bench_configs.run_all(torch, args.keep_top))
    if rank == 0 and world == 1 and not args.no_cpu:
        line["cpu_baseline"] = cpu_baseline(torch, g, w, ops, candidates, out["r"][0], out["r"][1])
        line["cpu_baseline"]["gpu_over_cpu_1core"] = line["value"] / line["cpu_baseline"]["value"]
        line["cpu_baseline"]["gpu_over_cpu_all_cores"] = line["value"] / line["cpu_baseline"]["all_cores"]["value"]
    finish()


if __name__ == "__main__":
    main()
