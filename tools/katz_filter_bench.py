#!/usr/bin/env python3
"""Time the scoring of `filter.py --model katz` on the full-scale stand-ins: the column kernel (eps_katz_column_scores) against
the route the parent code offered -- candidate lists + the pair kernel (eps_katz_pair_scores) on the same blocks; one JSON line
per step.

Without --step the tool is a driver: it runs its steps as child processes, each under its own `timeout -k 10`, chained with `&&`
(a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  collab: the collab-like stand-in (EPS_SYNTH_SCALE = --scale), every 2-hop non-edge, both routes in full.
  ddi:    the ddi-like stand-in: the pair route on the candidates of --sample seeded columns, scaled by candidates to the whole
          set (in full it runs for minutes); the column route on the same sample and in full.

Per route: HIP events around the scoring calls of all blocks (candidate generation is outside), --warmup runs, then --reps
alternating runs of the two routes; median, min and max are reported, and candidates/s from the median.  The column route is
also timed with ONE candidate per non-empty column and one candidate per work unit: that launch builds every column's table
once and scores next to nothing.  The table-build share scales it by the builds of the full run (a column split over several
work units is built once per unit) -- and the column route is timed at other work-unit sizes (--chunks), which trade rebuilds
against balance.  Before anything is timed the two routes' scores are compared (both are within one float32 ulp of float64 truth in
the test suite, so they differ by at most two).

Run:  python tools/katz_filter_bench.py [--scale 1.0 --reps 5 --warmup 2 --sample 64]
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = {"collab": 900, "ddi": 600}


def _event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warmup):
    """name -> {median, min, max} ms of every route, the routes taking turns inside one process."""
    ts = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            t = _event_ms(fn)
            if i >= warmup:
                ts[k].append(t)
    return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            for k, v in ts.items()}


class Blocks:
    """The candidate blocks of a graph as the filter's block route makes them, resident on the device; optionally only the
    candidates of the columns flagged in ``keep`` (bool[N])."""

    def __init__(self, g, keep=None):
        import torch
        from eps_amd import candidates
        self.g, self.items = g, []
        for lo, hi in candidates.column_blocks(g):
            pairs = candidates.expand_block(g, lo, hi, long_pairs=False)[0]
            u, v = pairs[0].to(torch.int32), pairs[1].to(torch.int32)
            if keep is not None:
                m = keep[v.long()]
                u, v = u[m], v[m]
            if u.numel() == 0:
                continue
            u, v = u.contiguous(), v.contiguous()
            colptr = torch.searchsorted(v, torch.arange(lo, hi + 1, dtype=v.dtype, device=v.device)).to(torch.int64)
            self.items.append((lo, hi, colptr, u, v))
        self.candidates = sum(int(it[3].numel()) for it in self.items)

    def first_of_each_column(self):
        """The same blocks with one candidate per non-empty column."""
        import torch
        b = Blocks.__new__(Blocks)
        b.g, b.items = self.g, []
        for lo, hi, colptr, u, v in self.items:
            has = colptr[1:] > colptr[:-1]
            first = colptr[:-1][has]
            cp = torch.zeros_like(colptr)
            torch.cumsum(has.to(torch.int64), 0, out=cp[1:])
            b.items.append((lo, hi, cp, u[first].contiguous(), v[first].contiguous()))
        b.candidates = sum(int(it[3].numel()) for it in b.items)
        return b

    def work_units(self, chunk=0):
        from eps_amd import ops
        return sum(-(-int(it[3].numel()) // (chunk or ops.katz_columns_chunk(it[3].numel()))) for it in self.items)

    def table_builds(self, chunk=0):
        """(column, work unit) meetings: every one builds the column's table.  chunk 0: each block's default unit."""
        import torch
        from eps_amd import ops
        tot, given = 0, chunk
        for lo, hi, colptr, u, v in self.items:
            chunk = given or ops.katz_columns_chunk(u.numel())
            s, e = colptr[:-1], colptr[1:]
            has = e > s
            tot += int((torch.div(e[has] - 1, chunk, rounding_mode="floor") - torch.div(s[has], chunk, rounding_mode="floor") + 1).sum().item())
        return tot

    def columns(self, gt, p_in, coeffs, chunk=0):
        from eps_amd import ops
        g = self.g
        return [ops.katz_column_scores(g.rowptr, g.col, g.val, gt.rowptr, gt.col, gt.val, p_in, g.n_rows, lo, hi, colptr, u, coeffs,
                                       chunk=chunk)
                for lo, hi, colptr, u, v in self.items]

    def pairs(self, gt, p_out, p_in, coeffs):
        from eps_amd import ops
        g = self.g
        return [ops.katz_pair_scores(g.rowptr, g.col, g.val, gt.rowptr, gt.col, gt.val, p_out, p_in, g.n_rows, u, v, coeffs)
                for lo, hi, colptr, u, v in self.items]


def _ulp_apart(a, b):
    """Largest distance of two float32 tensors in units in the last place (ordered-integer view)."""
    import torch
    def key(x):
        i = x.view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max().item()) if a.numel() else 0


def _graph(dataset, scale, dev):
    import torch
    from eps_amd import datasets, heuristics
    from eps_amd.graph import add_edges
    os.environ["EPS_SYNTH_SCALE"] = str(scale)
    ei, ew, _, data = datasets.get_data(argparse.Namespace(dataset=dataset, synthetic=True, use_feature=False))
    g = add_edges(dataset, ei.to(dev), ew.to(dev), torch.zeros((2, 0), dtype=torch.long, device=dev), data.num_nodes)
    return g, heuristics._katz_transpose(g), heuristics.katz_coefficients()


def _compare(blocks, gt, p_out, p_in, coeffs, a, with_pairs=True):
    import torch
    from eps_amd import heuristics, ops
    rec = {"candidates": blocks.candidates, "blocks": len(blocks.items),
           "default_chunk": [ops.katz_columns_chunk(it[3].numel()) for it in blocks.items],
           "work_units": blocks.work_units(), "table_builds": blocks.table_builds(),
           "three_hop_steps": sum(heuristics.katz_column_steps(blocks.g, it[3]) for it in blocks.items)}
    fns = {"columns": lambda: blocks.columns(gt, p_in, coeffs)}
    ones = blocks.first_of_each_column()
    rec["non_empty_columns"] = ones.candidates
    # (one candidate per column AND per work unit: every column's table is built once, by as many workgroups as the full run has)
    fns["columns_one_candidate_per_column"] = lambda: ones.columns(gt, p_in, coeffs, chunk=1)
    for c in a.chunks:
        fns[f"columns_chunk_{c}"] = (lambda c: lambda: blocks.columns(gt, p_in, coeffs, chunk=c))(c)
        rec[f"table_builds_chunk_{c}"] = blocks.table_builds(c)
    if with_pairs:
        got = torch.cat(blocks.columns(gt, p_in, coeffs))
        held = []
        first_ms = _event_ms(lambda: held.append(torch.cat(blocks.pairs(gt, p_out, p_in, coeffs))))
        ref = held.pop()
        if first_ms > a.slow_ms:                 # (a pair route of minutes: two runs of each route, the first one above the warm-up)
            a = argparse.Namespace(**{**vars(a), "reps": 2, "warmup": 0})
            rec["reps_reduced_to"] = 2
        rec["max_ulp_between_routes"] = _ulp_apart(got, ref)
        rec["scores_bitwise_equal"] = bool(torch.equal(got, ref))
        del got, ref
        fns["pairs"] = lambda: blocks.pairs(gt, p_out, p_in, coeffs)
    rec.update(alternate(fns, a.reps, a.warmup))
    for k in ("columns", "pairs"):
        if k in rec:
            rec[k]["candidates_per_s"] = round(blocks.candidates / (rec[k]["median_ms"] * 1e-3), 1)
    # the build-only launch, scaled from one build per column to the builds of the full run, over the full run
    rec["table_build_share"] = round(rec["columns_one_candidate_per_column"]["median_ms"] * rec["table_builds"]
                                     / max(rec["non_empty_columns"], 1) / rec["columns"]["median_ms"], 3)
    if with_pairs:
        rec["speedup_median"] = round(rec["pairs"]["median_ms"] / rec["columns"]["median_ms"], 2)
        # faster by more than the run-to-run spread of the two measurements: the slowest column run against the fastest pair run
        rec["columns_faster_beyond_spread"] = bool(rec["columns"]["max_ms"] < rec["pairs"]["min_ms"])
        rec["mean_degree_of_candidates"] = round(rec["three_hop_steps"] / max(blocks.candidates, 1), 2)
    return rec


def step_collab(a, dev):
    g, (gt, p_out, p_in), coeffs = _graph("collab", a.scale, dev)
    out = {"step": "collab", "scale": a.scale, "nodes": g.n_rows, "entries": g.nnz()}
    out["full"] = _compare(Blocks(g), gt, p_out, p_in, coeffs, a)
    return out


def step_ddi(a, dev):
    import torch
    g, (gt, p_out, p_in), coeffs = _graph("ddi", a.scale, dev)
    out = {"step": "ddi", "scale": a.scale, "nodes": g.n_rows, "entries": g.nnz(), "sample_columns": a.sample}
    keep = torch.zeros(g.n_rows, dtype=torch.bool, device=dev)
    gen = torch.Generator().manual_seed(64)
    keep[torch.randperm(g.n_rows, generator=gen)[:a.sample].to(dev)] = True
    out["sample"] = _compare(Blocks(g, keep), gt, p_out, p_in, coeffs, a)
    out["full"] = _compare(Blocks(g), gt, p_out, p_in, coeffs, a, with_pairs=False)
    scale = out["full"]["candidates"] / max(out["sample"]["candidates"], 1)
    out["pairs_full_estimate_ms"] = round(out["sample"]["pairs"]["median_ms"] * scale, 1)
    out["speedup_full_estimate"] = round(out["pairs_full_estimate_ms"] / out["full"]["columns"]["median_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--chunks", type=int, nargs="*", default=[512, 2048, 8192, 32768], help="the column route also at these candidates per work unit")
    ap.add_argument("--slow_ms", type=float, default=20000.0, help="a first pair-route run longer than this: 2 reps, no further warm-up")
    a = ap.parse_args()
    if a.step is None:
        common = f"--scale {a.scale} --reps {a.reps} --warmup {a.warmup} --sample {a.sample} --slow_ms {a.slow_ms} --chunks {' '.join(map(str, a.chunks))}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in ("ddi", "collab"))
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("katz_filter_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    res = {"collab": step_collab, "ddi": step_ddi}[a.step](a, dev)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
