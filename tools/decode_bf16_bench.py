#!/usr/bin/env python3
"""Measure the bf16 screening decode (eps_mlp_decode_bf16, filter.py --decode_precision bf16); one JSON line per step.

Without --step the tool is a driver: it runs its three steps as child processes, each under its own `timeout -k 10`, chained
with `&&` (a step that fails, faults or runs out of time ends the run; nothing else is started on the GPU after it):

  kernel: eps_mlp_decode against eps_mlp_decode_bf16 on the SAME --edges random edges of a ppa-sized table (N = 576,289,
      H = 256, L = 3), HIP events, median of --reps after --warmup; edges/s, the ratio, and the share of the f32 / bf16 MFMA peak
      under the FLOP model of BASELINE.md (2 H^2 (L - 1) + 3 H per edge).
  filter: filter.py --dataset ddi --synthetic --model gcn --keep_top K under both precisions (wall time of the scoring section
      and of the whole command; a freshly initialised checkpoint).
  recall: the share of the fp32 run's K rows that the bf16 run also wrote, for G in {1, 1.25, 1.5, 2, 4}, on the ddi-like and
      collab-like stand-ins with a seeded, briefly trained GCN (random weights give scores too flat to mean anything).

Run:  python tools/decode_bf16_bench.py [--edges 4194304 --keep_top 100000 --reps 10 --warmup 3 --epochs 3]
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12
PEAK_BF16_MFMA = 16 * PEAK_F32_MFMA       # the f32-input MFMA runs at 1/16 of the bf16 rate on gfx950
GUARDS = (1.0, 1.25, 1.5, 2.0, 4.0)
STEP_SECONDS = {"kernel": 240, "filter": 300, "recall": 600}


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def step_kernel(a, dev):
    import torch
    from eps_amd import ops
    n, H, L, E = 576_289, 256, 3, a.edges
    g = torch.Generator(device=dev).manual_seed(1)
    h = torch.randn(n, H, device=dev, generator=g)
    u = torch.randint(0, n, (E,), device=dev, dtype=torch.int32, generator=g)
    v = torch.randint(0, n, (E,), device=dev, dtype=torch.int32, generator=g)
    ws = [torch.randn(H if i < L - 1 else 1, H, device=dev, generator=g) / H ** 0.5 for i in range(L)]
    bs = [torch.randn(H if i < L - 1 else 1, device=dev, generator=g) * 0.1 for i in range(L)]
    hb = ops.to_bf16(h)
    wb = [ops.to_bf16(w) for w in ws[:-1]] + [ws[-1]]
    flop = E * (2 * H * H * (L - 1) + 3 * H)
    ms32, lo32 = timed(lambda: ops.mlp_decode(h, u, v, ws, bs, apply_sigmoid=False), a.reps, a.warmup)
    ms16, lo16 = timed(lambda: ops.mlp_decode_bf16(hb, u, v, wb, bs, apply_sigmoid=False), a.reps, a.warmup)
    conv, _ = timed(lambda: ops.to_bf16(h), a.reps, a.warmup)
    d = (ops.mlp_decode_bf16(hb, u, v, wb, bs, apply_sigmoid=False) - ops.mlp_decode(h, u, v, ws, bs, apply_sigmoid=False)).abs()
    return {"step": "kernel", "nodes": n, "H": H, "L": L, "edges": E,
            "fp32": {"ms": round(ms32, 3), "min_ms": round(lo32, 3), "edges_per_s": round(E / (ms32 * 1e-3), 1),
                     "frac_f32_mfma_peak": round(flop / (ms32 * 1e-3) / PEAK_F32_MFMA, 3)},
            "bf16": {"ms": round(ms16, 3), "min_ms": round(lo16, 3), "edges_per_s": round(E / (ms16 * 1e-3), 1),
                     "frac_bf16_mfma_peak": round(flop / (ms16 * 1e-3) / PEAK_BF16_MFMA, 4)},
            "speedup": round(ms32 / ms16, 3), "table_to_bf16_ms": round(conv, 3),
            "logit_abs_diff": {"max": float(d.max()), "mean": float(d.mean())}}


def _trained(dataset, epochs, dev, hidden=None):
    """(args, data, model in eval mode, losses): the synthetic stand-in and a GCN trained for ``epochs`` epochs from seed 0."""
    import torch
    from eps_amd import datasets, models, training
    os.environ.pop("EPS_SYNTH_SCALE", None)
    args = models.default_model_configs(argparse.Namespace(dataset=dataset, model="gcn", synthetic=True,
                                                           **{k: None for k in models._KEYS}))
    if hidden:
        args.hidden_channels = hidden
    _, _, split_edge, data = datasets.get_data(args)
    data = data.to(dev)
    torch.manual_seed(0)
    model = models.build_model(args, data, dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    losses = [training.train(model, data, dataset, split_edge, opt, args.batch_size, True, "gcn", dev) for _ in range(epochs)]
    return args, data, model.eval(), [round(float(x), 4) for x in losses]


def step_filter(a, dev):
    import torch
    from eps_amd import filter_stage
    out = {"step": "filter", "keep_top": a.keep_top}
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            args, data, model, _ = _trained("ddi", 0, dev)
            os.makedirs("models")
            torch.save(model.state_dict(), "models/ddi_gcn||0|0.pt")
            argv = ["--dataset", "ddi", "--model", "gcn", "--checkpoint", "ddi_gcn||0|0.pt", "--synthetic", "--keep_top", str(a.keep_top)]
            for prec in ("fp32", "bf16", "fp32", "bf16"):          # (the first pair also pays the one-off set-up: the second is quoted)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                filter_stage.main(argv + ["--decode_precision", prec])
                torch.cuda.synchronize()
                out[prec] = {"command_s": round(time.perf_counter() - t0, 3), "scored_s": round(filter_stage.LAST_TIMING["scored_s"], 4),
                             "gpu_ms": round(filter_stage.LAST_TIMING["gpu_ms"], 2), "candidates": filter_stage.LAST_TIMING["candidates"]}
        finally:
            os.chdir(cwd)
    out["scored_speedup"] = round(out["fp32"]["gpu_ms"] / out["bf16"]["gpu_ms"], 3)
    return out


def step_recall(a, dev):
    import torch
    from eps_amd import filter_stage
    out = {"step": "recall", "epochs": a.epochs, "guards": list(GUARDS)}
    for dataset, keep in (("ddi", a.keep_top), ("collab", a.keep_top)):
        args, data, model, losses = _trained(dataset, a.epochs, dev)
        with torch.no_grad():
            p32, s32, seen = filter_stage.gnn_half_topk(args, model, data, keep, 0, 1)
            want = set(((p32[1] << 32) | p32[0]).tolist())
            rec = {}
            for g in GUARDS:
                pb, _, _ = filter_stage.gnn_half_topk(args, model, data, keep, 0, 1, precision="bf16", guard=g)
                rec[f"{g:g}"] = round(len(want & set(((pb[1] << 32) | pb[0]).tolist())) / max(len(want), 1), 6)
        out[dataset] = {"nodes": data.num_nodes, "H": args.hidden_channels, "layers": args.num_layers, "keep_top": keep,
                        "rows": len(want), "candidates": seen, "losses": losses, "distinct_fp32_scores": int(torch.unique(s32).numel()),
                        "recall": rec}
    ok = [g for g in GUARDS if all(out[d]["recall"][f"{g:g}"] == 1.0 for d in ("ddi", "collab"))]
    out["smallest_guard_with_recall_1"] = ok[0] if ok else None
    out["default_guard_rule"] = "twice the smallest measured guard whose recall is 1.0 on both stand-ins"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--edges", type=int, default=1 << 22)
    ap.add_argument("--keep_top", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    a = ap.parse_args()
    if a.step is None:
        common = f"--edges {a.edges} --keep_top {a.keep_top} --reps {a.reps} --warmup {a.warmup} --epochs {a.epochs}"
        chain = " && ".join(f"timeout -k 10 {STEP_SECONDS[s]} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} "
                            f"--step {s} {common}" for s in ("kernel", "filter", "recall"))
        raise SystemExit(subprocess.call(["bash", "-c", chain]))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("decode_bf16_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    res = {"kernel": step_kernel, "filter": step_filter, "recall": step_recall}[a.step](a, dev)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
