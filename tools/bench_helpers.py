"""What the model bench tools (ncn_bench.py, buddy_bench.py) share: the HIP-event timer, the stand-in datasets on the device, one
batch of training.train, the per-dataset default arguments and one training step."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    import torch
    ts = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def rate(rec, n_bytes):
    rec["GB_per_s"] = round(n_bytes / (rec["median_ms"] * 1e-3) / 1e9, 1)
    return rec


def stand_in(dataset, scale, dev):
    import torch
    from eps_amd import datasets
    from eps_amd.graph import add_edges
    os.environ["EPS_SYNTH_SCALE"] = str(scale)
    ei, ew, split_edge, data = datasets.get_data(argparse.Namespace(dataset=dataset, synthetic=True, use_feature=dataset == "collab"))
    data = data.to(dev)
    data.adj_t = add_edges(dataset, ei.to(dev), ew.to(dev), torch.zeros((2, 0), dtype=torch.long, device=dev), data.num_nodes)
    data.full_adj_t = data.adj_t
    return split_edge, data


def train_batch(dataset, split_edge, data, batch_size, dev):
    """The pairs of one step of training.train: a batch of positives in both directions, then as many negatives."""
    import torch
    from eps_amd import training
    from eps_amd.rank_helpers import to_undirected
    torch.manual_seed(7)
    pos = split_edge['train']['edge'].to(dev)
    pos_edge = to_undirected(pos[torch.randperm(pos.size(0), device=dev)[:batch_size]].t())
    if dataset == "collab":
        neg_edge = torch.randint(0, data.num_nodes, pos_edge.size(), dtype=torch.long, device=dev)
    else:
        row, col, _ = data.adj_t.coo()
        neg_edge = training.negative_sampling(torch.stack([col, row]), data.num_nodes, pos_edge.size(1))
    return pos_edge, neg_edge


def default_args(dataset, model):
    from eps_amd import models
    keys = ["num_layers", "hidden_channels", "dropout", "batch_size", "lr", "epochs", "use_feature", "use_learnable_embedding"]
    return models.default_model_configs(argparse.Namespace(dataset=dataset, model=model, **{k: None for k in keys}))


def train_step(model, data, pos_edge, neg_edge, opt):
    import torch
    opt.zero_grad()
    out = model(data.x, torch.cat([pos_edge, neg_edge], 1), data.adj_t).squeeze()
    k = pos_edge.size(1)
    loss = -torch.log(out[:k] + 1e-8).mean() - torch.log(1 - out[k:] + 1e-8).mean()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    opt.step()
    return loss
