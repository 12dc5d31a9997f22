"""GPU: filter.py --keep_per_node k with two ranks on ONE GPU (gloo as the transport, both ranks on cuda:0).  Candidate columns
are sharded, a column belongs to one rank, so each rank cuts its own columns and the kept rows travel through the whole-file
gather: the two-rank file equals the one-rank file bit for bit."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = "0.05"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, workdir, argv):
    sys.path.insert(0, ROOT)
    os.chdir(workdir)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), EPS_SYNTH_SCALE=SCALE)
    import eps_amd  # noqa: F401
    from eps_amd import candidates, filter_stage
    candidates.DEFAULT_BLOCK_PATHS = 30_000          # several blocks per rank
    filter_stage.main(argv + ["--dist_backend", "gloo", "--device", "0"])
    torch.distributed.destroy_process_group()


def test_filter_two_ranks_per_node(eps, dev, tmp_path, monkeypatch):
    from eps_amd import filter_stage
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", SCALE)
    argv = lambda run: ["--dataset", "collab", "--model", "adamic_ogb", "--checkpoint", f"collab_adamic_ogb||0|{run}.pt",  # noqa: E731
                        "--synthetic", "--keep_per_node", "7"]
    single = torch.load(filter_stage.main(argv(0)))
    mp.spawn(_rank_main, args=(2, _free_port(), str(tmp_path), argv(1)), nprocs=2, join=True)
    multi = torch.load("filtered_edges/collab_adamic_ogb__0_1_sorted_edges.pt")
    assert single.shape[0] > 1000 and int(torch.bincount(single[:, 1].long()).max()) == 7
    assert torch.equal(single, multi)
