"""GPU, world_size 2 on the one GPU (gloo): the device draw over a placed store whose peer rows
are read from the peer's mapped buffer.

Each rank builds the 600-node test graph, the placement over 2 ranks (60 rows buffered per rank),
its FeatureStore, a PeerDirect over it and ``PlacedFeatures.from_store(..., peers=direct)``; a
NeighborSampler over that draws two batches of its rank's share of an epoch. X0 must equal the host
table's rows at the batch's input nodes bit for bit on both ranks, and every source — this rank's
buffer, the peer's mapped buffer, the host table — must have served rows."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
WORLD = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), GNN_DIST_BACKEND="gloo")
    import torch.distributed as dist

    try:
        from gnn_amd import placement, staging
        from gnn_amd.neighbor import NeighborSampler
        from gnn_amd.placed import PlacedFeatures
        from gnn_amd.train import init_distributed
        from test_exact_cpu import make_world
        from test_placed_cpu import C, NN, TRAIN, _labels

        init_distributed()
        dev = torch.device("cuda", 0)
        lap, feats = make_world("graphsage", NN, 48)
        feats = feats.to(torch.float16)
        pl = placement.create_buffer(lap, TRAIN, 60, list(range(world)), 2, alpha=0)
        store = staging.FeatureStore(feats, pl.gpu_buffer_group[rank], dev, rank)
        direct = staging.PeerDirect(store, feats=feats, buffer_nodes=pl.gpu_buffer_group)
        pf = None
        ok, counts = True, None
        try:
            pf = PlacedFeatures.from_store(store, pl, rank, peers=direct)
            ns = NeighborSampler(lap, [10, 5], [1, 1], pf, _labels(NN, C), dev)
            batches = 0
            for b in ns.epoch(TRAIN, 130, seed=5, rank=rank, world_size=world):  # ends with pf.check()
                ok = ok and torch.equal(b.x0.cpu(), feats.float()[b.input_nodes.cpu()])
                batches += 1
            ok = ok and batches == 2
            counts = pf.counts()
            pf.close()  # releases the host table's registration; the next store registers it again
            pf = None
            # without the mapping the same nodes come from the host table
            alone = PlacedFeatures.from_store(store, pl, rank)
            b2 = NeighborSampler(lap, [10, 5], [1, 1], alone, _labels(NN, C), dev).sample(TRAIN[:130], 7)
            ok = ok and torch.equal(b2.x0.cpu(), feats.float()[b2.input_nodes.cpu()])
            ok = ok and alone.counts()["peers"] == [] and alone.counts()["host"] > 0
            alone.check()
            alone.close()
        finally:
            if pf is not None:
                pf.close()
            direct.close()  # collective
        q.put((rank, "ok" if ok else "X0 differs from the host table", counts))
    except Exception as e:  # report instead of leaving the parent waiting
        q.put((rank, f"error: {e!r}", None))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_placed_store_with_mapped_peers_world2():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        out = sorted([q.get(timeout=120) for _ in range(WORLD)], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank, status, counts in out:
        assert status == "ok", (rank, status)
        # every source is used: the own buffer, the peer's mapped buffer and the host table
        assert counts["own"] > 0 and len(counts["peers"]) == 1 and counts["peers"][0] > 0 and counts["host"] > 0, \
            (rank, counts)
