"""GPU, two ranks on the one GPU over gloo (the harness of tests/test_dist_gpu.py): peer rows of
an fp16 feature store. PeerDirect gathers them from the peer's mapped 16-bit buffer, PeerExchange
moves them in fp16 and widens in its final scatter; either way X0 holds
``feats.float()[input_nodes]`` bit for bit, and a rank pair whose stores differ in kind is
refused on both ranks."""
import numpy as np
import pytest
import torch

from test_dist_gpu import _env, _spawn

pytestmark = pytest.mark.gpu

F, K, N_IN = 37, 300, 500


def _table(world):
    g = torch.Generator().manual_seed(11)
    return (torch.randn(world * K, F, generator=g) * 20).half()


def _plan(rank, world, staging):
    rng = np.random.default_rng(10 + rank)
    empty = np.zeros(0, np.int64)
    peer = 1 - rank
    peer_pos, peer_src = [empty] * world, [empty] * world
    peer_pos[peer] = np.sort(rng.choice(N_IN, 200, replace=False)).astype(np.int64)
    peer_src[peer] = rng.integers(0, K, 200).astype(np.int64)
    peer_src[peer][0] = K - 1  # the last slot of the peer's buffer
    return staging.StagePlan(N_IN, empty, empty, empty, None, peer_pos, peer_src), peer_pos[peer], peer_src[peer]


def _peer_rows_worker(rank, world, port, q, direct):
    _env(rank, world, port)
    import torch.distributed as dist

    try:
        from gnn_amd import staging
        from gnn_amd.train import init_distributed

        init_distributed()
        dev = torch.device("cuda", 0)
        feats = _table(world)
        nodes = [np.arange(r * K, (r + 1) * K) for r in range(world)]  # rank r buffers nodes [r K, (r+1) K)
        store = staging.FeatureStore(feats, nodes[rank], dev, rank)
        assert store.gpu_buffer.dtype == torch.float16 and store.ld_rows == 64
        if direct:
            ex = staging.PeerDirect(store, feats=feats, buffer_nodes=nodes)
            assert ex.kind == 1 and ex.ld == 64 and ex.verified_rows == 3
        else:
            ex = staging.PeerExchange()
        plan, pos, src = _plan(rank, world, staging)
        x0 = torch.full((N_IN, store.ld), -1.0, device=dev)
        st = torch.cuda.Stream(device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            for _ in range(2):
                ex.exchange(plan, x0, store)
        torch.cuda.synchronize()
        got = x0.cpu()
        want = torch.zeros((len(src), store.ld))
        want[:, :F] = feats.float()[torch.from_numpy((1 - rank) * K + src)]
        ok = torch.equal(got[torch.from_numpy(pos)].view(torch.int32), want.view(torch.int32))
        untouched = np.setdiff1d(np.arange(N_IN), pos)
        ok = ok and bool((got[torch.from_numpy(untouched)] == -1.0).all())
        if direct:
            ex.close()
        q.put((rank, "ok" if ok else "rows differ", None, None))
    except Exception as e:  # report instead of leaving the parent waiting
        q.put((rank, f"error: {e!r}", None, None))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _mismatch_worker(rank, world, port, q):
    """Rank 0 holds an fp16 store, rank 1 a bf16 one: PeerDirect must raise on both."""
    _env(rank, world, port)
    import torch.distributed as dist

    try:
        from gnn_amd import staging
        from gnn_amd.train import init_distributed

        init_distributed()
        dev = torch.device("cuda", 0)
        feats = _table(world)
        if rank == 1:
            feats = feats.bfloat16()
        store = staging.FeatureStore(feats, np.arange(rank * K, (rank + 1) * K), dev, rank)
        status = "no error raised"
        try:
            staging.PeerDirect(store)
        except RuntimeError as e:
            status = "ok" if "kind" in str(e) and "PeerDirect unavailable" in str(e) else f"other error: {e}"
        q.put((rank, status, None, None))
    except Exception as e:
        q.put((rank, f"error: {e!r}", None, None))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "alltoall"])
def test_peer_rows_from_fp16_store_bit_exact(direct):
    out = _spawn(_peer_rows_worker, extra=(direct,))
    for rank, status, _, _ in out:
        assert status == "ok", f"rank {rank}: {status}"


def test_peer_direct_refuses_mismatched_kinds():
    out = _spawn(_mismatch_worker)
    assert len(out) == 2
    for rank, status, _, _ in out:
        assert status == "ok", f"rank {rank}: {status}"
