"""GPU, two ranks on the one GPU over gloo (the harness of tests/test_dist_gpu.py): peer rows of a
keep16 fp16 feature store delivered into a 16-bit X0 unwidened — PeerDirect copies them from the
peer's mapped buffer, PeerExchange moves them in fp16 and scatters them as they travelled — so X0
holds ``feats[input_nodes]`` bit for bit, pads zero, rows of other sources untouched."""
import numpy as np
import pytest
import torch

from test_dist_gpu import _env, _spawn
from test_feat16_dist_gpu import F, K, N_IN, _plan, _table

pytestmark = pytest.mark.gpu


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
        store = staging.FeatureStore(feats, nodes[rank], dev, rank, keep16=True)
        assert store.keep16 and store.gpu_buffer.dtype == torch.float16 and store.ld_rows == 64
        ex = staging.PeerDirect(store, feats=feats, buffer_nodes=nodes) if direct else staging.PeerExchange()
        plan, pos, src = _plan(rank, world, staging)
        assert len(src) > 0  # the peer supplies rows
        x0 = torch.full((N_IN, store.ld_rows), -1.0, dtype=torch.float16, device=dev)
        st = torch.cuda.Stream(device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            for _ in range(2):
                ex.exchange(plan, x0, store)
        torch.cuda.synchronize()
        got = x0.cpu()
        want = torch.zeros((len(src), store.ld_rows), dtype=torch.float16)
        want[:, :F] = feats[torch.from_numpy((1 - rank) * K + src)]
        ok = torch.equal(got[torch.from_numpy(pos)].view(torch.int16), want.view(torch.int16))
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


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "alltoall"])
def test_peer_rows_into_16bit_x0_bit_exact(direct):
    out = _spawn(_peer_rows_worker, extra=(direct,))
    assert len(out) == 2
    for rank, status, _, _ in out:
        assert status == "ok", f"rank {rank}: {status}"
