"""GPU: a keep16 feature store end to end — X0 staged in the table's 16-bit dtype by every route,
and training / evaluation from it through the native step (GNN_SL_XKIND: layer 0 aggregates from
the 16-bit rows) against the same table's widened X0.

The 16-bit aggregation is bit-identical to the fp32 one on the widened rows and everything after it
is the same code on the same values, so the comparisons are exact: equal losses, torch.equal
parameters, equal evaluation figures. Only the Python fall-back test has a tolerance, the one
tests/test_executor_gpu.py::test_executor_matches_python_step uses for the loss.
"""
import numpy as np
import pytest
import torch

from gnn_amd import loader, staging
from gnn_amd.models import build_model
from gnn_amd.train import Trainer

from test_feat16_gpu import DTYPES, IDS, ROUTES, _loader, _world

pytestmark = pytest.mark.gpu


def _i16(t):
    return t.contiguous().view(torch.int16)


def _table(N, F, dtype, seed):
    return (torch.randn(N, F, generator=torch.Generator().manual_seed(seed)) * 3).to(dtype)


# ------------------------------------------------------------------------------------------
# staging
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native_loader", [True, False], ids=["native_loader", "python_loader"])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("F", [30, 37])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stager_keeps_x0_16bit(dev, monkeypatch, dtype, F, route, native_loader):
    """X0 of a keep16 store: the table's dtype, feats[input_nodes] bit for bit in ld_rows-element
    rows with zero pads — by the one-call native stage, the Python sequence with the two-source
    gather, and the two-launch form; both loaders; own-buffer and host rows both in use."""
    monkeypatch.setattr(staging, "_NATIVE_STAGE", ROUTES[route][0])
    monkeypatch.setattr(staging, "_GATHER2", ROUTES[route][1])
    staged_natively = []
    real_stage = loader.NativeBatch.stage
    monkeypatch.setattr(loader.NativeBatch, "stage",
                        lambda self, *a, **k: (staged_natively.append(1), real_stage(self, *a, **k))[1])
    lap, labels, train, pl = _world()
    feats = _table(lap.shape[0], F, dtype, F)
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0, keep16=True)
    assert store.keep16 and store.ld_rows == 64
    ld = _loader(loader.NativeLoader if native_loader else loader.BatchLoader, store)
    try:
        stager = staging.Stager(store)
        n_host = n_own = 0
        for _, lb in zip(range(3), ld.epoch(1)):
            fn = (loader.ToDevice(lb.host, dev) if native_loader else
                  (lambda: lb.host.to_device(dev, with_coo=False)))
            staged = stager.issue(lb.plan, fn)
            x0 = staged.wait()
            torch.cuda.synchronize()
            assert x0.dtype == dtype and x0.shape[1] == F and x0.stride(0) == store.ld_rows
            nodes = torch.from_numpy(np.asarray(lb.host.input_nodes, np.int64))
            assert torch.equal(_i16(x0.cpu()), _i16(feats[nodes]))
            full = x0.as_strided((x0.shape[0], store.ld_rows), (store.ld_rows, 1))
            assert not bool(_i16(full[:, F:]).any())  # zero pads (+0: all bits clear)
            assert staged.batch is not None and len(staged.adjs) == 3
            n_host += len(lb.plan.host_pos)
            n_own += len(lb.plan.own_pos)
        assert n_host > 0 and n_own > 0
        assert bool(staged_natively) == (native_loader and route == "native")
    finally:
        ld.close()


# ------------------------------------------------------------------------------------------
# training and evaluation
# ------------------------------------------------------------------------------------------
def _train_eval(dev, feats, keep16, model, F, nhid=16, orders=(1, 1, 1), steps=3, prefetch=False, native=True):
    """`steps` Trainer.step calls and one Trainer.evaluate from a store of `feats`; returns
    (losses, parameters, evaluation dict, dtype of X0)."""
    lap, labels, train, pl = _world()
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0, keep16=keep16)
    ld = _loader(loader.NativeLoader, store, seed=4, device_extract=True)
    try:
        stager = staging.Stager(store)
        torch.manual_seed(0)
        net = build_model(model, F, nhid, list(orders), 7, dropout=0.1, fused=True).to(dev)
        tr = Trainer(net, 0.01, dev)
        assert (tr.executor is not None) == native
        losses, x0_dtype = [], None
        for it, lb in zip(range(steps), ld.epoch(1)):
            staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
            x0 = staged.wait()
            db = staged.batch
            x0_dtype = x0.dtype
            if native:
                assert tr.executor.supports(x0, staged.adjs, db.sampled_nodes, db.labels)
            torch.manual_seed(100 + it)
            if prefetch:
                tr.executor.prefetch(x0, staged.adjs, db.sampled_nodes, db.labels)
                assert tr.executor._pre is not None
            losses.append(float(tr.step(x0, staged.adjs, db.sampled_nodes, db.labels)))
            if native:
                assert tr.executor._pre is None
        torch.cuda.synchronize()
    finally:
        ld.close()
    ld = _loader(loader.NativeLoader, store, seed=4, device_extract=True)  # a loader with nothing in flight
    try:
        def eval_batches():
            for lb in ld.sequential(train[:200], 128):
                staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
                x0 = staged.wait()
                if native:
                    assert tr.executor.supports(x0, staged.adjs, staged.batch.sampled_nodes, staged.batch.labels,
                                                inference=True)
                yield x0, staged.adjs, staged.batch.sampled_nodes, staged.batch.labels

        ev = tr.evaluate(eval_batches())
        assert ev["batches"] == 2 and ev["rows"] == 200
    finally:
        ld.close()
    return losses, [p.detach().clone() for p in net.parameters()], ev, x0_dtype


def _same(a, b):
    (la, pa, ea, _), (lb, pb, eb, _) = a, b
    assert la == lb and all(np.isfinite(la)), (la, lb)
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(x, y), ("parameter differs", i)
    assert ea.keys() == eb.keys()
    for k in ea:  # an undefined F1 is NaN on both sides
        assert ea[k] == eb[k] or (ea[k] != ea[k] and eb[k] != eb[k]), k


@pytest.mark.parametrize("model", ["graphsage", "gcn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_training_and_evaluation_parity_with_widened_x0(dev, dtype, model):
    """Three steps + an evaluation pass from a keep16 store == the same from the same table without
    keep16 (X0 widened by the gathers): losses, every parameter, the evaluation dict."""
    F = 30
    feats = _table(_world()[0].shape[0], F, dtype, 3)
    kept = _train_eval(dev, feats, True, model, F)
    wide = _train_eval(dev, feats, False, model, F)
    assert kept[3] == dtype and wide[3] == torch.float32
    _same(kept, wide)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_prefetch_then_step_equals_plain_step(dev, dtype):
    """prefetch + step (phases 1 + 2: the 16-bit layer-0 aggregation issued ahead) == the plain step."""
    F = 37
    feats = _table(_world()[0].shape[0], F, dtype, 8)
    _same(_train_eval(dev, feats, True, "graphsage", F, prefetch=True), _train_eval(dev, feats, True, "graphsage", F))


def test_python_fallback_runs_from_keep16_store(dev, monkeypatch):
    """GNN_NATIVE_STEP=0: the autograd path takes the 16-bit X0 (the aggregation as it is,
    x[sampled] widened). Its first loss against the native step's within
    test_executor_matches_python_step's bound: |a - b| <= 1e-6 |a| + 1e-7."""
    F = 30
    feats = _table(_world()[0].shape[0], F, torch.float16, 3)
    native = _train_eval(dev, feats, True, "graphsage", F, steps=1)
    monkeypatch.setenv("GNN_NATIVE_STEP", "0")
    python = _train_eval(dev, feats, True, "graphsage", F, steps=1, native=False)
    assert python[3] == torch.float16
    a, b = python[0][0], native[0][0]
    assert np.isfinite(a) and abs(a - b) <= 1e-6 * abs(a) + 1e-7, (a, b)


# ------------------------------------------------------------------------------------------
# against the in-place row-indexed GEMM route of the fp32 step
# ------------------------------------------------------------------------------------------
def _big_step(dev, feats, keep16, F, nhid):
    """One GraphSAGE step whose layer 0 has >= 2048 rows (two layers, samp 2304)."""
    lap, labels, train, pl = _world(N=12000)
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0, keep16=keep16)
    ld = loader.NativeLoader(lap, labels, train, 2304, 512, [1, 1], pl.device_id_of_nodes_group[0],
                             pl.idx_of_nodes_on_device_group[0], rank=0, world_size=1, store=store, workers=2, seed=6,
                             device_extract=True)
    try:
        stager = staging.Stager(store)
        torch.manual_seed(0)
        net = build_model("graphsage", F, nhid, [1, 1], 7, dropout=0.1, fused=True).to(dev)
        tr = Trainer(net, 0.01, dev)
        lb = next(iter(ld.epoch(1)))
        staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
        x0 = staged.wait()
        db = staged.batch
        assert tr.executor.supports(x0, staged.adjs, db.sampled_nodes, db.labels)
        M0 = staged.adjs[0].shape[0]
        torch.manual_seed(100)
        loss = float(tr.step(x0, staged.adjs, db.sampled_nodes, db.labels))
        grads = [p.grad.detach().clone() for p in tr.params]
        torch.cuda.synchronize()
    finally:
        ld.close()
    return loss, grads, M0, x0


def test_parity_with_the_indexed_gemm_route(dev, monkeypatch):
    """A layer 0 the fp32 step runs through the row-indexed split3 GEMMs (x[sampled] read in place):
    M >= 2048 rows, ceil(M / 128) * ceil(nhid / 128) * 2 >= 256 tiles, an even F whose padded rows
    keep X0's stride (F = 30 in 32-float rows: the aggregation output has the stride of X0). The
    keep16 step always gathers x[sampled] (widening); it equals the widened step with the indexed
    route (GNN_STEP_GATHER unset) and with the gathered route (GNN_STEP_GATHER=1), bit for bit."""
    F, nhid = 30, 1024
    monkeypatch.delenv("GNN_STEP_GATHER", raising=False)
    monkeypatch.delenv("GNN_GEMM_ALGO", raising=False)
    feats = _table(12000, F, torch.float16, 12)
    kept = _big_step(dev, feats, True, F, nhid)
    indexed = _big_step(dev, feats, False, F, nhid)
    monkeypatch.setenv("GNN_STEP_GATHER", "1")
    gathered = _big_step(dev, feats, False, F, nhid)
    M0, x32 = indexed[2], indexed[3]
    assert M0 >= 2048 and -(-M0 // 128) * (nhid // 128) * 2 >= 256
    assert x32.dtype == torch.float32 and x32.stride(0) == 32 and kept[3].dtype == torch.float16
    for name, other in (("GNN_STEP_GATHER=1", gathered), ("indexed", indexed)):
        assert kept[0] == other[0], (name, kept[0], other[0])
        for i, (a, b) in enumerate(zip(kept[1], other[1])):
            assert torch.equal(a, b), (name, "gradient differs", i)
