"""GPU: the softmax cross-entropy loss through the native step executor (GNN_SH_LOSS_KIND,
include/gnn_step.h), NativeStep / Trainer / Evaluator with sigmoid_loss=False.

The executor and the Python fused path (GNN.forward_loss -> gnn_amd.fused.head_ce_loss) run the
same kernels with the same seeds: compared within the tolerances of tests/test_executor_gpu.py
(loss 1e-6 |loss| + 1e-7, gradients and parameters 1e-5 in relative L2: the vendor GEMM calls may
round differently from torch.mm's). The evaluation step's loss is compared bit for bit with the
training entry point in eval() mode, and its logits and counts with a BCE-kind evaluation (the
loss kind changes nothing else). The three small specs of tests/test_eval_gpu.py: the vendor-GEMM
routes (tiny GCN), 172 classes, and the split3 / row-indexed routes (30k nodes).
"""
import numpy as np
import pytest
import torch

from gnn_amd import _lib, graphs, metrics, sampler, staging
from gnn_amd import executor as E
from gnn_amd.models import build_model, loss as loss_fn
from gnn_amd.train import Evaluator, Trainer

pytestmark = pytest.mark.gpu

_cache = {}
SPECS = {
    # name: (graph spec, dataset seed, model, nhid, samp, batch)
    "tiny_gcn": (graphs.TINY, 1, "gcn", 128, 600, 64),
    "tiny_sage_172": (graphs.GraphSpec("tiny172", 3000, 15000, 128, 172, 0.66, 0.1), 2, "graphsage", 512, 600, 64),
    "mid_sage": (graphs.GraphSpec("mid30k", 30000, 450000, 100, 47, 0.66, 0.1), 3, "graphsage", 512, 4200, 256),
}
NAMES = ["tiny_gcn", "tiny_sage_172", "mid_sage"]


def _graph(name):
    key = ("graph", name)
    if key not in _cache:
        spec, seed, model, *_ = SPECS[name]
        A, labels, feats, ncls, train, *_ = graphs.make_dataset(spec, seed=seed)
        _cache[key] = (A.shape[0], graphs.lap_matrix(A, model), labels, feats, ncls, train)
    return _cache[key]


def _batch(name, dev, bs=None, which=0):
    """(x0, adjs, sampled_nodes, labels), F, classes"""
    key = ("batch", name, bs, which)
    if key not in _cache:
        _, _, model, nhid, samp, bs0 = SPECS[name]
        N, lap, labels, feats, ncls, train = _graph(name)
        nodes = sampler.rank_batches(train, bs or bs0, 0, 1, 1)[which]
        hb = sampler.ladies_sample_host(3 + which, nodes, np.array([samp] * 5), N, lap, labels, [1, 1, 1],
                                        np.full(N, -1), np.zeros(N, np.int64), None, 1.0, [0], device_extract=True)
        db = hb.to_device(dev, with_coo=False)
        F = feats.shape[1]
        x = torch.zeros((hb.num_input_nodes, staging.padded_ld(F)), dtype=torch.float32)
        x[:, :F] = feats[torch.from_numpy(np.asarray(hb.input_nodes, np.int64))]
        _cache[key] = ((x.to(dev)[:, :F], db.adjs, db.sampled_nodes, db.labels), F, ncls)
    return _cache[key]


def _trainer(name, dev, sigmoid_loss=False, native=True):
    _, _, model, nhid, *_ = SPECS[name]
    _, F, ncls = _batch(name, dev)
    torch.manual_seed(0)
    m = build_model(model, F, nhid, [1, 1, 1], ncls, 0.1, fused=True).to(dev)
    tr = Trainer(m, 0.01, dev, sigmoid_loss=sigmoid_loss)
    assert tr.executor is not None
    assert tr.executor.template[E.H_LOSS_KIND] == (0 if sigmoid_loss else 1)
    if not native:
        tr.executor = None
    return tr


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@pytest.mark.parametrize("name", NAMES)
def test_ce_native_step_matches_python_fused_path(dev, name):
    args, _, _ = _batch(name, dev)
    assert bool(torch.all(args[3].sum(1) == 1))  # one class per node: one-hot label rows
    ta = _trainer(name, dev, native=False)  # forward_loss (head_ce_loss) + autograd
    tb = _trainer(name, dev)
    assert tb.executor.supports(*args)
    for it in range(2):
        torch.manual_seed(100 + it)
        la = ta.step(*args)
        ga = [p.grad.detach().clone() for p in ta.params]
        torch.manual_seed(100 + it)
        lb = tb.step(*args)
        gb = [p.grad.detach().clone() for p in tb.params]
        torch.cuda.synchronize()
        print(name, it, float(la), float(lb), max(_rel(x, y) for x, y in zip(gb, ga)))
        assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(la)) + 1e-7, (it, float(la), float(lb))
        for i, (x, y) in enumerate(zip(gb, ga)):
            assert _rel(x, y) <= 1e-5, (it, i, _rel(x, y))
    for p, q in zip(tb.params, ta.params):
        assert _rel(p.detach(), q.detach()) <= 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_ce_is_in_force_and_the_evaluation_loss_is_the_step_loss(dev, name):
    args, _, ncls = _batch(name, dev)
    ce, bce = _trainer(name, dev), _trainer(name, dev, sigmoid_loss=True)  # the same initial parameters
    ex, net = ce.executor, ce.model
    net.eval()
    bce.model.eval()
    l_ce = ex.step(*args).clone()  # the training entry point with training = 0
    l_bce = bce.executor.step(*args).clone()
    with torch.no_grad():
        ref = loss_fn(net(*args[:3]), args[3], False, dev)
    torch.cuda.synchronize()
    assert float(l_ce) != float(l_bce)
    torch.testing.assert_close(l_ce, ref, rtol=1e-5, atol=0.0)
    net.train()  # evaluate() never drops out, whatever the model's mode
    loss, counts, logits = ex.evaluate(*args, mode=1, want_logits=True)
    loss_b, counts_b, logits_b = ex.evaluate(*args, mode=1, want_logits=True, sigmoid_loss=True)
    torch.cuda.synchronize()
    assert torch.equal(loss, l_ce), (float(loss), float(l_ce))
    assert torch.equal(logits, logits_b) and torch.equal(counts, counts_b)
    assert torch.equal(loss_b, l_bce)  # mode 1 under the BCE kind: still the BCE loss, bit for bit
    assert int(counts[0].sum() + counts[2].sum()) == args[3].shape[0]  # one true class per row
    # mode is independent of the kind
    loss0, counts0, _ = ex.evaluate(*args, mode=0)
    assert torch.equal(loss0, l_ce) and torch.equal(counts0, bce.executor.evaluate(*args, mode=0)[1])


def test_trainer_evaluate_with_ce_stays_native_over_three_batches(dev):
    name = "tiny_gcn"
    data = [_batch(name, dev, bs=bs, which=w)[0] for bs, w in ((64, 0), (40, 1), (17, 2))]
    assert [d[3].shape[0] for d in data] == [64, 40, 17]
    tr = _trainer(name, dev)
    ev = Evaluator(tr.model, dev, sigmoid_loss=False, executor=tr.executor)
    assert ev.mode == 1
    for d in data:
        ev.add(*d)
    assert ev.native_batches == 3
    res = tr.evaluate(iter(data))
    assert res == ev.result() and res["batches"] == 3 and res["rows"] == 121
    fb = Evaluator(tr.model, dev, sigmoid_loss=False, executor=None)  # model.forward_loss under no_grad
    for d in data:
        fb.add(*d)
    assert fb.native_batches == 0
    ref = fb.result()
    print(res["loss"], ref["loss"])
    assert abs(res["loss"] - ref["loss"]) <= 1e-6 * abs(ref["loss"])
    c = np.sum([tr.executor.evaluate(*d, mode=1)[1].cpu().numpy().astype(np.int64) for d in data], axis=0)
    assert (res["micro_f1"], res["macro_f1"]) == metrics.f1_from_counts(c[0], c[1], c[2], 1)


@pytest.mark.parametrize("name", NAMES)
def test_ce_prefetch_then_step_is_bit_identical(dev, name):
    args, _, _ = _batch(name, dev)
    tr = _trainer(name, dev)
    ex = tr.executor
    tr.model.train()
    torch.manual_seed(7)
    l0, g0 = ex.step(*args).clone(), ex.flat_grad.clone()
    torch.manual_seed(7)
    ex.prefetch(*args)  # phase 1
    l1, g1 = ex.step(*args).clone(), ex.flat_grad.clone()  # phase 2
    torch.cuda.synchronize()
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and float(g0.abs().sum()) > 0


def test_unknown_loss_kind_is_refused_before_any_launch(dev):
    args, _, ncls = _batch("tiny_gcn", dev)
    ex = _trainer("tiny_gcn", dev).executor
    L, st = _lib.lib(), _lib.stream_of(dev)
    d = ex._desc(*args, seeds=False)
    loss = torch.full((), -7.0, device=dev)
    counts = torch.full((3, ncls), -7, dtype=torch.int32, device=dev)
    d[E.H_LOSS] = loss.data_ptr()
    need = L.gnn_train_step_workspace_bytes(d.ctypes.data)
    assert 0 < L.gnn_eval_step_workspace_bytes(d.ctypes.data) < need
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ex.flat_grad.fill_(-7.0)
    for kind in (2, -1):
        d[E.H_LOSS_KIND] = kind
        assert L.gnn_train_step_workspace_bytes(d.ctypes.data) == 0 and b"loss kind" in L.gnn_last_error()
        assert L.gnn_eval_step_workspace_bytes(d.ctypes.data) == 0 and b"loss kind" in L.gnn_last_error()
        assert L.gnn_train_step_f32(d.ctypes.data, ws.data_ptr(), need, st) != 0 and b"loss kind" in L.gnn_last_error()
        assert L.gnn_eval_step_f32(d.ctypes.data, None, 0, counts.data_ptr(), 1, ws.data_ptr(), need, st) != 0
        assert b"loss kind" in L.gnn_last_error()
    torch.cuda.synchronize()
    assert float(loss) == -7.0 and torch.all(counts == -7) and torch.all(ex.flat_grad == -7.0)
