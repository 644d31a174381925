"""Native evaluation on the GPU: the fused evaluation head (gnn_head_eval_f32), the forward-only
executor call (gnn_eval_step_f32, NativeStep.evaluate) and Trainer.evaluate.

The head runs the training head's dot products in the same order, so its logits and loss are
compared BIT FOR BIT with gnn_head_bce_fwd_f32(training=0); its per-class counts are integers and
are compared exactly with numpy on the logits it returned. The step is compared bit for bit with
the training step's loss in eval() mode (same kernels, same routing) and with the Python fused
path within the tolerances of tests/test_executor_gpu.py (logits 1e-5 in relative L2, loss
1e-6 |loss| + 1e-7: the vendor GEMM calls may round differently from torch.mm's).
"""
import numpy as np
import pytest
import torch

from gnn_amd import _lib, graphs, metrics, sampler, staging
from gnn_amd import executor as E
from gnn_amd.custom_sparse_ops import CsrOperand
from gnn_amd.models import build_model
from gnn_amd.train import Evaluator, Trainer

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ kernel level
def _np_counts(z, y, mode):
    """utils.calc_f1's predictions (utils.py:142-149) as per-class tp / fp / fn, in numpy."""
    C = z.shape[1]
    if mode == 0:
        pred, true = z > 0, y > 0.5
    else:
        pred = np.argmax(z, axis=1)[:, None] == np.arange(C)  # np.argmax: the first index wins
        true = np.argmax(y, axis=1)[:, None] == np.arange(C)
    return np.stack([(pred & true).sum(0), (pred & ~true).sum(0), (true & ~pred).sum(0)]).astype(np.int32)


def _head_inputs(M, D, C, dev, seed, zero_row=True):
    g = torch.Generator().manual_seed(seed)
    ldx, ldl = D + 4, C + 3
    xs = torch.randn(max(M, 1), ldx, generator=g)
    if zero_row and M >= 3:
        xs[1] = 0.0  # an all-zero input row: norm 0, the logits are the bias
    W = torch.randn(C, D, generator=g)  # unit-norm rows of x: logits ~ N(0, 1) + bias
    b = torch.randn(C, generator=g) * 0.5
    ys = (torch.rand(max(M, 1), ldl, generator=g) < 0.3).float()
    return xs.to(dev), ldx, W.to(dev), b.to(dev), ys.to(dev), ldl


def _run_train_head(x, ldx, M, D, W, b, C, y, ldl, dev):
    xd, z = torch.empty(max(M, 1), D, device=dev), torch.empty(max(M, 1), C, device=dev)
    nrm, rl, lo = torch.empty(max(M, 1), device=dev), torch.empty(max(M, 1), device=dev), torch.empty((), device=dev)
    L = _lib.lib()
    _lib.check(L.gnn_head_bce_fwd_f32(x.data_ptr(), ldx, M, D, W.data_ptr(), b.data_ptr(), C, y.data_ptr(), ldl, 0.1,
                                      99, 0, xd.data_ptr(), z.data_ptr(), nrm.data_ptr(), rl.data_ptr(), lo.data_ptr(),
                                      _lib.stream_of(dev)), "gnn_head_bce_fwd_f32")
    return z[:M], lo


def _run_eval_head(x, ldx, M, D, W, b, C, y, ldl, mode, dev, ldz=None, scored=True):
    ldz = C + 5 if ldz is None else ldz
    z = torch.full((max(M, 1), ldz), -7.0, device=dev)
    rl = torch.empty(max(M, 1), device=dev)
    rm = torch.empty(max(M, 1) * 8, dtype=torch.int64, device=dev)
    lo = torch.full((), -7.0, device=dev)
    counts = torch.full((3, C), -7, dtype=torch.int32, device=dev)
    L = _lib.lib()
    rc = L.gnn_head_eval_f32(x.data_ptr(), ldx, M, D, W.data_ptr(), b.data_ptr(), C, y.data_ptr() if scored else None,
                             ldl, z.data_ptr(), ldz, rl.data_ptr(), rm.data_ptr(), lo.data_ptr(), counts.data_ptr(),
                             mode, _lib.stream_of(dev))
    return rc, z, lo, counts


@pytest.mark.parametrize("C", [1, 7, 8, 9, 64, 65, 172, 256])
@pytest.mark.parametrize("D", [4, 1024, 1028, 2048])
def test_head_eval_matches_training_head_and_numpy(dev, D, C):
    """Every (D, C) of the list — both PV instantiations, the masked last piece (1028), the
    8-class block edge and the 64-lane slot edges — at M = 1, 3, 130, padded row strides, one
    all-zero row: logits and loss bit-equal to the training head with training = 0, counts equal
    to numpy on the downloaded logits in both modes."""
    for M in (1, 3, 130):
        x, ldx, W, b, y, ldl = _head_inputs(M, D, C, dev, 1000 * D + 10 * C + M)
        z_ref, lo_ref = _run_train_head(x, ldx, M, D, W, b, C, y, ldl, dev)
        for mode in (0, 1):
            rc, z, lo, counts = _run_eval_head(x, ldx, M, D, W, b, C, y, ldl, mode, dev)
            assert rc == 0, _lib.lib().gnn_last_error()
            torch.cuda.synchronize()
            assert torch.equal(z[:M, :C], z_ref), (M, mode, "logits differ from gnn_head_bce_fwd_f32")
            assert torch.all(z[:M, C:] == -7.0)  # nothing past a row's C logits
            assert torch.equal(lo, lo_ref), (M, mode, float(lo), float(lo_ref))
            want = _np_counts(z[:M, :C].cpu().numpy(), y[:M, :C].cpu().numpy(), mode)
            assert np.array_equal(counts.cpu().numpy(), want), (M, mode)
        if M >= 3:
            assert torch.equal(z[1, :C], b)  # the all-zero row


def test_head_eval_argmax_ties_take_the_first_index(dev):
    M, D, C = 130, 1024, 41
    x, ldx, W, b, y, ldl = _head_inputs(M, D, C, dev, 5, zero_row=False)
    W[5] = W[2]  # identical rows of W: identical dot products, so exactly tied logits
    b[2] = b[5] = 10.0  # ... and the row maximum
    rc, z, lo, counts = _run_eval_head(x, ldx, M, D, W, b, C, y, ldl, 1, dev)
    assert rc == 0
    zc, yc = z[:M, :C].cpu().numpy(), y[:M, :C].cpu().numpy()
    assert np.array_equal(zc[:, 2], zc[:, 5]) and np.all(zc.max(axis=1) == zc[:, 2])
    c = counts.cpu().numpy()
    assert np.array_equal(c, _np_counts(zc, yc, 1))
    assert c[0, 2] + c[1, 2] == M and c[0, 5] + c[1, 5] == 0  # every row predicts class 2, none class 5
    assert int((c[0] + c[2]).sum()) == M and int(c[1].sum()) == int(c[2].sum())


def test_head_eval_predict_touches_neither_loss_nor_counts(dev):
    M, D, C = 130, 1028, 65
    x, ldx, W, b, y, ldl = _head_inputs(M, D, C, dev, 6)
    z_ref, _ = _run_train_head(x, ldx, M, D, W, b, C, y, ldl, dev)
    rc, z, lo, counts = _run_eval_head(x, ldx, M, D, W, b, C, y, ldl, 0, dev, scored=False)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(z[:M, :C], z_ref)
    assert float(lo) == -7.0 and torch.all(counts == -7)


def test_head_eval_empty_batch_and_validation(dev):
    x, ldx, W, b, y, ldl = _head_inputs(3, 1024, 9, dev, 7)
    rc, z, lo, counts = _run_eval_head(x, ldx, 0, 1024, W, b, 9, y, ldl, 0, dev)
    assert rc == 0 and float(lo) == 0.0 and torch.all(counts == 0) and torch.all(z == -7.0)
    # a bad D or C returns a status and launches nothing: every output keeps its fill (the buffers
    # are sized for the largest of these shapes all the same)
    x, W = torch.zeros(3, 2056, device=dev), torch.zeros(300 * 2056, device=dev)
    b, y = torch.zeros(300, device=dev), torch.zeros(3, 300, device=dev)
    L = _lib.lib()
    for D, C in ((1022, 9), (2052, 9), (1024, 257), (1024, 0)):
        z = torch.full((3, 300), -7.0, device=dev)
        rl = torch.empty(3, device=dev)
        rm = torch.empty(24, dtype=torch.int64, device=dev)
        lo = torch.full((), -7.0, device=dev)
        counts = torch.full((3, 300), -7, dtype=torch.int32, device=dev)
        rc = L.gnn_head_eval_f32(x.data_ptr(), 2056, 3, D, W.data_ptr(), b.data_ptr(), C, y.data_ptr(), 300,
                                 z.data_ptr(), 300, rl.data_ptr(), rm.data_ptr(), lo.data_ptr(), counts.data_ptr(), 0,
                                 _lib.stream_of(dev))
        assert rc != 0 and L.gnn_last_error(), (D, C)
        torch.cuda.synchronize()
        assert float(lo) == -7.0 and torch.all(counts == -7) and torch.all(z == -7.0), (D, C)


# -------------------------------------------------------------------------------- step level
_cache = {}
SPECS = {
    # name: (graph spec, dataset seed, model, nhid, samp, batch)
    "tiny_gcn": (graphs.TINY, 1, "gcn", 128, 600, 64),  # the vendor-GEMM routes
    "tiny_sage_172": (graphs.GraphSpec("tiny172", 3000, 15000, 128, 172, 0.66, 0.1), 2, "graphsage", 512, 600, 64),
    # layers 0 and 1 with M >= 4096 at nhid 512: the split3 and the row-indexed routes
    "mid_sage": (graphs.GraphSpec("mid30k", 30000, 450000, 100, 47, 0.66, 0.1), 3, "graphsage", 512, 4200, 256),
}


def _graph(name):
    key = ("graph", name)
    if key not in _cache:
        spec, seed, model, *_ = SPECS[name]
        A, labels, feats, ncls, train, *_ = graphs.make_dataset(spec, seed=seed)
        _cache[key] = (A.shape[0], graphs.lap_matrix(A, model), labels, feats, ncls, train)
    return _cache[key]


def _batch(name, dev, bs=None, which=0):
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
        _cache[key] = (model, nhid, F, ncls, db, x.to(dev)[:, :F])
    return _cache[key]


def _trainer(name, dev):
    _, _, model, nhid, *_ = SPECS[name]
    _, _, F, ncls, _, _ = _batch(name, dev)
    torch.manual_seed(0)
    m = build_model(model, F, nhid, [1, 1, 1], ncls, 0.1, fused=True).to(dev)
    tr = Trainer(m, 0.01, dev)
    assert tr.executor is not None
    return tr


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _descriptor(ex, x0, db, forward_only):
    return ex._desc(x0, db.adjs, db.sampled_nodes, db.labels, seeds=False, forward_only=forward_only)


@pytest.mark.parametrize("name", ["tiny_gcn", "tiny_sage_172", "mid_sage"])
def test_eval_step_matches_training_forward_and_python_path(dev, name):
    model, nhid, F, ncls, db, x0 = _batch(name, dev)
    if name == "mid_sage":
        for op in db.adjs[:2]:  # split3 fills the chip: ceil(M / 128) * (512 / 128) * 2 products
            assert op.shape[0] >= 4096 and -(-op.shape[0] // 128) * 4 * 2 >= 256
    tr = _trainer(name, dev)
    ex, net = tr.executor, tr.model
    args = (x0, db.adjs, db.sampled_nodes, db.labels)
    assert ex.supports(*args) and ex.supports(*args, inference=True)
    net.eval()
    loss_step = ex.step(*args).clone()  # the training entry point with training = 0
    with torch.no_grad():
        loss_py, out_py = net.forward_loss(*args)
    net.train()  # evaluate() never drops out, whatever the model's mode
    L = _lib.lib()
    for mode in (0, 1):
        loss, counts, logits = ex.evaluate(*args, mode=mode, want_logits=True)
        assert loss.is_cuda and counts.is_cuda and logits.is_cuda
        torch.cuda.synchronize()
        assert torch.equal(loss, loss_step), (mode, float(loss), float(loss_step))
        assert logits.shape == out_py.shape and _rel(logits, out_py) <= 1e-5, _rel(logits, out_py)
        assert abs(float(loss) - float(loss_py)) <= 1e-6 * abs(float(loss_py)) + 1e-7
        assert np.array_equal(counts.cpu().numpy(), _np_counts(logits.cpu().numpy(), db.labels.cpu().numpy(), mode))
        assert ex.evaluate(*args, mode=mode)[2] is None
    # predict: logits only, the same bits
    lo, cn, z = ex.evaluate(x0, db.adjs, db.sampled_nodes)
    assert lo is None and cn is None and torch.equal(z, logits)
    # no backward buffer in the evaluation plan
    d = _descriptor(ex, x0, db, forward_only=False)
    ev_bytes, tr_bytes = L.gnn_eval_step_workspace_bytes(d.ctypes.data), L.gnn_train_step_workspace_bytes(d.ctypes.data)
    assert 0 < ev_bytes < tr_bytes, (ev_bytes, tr_bytes)
    # a batch without transposes or row maps: refused for training, taken for evaluation
    bare = [CsrOperand(op.rowptr, op.col, op.val, op.shape) for op in db.adjs]
    sn = [s.clone() for s in db.sampled_nodes]
    assert not ex.supports(x0, bare, sn, db.labels) and ex.supports(x0, bare, sn, db.labels, inference=True)
    d = ex._desc(x0, bare, sn, db.labels, seeds=False, forward_only=True)
    for li in range(3):
        base = E.HEADER + li * E.LAYER_SLOTS
        assert d[base + E.L_TROWPTR] == 0 and d[base + E.L_RMAP] == 0
    loss2, counts2, logits2 = ex.evaluate(x0, bare, sn, db.labels, mode=1, want_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(loss2, loss_step) and torch.equal(counts2, counts) and torch.equal(logits2, logits)


def test_eval_step_validates_before_launching(dev):
    model, nhid, F, ncls, db, x0 = _batch("tiny_gcn", dev)
    ex = _trainer("tiny_gcn", dev).executor
    L = _lib.lib()
    d = _descriptor(ex, x0, db, forward_only=True)
    loss = torch.full((), -7.0, device=dev)
    counts = torch.full((3, ncls), -7, dtype=torch.int32, device=dev)
    d[E.H_LOSS] = loss.data_ptr()
    need = L.gnn_eval_step_workspace_bytes(d.ctypes.data)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    st = _lib.stream_of(dev)
    assert L.gnn_eval_step_f32(d.ctypes.data, None, 0, counts.data_ptr(), 0, ws.data_ptr(), need - 1, st) != 0
    assert b"too small" in L.gnn_last_error()
    assert L.gnn_eval_step_f32(d.ctypes.data, None, 0, counts.data_ptr(), 0, ws.data_ptr() + 64, need, st) != 0
    assert b"aligned" in L.gnn_last_error()
    assert L.gnn_eval_step_f32(d.ctypes.data, None, 0, counts.data_ptr(), 2, ws.data_ptr(), need, st) != 0
    d2 = d.copy()
    d2[E.H_PHASE] = 1
    assert L.gnn_eval_step_f32(d2.ctypes.data, None, 0, counts.data_ptr(), 0, ws.data_ptr(), need, st) != 0
    assert b"phase" in L.gnn_last_error()
    torch.cuda.synchronize()
    assert float(loss) == -7.0 and torch.all(counts == -7)
    assert L.gnn_eval_step_f32(d.ctypes.data, None, 0, counts.data_ptr(), 0, ws.data_ptr(), need, st) == 0
    torch.cuda.synchronize()
    assert float(loss) > 0 and torch.all(counts >= 0)


@pytest.mark.parametrize("name", ["tiny_sage_172", "mid_sage"])
def test_training_is_bit_identical_around_an_evaluation(dev, name):
    """The evaluation shares the aux stream and the vendor-GEMM handles with the training step: a
    training step before and after an evaluation gives the loss and gradients of two training
    steps with no evaluation between them, bit for bit."""
    model, nhid, F, ncls, db, x0 = _batch(name, dev)
    args = (x0, db.adjs, db.sampled_nodes, db.labels)
    res = []
    for with_eval in (False, True):
        tr = _trainer(name, dev)
        out = []
        for it in range(2):
            torch.manual_seed(100 + it)
            out.append((tr.step(*args).clone(), [p.grad.detach().clone() for p in tr.params]))
            if with_eval and it == 0:
                tr.executor.evaluate(*args, mode=0, want_logits=True)
                assert tr.model.training
        torch.cuda.synchronize()
        res.append(out)
    for (la, ga), (lb, gb) in zip(*res):
        assert torch.equal(la, lb)
        for i, (x, y) in enumerate(zip(ga, gb)):
            assert torch.equal(x, y), ("gradient differs", i)


def test_trainer_evaluate_pools_three_batches(dev):
    name = "tiny_gcn"
    batches = [_batch(name, dev, bs=bs, which=w) for bs, w in ((64, 0), (40, 1), (17, 2))]
    data = [(b[5], b[4].adjs, b[4].sampled_nodes, b[4].labels) for b in batches]
    assert [d[3].shape[0] for d in data] == [64, 40, 17]
    tr = _trainer(name, dev)
    tr.model.train()
    res = tr.evaluate(iter(data))
    assert tr.model.training and res["batches"] == 3 and res["rows"] == 121
    # by hand: each batch through the executor, pooled on the host
    per = [tr.executor.evaluate(*d, mode=0) for d in data]
    torch.cuda.synchronize()
    counts = np.sum([c.cpu().numpy().astype(np.int64) for _, c, _ in per], axis=0)
    micro, macro = metrics.f1_from_counts(counts[0], counts[1], counts[2], 0)
    assert res["micro_f1"] == micro and res["macro_f1"] == macro
    rows = [64.0, 40.0, 17.0]
    assert res["loss"] == sum(float(l.double()) * r for (l, _, _), r in zip(per, rows)) / 121.0
    mb = [metrics.f1_from_counts(*c.cpu().numpy(), 0)[0] for _, c, _ in per]
    assert res["ref_batch_weighted_micro_f1"] == sum(m * r for m, r in zip(mb, rows)) / 121.0
    # mode 1 on request; one host copy: add() hands back device tensors and synchronises nothing
    res1 = tr.evaluate(data, mode=1)
    c1 = np.sum([tr.executor.evaluate(*d, mode=1)[1].cpu().numpy().astype(np.int64) for d in data], axis=0)
    assert (res1["micro_f1"], res1["macro_f1"]) == metrics.f1_from_counts(c1[0], c1[1], c1[2], 1)
    ev = Evaluator(tr.model, dev, executor=tr.executor)
    for d in data:
        loss, cn = ev.add(*d)
        assert loss.is_cuda and cn.is_cuda and cn.dtype == torch.int32
    assert ev.native_batches == 3 and ev._buf.is_cuda
    assert ev.result() == res
    assert torch.equal(ev.predict(*data[2][:3]), tr.executor.evaluate(*data[2], want_logits=True)[2])
