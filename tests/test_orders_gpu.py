"""Order-0 (dense) layers in the native step (GNN_SL_DENSE, include/gnn_step.h): models built with
the reference's ``--orders`` holding zeros (main.py:41, models.py:17-21, 59-60) train and evaluate
through gnn_train_step_f32 / gnn_eval_step_f32, against the Python fused path, the reference's CPU
path, their own schedule variants (bit for bit), and end to end from the native loader and staging.

Graphs: *small* = graphs.TINY (samp 600, batch 64, nhid 128: the vendor-GEMM routes) and *mid* =
40 k nodes, 100 features (samp 8192, batch 512, nhid 512: the order-0 layers run over > 8 k rows, so
they take the split3 routes — asserted below, so that a change of the generator cannot move the
case onto the vendor GEMM unnoticed).
"""
import numpy as np
import pytest
import torch

from gnn_amd import _lib, graphs, loader, metrics, placement, sampler, staging
from gnn_amd import executor as E
from gnn_amd.models import build_model
from gnn_amd.models import loss as loss_fn
from gnn_amd.train import Evaluator, Trainer

pytestmark = pytest.mark.gpu

MID = graphs.GraphSpec("mid", 40_000, 1_600_000, 100, 41, 0.66, 0.1)
# name: (graph spec, dataset seed, samp, batch, nhid)
GRAPHS = {"small": (graphs.TINY, 1, 600, 64, 128), "mid": (MID, 3, 8192, 512, 512)}
_cache = {}


def _graph(name, model):
    key = ("graph", name, model)
    if key not in _cache:
        for k in [k for k in _cache if k[0] == "graph" and k[1] != name]:
            del _cache[k]  # one graph's tables at a time
        spec, seed, *_ = GRAPHS[name]
        A, labels, feats, ncls, train, *_ = graphs.make_dataset(spec, seed=seed)
        _cache[key] = (A.shape[0], graphs.lap_matrix(A, model), labels, feats, ncls, train)
    return _cache[key]


def _host_batch(name, model, orders, which=0, bs=None, device_extract=True):
    _, _, samp, bs0, _ = GRAPHS[name]
    N, lap, labels, feats, ncls, train = _graph(name, model)
    nodes = sampler.rank_batches(train, bs or bs0, 0, 1, 1)[which]
    return sampler.ladies_sample_host(3 + which, nodes, np.array([samp] * 5), N, lap, labels, list(orders),
                                      np.full(N, -1), np.zeros(N, np.int64), None, 1.0, [0],
                                      device_extract=device_extract)


def _x0(hb, feats, dev):
    F = feats.shape[1]
    x = torch.zeros((hb.num_input_nodes, staging.padded_ld(F)), dtype=torch.float32)
    x[:, :F] = feats[torch.from_numpy(np.asarray(hb.input_nodes, np.int64))]
    return x.to(dev)[:, :F]


def _batch(name, model, orders, dev, which=0, bs=None):
    """(F, classes, DeviceBatch, x0) of one sampled batch; computed once and left unchanged."""
    key = ("batch", name, model, tuple(orders), which, bs)
    if key not in _cache:
        hb = _host_batch(name, model, orders, which, bs)
        feats, ncls = _graph(name, model)[3:5]
        _cache[key] = (feats.shape[1], ncls, hb.to_device(dev, with_coo=False), _x0(hb, feats, dev))
    return _cache[key]


def _args(b):
    F, ncls, db, x0 = b
    return x0, db.adjs, db.sampled_nodes, db.labels


def _trainer(name, model, orders, b, dev, native=True):
    torch.manual_seed(0)
    m = build_model(model, b[0], GRAPHS[name][4], list(orders), b[1], 0.1, fused=True).to(dev)
    tr = Trainer(m, 0.01, dev)
    assert tr.executor is not None, "the native step refused the model"
    if not native:
        tr.executor = None
    return tr


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _fills(M, N, n):  # step.hip fills(): one 128 x 128 split3 tile per CU
    return -(-M // 128) * -(-N // 128) * n >= 256


def _assert_mid_routes(orders, args):
    """Every order-0 layer of a *mid* batch runs over enough rows for the split3 forward
    (fills(M, 512, 1)) and the split3 weight gradient (M >= 2048)."""
    rows = E.NativeStep._rows(args[0], args[1])
    dense = [m for m, o in zip(rows, orders) if o == 0]
    assert dense, orders
    for m in dense[:1]:  # the bottom-most order-0 layer: the large one
        assert _fills(m, 512, 1) and m >= 2048, (orders, rows)


def _grads(tr):
    """The step's gradients; a parameter the Python path never used (.grad None: an order-0 SAGE
    layer's linearB) counts as all-zero."""
    return [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in tr.params]


def _steps(tr, args, n=2, **kw):
    losses, grads = [], []
    for it in range(n):
        torch.manual_seed(100 + it)
        losses.append(tr.step(*args, **kw).clone())
        grads.append(_grads(tr))
    torch.cuda.synchronize()
    return losses, grads


def _assert_bit_identical(a, b, what):
    (la, ga), (lb, gb) = a, b
    for s, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), (what, "loss", s, float(x), float(y))
    for s, (xs, ys) in enumerate(zip(ga, gb)):
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(x, y), (what, "gradient", s, i)


# ------------------------------------------------------------------------------ 1. accepted
def test_trainer_takes_models_with_order_zero_layers(dev):
    b = _batch("small", "graphsage", [1, 0, 1, 0], dev)
    torch.manual_seed(0)
    net = build_model("graphsage", b[0], 128, [1, 0, 1, 0], b[1], 0.1, fused=True).to(dev)
    tr = Trainer(net, 0.01, dev)
    assert tr.executor is not None
    args = _args(b)
    assert [a is None for a in args[1]] == [False, True, False, True]
    assert tr.executor.supports(*args) and tr.executor.supports(*args, inference=True)
    # an operand where the model has an order-0 layer, or none where it aggregates: not this executor's
    adjs = list(args[1])
    assert not tr.executor.supports(args[0], [adjs[0], adjs[0], adjs[2], None], args[2], args[3])
    assert not tr.executor.supports(args[0], [None] + adjs[1:], args[2], args[3])
    assert not tr.executor.supports(args[0], adjs[:3], args[2], args[3])
    d = tr.executor._desc(*args, seeds=False)
    assert [int(d[E.HEADER + li * E.LAYER_SLOTS + E.L_DENSE]) for li in range(4)] == [0, 1, 0, 1]
    assert E.L_DENSE == 26
    # an order-0 SAGE layer's linearB takes no part: its slots stay 0
    for li in (1, 3):
        base = E.HEADER + li * E.LAYER_SLOTS
        assert all(d[base + s] == 0 for s in (E.L_WB, E.L_BB, E.L_GWB, E.L_GBB, E.L_ROWPTR, E.L_NSAMPLED))
        assert d[base + E.L_M] == d[base + E.L_K] == d[base - E.LAYER_SLOTS + E.L_M]
    bad = build_model("graphsage", b[0], 128, [1, 2], b[1], 0.1, fused=True).to(dev)
    with pytest.raises(ValueError, match="order"):
        E.NativeStep(bad)


# ------------------------------------------------------------------------------ 2. Python path
CASES = [("small", "graphsage", [1, 0, 1, 0]), ("small", "graphsage", [0, 1, 1]), ("small", "graphsage", [1, 1, 0]),
         ("small", "graphsage", [1, 0, 0, 1]), ("small", "graphsage", [0]), ("small", "gcn", [1, 0, 1, 0]),
         ("small", "gcn", [0, 1]), ("mid", "graphsage", [1, 0, 1, 0]), ("mid", "graphsage", [0, 1, 1]),
         ("mid", "gcn", [1, 0, 1, 0])]


@pytest.mark.parametrize("name,model,orders", CASES, ids=lambda v: "".join(map(str, v)) if isinstance(v, list) else v)
def test_native_step_matches_python_fused_path(dev, name, model, orders):
    """Same seeds, three Adam steps in training mode (dropout 0.1): loss within 1e-6 |loss| + 1e-7,
    every gradient and the final parameters within 1e-5 in relative L2 (tests/test_executor_gpu.py's
    bounds: same kernels, the vendor GEMM calls may round differently from torch.mm's)."""
    b = _batch(name, model, orders, dev)
    args = _args(b)
    if name == "mid":
        _assert_mid_routes(orders, args)
    ta = _trainer(name, model, orders, b, dev, native=False)
    tb = _trainer(name, model, orders, b, dev, native=True)
    assert tb.executor.supports(*args)
    for it in range(3):
        torch.manual_seed(100 + it)
        la = ta.step(*args)
        unused = [p.grad is None for p in ta.params]
        ga = _grads(ta)
        torch.manual_seed(100 + it)
        lb = tb.step(*args)
        gb = _grads(tb)
        torch.cuda.synchronize()
        print(f"{name} {model} {orders} step {it}: loss {float(la):.8f} / {float(lb):.8f}, max gradient error "
              f"{max(_rel(x, y) for x, y, u in zip(gb, ga, unused) if not u):.2e}")
        assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(la)) + 1e-7, (it, float(la), float(lb))
        for i, (x, y, u) in enumerate(zip(gb, ga, unused)):
            if u:
                assert not bool(x.any()), ("a gradient the Python path leaves None is not zero", it, i)
            else:
                assert _rel(x, y) <= 1e-5, (it, i, _rel(x, y))
        if model == "graphsage":
            # an order-0 layer's linearB takes no part: its gradients stay zero on both paths (the
            # Python path's None becomes a zero tensor in the optimizer), so Adam leaves it alone
            for li, o in enumerate(orders):
                for p in tb.model.encoder.gcs[li].linearB.parameters():
                    assert bool(p.grad.any()) == (o != 0), (it, li)
    for p, q in zip(tb.params, ta.params):
        assert _rel(p.detach(), q.detach()) <= 1e-5


# ------------------------------------------------------------------------------ 3. CPU reference
@pytest.mark.parametrize("model", ["graphsage", "gcn"])
def test_native_step_matches_cpu_reference(dev, model):
    """The executor on a *mid* [1,0,1,0] batch against the reference's CPU path on the same draw
    (oracle.cpu_reference: torch.sparse.mm + the reference's modules), eval mode: loss rtol 1e-4,
    every gradient within 1e-4 in relative L2 (test_config2_executor_step_matches_cpu_reference's
    bounds)."""
    from oracle.cpu_reference import cpu_inputs, torch_spmm

    orders = [1, 0, 1, 0]
    hb_cpu = _host_batch("mid", model, orders, device_extract=False)  # the same draw, extracted on the host
    hb_gpu = _host_batch("mid", model, orders)
    assert [list(s) for s in hb_gpu.sampled_nodes] == [list(s) for s in hb_cpu.sampled_nodes]
    feats, ncls = _graph("mid", model)[3:5]
    F = feats.shape[1]
    adjs_c, x0_c, sampled_c, y_c = cpu_inputs(hb_cpu, feats)
    torch.manual_seed(0)
    ref = build_model(model, F, 512, orders, ncls, 0.1, spmm_fn=torch_spmm)
    ref.eval()
    lo_r = loss_fn(ref(x0_c, adjs_c, sampled_c), y_c, True, "cpu")
    lo_r.backward()
    b = _batch("mid", model, orders, dev)
    args = _args(b)
    _assert_mid_routes(orders, args)
    tr = _trainer("mid", model, orders, b, dev)
    tr.model.eval()
    assert tr.executor.supports(*args)
    lo = tr.executor.step(*args)
    torch.cuda.synchronize()
    print(f"{model}: loss {float(lo):.8f} / reference {float(lo_r):.8f}")
    np.testing.assert_allclose(float(lo), float(lo_r.detach()), rtol=1e-4)
    assert len(tr.params) == len(list(ref.parameters()))
    for (pn, p), pr in zip(tr.model.named_parameters(), ref.parameters()):
        if pr.grad is None:  # an order-0 SAGE layer's linearB
            assert not bool(p.grad.any()), pn
            continue
        g, gr = p.grad.detach().cpu().double(), pr.grad.detach().double()
        rel = float((g - gr).norm() / max(float(gr.norm()), 1e-30))
        print(f"  {pn}: relative gradient error {rel:.2e}")
        assert rel < 1e-4, f"{pn}: relative gradient error {rel:.2e}"


# ------------------------------------------------------------------------------ 4. variants
@pytest.mark.parametrize("name,orders", [("mid", [1, 0, 1, 0]), ("small", [0, 1, 1])], ids=["mid1010", "small011"])
def test_schedule_variants_are_bit_identical(dev, monkeypatch, name, orders):
    """The default step against GNN_STEP_FUSE_AGG=0 (an aggregating layer above an order-0 layer
    folded into that layer's tail backward, or launched on its own), GNN_STEP_SMALL_OVERLAP=0,
    GNN_STEP_OVERLAP=1, gradient-ready events, and prefetch + step (phases 1 + 2; a no-op in front of
    an order-0 layer 0): loss and every gradient torch.equal over two Adam steps."""
    b = _batch(name, "graphsage", orders, dev)
    args = _args(b)
    if name == "mid":
        _assert_mid_routes(orders, args)
    envs = ("GNN_STEP_FUSE_AGG", "GNN_STEP_SMALL_OVERLAP", "GNN_STEP_OVERLAP")
    for k in envs:
        monkeypatch.delenv(k, raising=False)
    base = _steps(_trainer(name, "graphsage", orders, b, dev), args)
    for v in ({"GNN_STEP_FUSE_AGG": "0"}, {"GNN_STEP_SMALL_OVERLAP": "0"}, {"GNN_STEP_OVERLAP": "1"},
              {"events": True}, {"prefetch": True}):
        for k in envs:
            monkeypatch.delenv(k, raising=False)
        for k, val in v.items():
            if k in envs:
                monkeypatch.setenv(k, val)
        tr = _trainer(name, "graphsage", orders, b, dev)
        if v.get("events"):
            evs = [torch.cuda.Event() for _ in range(1 + len(orders))]
            step = tr.executor.step
            tr.executor.step = lambda *a, **kw: step(*a, grad_events=evs, **kw)
        if v.get("prefetch"):
            losses, grads = [], []
            for it in range(2):
                torch.manual_seed(100 + it)
                tr.executor.prefetch(*args)
                assert (getattr(tr.executor, "_pre", None) is not None) == (orders[0] != 0)
                losses.append(tr.step(*args).clone())
                assert tr.executor._pre is None
                grads.append(_grads(tr))
            torch.cuda.synchronize()
            got = (losses, grads)
        else:
            got = _steps(tr, args)
        _assert_bit_identical(got, base, v)


def test_timing_records_name_aggregations_only(dev):
    """GNN_SH_TIMING through a step with order-0 layers: records for the aggregations alone, under
    their own layer numbers (the layer-2 backward may be folded into layer 1's tail: no record)."""
    from gnn_amd import custom_sparse_ops as cso

    orders = [1, 0, 1, 0]
    b = _batch("small", "graphsage", orders, dev)
    tr = _trainer("small", "graphsage", orders, b, dev)
    cso.take_timing_records()
    cso.enable_timing(True)
    try:
        tr.step(*_args(b))
    finally:
        cso.enable_timing(False)
    names = [r[0] for r in cso.take_timing_records()]
    assert names[:2] == ["fwd_L0", "fwd_L2"] and names[2:] in ([], ["bwd_L2"]), names


def test_phases_with_order_zero_layer_0_at_the_c_abi(dev):
    """NativeStep.prefetch never issues a phase-1 call in front of an order-0 layer 0, so the C
    entry point is driven directly on [0,1,1]: phase 1 launches nothing (the loss and the gradients
    keep their fill) and records the gate of layer 0; phase 2 in the same workspace then gives
    phase 0's loss and gradients bit for bit."""
    orders = [0, 1, 1]
    b = _batch("small", "graphsage", orders, dev)
    args = _args(b)
    ex = _trainer("small", "graphsage", orders, b, dev).executor
    torch.manual_seed(100)
    d0 = ex._desc(*args, seeds=True)
    loss = torch.full((), -7.0, device=dev)
    d0[E.H_LOSS] = loss.data_ptr()
    L = _lib.lib()
    need = L.gnn_train_step_workspace_bytes(d0.ctypes.data)
    assert need > 0
    st = _lib.stream_of(dev)

    def call(phase, ws, gate=None):
        d = d0.copy()
        d[E.H_PHASE] = phase
        if gate is not None:
            gate.record()  # creates the underlying event; the step re-records it
            d[E.H_STAGE_EVENT], d[E.H_STAGE_LAYER] = gate.cuda_event, 0
        _lib.check(L.gnn_train_step_f32(d.ctypes.data, ws.data_ptr(), need, st), f"phase {phase}")

    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call(0, ws)
    torch.cuda.synchronize()
    want = (loss.clone(), ex.flat_grad.clone())
    assert float(want[0]) > 0
    loss.fill_(-7.0)
    ex.flat_grad.fill_(-7.0)
    ws2 = torch.empty(need, dtype=torch.uint8, device=dev)
    gate, t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    t0.record()
    call(1, ws2, gate)
    t1.record()
    torch.cuda.synchronize()
    assert float(loss) == -7.0 and bool((ex.flat_grad == -7.0).all()), "phase 1 wrote something"
    assert t0.elapsed_time(gate) >= 0.0 and gate.elapsed_time(t1) >= 0.0
    call(2, ws2)
    torch.cuda.synchronize()
    assert torch.equal(loss, want[0])
    # an order-0 layer's linearB views are never written: they keep the fill, all else is phase 0's
    untouched = ex.flat_grad == -7.0
    assert int(untouched.sum()) == sum(p.numel() for p in ex.enc.gcs[0].linearB.parameters())
    assert torch.equal(ex.flat_grad[~untouched], want[1][~untouched])


# ------------------------------------------------------------------------------ 5. staging gate
@pytest.mark.parametrize("layer", [1, 2, 0])
def test_staging_gate_is_recorded_within_the_step(dev, layer):
    """The gate (GNN_SH_STAGE_EVENT) on an order-0 layer ([1,0,1,0], layer 1), on an aggregating one
    (layer 2) and on layer 0: its timestamp lies between events recorded around the step, and a
    stream waiting on it completes. Results do not depend on the gate."""
    orders = [1, 0, 1, 0]
    b = _batch("small", "graphsage", orders, dev)
    args = _args(b)
    base = _steps(_trainer("small", "graphsage", orders, b, dev), args, n=1)
    tr = _trainer("small", "graphsage", orders, b, dev)
    gate, t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    side = torch.cuda.Stream(dev)
    done = torch.cuda.Event()
    torch.manual_seed(100)
    t0.record()
    loss = tr.executor.step(*args, stage_gate=(gate, layer)).clone()
    t1.record()
    side.wait_event(gate)
    done.record(side)
    side.synchronize()
    torch.cuda.synchronize()
    assert done.query() and gate.query()
    assert t0.elapsed_time(gate) >= 0.0 and gate.elapsed_time(t1) >= 0.0, (t0.elapsed_time(gate), gate.elapsed_time(t1))
    _assert_bit_identical(([loss], [_grads(tr)]), base, ("gate", layer))


def test_staging_gate_with_order_zero_layer_0(dev):
    """Layer 0 of order 0 and the gate on it: prefetch is a no-op, the step records the gate."""
    orders = [0, 1, 1]
    b = _batch("small", "graphsage", orders, dev)
    args = _args(b)
    tr = _trainer("small", "graphsage", orders, b, dev)
    gate, t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    tr.executor.prefetch(*args, stage_gate=(gate, 0))
    assert getattr(tr.executor, "_pre", None) is None
    t0.record()
    tr.executor.step(*args, stage_gate=(gate, 0))
    t1.record()
    side = torch.cuda.Stream(dev)
    side.wait_event(gate)
    side.synchronize()
    torch.cuda.synchronize()
    assert t0.elapsed_time(gate) >= 0.0 and gate.elapsed_time(t1) >= 0.0


# ------------------------------------------------------------------------------ 6. evaluation
def _np_counts(z, y, mode):
    C = z.shape[1]
    if mode == 0:
        pred, true = z > 0, y > 0.5
    else:
        pred = np.argmax(z, axis=1)[:, None] == np.arange(C)
        true = np.argmax(y, axis=1)[:, None] == np.arange(C)
    return np.stack([(pred & true).sum(0), (pred & ~true).sum(0), (true & ~pred).sum(0)]).astype(np.int32)


@pytest.mark.parametrize("name,model,orders", [("small", "graphsage", [1, 0, 1, 0]), ("small", "gcn", [0, 1]),
                                               ("small", "graphsage", [0]), ("mid", "graphsage", [1, 0, 1, 0])],
                         ids=["small_sage1010", "small_gcn01", "small_sage0", "mid_sage1010"])
def test_evaluation_matches_training_forward_and_python_path(dev, name, model, orders):
    """tests/test_eval_gpu.py's checks with order-0 layers: evaluate's loss torch.equal to the
    training step's with model.eval(), logits within 1e-5 in relative L2 of model.forward_loss
    under no_grad, counts equal to numpy and gnn_amd.metrics on those logits; the predict form (no
    labels) with a top layer of order 0; the evaluation workspace below the training one."""
    b = _batch(name, model, orders, dev)
    args = _args(b)
    tr = _trainer(name, model, orders, b, dev)
    ex, net = tr.executor, tr.model
    assert ex.supports(*args, inference=True)
    net.eval()
    loss_step = ex.step(*args).clone()
    with torch.no_grad():
        loss_py, out_py = net.forward_loss(*args)
    net.train()
    for mode in (0, 1):
        loss, counts, logits = ex.evaluate(*args, mode=mode, want_logits=True)
        torch.cuda.synchronize()
        assert torch.equal(loss, loss_step), (mode, float(loss), float(loss_step))
        assert logits.shape == out_py.shape and _rel(logits, out_py) <= 1e-5, _rel(logits, out_py)
        assert abs(float(loss) - float(loss_py)) <= 1e-6 * abs(float(loss_py)) + 1e-7
        assert np.array_equal(counts.cpu().numpy(), _np_counts(logits.cpu().numpy(), args[3].cpu().numpy(), mode))
        assert torch.equal(counts, metrics.prediction_counts(logits, args[3], mode).to(torch.int32))
    lo, cn, z = ex.evaluate(*args[:3])  # predict: sized from the top layer's M, also without an operand
    assert lo is None and cn is None and torch.equal(z, logits)
    ev = Evaluator(net, dev, executor=ex)
    assert torch.equal(ev.predict(*args[:3]), logits)
    d = ex._desc(*args, seeds=False)
    L = _lib.lib()
    ev_bytes, tr_bytes = L.gnn_eval_step_workspace_bytes(d.ctypes.data), L.gnn_train_step_workspace_bytes(d.ctypes.data)
    assert 0 < ev_bytes < tr_bytes, (ev_bytes, tr_bytes)


def test_trainer_evaluate_pools_three_batches(dev):
    orders = [1, 0, 1, 0]
    batches = [_batch("small", "graphsage", orders, dev, which=w, bs=bs) for bs, w in ((64, 0), (40, 1), (17, 2))]
    data = [_args(b) for b in batches]
    assert [d[3].shape[0] for d in data] == [64, 40, 17]
    tr = _trainer("small", "graphsage", orders, batches[0], dev)
    tr.model.train()
    res = tr.evaluate(iter(data))
    assert tr.model.training and res["batches"] == 3 and res["rows"] == 121
    per = [tr.executor.evaluate(*d, mode=0) for d in data]
    torch.cuda.synchronize()
    counts = np.sum([c.cpu().numpy().astype(np.int64) for _, c, _ in per], axis=0)
    micro, macro = metrics.f1_from_counts(counts[0], counts[1], counts[2], 0)
    assert res["micro_f1"] == micro and res["macro_f1"] == macro
    rows = [64.0, 40.0, 17.0]
    assert res["loss"] == sum(float(l.double()) * r for (l, _, _), r in zip(per, rows)) / 121.0
    ev = Evaluator(tr.model, dev, executor=tr.executor)
    for d in data:
        ev.add(*d)
    assert ev.native_batches == 3 and ev.result() == res


# ------------------------------------------------------------------------------ 7. 16-bit X0
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_order_zero_layer_0_from_16bit_x0(dev, dtype):
    """[0,1,1] from an fp16 / bf16 X0 (GNN_SL_XKIND): the rows are widened once into the workspace
    and the layer runs as fp32 — loss and gradients torch.equal to the step on the widened X0,
    training and evaluation."""
    orders = [0, 1, 1]
    b = _batch("small", "graphsage", orders, dev)
    _, adjs, sn, labels = _args(b)
    F = b[0]
    n = b[3].shape[0]
    g = torch.Generator().manual_seed(5)
    tab = (torch.randn(n, F, generator=g) * 3).to(dtype)
    x16 = torch.zeros((n, staging.padded_ld(F, 64)), dtype=dtype)
    x16[:, :F] = tab
    x16 = x16.to(dev)[:, :F]
    x32 = torch.zeros((n, staging.padded_ld(F)), dtype=torch.float32)
    x32[:, :F] = tab.float()
    x32 = x32.to(dev)[:, :F]
    res = []
    for x0 in (x16, x32):
        tr = _trainer("small", "graphsage", orders, b, dev)
        assert tr.executor.supports(x0, adjs, sn, labels)
        d = tr.executor._desc(x0, adjs, sn, labels, seeds=False)
        assert d[E.HEADER + E.L_XKIND] == (0 if x0.dtype == torch.float32 else (1 if dtype == torch.float16 else 2))
        out = _steps(tr, (x0, adjs, sn, labels))
        lo, cn, z = tr.executor.evaluate(x0, adjs, sn, labels, want_logits=True)
        torch.cuda.synchronize()
        res.append((out, lo.clone(), cn.clone(), z.clone()))
    _assert_bit_identical(res[0][0], res[1][0], dtype)
    for x, y in zip(res[0][1:], res[1][1:]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------ 8. pipeline
def _pipeline_world():
    if "pipe" not in _cache:
        N, lap, labels, feats, ncls, train = _graph("small", "graphsage")
        pl = placement.create_buffer(lap, train, 400, [0], 2, alpha=0)
        _cache["pipe"] = (lap, labels, feats, ncls, train, pl)
    return _cache["pipe"]


def _eq(x, y, what):
    x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    y = y.numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    assert x.shape == y.shape and np.array_equal(x, y), what


def test_pipeline_native_loader_staging_and_step(dev):
    """NativeLoader(orders=[1,0,1,0]) against BatchLoader on *small*: the same batches bit for bit;
    native staging (gnn_stage_batch_f32) == the Python sequence of staging calls; and three staged
    batches through Trainer.step on the executor == through the Python path (item 2's bounds)."""
    orders = [1, 0, 1, 0]
    lap, labels, feats, ncls, train, pl = _pipeline_world()
    dev_of, idx_on = pl.device_id_of_nodes_group[0], pl.idx_of_nodes_on_device_group[0]
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
    kw = dict(store=store, workers=2, seed=5, device_extract=True)
    a = loader.BatchLoader(lap, labels, train, 600, 64, orders, dev_of, idx_on, **kw)
    b = loader.NativeLoader(lap, labels, train, 600, 64, orders, dev_of, idx_on, **kw)
    F = feats.shape[1]
    torch.manual_seed(0)
    net_a = build_model("graphsage", F, 128, orders, ncls, 0.1, fused=True).to(dev)
    torch.manual_seed(0)
    net_b = build_model("graphsage", F, 128, orders, ncls, 0.1, fused=True).to(dev)
    ta, tb = Trainer(net_a, 0.01, dev), Trainer(net_b, 0.01, dev)
    assert tb.executor is not None
    ta.executor = None
    stager = staging.Stager(store)
    built = []
    try:
        for it, (pa, pb) in zip(range(3), zip(a.epoch(1), b.epoch(1))):
            ha, hb = pa.host, pb.host
            assert ha.seed == hb.seed
            _eq(ha.input_nodes, hb.input_nodes, "input nodes")
            _eq(ha.labels, hb.labels, "labels")
            assert [L is None for L in ha.layers] == [L is None for L in hb.layers] == [False, True, False, True]
            for li, (La, Lb) in enumerate(zip(ha.layers, hb.layers)):
                if La is None:
                    continue
                assert La.shape == Lb.shape and La.on_device == Lb.on_device and La.nnz == Lb.nnz
                for k in ("fullrowptr", "rowptr", "colidx", "normfact", "csc_colptr", "csc_rows", "rows", "cols"):
                    va, vb = getattr(La, k), getattr(Lb, k)
                    assert (va is None) == (vb is None), (li, k)
                    if va is not None:
                        _eq(va, vb, f"layer {li} {k}")
            for li, (sa, sb) in enumerate(zip(ha.sampled_nodes, hb.sampled_nodes)):
                _eq(np.asarray(sa, np.int64), sb, f"sampled {li}")
            sa = stager.issue(pa.plan, lambda: pa.host.to_device(dev, with_coo=False))
            sb = stager.issue(pb.plan, loader.ToDevice(pb.host, dev, on_built=built.append))
            assert sb.batch.raw is None and built[-1] is sb.batch, "the native staging call ran"
            xa, xb = sa.wait(), sb.wait()
            torch.cuda.synchronize()
            assert torch.equal(xa, xb)
            da, db = sa.batch, sb.batch
            assert torch.equal(da.labels, db.labels)
            for x, y in zip(da.sampled_nodes, db.sampled_nodes):
                assert torch.equal(x, y)
                ra, rb = getattr(x, "_gnn_rmap", None), getattr(y, "_gnn_rmap", None)
                assert (ra is None) == (rb is None) and (ra is None or torch.equal(ra, rb))
            for li, (oa, ob) in enumerate(zip(sa.adjs, sb.adjs)):
                assert (oa is None) == (ob is None) == (orders[li] == 0)
                if oa is None:
                    continue
                assert oa.shape == ob.shape and oa.nnz == ob.nnz
                for k in ("rowptr", "col", "val"):
                    assert torch.equal(getattr(oa, k), getattr(ob, k)), (li, k)
                assert (oa._t is None) == (ob._t is None), li
                if oa._t is not None:
                    for k in ("rowptr", "col", "val"):
                        assert torch.equal(getattr(oa._t, k), getattr(ob._t, k)), (li, "t", k)
            # the natively staged batch through both trainers
            args = (xb, sb.adjs, db.sampled_nodes, db.labels)
            assert tb.executor.supports(*args)
            torch.manual_seed(100 + it)
            la = ta.step(*args)
            unused = [p.grad is None for p in ta.params]
            ga = _grads(ta)
            torch.manual_seed(100 + it)
            lb = tb.step(*args)
            gb = _grads(tb)
            torch.cuda.synchronize()
            assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(la)) + 1e-7, (it, float(la), float(lb))
            for i, (x, y, u) in enumerate(zip(gb, ga, unused)):
                assert (not bool(x.any())) if u else _rel(x, y) <= 1e-5, (it, i)
        assert it == 2
        for p, q in zip(tb.params, ta.params):
            assert _rel(p.detach(), q.detach()) <= 1e-5
    finally:
        a.close()
        b.close()
