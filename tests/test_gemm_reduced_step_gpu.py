"""GPU: the reduced-precision GEMM modes in the training and evaluation step (GNN_SL_GEMM,
include/gnn_step.h; NativeStep / Trainer ``gemm=``; GNN_GEMM_ALGO=split2 / bf16 process-wide).

Batches (tests/test_orders_gpu.py's): *mid* = 40 k nodes, 100 features, samp 8192, batch 512,
nhid 512 — its big layers route to the split kernel; *small* = graphs.TINY — the vendor-GEMM
routes, where a mode changes nothing. Models: SAGE [1,1], SAGE [1,0,1], GCN [1,1].

The independent oracle (item 6 below) needs no tolerance: the Python fused path with fused.gemm
replaced by "round every operand (fused.round_operand), then split3" must give the same bits as
the mode itself, because the kernel accumulates the exact products of the rounded operands in
split3's order.
"""
import numpy as np
import pytest
import torch

from gnn_amd import _lib, fused
from gnn_amd import executor as E
from gnn_amd.models import build_model
from gnn_amd.train import Trainer

from test_orders_gpu import GRAPHS, _args, _assert_bit_identical, _batch, _fills, _grads, _rel, _steps

pytestmark = pytest.mark.gpu

MODELS = [("graphsage", [1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1])]
CASES = [(name, model, orders) for name in ("small", "mid") for model, orders in MODELS]
_ids = lambda v: "".join(map(str, v)) if isinstance(v, list) else v  # noqa: E731
ENVS = ("GNN_GEMM_ALGO", "GNN_STEP_OVERLAP", "GNN_STEP_SMALL_OVERLAP", "GNN_STEP_FUSE_AGG", "GNN_GEMM_WIDE",
        "GNN_STEP_GATHER")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENVS:
        monkeypatch.delenv(k, raising=False)


def _trainer(name, model, orders, b, dev, native=True, gemm=None):
    torch.manual_seed(0)
    m = build_model(model, b[0], GRAPHS[name][4], list(orders), b[1], 0.1, fused=True).to(dev)
    tr = Trainer(m, 0.01, dev, gemm=gemm)
    assert tr.executor is not None, "the native step refused the model"
    if not native:
        tr.executor = None
    return tr


def _assert_mid_layer0_on_split_kernel(model, args):
    """Layer 0 of a *mid* batch: forward pair and weight gradients on the split kernel."""
    M = args[1][0].shape[0]
    assert _fills(M, 512, 2 if model == "graphsage" else 1) and M >= 2048, M


def _rounding_gemm(modes, F0):
    """fused.gemm with every operand rounded as layer's mode says, then split3 — the oracle.
    modes: one name, or [layer 0's, the other layers']: a product is layer 0's iff one of its
    dimensions is the feature count F0 (forward K, weight-gradient N; layer 0 has no input gradient)."""
    orig = fused.gemm

    def wrapped(a_km, b_km, As, Bs, M, N, K, algo=None):
        mode = modes if isinstance(modes, str) else modes[0 if F0 in (N, K) else 1]
        return orig(a_km, b_km, [fused.round_operand(a, mode) for a in As], [fused.round_operand(b, mode) for b in Bs],
                    M, N, K, algo="split3")

    return wrapped


# ------------------------------------------------------------------------------ 5. native ≡ Python path
@pytest.mark.parametrize("mode", fused.GEMM_REDUCED)
@pytest.mark.parametrize("name,model,orders", CASES, ids=_ids)
def test_native_step_matches_python_fused_path(dev, monkeypatch, name, model, orders, mode):
    """The native step with gemm=mode against the Python fused path under GNN_GEMM_ALGO=mode: the
    assertions of tests/test_orders_gpu.py::test_native_step_matches_python_fused_path (loss within
    1e-6 |loss| + 1e-7, gradients and final parameters within 1e-5 in relative L2, three steps).

    The bound is the full-precision paths' although a rounding mode is a step function of the
    operands (under bf16 a last-bit change of an activation or a weight near a rounding boundary
    moves the operand by 2^-8, so a 3e-8 difference between the two trainers' parameters grows
    ~100x per Adam step in the model whose order-0 layer feeds 8 k x 1024 activations to a bf16
    product). It holds because the two paths do not start to differ: the one product they used to
    sum in different orders, the head's bias gradient, is gnn_head_bias_grad_f32 on both."""
    b = _batch(name, model, orders, dev)
    args = _args(b)
    if name == "mid":
        _assert_mid_layer0_on_split_kernel(model, args)
    ta = _trainer(name, model, orders, b, dev, native=False)
    tb = _trainer(name, model, orders, b, dev, native=True, gemm=mode)
    for it in range(3):
        monkeypatch.setenv("GNN_GEMM_ALGO", mode)
        torch.manual_seed(100 + it)
        la = ta.step(*args)
        unused = [p.grad is None for p in ta.params]
        ga = _grads(ta)
        monkeypatch.delenv("GNN_GEMM_ALGO")  # the executor's descriptor carries the mode
        torch.manual_seed(100 + it)
        lb = tb.step(*args)
        gb = _grads(tb)
        torch.cuda.synchronize()
        print(f"{name} {model} {orders} {mode} step {it}: loss {float(la):.8f} / {float(lb):.8f}, max gradient "
              f"error {max(_rel(x, y) for x, y, u in zip(gb, ga, unused) if not u):.2e}")
        assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(la)) + 1e-7, (it, float(la), float(lb))
        for i, (x, y, u) in enumerate(zip(gb, ga, unused)):
            if u:
                assert not bool(x.any()), (it, i)
            else:
                assert _rel(x, y) <= 1e-5, (it, i, _rel(x, y))
    for p, q in zip(tb.params, ta.params):
        assert _rel(p.detach(), q.detach()) <= 1e-5


@pytest.mark.parametrize("mode", fused.GEMM_REDUCED)
@pytest.mark.parametrize("model,orders", MODELS, ids=_ids)
def test_native_step_matches_python_fused_path_from_equal_parameters(dev, monkeypatch, model, orders, mode):
    """The same comparison on *mid* with the native trainer's parameters copied from the Python
    trainer's before each of four steps: the two paths issue the same kernels with the same routing
    under a mode, so from equal parameters they agree as closely as under split3 — the bounds of the
    test above at every step (loss within 1e-6 |loss| + 1e-7, every gradient within 1e-5 in relative
    L2; measured <= 6e-8 in every mode)."""
    name = "mid"
    b = _batch(name, model, orders, dev)
    args = _args(b)
    ta = _trainer(name, model, orders, b, dev, native=False)
    tb = _trainer(name, model, orders, b, dev, native=True, gemm=mode)
    for it in range(4):
        with torch.no_grad():
            for p, q in zip(tb.params, ta.params):
                p.copy_(q)
        monkeypatch.setenv("GNN_GEMM_ALGO", mode)
        torch.manual_seed(100 + it)
        la = ta.step(*args)
        ga = _grads(ta)
        monkeypatch.delenv("GNN_GEMM_ALGO")
        torch.manual_seed(100 + it)
        lb = tb.step(*args)
        gb = _grads(tb)
        torch.cuda.synchronize()
        assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(la)) + 1e-7, (it, float(la), float(lb))
        for i, (x, y) in enumerate(zip(gb, ga)):
            assert _rel(x, y) <= 1e-5, (it, i, _rel(x, y))


# ------------------------------------------------------------------------------ 6. the oracle
@pytest.mark.parametrize("mode", fused.GEMM_REDUCED)
@pytest.mark.parametrize("name,model,orders", CASES, ids=_ids)
def test_mode_equals_split3_of_rounded_operands(dev, monkeypatch, name, model, orders, mode):
    """Python fused path: GNN_GEMM_ALGO=mode against fused.gemm patched to round every A and B and
    call split3 — loss and every gradient torch.equal over two Adam steps."""
    b = _batch(name, model, orders, dev)
    args = _args(b)
    monkeypatch.setenv("GNN_GEMM_ALGO", mode)
    got = _steps(_trainer(name, model, orders, b, dev, native=False), args)
    monkeypatch.delenv("GNN_GEMM_ALGO")
    if name == "mid":  # the mode is not split3 here
        base = _steps(_trainer(name, model, orders, b, dev, native=False), args, n=1)
        assert not torch.equal(base[1][0][0], got[1][0][0])
    monkeypatch.setattr(fused, "gemm", _rounding_gemm(mode, b[0]))
    want = _steps(_trainer(name, model, orders, b, dev, native=False), args)
    _assert_bit_identical(got, want, (mode, "rounded operands + split3"))


# ------------------------------------------------------------------------------ 7. slot and environment
@pytest.mark.parametrize("name,model,orders", [("mid", "graphsage", [1, 0, 1]), ("mid", "gcn", [1, 1]),
                                               ("small", "graphsage", [1, 1])], ids=_ids)
def test_descriptor_slot_equals_environment_route(dev, monkeypatch, name, model, orders):
    b = _batch(name, model, orders, dev)
    args = _args(b)
    default = _steps(_trainer(name, model, orders, b, dev), args)
    _assert_bit_identical(_steps(_trainer(name, model, orders, b, dev, gemm="split3"), args), default, "split3 slot")
    assert E.L_GEMM == 27
    for gemm, want in ((None, 0), ("split3", 3), ("split2", 2), ("bf16", 1)):
        d = _trainer(name, model, orders, b, dev, gemm=gemm).executor._desc(*args, seeds=False)
        assert [int(d[E.HEADER + li * E.LAYER_SLOTS + E.L_GEMM]) for li in range(len(orders))] == [want] * len(orders)
    for mode in fused.GEMM_REDUCED:
        slot = _steps(_trainer(name, model, orders, b, dev, gemm=mode), args)
        monkeypatch.setenv("GNN_GEMM_ALGO", mode)
        env = _steps(_trainer(name, model, orders, b, dev), args)
        # a slot of 3 overrides the environment's mode
        forced = _steps(_trainer(name, model, orders, b, dev, gemm="split3"), args, n=1)
        monkeypatch.delenv("GNN_GEMM_ALGO")
        _assert_bit_identical(slot, env, (mode, "slot against environment"))
        _assert_bit_identical(forced, (default[0][:1], default[1][:1]), (mode, "slot 3 under the environment"))
        if name == "mid":
            assert not torch.equal(slot[1][0][0], default[1][0][0]), mode


def test_per_layer_modes(dev, monkeypatch):
    """A per-layer list on SAGE [1,0,1] (*mid*: layers 0 and 1 on the split kernel, the 512-row top
    layer on the vendor GEMM): ["bf16", "split3", "split3"] differs from both uniform settings in
    the layer-0 gradients and matches the Python path whose fused.gemm rounds layer 0's operands to
    bf16 and leaves the others (native against Python: the bounds of item 5 — the vendor-GEMM
    products may round differently; the modes themselves differ by ~2^-9, far above them).
    On SAGE [1,1] the issue's ["bf16", "split3"]: layer 1 is the 512-row top layer, on the vendor
    GEMM under every mode, so the list can only differ from uniform split3; it equals uniform bf16."""
    name, model = "mid", "graphsage"
    for orders, mix in (([1, 0, 1], ["bf16", "split3", "split3"]), ([1, 1], ["bf16", "split3"])):
        b = _batch(name, model, orders, dev)
        args = _args(b)
        got = _steps(_trainer(name, model, orders, b, dev, gemm=mix), args)
        uni = {m: _steps(_trainer(name, model, orders, b, dev, gemm=m), args) for m in ("bf16", "split3")}
        layer0 = [i for i, (n, _) in enumerate(_trainer(name, model, orders, b, dev).model.named_parameters())
                  if "gcs.0." in n and "linear" in n and "weight" in n]
        assert layer0
        for i in layer0:
            assert not torch.equal(got[1][0][i], uni["split3"][1][0][i]), (orders, i)
            if len(orders) == 3:
                assert not torch.equal(got[1][0][i], uni["bf16"][1][0][i]), (orders, i)
        if len(orders) == 2:
            _assert_bit_identical(got, uni["bf16"], "top layer on the vendor GEMM")
        with monkeypatch.context() as mp:
            mp.setattr(fused, "gemm", _rounding_gemm(["bf16", "split3"], b[0]))
            want = _steps(_trainer(name, model, orders, b, dev, native=False), args)
        for s in range(2):
            assert abs(float(got[0][s]) - float(want[0][s])) <= 1e-6 * abs(float(want[0][s])) + 1e-7
            for i, (x, y) in enumerate(zip(got[1][s], want[1][s])):
                assert _rel(x, y) <= 1e-5, (orders, s, i, _rel(x, y))
            for i in layer0:  # and no uniform setting is that close
                assert _rel(uni["split3"][1][s][i], want[1][s][i]) > 1e-5


def test_bad_names(dev):
    b = _batch("small", "graphsage", [1, 1], dev)
    net = build_model("graphsage", b[0], 128, [1, 1], b[1], 0.1, fused=True).to(dev)
    for bad in ("fp8", "f32", ["bf16"], ["bf16", "tf32"]):
        with pytest.raises(ValueError):
            E.NativeStep(net, gemm=bad)
        with pytest.raises(ValueError):
            Trainer(net, 0.01, dev, gemm=bad)
    plain = build_model("graphsage", b[0], 128, [1, 1], b[1], 0.1, fused=False).to(dev)
    with pytest.raises(ValueError, match="native step"):
        Trainer(plain, 0.01, dev, gemm="bf16")  # no executor: the Python path reads only the environment
    assert Trainer(plain, 0.01, dev).executor is None


# ------------------------------------------------------------------------------ 8. evaluation, schedules
@pytest.mark.parametrize("mode", fused.GEMM_REDUCED)
@pytest.mark.parametrize("name,model,orders", [("mid", "graphsage", [1, 0, 1]), ("mid", "gcn", [1, 1])], ids=_ids)
def test_evaluation_under_a_mode(dev, name, model, orders, mode):
    b = _batch(name, model, orders, dev)
    args = _args(b)
    tr = _trainer(name, model, orders, b, dev, gemm=mode)
    tr.model.eval()
    loss_step = tr.executor.step(*args).clone()
    tr.model.train()
    loss, counts, _ = tr.executor.evaluate(*args)
    res = tr.evaluate([args])
    torch.cuda.synchronize()
    assert torch.equal(loss, loss_step), (float(loss), float(loss_step))
    assert res["batches"] == 1 and np.float32(res["loss"]) == np.float32(float(loss_step))
    if mode == "bf16":  # the slot reached the shared forward (a split2 loss may round to split3's)
        base = _trainer(name, model, orders, b, dev)
        assert not torch.equal(base.executor.evaluate(*args)[0], loss)


def test_phases_and_overlap_variants_under_a_mode(dev, monkeypatch):
    name, model, orders, mode = "mid", "graphsage", [1, 0, 1], "split2"
    b = _batch(name, model, orders, dev)
    args = _args(b)
    base = _steps(_trainer(name, model, orders, b, dev, gemm=mode), args)
    tr = _trainer(name, model, orders, b, dev, gemm=mode)
    losses, grads = [], []
    for it in range(2):  # phases 1 + 2
        torch.manual_seed(100 + it)
        tr.executor.prefetch(*args)
        assert tr.executor._pre is not None
        losses.append(tr.step(*args).clone())
        grads.append(_grads(tr))
    torch.cuda.synchronize()
    _assert_bit_identical((losses, grads), base, "phases 1 + 2")
    for env in ({"GNN_STEP_OVERLAP": "1"}, {"GNN_STEP_SMALL_OVERLAP": "0"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            _assert_bit_identical(_steps(_trainer(name, model, orders, b, dev, gemm=mode), args), base, env)
            mp.setenv("GNN_GEMM_ALGO", mode)  # and through the environment route
            _assert_bit_identical(_steps(_trainer(name, model, orders, b, dev), args), base, (env, "environment"))


# ------------------------------------------------------------------------------ 9. bad slot
@pytest.mark.parametrize("value", [4, -1])
def test_bad_slot_is_refused(dev, value):
    b = _batch("small", "graphsage", [1, 1], dev)
    args = _args(b)
    ex = _trainer("small", "graphsage", [1, 1], b, dev).executor
    d = ex._desc(*args, seeds=False)
    L = _lib.lib()
    assert L.gnn_train_step_workspace_bytes(d.ctypes.data) > 0 and L.gnn_eval_step_workspace_bytes(d.ctypes.data) > 0
    d[E.HEADER + E.LAYER_SLOTS + E.L_GEMM] = value
    assert L.gnn_train_step_workspace_bytes(d.ctypes.data) == 0
    assert b"layer 1" in L.gnn_last_error() and b"pieces" in L.gnn_last_error()
    assert L.gnn_eval_step_workspace_bytes(d.ctypes.data) == 0
    assert b"layer 1" in L.gnn_last_error()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    loss = torch.full((), -7.0, device=dev)
    d[E.H_LOSS] = loss.data_ptr()
    assert L.gnn_train_step_f32(d.ctypes.data, ws.data_ptr(), 1 << 20, _lib.stream_of(dev)) == -22
    torch.cuda.synchronize()
    assert float(loss) == -7.0  # nothing was launched
