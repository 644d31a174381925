"""GPU: the fused head with the softmax cross-entropy loss (gnn_head_ce_fwd_f32 / gnn_head_ce_bwd_f32,
gnn_head_eval_loss_f32; gnn_amd.fused.head_ce_loss), kernel level.

Reference: GNN.forward's tail (models.py:90-97) and utils.loss with sigmoid_loss=False
(utils.py:138-140): F.normalize -> F.linear -> CrossEntropyLoss(reduction="none") over float target
rows, weighted 1/M and summed, evaluated in fp64. Tolerances are those the BCE head is held to
(tests/test_fused_gpu.py): z, dW, db, dz rtol 1e-4 / atol 1e-5 (row reductions of up to 2048 terms
in another order), the loss rtol 1e-5 (+ atol 1e-7: C = 1 gives exactly 0), dx per row. The row
pass is the BCE head's, so z, xd and the norm are compared with it BIT FOR BIT, and so are the
evaluation head's loss and logits with the training head's.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gnn_amd import _lib

pytestmark = pytest.mark.gpu


def _ce_ref(x, W, b, y, mask=None, p=0.0):
    h = F.normalize(x, p=2, dim=1)
    if mask is not None:
        h = h * mask / (1 - p)
    z = F.linear(h, W, b)
    rows = torch.nn.CrossEntropyLoss(reduction="none")(z, y)
    return (rows / x.shape[0]).sum(), z


def _run_ce(x, ldx, M, D, W, b, C, y, ldl, p, seed, training, gl, dev, bce=False):
    """gnn_head_{ce,bce}_fwd_f32 then _bwd_f32 through ctypes; every output as a tensor."""
    n = max(M, 1)
    o = {"xd": torch.empty(n, D, device=dev), "z": torch.empty(n, C, device=dev), "nrm": torch.empty(n, device=dev),
         "lse": torch.empty(n, device=dev), "rl": torch.empty(n, device=dev), "loss": torch.empty((), device=dev),
         "dz": torch.empty(n, C, device=dev), "dx": torch.empty(n, D, device=dev)}
    g = torch.full((), float(gl), device=dev)
    L, st = _lib.lib(), _lib.stream_of(dev)
    fwd = [x.data_ptr(), ldx, M, D, W.data_ptr(), b.data_ptr(), C, y.data_ptr(), ldl, p, seed, training,
           o["xd"].data_ptr(), o["z"].data_ptr(), o["nrm"].data_ptr(), o["rl"].data_ptr(), o["loss"].data_ptr()]
    bwd = [x.data_ptr(), ldx, M, D, W.data_ptr(), C, y.data_ptr(), ldl, g.data_ptr(), p, seed, training,
           o["z"].data_ptr(), o["nrm"].data_ptr(), o["dz"].data_ptr(), o["dx"].data_ptr(), D]
    if bce:
        _lib.check(L.gnn_head_bce_fwd_f32(*fwd, st), "gnn_head_bce_fwd_f32")
        _lib.check(L.gnn_head_bce_bwd_f32(*bwd, st), "gnn_head_bce_bwd_f32")
    else:
        _lib.check(L.gnn_head_ce_fwd_f32(*fwd, o["lse"].data_ptr(), st), "gnn_head_ce_fwd_f32")
        _lib.check(L.gnn_head_ce_bwd_f32(*bwd, o["lse"].data_ptr(), st), "gnn_head_ce_bwd_f32")
    torch.cuda.synchronize()
    return o


def _inputs(M, D, C, seed, bias=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g)
    x[0] *= 1e-3
    if M > 3:
        x[3] = 0.0  # a zero row: the norm is clamped to 1e-12
    W = torch.randn(C, D, generator=g) * 0.1
    b = torch.randn(C, generator=g) if bias is None else bias
    y = F.one_hot(torch.randint(0, C, (M,), generator=g), C).float()
    if M > 1:
        y[1] = torch.rand(C, generator=g)  # soft targets: probabilities that need not sum to 1
    if M > 2:
        y[2] = 0.0  # an all-zero label row contributes 0
    return x, W, b, y


def _check_against_fp64(dev, M, D, C, x, W, b, y):
    from gnn_amd.fused import head_ce_loss

    leaves64 = [t.double().requires_grad_(True) for t in (x, W, b)]
    l64, z64 = _ce_ref(*leaves64, y.double())
    z64.retain_grad()
    (l64 * M).backward()  # dz is O(1)
    leaves = [t.to(dev).requires_grad_(True) for t in (x, W, b)]
    lo, z = head_ce_loss(*leaves, y.to(dev), p=0.1, training=False)
    (lo * M).backward()
    lo, l64 = lo.detach(), l64.detach()
    raw = _run_ce(leaves[0].detach(), D, M, D, leaves[1].detach(), leaves[2].detach(), C, y.to(dev), C, 0.1, 0, 0,
                  float(M), dev)
    assert torch.equal(raw["z"], z) and torch.equal(raw["loss"], lo)
    assert torch.equal(raw["dx"], leaves[0].grad)
    for t in (z, lo, raw["dz"], raw["lse"], *[a.grad for a in leaves]):
        assert bool(torch.isfinite(t).all())
    print(f"M={M} D={D} C={C} loss={float(lo):.9g} ref={float(l64):.9g} "
          f"z_err={float((z.cpu().double() - z64.detach()).abs().max()):.3g} "
          f"dz_err={float((raw['dz'].cpu().double() - z64.grad).abs().max()):.3g}")
    np.testing.assert_allclose(z.detach().cpu().numpy(), z64.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(lo), float(l64), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(raw["dz"].cpu().numpy(), z64.grad.numpy(), rtol=1e-4, atol=1e-5)
    for a, r in zip(leaves[1:], leaves64[1:]):
        np.testing.assert_allclose(a.grad.cpu().numpy(), r.grad.numpy(), rtol=1e-4, atol=1e-5)
    # d(x) = (d(xn) - xn (xn · d(xn))) / ||x||: the projection cancels, so the error scales with
    # the row's gradient magnitude — tolerance per row (tests/test_fused_gpu.py)
    got, ref = leaves[0].grad.cpu().double().numpy(), leaves64[0].grad.numpy()
    rowmax = np.abs(ref).max(axis=1, keepdims=True)
    assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-5 * np.maximum(rowmax, 1.0))
    return lo, l64


@pytest.mark.parametrize("M,D,C", [(512, 1024, 41), (37, 512, 41), (1, 64, 3), (100, 2048, 64), (5, 4, 1),
                                   (512, 1024, 172), (33, 2048, 256), (7, 512, 65)]
                         + [(130, D, C) for D in (1024, 1028) for C in (7, 8, 9, 64, 65)])
def test_head_ce_matches_torch(dev, M, D, C):
    """Eval mode against fp64 torch: the BCE head's shapes, plus the 8-class block edge, the
    64-lane slot edge and the masked last piece (D = 1028)."""
    lo, _ = _check_against_fp64(dev, M, D, C, *_inputs(M, D, C, M * 7 + D + C))
    if C == 1:
        assert float(lo) == 0.0


def test_head_ce_large_logits(dev):
    """Logits near ±200: the terms y_j (lse - z_j) are subtracted per class, so nothing cancels
    and nothing overflows."""
    M, D, C = 130, 1024, 41
    lo, l64 = _check_against_fp64(dev, M, D, C, *_inputs(M, D, C, 11, bias=torch.linspace(-200, 200, C)))
    assert float(l64) > 100.0  # the case is what it claims to be


def _strided_inputs(M, D, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    ldx, ldl = D + 4, C + 3
    xs = torch.randn(M, ldx, generator=g)
    xs[1] = 0.0
    W = torch.randn(C, D, generator=g)
    b = torch.randn(C, generator=g) * 0.5
    ys = torch.zeros(M, ldl)
    ys[:, :C] = F.one_hot(torch.randint(0, C, (M,), generator=g), C).float()
    return xs.to(dev), ldx, W.to(dev), b.to(dev), ys.to(dev), ldl


def _run_eval(fn_kind, x, ldx, M, D, W, b, C, y, ldl, mode, dev, width=None):
    """fn_kind None: gnn_head_eval_f32; else gnn_head_eval_loss_f32 with that kind. Outputs are
    poisoned with -7 and sized for `width` classes (default C)."""
    n, width = max(M, 1), C if width is None else width
    z = torch.full((n, width + 5), -7.0, device=dev)
    rl = torch.empty(n, device=dev)
    rm = torch.empty(n * 8, dtype=torch.int64, device=dev)
    lo = torch.full((), -7.0, device=dev)
    counts = torch.full((3, width), -7, dtype=torch.int32, device=dev)
    L = _lib.lib()
    args = [x.data_ptr(), ldx, M, D, W.data_ptr(), b.data_ptr(), C, y.data_ptr(), ldl, z.data_ptr(), width + 5,
            rl.data_ptr(), rm.data_ptr(), lo.data_ptr(), counts.data_ptr(), mode]
    if fn_kind is None:
        rc = L.gnn_head_eval_f32(*args, _lib.stream_of(dev))
    else:
        rc = L.gnn_head_eval_loss_f32(*args, fn_kind, _lib.stream_of(dev))
    torch.cuda.synchronize()
    return rc, z, lo, counts


@pytest.mark.parametrize("D,C", [(4, 1), (1024, 41), (1028, 65), (2048, 256)])
def test_head_ce_bit_identities(dev, D, C):
    M = 130
    x, ldx, W, b, y, ldl = _strided_inputs(M, D, C, dev, 1000 * D + C)
    for training in (0, 1):
        ce = _run_ce(x, ldx, M, D, W, b, C, y, ldl, 0.1, 99, training, 1.0, dev)
        bce = _run_ce(x, ldx, M, D, W, b, C, y, ldl, 0.1, 99, training, 1.0, dev, bce=True)
        for k in ("z", "xd", "nrm"):
            assert torch.equal(ce[k], bce[k]), (training, k)
        if training and D >= 1024:  # dropout was on (row 1 is the all-zero row)
            assert abs(float((ce["xd"][2:] != 0).float().mean()) - 0.9) < 0.01
        if C > 1:
            assert not torch.equal(ce["loss"], bce["loss"]) and not torch.equal(ce["dz"], bce["dz"])
        if training == 0:
            ce0 = ce
    for mode in (0, 1):
        rc1, z1, lo1, cn1 = _run_eval(1, x, ldx, M, D, W, b, C, y, ldl, mode, dev)
        rc0, z0, lo0, cn0 = _run_eval(0, x, ldx, M, D, W, b, C, y, ldl, mode, dev)
        rcp, zp, lop, cnp = _run_eval(None, x, ldx, M, D, W, b, C, y, ldl, mode, dev)
        assert rc1 == 0 and rc0 == 0 and rcp == 0, _lib.lib().gnn_last_error()
        assert torch.equal(lo1, ce0["loss"]), (mode, float(lo1), float(ce0["loss"]))
        assert torch.equal(z1[:, :C], ce0["z"]) and torch.all(z1[:, C:] == -7.0)
        assert torch.equal(cn1, cn0) and int(cn1[0].sum() + cn1[2].sum()) > 0
        assert torch.equal(z0, zp) and torch.equal(lo0, lop) and torch.equal(cn0, cnp)


def test_head_ce_dropout(dev):
    """Training mode (as test_head_bce_dropout): the mask the forward drew, read back from the
    stored dropout output, reproduces the loss under torch autograd, and the backward regenerates
    the same mask."""
    M, D, C, p = 512, 1024, 41, 0.1
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, D, generator=g).to(dev)
    W = (torch.randn(C, D, generator=g) * 0.1).to(dev)
    b = torch.randn(C, generator=g).to(dev)
    y = F.one_hot(torch.randint(0, C, (M,), generator=g), C).float().to(dev)
    o = _run_ce(x, D, M, D, W, b, C, y, C, p, 1234, 1, 2.0, dev)
    mask = (o["xd"] != 0).float()
    assert abs(mask.mean().item() - (1 - p)) < 0.005
    xr = x.clone().requires_grad_(True)
    lr, zr = _ce_ref(xr, W, b, y, mask, p)
    (2.0 * lr).backward()
    torch.testing.assert_close(o["xd"], F.normalize(x, dim=1) * mask / (1 - p), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(o["z"], zr, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(o["loss"], lr.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(o["dx"], xr.grad, rtol=1e-4, atol=1e-6)


def test_head_ce_validation_and_empty_batch(dev):
    L, st = _lib.lib(), _lib.stream_of(dev)
    x, W = torch.zeros(3, 2056, device=dev), torch.zeros(300 * 2056, device=dev)
    b, y = torch.zeros(300, device=dev), torch.zeros(3, 300, device=dev)

    def poisoned():
        return {k: torch.full(s, -7.0, device=dev) for k, s in
                (("xd", (3, 2056)), ("z", (3, 300)), ("nrm", (3,)), ("rl", (3,)), ("loss", ()), ("lse", (3,)),
                 ("dz", (3, 300)), ("dx", (3, 2056)))}

    for D, C in ((1022, 9), (2052, 9), (1024, 257), (1024, 0)):
        o = poisoned()
        rc = L.gnn_head_ce_fwd_f32(x.data_ptr(), 2056, 3, D, W.data_ptr(), b.data_ptr(), C, y.data_ptr(), 300, 0.1, 1, 0,
                                   o["xd"].data_ptr(), o["z"].data_ptr(), o["nrm"].data_ptr(), o["rl"].data_ptr(),
                                   o["loss"].data_ptr(), o["lse"].data_ptr(), st)
        assert rc != 0 and b"gnn_head_ce_fwd_f32" in L.gnn_last_error(), (D, C)
        rc = L.gnn_head_ce_bwd_f32(x.data_ptr(), 2056, 3, D, W.data_ptr(), C, y.data_ptr(), 300, None, 0.1, 1, 0,
                                   o["z"].data_ptr(), o["nrm"].data_ptr(), o["dz"].data_ptr(), o["dx"].data_ptr(), 2056,
                                   o["lse"].data_ptr(), st)
        assert rc != 0 and b"gnn_head_ce_bwd_f32" in L.gnn_last_error(), (D, C)
        rc, z, lo, counts = _run_eval(1, x, 2056, 3, D, W, b, C, y, 300, 0, dev, width=300)
        assert rc != 0 and L.gnn_last_error(), (D, C)
        torch.cuda.synchronize()
        assert all(bool(torch.all(t == -7.0)) for t in o.values()), (D, C)
        assert float(lo) == -7.0 and torch.all(counts == -7) and torch.all(z == -7.0), (D, C)
    # an unknown loss kind: a status and an error text, nothing launched
    for kind in (2, -1):
        rc, z, lo, counts = _run_eval(kind, x, 2056, 3, 1024, W, b, 9, y, 300, 1, dev)
        assert rc != 0 and b"loss kind" in L.gnn_last_error()
        assert float(lo) == -7.0 and torch.all(counts == -7) and torch.all(z == -7.0)
    # M = 0: no row pass, a zero loss
    o = poisoned()
    rc = L.gnn_head_ce_fwd_f32(x.data_ptr(), 2056, 0, 1024, W.data_ptr(), b.data_ptr(), 9, y.data_ptr(), 300, 0.1, 1, 0,
                               o["xd"].data_ptr(), o["z"].data_ptr(), o["nrm"].data_ptr(), o["rl"].data_ptr(),
                               o["loss"].data_ptr(), o["lse"].data_ptr(), st)
    assert rc == 0
    assert L.gnn_head_ce_bwd_f32(x.data_ptr(), 2056, 0, 1024, W.data_ptr(), 9, y.data_ptr(), 300, None, 0.1, 1, 0,
                                 o["z"].data_ptr(), o["nrm"].data_ptr(), o["dz"].data_ptr(), o["dx"].data_ptr(), 2056,
                                 o["lse"].data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert float(o["loss"]) == 0.0
    assert all(bool(torch.all(o[k] == -7.0)) for k in ("xd", "z", "nrm", "lse", "dz", "dx"))
    rc, z, lo, counts = _run_eval(1, x, 2056, 0, 1024, W, b, 9, y, 300, 1, dev)
    assert rc == 0 and float(lo) == 0.0 and torch.all(counts == 0) and torch.all(z == -7.0)
