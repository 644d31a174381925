"""GPU: gnn_head_bias_grad_f32, the fixed-order column sum that both the native step and the Python
fused path's head backward use for the bias gradient (include/gnn_layers.h)."""
import pytest
import torch

from gnn_amd import _lib, fused

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M,C", [(512, 41), (1, 1), (257, 3), (1000, 256), (0, 7)])
def test_head_bias_grad_is_the_column_sum(dev, M, C):
    """Against fp64: a sum of M fp32 terms in any order is within M · 2^-24 · Σ|dz| of the exact
    one. Deterministic (fixed order), and M = 0 writes zeros."""
    g = torch.Generator().manual_seed(M + C)
    dz = torch.randn(M, C, generator=g).to(dev)
    db = fused._head_bias_grad(dz)
    again = fused._head_bias_grad(dz)
    torch.cuda.synchronize()
    assert db.shape == (C,) and torch.equal(db, again)
    ref = dz.double().sum(0)
    bound = M * 2.0 ** -24 * dz.double().abs().sum(0) + 1e-30
    assert bool(((db.double() - ref).abs() <= bound).all())
    if M == 0:
        assert not bool(db.any())


def test_head_bias_grad_rejects_bad_sizes():
    L = _lib.lib()
    assert L.gnn_head_bias_grad_f32(None, -1, 4, None, None) == -22
    assert L.gnn_head_bias_grad_f32(None, 4, 0, None, None) == 0  # no class: nothing launched
