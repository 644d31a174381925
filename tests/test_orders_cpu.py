"""Order-0 (dense) layers in the step descriptor (GNN_SL_DENSE, include/gnn_step.h), host side: the
workspace queries of gnn_train_step_f32 / gnn_eval_step_f32 validate the slot and the shapes of an
order-0 layer, plan no aggregation buffer for it, and leave every descriptor with the slot at 0
exactly as it was (no GPU: the queries launch nothing).
"""
import numpy as np
import pytest

from gnn_amd import _lib, executor

SAGE, GCN = executor.SAGE, executor.GCN
# (M, K, nnz) per layer; layers 1 and 3 are square so that they may be order 0 with the same shapes
DIMS = [(300, 900, 9000), (300, 300, 3000), (64, 300, 1500), (64, 64, 600)]
# gnn_train_step_workspace_bytes / gnn_eval_step_workspace_bytes of _desc([1,1,1,1]) as the library
# gave them before GNN_SL_DENSE had a meaning (recorded from a build of the parent commit)
PARENT_BYTES = {SAGE: (1196544, 456448), GCN: (640000, 321792)}


def _desc(orders, kind=SAGE, dims=DIMS, F=37, ldx=64, nhid=16, bare=False):
    """A descriptor the workspace queries accept: shapes and (fake, aligned) pointers only.
    bare: an order-0 layer's ignored slots (operand sizes, sampled count) left 0."""
    nl = len(orders)
    d = np.zeros(executor.HEADER + executor.LAYER_SLOTS * nl, np.int64)
    d[executor.H_VERSION], d[executor.H_LAYERS], d[executor.H_KIND] = executor.VERSION, nl, kind
    d[executor.H_X0], d[executor.H_LDX0], d[executor.H_F0] = 4096, ldx, F
    d[executor.H_CLASSES], d[executor.H_NHID] = 7, nhid
    for li, ((M, K, nnz), o) in enumerate(zip(dims, orders)):
        b = executor.HEADER + li * executor.LAYER_SLOTS
        d[b + executor.L_M], d[b + executor.L_K] = M, K
        d[b + executor.L_DENSE] = int(o == 0)
        if o or not bare:
            d[b + executor.L_NNZ], d[b + executor.L_NSAMPLED] = nnz, M
    return d


def _sizes(d):
    L = _lib.lib()
    return L.gnn_train_step_workspace_bytes(d.ctypes.data), L.gnn_eval_step_workspace_bytes(d.ctypes.data)


def test_slot_number():
    assert executor.L_DENSE == 26 and executor.LAYER_SLOTS == 32 and executor.VERSION == 1


@pytest.mark.parametrize("kind", [SAGE, GCN])
def test_bad_dense_flag_is_refused(kind):
    L = _lib.lib()
    for bad in (2, -1, 7):
        d = _desc([1, 1, 1, 1], kind)
        d[executor.HEADER + 2 * executor.LAYER_SLOTS + executor.L_DENSE] = bad
        assert _sizes(d) == (0, 0), bad
        assert b"layer 2" in L.gnn_last_error() and b"dense" in L.gnn_last_error()


@pytest.mark.parametrize("kind", [SAGE, GCN])
def test_order_zero_layer_shapes_are_checked(kind):
    L = _lib.lib()
    assert all(b > 0 for b in _sizes(_desc([1, 0, 1, 0], kind)))
    # K != M
    dims = list(DIMS)
    dims[1] = (300, 200, 0)
    assert _sizes(_desc([1, 0, 1, 0], kind, dims)) == (0, 0)
    assert b"layer 1" in L.gnn_last_error()
    # M != M_{l-1} (with K = M, so only the chain is wrong)
    dims[1] = (200, 200, 0)
    dims[2] = (64, 200, 1500)
    assert _sizes(_desc([1, 0, 1, 0], kind, dims)) == (0, 0)
    assert b"layer 1" in L.gnn_last_error()
    # an order-0 layer 0: K = M = the rows of x0
    assert all(b > 0 for b in _sizes(_desc([0, 1], kind, [(900, 900, 0), (64, 900, 1500)])))
    assert _sizes(_desc([0, 1], kind, [(900, 800, 0), (64, 900, 1500)])) == (0, 0)
    # the ignored slots of an order-0 layer (operand sizes, sampled count) may be 0 or anything
    assert _sizes(_desc([1, 0, 1, 0], kind, bare=True)) == _sizes(_desc([1, 0, 1, 0], kind))


@pytest.mark.parametrize("kind", [SAGE, GCN])
def test_workspace_shrinks_without_the_aggregation_buffers(kind):
    full = _sizes(_desc([1, 1, 1, 1], kind))
    mixed = _sizes(_desc([1, 0, 1, 0], kind))
    assert 0 < mixed[0] < full[0], (mixed, full)
    assert 0 < mixed[1] <= full[1], (mixed, full)
    for orders, dims in (([1, 0, 1, 0], DIMS), ([0, 1], [(900, 900, 0), (64, 900, 1500)]), ([0], [(900, 900, 0)])):
        tr, ev = _sizes(_desc(orders, kind, dims))
        assert 0 < ev < tr, (orders, ev, tr)
    # a 16-bit X0 under an order-0 layer 0: widened once into the workspace, so the training plan
    # grows by exactly those rows (900 rows of 64 floats) over the fp32 plan's
    d = _desc([0, 1], kind, [(900, 900, 0), (64, 900, 1500)])
    f32 = _sizes(d)
    d[executor.HEADER + executor.L_XKIND] = 1
    h16 = _sizes(d)
    assert h16[0] == f32[0] + 900 * 64 * 4 and f32[1] < h16[1] < h16[0]


@pytest.mark.parametrize("kind", [SAGE, GCN])
def test_aggregating_descriptors_keep_their_bytes(kind):
    """Slot 26 = 0 is every descriptor built before the slot had a meaning: the same plan."""
    assert _sizes(_desc([1, 1, 1, 1], kind)) == PARENT_BYTES[kind]
