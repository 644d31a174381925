"""Layer 0 aggregating from 16-bit feature rows, host side (no GPU): the 16-bit SpMM call's launch
geometry against the fp32 call's, its argument refusals, the step descriptor's input-kind slot, the
staging call's X0 kind, and FeatureStore(keep16=...).

The geometry matters because the summation order of an output depends on it (lane groups per row,
unit size, row / unit kernel, waves per row): equal geometry is what makes gnn_spmm_csr_h16_f32
bit-identical to gnn_spmm_csr_f32 on the widened rows (tests/test_agg16_gpu.py checks the bits).
"""
import ctypes

import numpy as np
import pytest
import torch

from gnn_amd import _lib, executor, loader, staging

from test_feat16_cpu import _loaders, world  # noqa: F401  (the module-scoped world fixture and its loaders)

X, Y = 256, 512  # 16-byte-aligned dummy pointers (the config queries read nothing)


def _cfg32(M, K, nnz, F, ldx, ldy, unit=0):
    out = (ctypes.c_int32 * 6)()
    _lib.check(_lib.lib().gnn_spmm_config(M, K, nnz, F, ldx, ldy, X, Y, unit, out), "gnn_spmm_config")
    name = ctypes.create_string_buffer(128)
    _lib.check(_lib.lib().gnn_spmm_kernel_name(M, K, nnz, F, ldx, ldy, X, Y, unit, 0, name, 128), "kernel_name")
    return list(out), name.value.decode()


def _cfg16(M, K, nnz, F, ldx, ldy, unit=0, x=X):
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().gnn_spmm_h16_config(M, K, nnz, F, ldx, ldy, x, Y, unit, out), "gnn_spmm_h16_config")
    return list(out)


def _wpr_of(kernel_name: str) -> int:
    """spmm_row_kernel<VW, NJ, U, WPR, RES> -> WPR; the unit kernel -> 0."""
    if not kernel_name.startswith("spmm_row_kernel"):
        return 0
    return int(kernel_name.split("<")[1].split(",")[3])


# (M, K, nnz): the config-2 layer shapes of DESIGN (layer 0 / 1 / 2 forward, layer 1 / 2 backward),
# the shapes of tests/test_spmm_gpu.py::test_row_kernel (nnz = M * mean), and K small and large
# around the L2-tile branch (nnz >= 8 K or not)
SHAPES = [(15768, 22153, 1821171), (8680, 15768, 868338), (15768, 8680, 868338), (512, 8680, 14876),
          (8680, 512, 14876),
          (512, 8684, 512 * 29), (8684, 512, 8684 * 2), (300, 700, 300 * 30), (257, 300, 257 * 12), (64, 90, 64 * 20),
          (4000, 100, 400000), (4000, 50000, 400000), (4000, 50001, 400000), (100, 1000, 2000)]
WIDTHS = [4, 64, 100, 512, 604, 1024, 2100]


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_h16_geometry_is_the_fp32_calls(monkeypatch, shape, F):
    for k in ("GNN_SPMM_G", "GNN_SPMM_NJ", "GNN_SPMM_VW", "GNN_SPMM_ROWK", "GNN_SPMM_ROWK_WPR", "GNN_SPMM_SMALL_U16"):
        monkeypatch.delenv(k, raising=False)
    M, K, nnz = shape
    for ldx in (F, (F + 63) // 64 * 64):
        for unit in (0, 64):
            c32, name = _cfg32(M, K, nnz, F, ldx, F, unit)
            c16 = _cfg16(M, K, nnz, F, ldx, F, unit)
            assert c32[0] == 4, "the fp32 reference call must be the 4-wide one"
            assert c16[:6] == c32, (shape, F, ldx, unit)
            assert c16[6] == _wpr_of(name), (name, c16)
            assert c16[7] == 4
            # X only 8-byte aligned (what the 16-bit call asks for): still the 4-wide geometry
            assert _cfg16(M, K, nnz, F, ldx, F, unit, x=264) == c16


@pytest.mark.parametrize("env", [{"GNN_SPMM_ROWK": "1"}, {"GNN_SPMM_ROWK": "1", "GNN_SPMM_ROWK_WPR": "4"},
                                 {"GNN_SPMM_ROWK": "1", "GNN_SPMM_ROWK_WPR": "8"}, {"GNN_SPMM_ROWK": "0"},
                                 {"GNN_SPMM_SMALL_U16": "0"}])
def test_h16_geometry_follows_the_experiment_switches(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for M, K, nnz in SHAPES[3:10]:
        c32, name = _cfg32(M, K, nnz, 1024, 1024, 1024)
        c16 = _cfg16(M, K, nnz, 1024, 1024, 1024)
        assert c16[:6] == c32 and c16[6] == _wpr_of(name), (env, M, K, nnz, name, c16)


def test_h16_workspace_is_the_fp32_calls():
    """One workspace query serves both calls: it depends on (M, nnz, F, unit) alone."""
    L = _lib.lib()
    for M, K, nnz in SHAPES:
        for F in (64, 604):
            c16 = _cfg16(M, K, nnz, F, F, F)
            assert L.gnn_spmm_workspace_bytes(M, nnz, F, 0) >= c16[5] * 2 * F * 4


def _h16(L, *, M=4, K=4, nnz=0, X=264, ldx=8, kind=1, Y=512, ldy=8, F=8):
    return L.gnn_spmm_csr_h16_f32(None, None, None, M, K, nnz, X, ldx, kind, Y, ldy, F, None, 0, 0, None)


def test_h16_argument_refusals_without_gpu():
    """Every refusal of include/gnn_spmm.h, with its message, before any HIP call (no device here)."""
    L = _lib.lib()
    for kind in (0, 3, -1):
        assert _h16(L, kind=kind) == -22 and b"kind" in L.gnn_last_error()
    assert _h16(L, X=266) == -22 and b"8-byte" in L.gnn_last_error()  # 2-byte aligned only
    assert _h16(L, X=260) == -22 and b"8-byte" in L.gnn_last_error()  # 4-byte aligned only
    assert _h16(L, ldx=10) == -22 and b"multiples of 4" in L.gnn_last_error()
    assert _h16(L, F=6) == -22 and b"multiples of 4" in L.gnn_last_error()
    assert _h16(L, ldy=10) == -22 and b"multiples of 4" in L.gnn_last_error()
    assert _h16(L, Y=520) == -22 and b"16-byte" in L.gnn_last_error()  # 8-byte aligned only
    assert _h16(L, F=12) == -22 and b"ldx" in L.gnn_last_error()
    assert _h16(L, F=12, ldx=12) == -22 and b"ldy" in L.gnn_last_error()
    assert _h16(L, M=-1) == -22 and b"negative" in L.gnn_last_error()
    # an empty problem with good arguments is a no-op, as in the fp32 call
    assert _h16(L, M=0) == 0
    assert _h16(L, F=0) == 0
    out = (ctypes.c_int32 * 8)()
    assert L.gnn_spmm_h16_config(4, 4, 4, 8, 8, 8, X, Y, 0, None) == -22


# ---- step descriptor -----------------------------------------------------------------------
def _desc(xkind0=0, xkind1=0, F=37, ldx=64, kind=executor.SAGE, nl=2):
    """A descriptor gnn_*_step_workspace_bytes accepts: shapes and (fake, aligned) pointers only."""
    d = np.zeros(executor.HEADER + executor.LAYER_SLOTS * nl, np.int64)
    d[executor.H_VERSION], d[executor.H_LAYERS], d[executor.H_KIND] = executor.VERSION, nl, kind
    d[executor.H_X0], d[executor.H_LDX0], d[executor.H_F0] = 4096, ldx, F
    d[executor.H_CLASSES], d[executor.H_NHID] = 7, 16
    dims = [(300, 900, 9000), (64, 300, 1500)]
    for li, (M, K, nnz) in enumerate(dims[:nl]):
        b = executor.HEADER + li * executor.LAYER_SLOTS
        d[b + executor.L_M], d[b + executor.L_K], d[b + executor.L_NNZ] = M, K, nnz
        d[b + executor.L_NSAMPLED] = M
    d[executor.HEADER + executor.L_XKIND] = xkind0
    if nl > 1:
        d[executor.HEADER + executor.LAYER_SLOTS + executor.L_XKIND] = xkind1
    return d


@pytest.mark.parametrize("kind", [executor.SAGE, executor.GCN])
def test_step_descriptor_input_kind(kind):
    L = _lib.lib()
    sizes = (L.gnn_train_step_workspace_bytes, L.gnn_eval_step_workspace_bytes)
    base = [fn(_desc(kind=kind).ctypes.data) for fn in sizes]
    assert all(b > 0 for b in base)
    for xk in (1, 2):
        # the same descriptor with only the slot flipped (F = 37 in 64-element rows: the padded
        # output rows are 64 floats either way), and ...
        assert [fn(_desc(xkind0=xk, kind=kind).ctypes.data) for fn in sizes] == base
    # ... a store's pair: an fp32 X0 has F rounded up to 32 floats a row, the 16-bit X0 of the same
    # table F rounded up to 64 elements; the step's workspace does not grow
    for F in (30, 37, 602):
        f32 = [fn(_desc(F=F, ldx=staging.padded_ld(F), kind=kind).ctypes.data) for fn in sizes]
        h16 = [fn(_desc(xkind0=1, F=F, ldx=staging.padded_ld(F, 64), kind=kind).ctypes.data) for fn in sizes]
        assert f32 == h16 and all(b > 0 for b in f32), F
    for bad in (dict(xkind0=3), dict(xkind0=-1), dict(xkind1=1), dict(xkind0=1, xkind1=2)):
        for fn in sizes:
            assert fn(_desc(kind=kind, **bad).ctypes.data) == 0, bad
            assert b"input kind" in L.gnn_last_error()
    # 16-bit rows the 4-element loads cannot read are refused too: an odd stride, no room for the pad
    for bad in (dict(ldx=66), dict(F=37, ldx=38)):
        for fn in sizes:
            assert fn(_desc(xkind0=1, **bad).ctypes.data) == 0, bad
    assert executor.L_XKIND == 25 and executor.VERSION == 1


# ---- staging -------------------------------------------------------------------------------
def test_stage_x0_kind_validation_without_gpu(world):  # noqa: F811
    """gnn_stage_plan / gnn_stage_batch_f32: an X0 kind that is neither 0 nor the feature kind is
    refused with a message before any HIP call; 0 and the store's kind plan alike."""
    L = _lib.lib()
    for tab, blob_kind in ((world[2].half(), 1), (world[2].bfloat16(), 2), (world[2], 0)):
        a_, b, _ = _loaders(world, tab)
        try:
            nb = next(iter(b.epoch(1))).host
            a = np.zeros(loader.STAGE_SLOTS, np.int64)
            a[loader.ST_DESC], a[loader.ST_HOST_BLOB] = nb.desc.ctypes.data, nb.ptr
            a[loader.ST_NUM_NODES], a[loader.ST_CSC_FROM], a[loader.ST_UPLOAD] = world[0].shape[0], 1, 1
            a[loader.ST_FEAT_KIND] = blob_kind
            out = np.zeros(loader.BLOB_MAX_LAYERS * loader.STAGE_OUT_SLOTS, np.int64)
            plain = L.gnn_stage_plan(a.ctypes.data, out.ctypes.data)
            assert plain > 0
            a[loader.ST_X0_KIND] = blob_kind
            assert L.gnn_stage_plan(a.ctypes.data, out.ctypes.data) == plain
            for bad in (k for k in (1, 2, 3, -1) if k != blob_kind):
                a[loader.ST_X0_KIND] = bad
                assert L.gnn_stage_plan(a.ctypes.data, out.ctypes.data) == 0
                assert b"X0 kind" in L.gnn_last_error()
                with pytest.raises(RuntimeError, match="X0 kind"):
                    _lib.check(L.gnn_stage_batch_f32(a.ctypes.data, None), "gnn_stage_batch_f32")
        finally:
            a_.close()
            b.close()
    assert loader.ST_X0_KIND == 22


def test_feature_store_keep16(world):  # noqa: F811
    _, _, feats, _, pl = world
    nodes = pl.gpu_buffer_group[0]
    with pytest.raises(ValueError, match="keep16"):
        staging.FeatureStore(feats, nodes, "cpu", 0, keep16=True)
    assert staging.FeatureStore(feats, nodes, "cpu", 0).keep16 is False
    for dtype, kind in ((torch.float16, 1), (torch.bfloat16, 2)):
        tab = feats.to(dtype)
        plain = staging.FeatureStore(tab, nodes, "cpu", 0)
        kept = staging.FeatureStore(tab, nodes, "cpu", 0, keep16=True)
        assert plain.keep16 is False and kept.keep16 is True
        for f in ("dtype", "kind", "F", "ld", "ld_rows", "zero_copy"):
            assert getattr(kept, f) == getattr(plain, f), f
        assert kept.kind == kind and kept.ld_rows == 64 and kept.ld == staging.padded_ld(feats.shape[1])
        assert kept.gpu_buffer.dtype == dtype and torch.equal(kept.gpu_buffer.view(torch.int16),
                                                              plain.gpu_buffer.view(torch.int16))
        # whole-word rows: what lets the fp32 gathers copy them
        w = staging.word_rows(kept.gpu_buffer)
        assert w.dtype == torch.float32 and tuple(w.shape) == (len(nodes), 32)
    with pytest.raises(RuntimeError, match="whole words"):
        staging.word_rows(torch.zeros(4, 7, dtype=torch.float16))


def test_models_accept_16bit_x_on_cpu():
    """The plain modules' layer 0 with a 16-bit x (the Trainer's fall-back path): the aggregation
    takes it, x[sampled] is widened, and the output equals the fp32 run's."""
    from gnn_amd.models import build_model

    torch.manual_seed(0)
    x16 = (torch.randn(12, 10) * 2).half()
    idx = torch.tensor([[0, 1, 2, 3, 3], [1, 5, 7, 0, 11]])
    adj = torch.sparse_coo_tensor(idx, torch.tensor([0.5, 1.0, 0.25, 2.0, 1.5]), (4, 12)).coalesce()
    sampled = torch.tensor([0, 3, 5, 9])
    for name in ("graphsage", "gcn"):
        net = build_model(name, 10, 8, [1], 3, dropout=0.0).eval()
        with torch.no_grad():
            assert torch.equal(net(x16, [adj], [sampled]), net(x16.float(), [adj], [sampled]))
