"""16-bit (fp16 / bf16) feature stores, host side: the 2-byte host row gather, the blob's 16-bit
host_rows section from both producers (header slots GNN_H_FEAT_KIND / GNN_H_LD_HOST_ROWS),
FeatureStore's dtype checks, and the staging call's kind validation. No GPU.

Every comparison is on bit patterns (int16 / byte views): the host side never converts.
"""
import numpy as np
import pytest
import torch

from gnn_amd import _lib, graphs, loader, placement, staging

F = 37


def _bits(t: torch.Tensor) -> np.ndarray:
    """The 16-bit patterns of an fp16 / bf16 tensor."""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _gather_b16(src: np.ndarray, idx, ld_dst: int, sentinel: int = 0xDEAD):
    L = _lib.sampler_lib()
    idx = np.asarray(idx, np.int64)
    dst = np.full((len(idx), ld_dst), sentinel, np.uint16)
    rc = L.gnn_host_gather_rows_b16(src.ctypes.data, src.shape[1], src.shape[0], idx.ctypes.data, len(idx),
                                    src.shape[1], dst.ctypes.data, ld_dst)
    return rc, dst


def test_host_gather_rows_b16():
    src = np.arange(50 * 7, dtype=np.uint16).reshape(50, 7) * 131 + 7  # distinct, both bytes in use
    idx = [3, 0, 49, 3]
    rc, dst = _gather_b16(src, idx, 8)
    assert rc == 0
    assert np.array_equal(dst[:, :7], src[idx]) and np.all(dst[:, 7] == 0)
    rc, dst = _gather_b16(src, [50], 8)
    assert rc != 0 and b"out of range" in _lib.sampler_lib().gnn_sampler_last_error()
    assert np.all(dst == 0xDEAD)  # refused before anything was written
    rc, _ = _gather_b16(src, [-1], 8)
    assert rc != 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_host_gather_rows_b16_float_patterns(dtype):
    table = (torch.randn(50, 7, generator=torch.Generator().manual_seed(5)) * 50).to(dtype)
    src = _bits(table)
    idx = [3, 0, 49, 3]
    rc, dst = _gather_b16(src, idx, 8)
    assert rc == 0
    assert np.array_equal(dst[:, :7], src[idx]) and np.all(dst[:, 7] == 0)
    assert _gather_b16(src, [50], 8)[0] != 0


def _setup():
    rng = np.random.default_rng(2)
    A = graphs.chung_lu(12_000, 90_000, 1.3, rng)
    lap = graphs.lap_matrix(A, "graphsage")
    N = A.shape[0]
    import scipy.sparse as sp

    cls = rng.integers(0, 7, N)
    labels = sp.csr_matrix((np.ones(N, np.int32), (np.arange(N), cls)), shape=(N, 7))
    feats = torch.randn(N, F, generator=torch.Generator().manual_seed(0))
    train = np.arange(0, 8000)
    pl = placement.create_buffer(lap, train, 1500, [0], 2, alpha=0)
    return lap, labels, feats, train, pl


@pytest.fixture(scope="module")
def world():
    return _setup()


def _loaders(world, feats):
    lap, labels, _, train, pl = world
    dev_of, idx_on = pl.device_id_of_nodes_group[0], pl.idx_of_nodes_on_device_group[0]
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], "cpu", 0)
    kw = dict(store=store, workers=3, seed=9)
    a = loader.BatchLoader(lap, labels, train, 400, 96, [1, 1, 1], dev_of, idx_on, **kw)
    b = loader.NativeLoader(lap, labels, train, 400, 96, [1, 1, 1], dev_of, idx_on, **kw)
    return a, b, store


def test_store_layout_16bit(world):
    _, _, feats, _, pl = world
    for dtype, kind in ((torch.float16, 1), (torch.bfloat16, 2)):
        tab = feats.to(dtype)
        store = staging.FeatureStore(tab, pl.gpu_buffer_group[0], "cpu", 0)
        assert store.dtype == dtype and store.kind == kind
        assert store.ld == staging.padded_ld(F) and store.ld_rows == 64 and store.ld_rows >= store.ld
        buf = store.gpu_buffer
        assert buf.dtype == dtype and tuple(buf.shape) == (len(pl.gpu_buffer_group[0]), 64)
        nodes = torch.from_numpy(np.asarray(pl.gpu_buffer_group[0], np.int64))
        assert np.array_equal(_bits(buf[:, :F]), _bits(tab[nodes])) and not _bits(buf[:, F:]).any()
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], "cpu", 0)
    assert store.dtype == torch.float32 and store.kind == 0 and store.ld_rows == store.ld
    assert store.gpu_buffer.dtype == torch.float32 and store.gpu_buffer.shape[1] == store.ld


def test_loaders_fp16_host_rows(world):
    """Both producers, fp16 store: host_rows is feats[host_src] bit for bit in ld_rows-wide rows
    with zero pads, the header names the kind and the stride, and the plans agree."""
    tab = world[2].half()
    a, b, store = _loaders(world, tab)
    src_bits = _bits(tab)
    n_host = 0
    try:
        for pa, pb in zip(a.epoch(1), b.epoch(1)):
            ha, hb = pa.host, pb.host
            qa, qb = pa.plan, pb.plan
            assert np.array_equal(np.asarray(ha.input_nodes), np.asarray(hb.input_nodes))
            for k in ("own_pos", "own_src", "host_pos"):
                assert np.array_equal(getattr(qa, k), getattr(qb, k)), k
            host_src = np.asarray(hb.nodes_idx_on_cpu, np.int64)
            assert np.array_equal(np.asarray(ha.nodes_idx_on_cpu, np.int64), host_src)
            assert int(hb.desc[loader.H_FEAT_KIND]) == 1 and int(hb.desc[loader.H_LD_HOST_ROWS]) == store.ld_rows == 64
            assert int(hb.desc[loader.H_LD_X0]) == store.ld and int(hb.desc[loader.H_VERSION]) == loader.BLOB_VERSION
            slot = hb._bb + loader.B_HOST_ROWS
            assert hb._count(slot) == len(host_src) * 64
            rows_b = hb._h(slot, np.dtype(np.uint16)).reshape(-1, 64)
            assert qa.host_rows.dtype == torch.float16 and tuple(qa.host_rows.shape) == (len(host_src), 64)
            rows_a = _bits(qa.host_rows)
            for rows in (rows_a, rows_b):
                assert np.array_equal(rows[:, :F], src_bits[host_src]) and not rows[:, F:].any()
            n_host += len(host_src)
    finally:
        a.close()
        b.close()
    assert n_host > 0  # the placement leaves rows on the host: the section was exercised


def test_loaders_fp32_blob_unchanged(world):
    """fp32 store: the two new header slots stay 0 and host_rows is feats[host_src], fp32, ld wide."""
    feats = world[2]
    a, b, store = _loaders(world, feats)
    try:
        for _, pb in zip(range(3), b.epoch(1)):
            hb = pb.host
            assert int(hb.desc[loader.H_FEAT_KIND]) == 0 and int(hb.desc[loader.H_LD_HOST_ROWS]) == 0
            host_src = torch.from_numpy(np.asarray(hb.nodes_idx_on_cpu, np.int64))
            want = torch.zeros((len(host_src), store.ld))
            want[:, :F] = feats[host_src]
            slot = hb._bb + loader.B_HOST_ROWS
            assert hb._count(slot) == want.numel()
            got = hb.blob[int(hb.desc[slot]):int(hb.desc[slot]) + want.numel() * 4]
            assert got.tobytes() == want.numpy().tobytes()
    finally:
        a.close()
        b.close()


def test_set_feat_b16_contract(world):
    """The setter refuses a bad kind, strides below F, a loader that has an fp32 table, and any
    call after the first submit."""
    lap, labels, feats, train, pl = world
    dev_of, idx_on = pl.device_id_of_nodes_group[0], pl.idx_of_nodes_on_device_group[0]
    L = _lib.sampler_lib()
    tab = feats.half()
    h16 = staging.FeatureStore(tab, pl.gpu_buffer_group[0], "cpu", 0)
    b = loader.NativeLoader(lap, labels, train, 100, 16, [1, 1], dev_of, idx_on, store=h16, workers=1)
    try:
        p = tab.data_ptr()
        assert L.gnn_loader_set_feat_b16(b.handle, p, F, F, 64, 3) == -22
        assert L.gnn_loader_set_feat_b16(b.handle, p, F, F, 64, 0) == -22
        assert L.gnn_loader_set_feat_b16(b.handle, p, F - 1, F, 64, 1) == -22
        assert L.gnn_loader_set_feat_b16(b.handle, p, F, F, h16.ld - 8, 1) == -22  # below ld_x0
        assert L.gnn_loader_set_feat_b16(b.handle, None, F, F, 64, 1) == -22
        assert L.gnn_loader_set_feat_b16(b.handle, p, F, F, 64, 1) == 0
        next(iter(b.epoch(1)))
        assert L.gnn_loader_set_feat_b16(b.handle, p, F, F, 64, 1) == -22
        assert b"already submitted" in L.gnn_sampler_last_error()
    finally:
        b.close()
    f32 = staging.FeatureStore(feats, pl.gpu_buffer_group[0], "cpu", 0)
    b = loader.NativeLoader(lap, labels, train, 100, 16, [1, 1], dev_of, idx_on, store=f32, workers=1)
    try:
        assert L.gnn_loader_set_feat_b16(b.handle, tab.data_ptr(), F, F, 64, 1) == -22
    finally:
        b.close()


def test_feature_store_dtype_errors(world):
    _, _, feats, _, pl = world
    nodes = pl.gpu_buffer_group[0]
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        staging.FeatureStore(feats.double(), nodes, "cpu", 0)
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        staging.FeatureStore(torch.zeros(feats.shape, dtype=torch.int8), nodes, "cpu", 0)
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="zero_copy"):
            staging.FeatureStore(feats.to(dtype), nodes, "cpu", 0, zero_copy=True)


def test_stage_kind_validation_without_gpu(world):
    """gnn_stage_plan / gnn_stage_batch_f32: a stage kind that is not the blob's is refused with a
    message before any HIP call (the upload included); the matching kind plans as usual."""
    L = _lib.lib()
    for tab, blob_kind in ((world[2].half(), 1), (world[2], 0)):
        a_, b, _ = _loaders(world, tab)
        try:
            nb = next(iter(b.epoch(1))).host
            assert int(nb.desc[loader.H_FEAT_KIND]) == blob_kind
            a = np.zeros(loader.STAGE_SLOTS, np.int64)
            a[loader.ST_DESC], a[loader.ST_HOST_BLOB] = nb.desc.ctypes.data, nb.ptr
            a[loader.ST_NUM_NODES], a[loader.ST_CSC_FROM], a[loader.ST_UPLOAD] = world[0].shape[0], 1, 1
            out = np.zeros(loader.BLOB_MAX_LAYERS * loader.STAGE_OUT_SLOTS, np.int64)
            a[loader.ST_FEAT_KIND] = blob_kind
            assert L.gnn_stage_plan(a.ctypes.data, out.ctypes.data) > 0
            for bad in (k for k in (0, 1, 2, 3, -1) if k != blob_kind):
                a[loader.ST_FEAT_KIND] = bad
                assert L.gnn_stage_plan(a.ctypes.data, out.ctypes.data) == 0
                assert b"feature kind" in L.gnn_last_error()
                with pytest.raises(RuntimeError, match="feature kind"):
                    _lib.check(L.gnn_stage_batch_f32(a.ctypes.data, None), "gnn_stage_batch_f32")
        finally:
            a_.close()
            b.close()


def test_gather_h16_argument_validation_without_gpu():
    """The 16-bit gathers refuse kind 0 / 3, negative sizes, F beyond a stride and NULL pointers
    before any launch; empty calls are no-ops."""
    L = _lib.lib()
    for kind in (0, 3):
        assert L.gnn_gather_rows_h16_f32(None, 8, kind, None, None, 8, None, 0, 8, None) == -22
        assert b"kind" in L.gnn_last_error()
        assert L.gnn_gather_rows2_h16_f32(None, 8, None, None, 0, None, 8, None, None, 0, kind, None, 8, 8, None) == -22
        assert b"kind" in L.gnn_last_error()
    assert L.gnn_gather_rows_h16_f32(None, 8, 1, None, None, 8, None, -5, 8, None) == -22
    assert L.gnn_gather_rows_h16_f32(None, 4, 1, None, None, 8, None, 1, 8, None) == -22
    assert b"stride" in L.gnn_last_error()
    assert L.gnn_gather_rows_h16_f32(None, 8, 2, None, None, 8, None, 1, 8, None) == -22
    assert b"NULL" in L.gnn_last_error()
    assert L.gnn_gather_rows_h16_f32(None, 8, 2, None, None, 8, None, 0, 8, None) == 0
    assert L.gnn_gather_rows2_h16_f32(None, 8, None, None, 0, None, 8, None, None, 0, 1, None, 8, 8, None) == 0
    assert L.gnn_gather_rows2_h16_f32(None, 8, None, None, 1, None, 8, None, None, 0, 1, None, 8, 8, None) == -22
