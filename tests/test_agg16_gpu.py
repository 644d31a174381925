"""GPU: the aggregation reading float16 / bfloat16 rows as they are (gnn_spmm_csr_h16_f32 through
custom_sparse_ops.spmm_csr).

Every fp16 and bf16 value is an fp32 value and the 16-bit kernels run the fp32 kernels' fmaf chains
with the fp32 call's geometry, so the reference is the fp32 call on the widened copy of X and the
comparison is on bit patterns (int32 views): nothing here has a tolerance of its own. Against the
C oracle the file uses tests/test_spmm_gpu.py's RTOL / ATOL.
"""
import numpy as np
import pytest
import torch

import oracle as O
from oracle.fixtures import powerlaw_lens, random_csr
from gnn_amd import _lib
from gnn_amd import custom_sparse_ops as cso

from test_spmm_gpu import ATOL, RTOL, _config2_operand, _layer2_like, _op

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _x16(dev, K, F, dtype, seed, ld=None):
    """(X16, X32): a 16-bit (K x F) operand in ld-element rows and its widened copy in the same
    layout (the whole padded buffer widened, then the same view)."""
    ld = F if ld is None else ld
    g = torch.Generator().manual_seed(seed)
    buf = torch.zeros((K, ld), dtype=dtype)
    buf[:, :F] = (torch.randn(K, F, generator=g) * 3).to(dtype)
    buf = buf.to(dev)
    return buf[:, :F], buf.float()[:, :F]


def _h16_calls(monkeypatch):
    """Count the 16-bit library calls spmm_csr makes (the widening fallback makes none)."""
    L = _lib.lib()
    calls = []
    real = L.gnn_spmm_csr_h16_f32

    class Spy:
        def __getattr__(self, name):
            if name == "gnn_spmm_csr_h16_f32":
                return lambda *a: (calls.append(1), real(*a))[1]
            return getattr(L, name)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    return calls


def _identical(op, X16, X32, **kw):
    a = cso.spmm_csr(op, X16, **kw)
    b = cso.spmm_csr(op, X32, **kw)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and a.shape == b.shape
    assert torch.equal(_i32(a), _i32(b))
    return a


def _width_case(dev, F):
    M, K = 257, 400
    rng = np.random.default_rng(F)
    lens = rng.integers(0, 90, M)
    lens[:6] = [0, 1, 63, 64, 65, K]
    full, rowptr, col, nf = random_csr(M, K, lens, rng)
    return M, K, (full, rowptr, col, nf), _op(dev, full, rowptr, col, nf, M, K)


# (F, row stride in elements)
WIDTHS = [(4, 4), (36, 36), (64, 64), (100, 100), (128, 128), (512, 512), (604, 640), (1024, 1024), (2100, 2100)]


@pytest.mark.parametrize("F,ld", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_feature_widths_bit_identical_and_oracle(dev, monkeypatch, dtype, F, ld):
    """Row lengths 0, 1, 63, 64, 65, K and random: the 16-bit call equals the fp32 call on the
    widened X bit for bit, and the oracle's A·X within the file's tolerance."""
    calls = _h16_calls(monkeypatch)
    M, K, (full, rowptr, col, nf), op = _width_case(dev, F)
    X16, X32 = _x16(dev, K, F, dtype, F, ld)
    Y = _identical(op, X16, X32)
    assert len(calls) == 1
    ocol, oval = O.build_operand(full, rowptr, col, nf)
    Yref = O.spmm_f32(rowptr, ocol, oval, np.ascontiguousarray(X32.cpu().numpy()))
    np.testing.assert_allclose(Y.cpu().numpy(), Yref, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("unit", [0, 1, 7, 64, 333])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unit_splits_bit_identical(dev, dtype, unit):
    """Cut rows and the combine, every unit size down to one nonzero per unit."""
    M, K = 150, 300
    rng = np.random.default_rng(unit)
    lens = powerlaw_lens(M, 40, 1.3, rng, K)
    lens[::17] = 0
    full, rowptr, col, nf = random_csr(M, K, lens, rng)
    op = _op(dev, full, rowptr, col, nf, M, K)
    for F, ld in ((604, 640), (64, 64)):
        X16, X32 = _x16(dev, K, F, dtype, unit + F, ld)
        _identical(op, X16, X32, unit_nnz=unit)


@pytest.mark.parametrize("unit", [0, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_row_runs_bit_identical(dev, dtype, unit):
    M, K, F = 8192, 700, 96
    rng = np.random.default_rng(unit + 5)
    lens = np.zeros(M, int)
    lens[3000:3010] = rng.integers(1, 60, 10)
    lens[5000] = 400
    lens[rng.choice(np.arange(5001, 6000), 300, replace=False)] = 1
    full, rowptr, col, nf = random_csr(M, K, lens, rng)
    op = _op(dev, full, rowptr, col, nf, M, K)
    X16, X32 = _x16(dev, K, F, dtype, 9)
    Y = _identical(op, X16, X32, unit_nnz=unit)
    assert bool((Y[:3000] == 0).all()) and bool((Y[6000:] == 0).all())


@pytest.mark.parametrize("wpr", ["1", "4", "8", None])
@pytest.mark.parametrize("shape", [(512, 8684, 1024, 1024, 29, 484), (8684, 512, 1024, 1024, 2, 40),
                                   (300, 700, 602, 640, 30, 400)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_kernel_bit_identical(dev, monkeypatch, dtype, wpr, shape):
    """The row kernel's 16-bit twin, every waves-per-row form (602 columns in 640-element rows run
    at the padded width 604)."""
    M, K, F, ld, mean, mx = shape
    monkeypatch.setenv("GNN_SPMM_ROWK", "1")
    if wpr is not None:
        monkeypatch.setenv("GNN_SPMM_ROWK_WPR", wpr)
    calls = _h16_calls(monkeypatch)
    rng = np.random.default_rng(M + F)
    full, rowptr, col, nf = _layer2_like(rng, M, K, mean, mx)
    op = _op(dev, full, rowptr, col, nf, M, K)
    Fk = (F + 3) // 4 * 4
    assert cso.spmm_config(M, op.nnz, Fk, ldx=ld, ldy=ld, K=K)["kernel"].startswith("spmm_row_kernel<4,")
    X16, X32 = _x16(dev, K, F, dtype, M, ld)
    _identical(op, X16, X32)
    assert len(calls) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_small_tiled_u16_bit_identical(dev, dtype):
    rng = np.random.default_rng(23)
    M, K, F = 512, 8684, 1024
    full, rowptr, col, nf = _layer2_like(rng, M, K, 29, 484)
    op = _op(dev, full, rowptr, col, nf, M, K)
    assert cso.spmm_config(M, op.nnz, F, K=K)["kernel"] == "spmm_unit_kernel<4, 64, 1, 16, false>"
    X16, X32 = _x16(dev, K, F, dtype, 23)
    _identical(op, X16, X32)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_column_tiles_and_xcd_map_bit_identical(dev, dtype):
    """nnz >= 8 K and F beyond one L2 tile: several column tiles in the XCD order."""
    rng = np.random.default_rng(77)
    M, K, F = 3000, 4096, 604
    full, rowptr, col, nf = _config2_operand(M, K, 40000, rng)
    op = _op(dev, full, rowptr, col, nf, M, K)
    assert op.nnz >= 8 * K
    cfg = cso.spmm_config(M, op.nnz, F, ldx=640, ldy=640, K=K)
    assert cfg["tiles"] > 1 and cfg["kernel"].startswith("spmm_unit_kernel<4,"), cfg
    X16, X32 = _x16(dev, K, F, dtype, 77, 640)
    _identical(op, X16, X32)


def _pattern_operand(dev, extra_rows):
    """A 4096-row permutation with value 1.0, plus `extra_rows` rows of 2-3 nonzeros."""
    rng = np.random.default_rng(4096)
    K = 4096
    perm = rng.permutation(K)
    rows = [[int(c)] for c in perm] + [sorted(rng.choice(K, 2 + (i % 2), replace=False).tolist())
                                       for i in range(extra_rows)]
    M = len(rows)
    rowptr = np.zeros(M + 1, np.int32)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.asarray(r, np.int32) for r in rows])
    val = np.ones(col.size, np.float32)
    val[K:] = rng.uniform(0.5, 2.0, col.size - K).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    return cso.CsrOperand(t(rowptr), t(col), t(val), (M, K)), perm


@pytest.mark.parametrize("kernel", ["row", "unit"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_bit_pattern(dev, monkeypatch, dtype, kernel):
    """All 65,536 patterns as 4,096 rows x 16 columns through a permutation (value 1.0: the output
    is the widened value itself) and a few mixing rows: the fp32 path's bits on X.float(), NaN
    exactly where it has NaN — once through the row kernel, once through the unit kernel."""
    monkeypatch.setenv("GNN_SPMM_ROWK", "1" if kernel == "row" else "0")
    op, perm = _pattern_operand(dev, 8)
    M, K = op.shape
    name = cso.spmm_config(M, op.nnz, 16, K=K)["kernel"]
    assert name.startswith("spmm_row_kernel<4," if kernel == "row" else "spmm_unit_kernel<4,"), name
    bits = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16))
    X16 = bits.view(dtype).view(4096, 16).to(dev)
    X32 = X16.float()
    a = cso.spmm_csr(op, X16)
    b = cso.spmm_csr(op, X32)
    torch.cuda.synchronize()
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan)
    assert torch.equal(_i32(a)[~nan], _i32(b)[~nan])
    # every NaN pattern of the table reaches the output through the permutation rows (the unit
    # kernel's masked slots multiply a row already in flight by 0, in both paths alike: an
    # infinity there is a NaN too, so only the row kernel's counts are the table's)
    n_nan = 2046 if dtype == torch.float16 else 254
    if kernel == "row":
        assert int(nan[:4096].sum()) == n_nan and int(torch.isinf(a[:4096]).sum()) == 2
    else:
        assert int(nan[:4096].sum()) >= n_nan


@pytest.mark.parametrize("case", ["F41", "offset"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_rows_widen_first(dev, monkeypatch, dtype, case):
    """Rows the 4-element loads cannot read (F = 41 with no room to pad; a base off by one
    element) go through the widening fallback: no 16-bit call, the fp32 path's result."""
    calls = _h16_calls(monkeypatch)
    M, K, _, op = _width_case(dev, 64)
    if case == "F41":
        X16 = (torch.randn(K, 41, generator=torch.Generator().manual_seed(1)) * 3).to(dtype).to(dev)
    else:
        flat = torch.zeros(K * 64 + 8, dtype=dtype, device=dev)
        flat[1:1 + K * 64] = (torch.randn(K * 64, generator=torch.Generator().manual_seed(2)) * 3).to(dtype).to(dev)
        X16 = flat[1:1 + K * 64].view(K, 64)
        assert X16.data_ptr() % 8 == 2
    a = cso.spmm_csr(op, X16)
    b = cso.spmm_csr(op, X16.float())
    torch.cuda.synchronize()
    assert not calls and torch.equal(_i32(a), _i32(b))


def test_residual_with_16bit_dense_raises(dev):
    M, K, _, op = _width_case(dev, 64)
    X16 = torch.zeros(K, 64, dtype=torch.float16, device=dev)
    rmap = torch.full((M,), -1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="no residual"):
        cso.spmm_csr(op, X16, residual=torch.zeros(4, 64, device=dev), rmap=rmap)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        cso.spmm_csr(op, X16.double())


def test_refusals_leave_y_untouched(dev):
    L = _lib.lib()
    M, K, _, op = _width_case(dev, 64)
    X = torch.ones(K, 64, dtype=torch.float16, device=dev)
    Yb = torch.full((M, 64 + 4), float("nan"), device=dev)
    ws = torch.empty(max(L.gnn_spmm_workspace_bytes(M, op.nnz, 64, 0), 256), dtype=torch.uint8, device=dev)
    st = _lib.stream_of(dev)
    rp, col, val = op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr()
    x, y, w, wb = X.data_ptr(), Yb.data_ptr(), ws.data_ptr(), ws.numel()

    def call(x=x, ldx=64, kind=1, y=y, ldy=68, F=64, w=w, wb=wb, unit=0):
        return L.gnn_spmm_csr_h16_f32(rp, col, val, M, K, op.nnz, x, ldx, kind, y, ldy, F, w, wb, unit, st)

    bad = [dict(kind=0), dict(kind=3), dict(x=x + 2), dict(x=x + 4), dict(ldx=66), dict(F=62), dict(ldy=70),
           dict(y=y + 8), dict(ldx=60), dict(ldy=60), dict(w=None, wb=0, unit=16), dict(wb=16, unit=16)]
    for kw in bad:
        assert call(**kw) != 0 and L.gnn_last_error(), kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(Yb).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(Yb[:, :64]).any()) and bool(torch.isnan(Yb[:, 64:]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_graph_capture(dev, dtype):
    """The 16-bit call captures into a HIP graph (no allocation, no host sync) and two replays
    reproduce the uncaptured call: cut rows and the combine launch included."""
    L = _lib.lib()
    rng = np.random.default_rng(31)
    M, K, F = 600, 900, 128
    lens = powerlaw_lens(M, 60, 1.3, rng, K)
    full, rowptr, col, nf = random_csr(M, K, lens, rng)
    op = _op(dev, full, rowptr, col, nf, M, K)
    X16, _ = _x16(dev, K, F, dtype, 31)
    want = cso.spmm_csr(op, X16)
    wsb = L.gnn_spmm_workspace_bytes(M, op.nnz, F, 0)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    Y = torch.full((M, F), float("nan"), device=dev)
    kind = cso.FEAT_KIND[dtype]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(L.gnn_spmm_csr_h16_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), M, K, op.nnz,
                                          X16.data_ptr(), F, kind, Y.data_ptr(), F, F, ws.data_ptr(), wsb, 0,
                                          _lib.stream_of(dev)), "gnn_spmm_csr_h16_f32")
    for _ in range(2):
        Y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_i32(Y), _i32(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_deterministic_and_timed(dev, dtype):
    """Two runs of a power-law operand agree bit for bit; with timing on, the record names the
    16-bit kernel and counts 2 bytes per gathered X element."""
    M, K, F = 2000, 3000, 604
    rng = np.random.default_rng(5)
    lens = powerlaw_lens(M, 80, 1.5, rng, 2500)
    full, rowptr, col, nf = random_csr(M, K, lens, rng)
    op = _op(dev, full, rowptr, col, nf, M, K)
    X16, X32 = _x16(dev, K, F, dtype, 5, 640)
    Y1 = cso.spmm_csr(op, X16)
    cso.enable_timing(True)
    try:
        cso.take_timing_records()
        Y2 = cso.spmm_csr(op, X16)
        cso.spmm_csr(op, X32)
        r16, r32 = cso.take_timing_records()
    finally:
        cso.enable_timing(False)
    assert torch.equal(_i32(Y1), _i32(Y2))
    kind = cso.FEAT_KIND[dtype]
    assert r16[4]["x_bytes"] == 2 and r32[4]["x_bytes"] == 4
    assert r16[2] == cso.algorithmic_bytes(M, op.nnz, F, 2) == r32[2] - op.nnz * F * 2
    stem32 = r32[3]  # spmm_unit_kernel<4, G, NJ, U, false>
    assert r16[3] == "spmm_unit16_kernel<%d, %s>" % (kind, ", ".join(stem32.split("<")[1].split(", ")[1:4]))
    assert r16[1] > 0 and r32[1] > 0


@pytest.mark.parametrize("timed", [False, True], ids=["plain", "timed"])
@pytest.mark.parametrize("unit,stem", [(0, "spmm_row"), (16, "spmm_unit"), (64, "spmm_unit")],
                         ids=["row", "cut", "whole"])
def test_every_launch_form_on_the_smallest_operand(dev, monkeypatch, unit, stem, timed):
    """Each launch the aggregation's host path can make, on the smallest operand that reaches it —
    4 rows of 0, 1, 16 and 40 entries over K = 64: the row kernel (forced on, unit_nnz 0), the unit
    kernel with the 40-entry row cut and combined (unit_nnz 16) and as one unit with nothing to
    combine (64) — for fp32 X without and with a residual (F = 12) and for fp16 / bf16 X (F = 8), with
    and without armed timing events. 16-bit equals fp32 on the widened X bit for bit; every result
    is the oracle's within the file's tolerance; a timed launch records the kernel it ran."""
    monkeypatch.setenv("GNN_SPMM_ROWK", "1" if unit == 0 else "0")
    M, K = 4, 64
    rng = np.random.default_rng(7)
    full, rowptr, col, nf = random_csr(M, K, np.array([0, 1, 16, 40]), rng)
    op = _op(dev, full, rowptr, col, nf, M, K)
    ocol, oval = O.build_operand(full, rowptr, col, nf)
    g = torch.Generator().manual_seed(11)
    Xf = torch.randn(K, 12, generator=g).to(dev)
    R = torch.randn(3, 12, generator=g).to(dev)
    rmap = torch.tensor([2, -1, 0, 1], dtype=torch.int32, device=dev)
    cso.enable_timing(timed)
    try:
        cso.take_timing_records()
        Yp = cso.spmm_csr(op, Xf, unit_nnz=unit)
        Yr = cso.spmm_csr(op, Xf, unit_nnz=unit, residual=R, rmap=rmap)
        h16 = []
        for dtype in DTYPES:
            X16, X32 = _x16(dev, K, 8, dtype, 3)
            h16.append((cso.spmm_csr(op, X16, unit_nnz=unit), cso.spmm_csr(op, X32, unit_nnz=unit), X32))
        recs = cso.take_timing_records()
    finally:
        cso.enable_timing(False)
    torch.cuda.synchronize()
    ref = O.spmm_f32(rowptr, ocol, oval, np.ascontiguousarray(Xf.cpu().numpy()))
    np.testing.assert_allclose(Yp.cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
    want = ref.copy()
    m = rmap.cpu().numpy()
    want[m >= 0] += R.cpu().numpy()[m[m >= 0]]
    np.testing.assert_allclose(Yr.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    for a, b, X32 in h16:
        assert torch.equal(_i32(a), _i32(b))
        ref16 = O.spmm_f32(rowptr, ocol, oval, np.ascontiguousarray(X32.cpu().numpy()))
        np.testing.assert_allclose(a.cpu().numpy(), ref16, rtol=RTOL, atol=ATOL)
    assert len(recs) == (6 if timed else 0)
    if timed:
        names = [r[3] for r in recs]
        assert names[0].startswith(stem + "_kernel<4, ") and names[0].endswith(", false>")
        assert names[1] == names[0].replace("false", "true")
        assert names[2].startswith(stem + "16_kernel<1, ") and names[4].startswith(stem + "16_kernel<2, ")
        assert names[3] == names[5] == names[0]
        assert all(r[1] > 0 for r in recs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_spmm_autograd_forwards_16bit(dev, dtype):
    """SparseDenseMM takes a 16-bit mat2 (fp32 out) and produces no gradient for it."""
    M, K, (full, rowptr, col, nf), op = _width_case(dev, 64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    A = cso.create_coo_tensor(t(full), t(rowptr), t(col), t(nf), M, K)
    X16, X32 = _x16(dev, K, 64, dtype, 3)
    Y = cso.spmm(A, X16)
    assert Y.dtype == torch.float32 and not Y.requires_grad
    assert torch.equal(_i32(Y), _i32(cso.spmm(A, X32)))
