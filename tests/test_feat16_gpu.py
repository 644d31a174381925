"""GPU: X0 from fp16 / bf16 feature stores (gnn_gather_rows_h16_f32, gnn_gather_rows2_h16_f32,
the staging routes, training from a 16-bit store).

fp16 -> fp32 and bf16 -> fp32 are exact, so nothing here has a tolerance: every comparison is on
bit patterns (int32 views) against torch's CPU ``.float()`` of the same 16-bit tensor.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib
from gnn_amd import custom_sparse_ops as cso
from gnn_amd import loader, placement, staging
from gnn_amd.graphs import chung_lu, row_normalize
from gnn_amd.models import build_model
from gnn_amd.train import Trainer

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _r(x, a):
    return (x + a - 1) // a * a


# ------------------------------------------------------------------------------------------
# every 16-bit pattern
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_all_bit_patterns_widen_exactly(dev, dtype, offset):
    """A 64 x 1024 table of all 65,536 patterns, rows permuted: finite values, both zeros,
    subnormals, both infinities and 65504 bit-equal to the CPU conversion, NaN patterns NaN —
    through the 16-byte-load kernel (aligned) and the scalar one (base off by one element)."""
    bits = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16))  # pattern i at position i
    table = bits.view(dtype).view(64, 1024)
    want = table.float()  # CPU conversion: the reference
    flat = torch.zeros(65536 + 8, dtype=dtype, device=dev)
    flat[offset:offset + 65536] = table.reshape(-1).to(dev)
    src = flat[offset:offset + 65536].view(64, 1024)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(1))
    dst = torch.full((64, 1024), 7.0, device=dev)
    cso.gather_rows(src, perm.to(dev), dst, None)
    got = dst.cpu()
    ref = want[perm]
    nan = torch.isnan(ref)
    assert int(nan.sum()) == (2046 if dtype == torch.float16 else 254)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(_i32(got)[~nan], _i32(ref)[~nan])
    # the named values, wherever the permutation put them
    if dtype == torch.float16:
        flatgot = got[torch.argsort(perm)].reshape(-1)
        assert float(flatgot[0x7BFF]) == 65504.0 and float(flatgot[0x0001]) == 2.0 ** -24
        assert float(flatgot[0x7C00]) == float("inf") and float(flatgot[0xFC00]) == float("-inf")
        assert _i32(flatgot[0x8000:0x8001]).item() == -2 ** 31  # -0


# ------------------------------------------------------------------------------------------
# shapes where the indexing can go wrong
# ------------------------------------------------------------------------------------------
ROWS = 1001  # source rows: identity gathers of the largest n fit


@pytest.mark.parametrize("F", [1, 7, 8, 9, 12, 37, 64, 512, 513, 608, 1030])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_rows_h16_shapes(dev, dtype, F):
    """n around the four rows of a workgroup, source strides padded to 64 / to 8 / unpadded,
    bases off by 0 / 1 / 4 elements (16-byte, scalar and 8-byte loads), index arrays NULL or
    given with repeated source rows; the destination is wider and longer than what is written
    and keeps its NaN prefill everywhere else, bit for bit."""
    g = torch.Generator().manual_seed(F)
    lds = sorted({_r(F, 64), _r(F, 8), F})
    tabs = {ld: (torch.randn(ROWS, ld, generator=g) * 50).to(dtype) for ld in lds}
    wide = {ld: t.float() for ld, t in tabs.items()}  # the CPU reference, made once
    combo = 0
    for n in (0, 1, 3, 4, 5, 1001):
        for ld in lds:
            for off in (0, 1, 4):
                flat = torch.zeros(ROWS * ld + 8, dtype=dtype, device=dev)
                flat[off:off + ROWS * ld] = tabs[ld].reshape(-1).to(dev)
                src = flat[off:off + ROWS * ld].view(ROWS, ld)[:, :F]
                for ldd in (_r(F + 1, 4), F + 1):
                    use_src, use_dst = bool(combo & 1), bool(combo & 2)
                    combo += 1
                    sidx = torch.randint(0, min(ROWS, 40), (n,), generator=g) if use_src else None  # repeats
                    didx = torch.randperm(n + 3, generator=g)[:n] if use_dst else None
                    dst = torch.full((n + 3, ldd), float("nan"), device=dev)
                    cso.gather_rows(src, None if sidx is None else sidx.to(dev), dst[:, :F],
                                    None if didx is None else didx.to(dev), n=n)
                    want = torch.full((n + 3, ldd), float("nan"))
                    rows = wide[ld][sidx if use_src else torch.arange(n), :F]
                    want[didx if use_dst else torch.arange(n), :F] = rows
                    assert torch.equal(_i32(dst.cpu()), _i32(want)), (n, ld, off, ldd, use_src, use_dst)
    assert combo >= 4


# ------------------------------------------------------------------------------------------
# the two-source call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,ld0,ld1,ldd", [(608, 640, 704, 608), (37, 64, 37, 40), (512, 512, 520, 512),
                                           (1030, 1088, 1032, 1032), (1032, 1088, 1032, 1032)])
@pytest.mark.parametrize("n0,n1", [(900, 1300), (0, 17), (33, 0)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_rows2_h16_matches_indexing(dev, dtype, F, ld0, ld1, ldd, n0, n1):
    """gnn_gather_rows2_h16_f32 against torch indexing, bit for bit: one source empty, both in
    use, a stride per source, and rows beyond the one-pass kernel (1030 at 4-byte loads, 1032 at
    16-byte loads) that take the one-source kernel per source."""
    g = torch.Generator().manual_seed(F + n0 + n1)
    t0 = (torch.randn(2000, ld0, generator=g) * 50).to(dtype)
    t1 = (torch.randn(max(n1, 1), ld1, generator=g) * 50).to(dtype)
    perm = torch.randperm(n0 + n1, generator=g)
    pos0, pos1 = perm[:n0], perm[n0:]
    idx0 = torch.randint(0, 2000, (n0,), generator=g)
    dst = torch.full((n0 + n1 + 2, ldd + 4), float("nan"), device=dev)
    cso.gather_rows2(t0.to(dev)[:, :F], idx0.to(dev), pos0.to(dev), n0, t1.to(dev)[:, :F], None, pos1.to(dev), n1,
                     dst[:, :F])
    want = torch.full((n0 + n1 + 2, ldd + 4), float("nan"))
    want[pos0, :F] = t0.float()[idx0, :F]
    if n1:
        want[pos1, :F] = t1.float()[:n1, :F]
    assert torch.equal(_i32(dst.cpu()), _i32(want))


def test_gather_h16_argument_errors_leave_dst_untouched(dev):
    L = _lib.lib()
    src = torch.ones(8, 16, dtype=torch.float16, device=dev)
    dst = torch.full((8, 16), float("nan"), device=dev)
    st = _lib.stream_of(dev)
    s, d = src.data_ptr(), dst.data_ptr()
    calls = [
        lambda: L.gnn_gather_rows_h16_f32(s, 16, 0, None, d, 16, None, 8, 16, st),  # kind 0 is the fp32 call's
        lambda: L.gnn_gather_rows_h16_f32(s, 16, 3, None, d, 16, None, 8, 16, st),
        lambda: L.gnn_gather_rows_h16_f32(s, 8, 1, None, d, 16, None, 8, 16, st),  # F > ld_src
        lambda: L.gnn_gather_rows_h16_f32(s, 16, 1, None, d, 8, None, 8, 16, st),  # F > ld_dst
        lambda: L.gnn_gather_rows_h16_f32(None, 16, 1, None, d, 16, None, 8, 16, st),
        lambda: L.gnn_gather_rows2_h16_f32(s, 16, None, None, 4, s, 16, None, None, 4, 0, d, 16, 16, st),
        lambda: L.gnn_gather_rows2_h16_f32(s, 16, None, None, 4, s, 16, None, None, 4, 3, d, 16, 16, st),
        lambda: L.gnn_gather_rows2_h16_f32(s, 16, None, None, 4, s, 8, None, None, 4, 2, d, 16, 16, st),
        lambda: L.gnn_gather_rows2_h16_f32(s, 16, None, None, 4, None, 16, None, None, 4, 2, d, 16, 16, st),
    ]
    for i, call in enumerate(calls):
        assert call() != 0 and L.gnn_last_error(), i
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        cso.gather_rows(src.double(), None, dst, None)
    with pytest.raises(RuntimeError, match="share"):
        cso.gather_rows2(src, None, None, 4, src.bfloat16(), None, None, 4, dst)


# ------------------------------------------------------------------------------------------
# Stager end to end (the setup of tests/test_staging_gpu.py)
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _world(N=6000, avg=16, seed=5):
    A = chung_lu(N, N * avg // 2, 1.3, np.random.default_rng(seed))
    lap = row_normalize(A)
    lap.sum_duplicates()
    labels = sp.csr_matrix((np.ones(N, np.float32), (np.arange(N), np.arange(N) % 7)), shape=(N, 7))
    train = np.arange(0, N, 2)
    pl = placement.create_buffer_ours(lap, train, 500, [0], 3, alpha=0)
    return lap, labels, train, pl


def _loader(cls, store, seed=21, **kw):
    lap, labels, train, pl = _world()
    return cls(lap, labels, train, 800, 128, [1, 1, 1], pl.device_id_of_nodes_group[0],
               pl.idx_of_nodes_on_device_group[0], rank=0, world_size=1, store=store, workers=2, seed=seed, **kw)


ROUTES = {"native": (True, True), "gather2": (False, True), "two_launches": (False, False)}


@pytest.mark.parametrize("native_loader", [True, False], ids=["native_loader", "python_loader"])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("F", [30, 37])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stager_x0_from_16bit_store(dev, monkeypatch, dtype, F, route, native_loader):
    """Three batches through Stager.issue: X0 == feats.float()[input_nodes] and zero pads, by
    the one-call native stage, the Python sequence with gather_rows2, and the two-launch form."""
    monkeypatch.setattr(staging, "_NATIVE_STAGE", ROUTES[route][0])
    monkeypatch.setattr(staging, "_GATHER2", ROUTES[route][1])
    staged_natively = []
    real_stage = loader.NativeBatch.stage
    monkeypatch.setattr(loader.NativeBatch, "stage",
                        lambda self, *a, **k: (staged_natively.append(1), real_stage(self, *a, **k))[1])
    lap, labels, train, pl = _world()
    feats = (torch.randn(lap.shape[0], F, generator=torch.Generator().manual_seed(F)) * 3).to(dtype)
    wide = feats.float()
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
    assert store.ld_rows == 64 and store.gpu_buffer.dtype == dtype
    ld = _loader(loader.NativeLoader if native_loader else loader.BatchLoader, store)
    try:
        stager = staging.Stager(store)
        n_host = n_own = 0
        for _, lb in zip(range(3), ld.epoch(1)):
            fn = (loader.ToDevice(lb.host, dev) if native_loader else
                  (lambda: lb.host.to_device(dev, with_coo=False)))
            staged = stager.issue(lb.plan, fn)
            x0 = staged.wait()
            torch.cuda.synchronize()
            nodes = torch.from_numpy(np.asarray(lb.host.input_nodes, np.int64))
            assert torch.equal(_i32(x0.cpu()), _i32(wide[nodes]))
            full = x0.as_strided((x0.shape[0], store.ld), (store.ld, 1))
            assert bool((full[:, F:] == 0).all())
            assert staged.batch is not None and len(staged.adjs) == 3
            n_host += len(lb.plan.host_pos)
            n_own += len(lb.plan.own_pos)
        assert n_host > 0 and n_own > 0  # both sources were in use
        assert bool(staged_natively) == (native_loader and route == "native")
    finally:
        ld.close()


# ------------------------------------------------------------------------------------------
# training and evaluation from a 16-bit store == from the fp32 store of the same values
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_training_parity_with_fp32_store(dev, dtype):
    lap, labels, train, pl = _world()
    F = 30
    feats16 = (torch.randn(lap.shape[0], F, generator=torch.Generator().manual_seed(3)) * 2).to(dtype)
    results = []
    for feats in (feats16, feats16.float()):
        store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
        ld = _loader(loader.NativeLoader, store, seed=4, device_extract=True)
        try:
            stager = staging.Stager(store)
            torch.manual_seed(0)
            net = build_model("graphsage", F, 16, [1, 1, 1], 7, dropout=0.1, fused=True).to(dev)
            tr = Trainer(net, 0.01, dev)
            losses = []
            for it, lb in zip(range(3), ld.epoch(1)):
                staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
                x0 = staged.wait()
                db = staged.batch
                assert tr.executor is not None and tr.executor.supports(x0, staged.adjs, db.sampled_nodes, db.labels)
                torch.manual_seed(100 + it)
                losses.append(float(tr.step(x0, staged.adjs, db.sampled_nodes, db.labels)))
            torch.cuda.synchronize()

        finally:
            ld.close()
        ld = _loader(loader.NativeLoader, store, seed=4, device_extract=True)  # a loader with nothing in flight
        try:
            def eval_batches():
                for lb in ld.sequential(train[:200], 128):
                    staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
                    x0 = staged.wait()
                    yield x0, staged.adjs, staged.batch.sampled_nodes, staged.batch.labels

            ev = tr.evaluate(eval_batches())
            assert ev["batches"] == 2 and ev["rows"] == 200
            results.append((losses, [p.detach().clone() for p in net.parameters()], ev))
        finally:
            ld.close()
    (l16, p16, e16), (l32, p32, e32) = results
    assert l16 == l32 and all(np.isfinite(l16))
    for a, b in zip(p16, p32):
        assert torch.equal(a, b)
    assert e16.keys() == e32.keys()
    for k in e16:  # counts, F1 figures and the loss: identical (an undefined F1 is NaN on both sides)
        assert e16[k] == e32[k] or (e16[k] != e16[k] and e32[k] != e32[k]), k
