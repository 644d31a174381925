"""GPU: the reduced-precision modes of the split GEMM kernel (gnn_gemm_f32_split, pieces 2 =
"split2" and 1 = "bf16"; include/gnn_layers.h).

1. Semantics: the result is the fp32-accumulated product of the ROUNDED operands
   (fused.round_operand): |C - A'·B'| <= 4e-6 (|A'|·|B'|) + 1e-30 against fp64, the bound of
   tests/test_gemm_gpu.py applied to the rounded operands. This pins the rounding (RNE on the last
   kept piece) and the product set (split2 keeps all four products of h + m).
2. Bit identity with split3 on operands that already fit the kept pieces: the accumulation order is
   split3's and the removed products are all zero, so torch.equal — layouts, load widths, k tail,
   split-k with both reduce kernels, tail tiles, K = 0.
3. The row-indexed forms equal the same mode's product of the gathered operand, bit for bit.
4. pieces = 3 through the new entry points is the split3 entry points, bit for bit.
"""
import ctypes

import pytest
import torch

from gnn_amd import _lib
from gnn_amd.fused import GEMM_PIECES, GEMM_REDUCED, gemm, round_operand

pytestmark = pytest.mark.gpu

LAYOUTS = [(False, False), (False, True), (True, True), (True, False)]


def _operand(rows, cols, ld, g, dev):
    """(rows x cols) as the kernel reads it, row stride ld rounded up to even (its contract)."""
    return torch.randn(rows, ld + (ld & 1), generator=g).to(dev)[:, :cols]


def _operands(a_km, b_km, M, N, K, nb, g, dev, lda_pad=0, ldb_pad=0):
    As = [_operand(K if a_km else M, M if a_km else K, (M if a_km else K) + lda_pad, g, dev) for _ in range(nb)]
    Bs = [_operand(K if b_km else N, N if b_km else K, (N if b_km else K) + ldb_pad, g, dev) for _ in range(nb)]
    return As, Bs


def _storage(ts):
    """The operands' whole padded rows (clone these to keep the even row stride)."""
    return [t.as_strided((t.shape[0], t.stride(0)), (t.stride(0), 1)) for t in ts]


def _rounded_in_place(ts, mode):
    """The operands replaced by their rounded values, storage (strides, padding, alignment) kept."""
    for t in ts:
        t.copy_(round_operand(t, mode))
    return ts


# ------------------------------------------------------------------------------ 1. semantics
@pytest.mark.parametrize("mode", GEMM_REDUCED)
@pytest.mark.parametrize("a_km,b_km", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(128, 128, 16), (300, 200, 77), (1, 5, 3), (130, 513, 602)])
def test_reduced_is_the_product_of_the_rounded_operands(dev, mode, a_km, b_km, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    As, Bs = _operands(a_km, b_km, M, N, K, 1, g, dev)
    (c,) = gemm(a_km, b_km, As, Bs, M, N, K, algo=mode)
    torch.cuda.synchronize()
    a = round_operand(As[0], mode).double().cpu()
    b = round_operand(Bs[0], mode).double().cpu()
    a, b = (a.t() if a_km else a), (b if b_km else b.t())
    err = (c.double().cpu() - a @ b).abs()
    bound = 4e-6 * (a.abs() @ b.abs()) + 1e-30
    print(f"{mode} {a_km} {b_km} {M}x{N}x{K}: max err / bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all()), f"max excess {(err - bound).max().item()}"


@pytest.mark.parametrize("mode", GEMM_REDUCED)
@pytest.mark.parametrize("a_km,b_km", LAYOUTS)
def test_reduced_equals_split3_of_the_rounded_operands(dev, mode, a_km, b_km):
    """The same statement with no tolerance: the mode on raw operands is split3 on round_operand of
    them, bit for bit — the kernel's pieces are split3's pieces of the rounded value, also where a
    split2 remainder rounds up to a whole unit of h (x' = h + ulp: about one element in 500, so
    every output here meets many)."""
    M, N, K = 130, 513, 602
    g = torch.Generator().manual_seed(11)
    As, Bs = _operands(a_km, b_km, M, N, K, 1, g, dev)
    if mode == "split2":  # and some elements exactly at the threshold and just below it, both signs
        edge = torch.tensor([0x3F80FF80, 0x3F80FF7F, 0xBF80FFFF - (1 << 32), 0x3FFFFF80, 0x40490FDB],
                            dtype=torch.int32).view(torch.float32).to(dev)
        As[0][0, :5] = edge
        Bs[0][0, :5] = -edge
        # 1 + 255/256 ulp-of-h rounds up to the next bf16; one fp32 ulp less keeps h and a full m
        assert round_operand(edge[:2], mode).view(torch.int32).tolist() == [0x3F810000, 0x3F80FF00]
    got = gemm(a_km, b_km, As, Bs, M, N, K, algo=mode)
    ref = gemm(a_km, b_km, _rounded_in_place([a.clone() for a in _storage(As)], mode),
               _rounded_in_place([b.clone() for b in _storage(Bs)], mode), M, N, K, algo="split3")
    raw = gemm(a_km, b_km, As, Bs, M, N, K, algo="split3")
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]), float((got[0] - ref[0]).abs().max())
    assert not torch.equal(got[0], raw[0])  # and the mode does round


# ------------------------------------------------------------------------------ 2. bit identity
def _assert_equals_split3(dev, mode, a_km, b_km, M, N, K, nb, lda_pad=0, ldb_pad=0):
    g = torch.Generator().manual_seed(M + 3 * N + 5 * K + nb)
    As, Bs = _operands(a_km, b_km, M, N, K, nb, g, dev, lda_pad, ldb_pad)
    _rounded_in_place(As + Bs, mode)
    got = gemm(a_km, b_km, As, Bs, M, N, K, algo=mode)
    ref = gemm(a_km, b_km, As, Bs, M, N, K, algo="split3")
    torch.cuda.synchronize()
    for x, y in zip(got, ref):
        assert torch.equal(x, y), (mode, a_km, b_km, M, N, K, float((x - y).abs().max()))
    assert bool(ref[0].any()) or K == 0


@pytest.mark.parametrize("mode", GEMM_REDUCED)
@pytest.mark.parametrize("a_km,b_km", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(300, 200, 77), (130, 513, 602)])
def test_prerounded_operands_equal_split3_layouts(dev, mode, a_km, b_km, M, N, K):
    _assert_equals_split3(dev, mode, a_km, b_km, M, N, K, 1)


@pytest.mark.parametrize("mode", GEMM_REDUCED)
def test_prerounded_operands_equal_split3_strides(dev, mode):
    _assert_equals_split3(dev, mode, False, False, 333, 512, 602, 2, lda_pad=2)  # 604-float rows: 16-byte loads
    _assert_equals_split3(dev, mode, False, True, 200, 602, 512, 1)              # 602-float rows: 8-byte loads


@pytest.mark.parametrize("mode", GEMM_REDUCED)
def test_prerounded_operands_equal_split3_split_k(dev, mode):
    L = _lib.lib()
    assert L.gnn_gemm_f32_split_workspace_bytes(GEMM_PIECES[mode], 512, 602, 5000, 2) > 0  # k is split
    _assert_equals_split3(dev, mode, True, True, 512, 602, 5000, 2)
    _assert_equals_split3(dev, mode, True, True, 101, 131, 3001, 1)  # M·N odd: the scalar reduce kernel


@pytest.mark.parametrize("mode", GEMM_REDUCED)
def test_prerounded_operands_equal_split3_tail_tiles(dev, mode):
    # 33 x 8 = 264 tiles: 256 whole, 8 tail tiles of 2 k pieces each (gemm.hip tail_plan): the
    # workspace is the 16 piece tiles
    M, N, K = 4224, 1024, 160
    assert _lib.lib().gnn_gemm_f32_split_workspace_bytes(GEMM_PIECES[mode], M, N, K, 1) == 8 * 2 * 128 * 128 * 4
    _assert_equals_split3(dev, mode, False, False, M, N, K, 1)


@pytest.mark.parametrize("mode", GEMM_REDUCED)
def test_reduced_k_zero(dev, mode):
    a = torch.zeros(10, 2, device=dev)[:, :0]
    b = torch.zeros(7, 2, device=dev)[:, :0]
    (c,) = gemm(False, False, [a], [b], 10, 7, 0, algo=mode)
    (r,) = gemm(False, False, [a], [b], 10, 7, 0, algo="split3")
    torch.cuda.synchronize()
    assert torch.equal(c, r) and torch.count_nonzero(c) == 0


# ------------------------------------------------------------------------------ 3. indexed forms
def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _indexed(dev, pieces, case, M, N, K, R, reference):
    """The indexed call of `pieces` (through gnn_gemm_f32_split_indexed) and `reference(a_km, b_km,
    As, Bs, M, N, K)` on the gathered operands, as test_split3_row_indexed_equals_gathered builds them."""
    g = torch.Generator().manual_seed(M + N + K)
    L = _lib.lib()
    st = _lib.stream_of(dev)
    src = torch.randn(R, K + (K & 1), generator=g).to(dev)
    idx = torch.randint(0, R, (M,), generator=g).to(dev)
    other = torch.randn(M, src.shape[1], generator=g).to(dev)
    if case == "a_fwd":  # C (M x N) = A[idx] (M x K) · Bᵀ, B (N x K)
        Bw = torch.randn(N, K + (K & 1), generator=g).to(dev)
        ref = reference(False, False, [src[idx][:, :K], other[:, :K]], [Bw[:, :K], Bw[:, :K]], M, N, K)
        out = [torch.empty(M, N, device=dev) for _ in range(2)]
        wsb = L.gnn_gemm_f32_split_workspace_bytes(pieces, M, N, K, 2)
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
        rc = L.gnn_gemm_f32_split_indexed(pieces, 0, 0, M, N, K, 2, _ptrs([src, other]), src.stride(0),
                                          _ptrs([idx, None]), R, _ptrs([Bw, Bw]), Bw.stride(0), None, 0,
                                          _ptrs(out), N, ws.data_ptr(), wsb, st)
    else:  # C (N x K) = Gᵀ (G: M x N, k-major over M) · X[idx] (M x K, k-major B)
        G = torch.randn(M, N + (N & 1), generator=g).to(dev)
        ref = reference(True, True, [G[:, :N], G[:, :N]], [src[idx][:, :K], other[:, :K]], N, K, M)
        out = [torch.empty(N, K, device=dev) for _ in range(2)]
        wsb = L.gnn_gemm_f32_split_workspace_bytes(pieces, N, K, M, 2)
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
        rc = L.gnn_gemm_f32_split_indexed(pieces, 1, 1, N, K, M, 2, _ptrs([G, G]), G.stride(0), None, 0,
                                          _ptrs([src, other]), src.stride(0), _ptrs([idx, None]), R,
                                          _ptrs(out), K, ws.data_ptr(), wsb, st)
    assert rc == 0, L.gnn_last_error()
    torch.cuda.synchronize()
    return out, ref


@pytest.mark.parametrize("mode", GEMM_REDUCED)
@pytest.mark.parametrize("case", ["a_fwd", "b_wgrad"])
@pytest.mark.parametrize("M,N,K,R", [(4100, 512, 602, 6000), (300, 130, 77, 1000)])
def test_reduced_row_indexed_equals_gathered(dev, mode, case, M, N, K, R):
    out, ref = _indexed(dev, GEMM_PIECES[mode], case, M, N, K, R, lambda *a: gemm(*a, algo=mode))
    for c, r in zip(out, ref):
        assert torch.equal(c, r)


# ------------------------------------------------------------------------------ 4. pieces = 3
@pytest.mark.parametrize("a_km,b_km,M,N,K,nb", [(False, False, 300, 200, 77, 2), (True, True, 512, 602, 5000, 2),
                                                (False, True, 130, 513, 602, 1), (True, False, 257, 64, 1024, 1)])
def test_three_pieces_is_split3(dev, a_km, b_km, M, N, K, nb):
    L = _lib.lib()
    g = torch.Generator().manual_seed(M + N + K)
    As, Bs = _operands(a_km, b_km, M, N, K, nb, g, dev)
    ref = gemm(a_km, b_km, As, Bs, M, N, K, algo="split3")
    out = [torch.full((M, N), float("nan"), device=dev) for _ in range(nb)]
    wsb = L.gnn_gemm_f32_split_workspace_bytes(3, M, N, K, nb)
    assert wsb == L.gnn_gemm_f32_split3_workspace_bytes(M, N, K, nb)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    _lib.check(L.gnn_gemm_f32_split(3, int(a_km), int(b_km), M, N, K, nb, _ptrs(As), As[0].stride(0), _ptrs(Bs),
                                    Bs[0].stride(0), _ptrs(out), N, ws.data_ptr(), wsb, _lib.stream_of(dev)),
               "gnn_gemm_f32_split")
    torch.cuda.synchronize()
    for c, r in zip(out, ref):
        assert torch.equal(c, r)


@pytest.mark.parametrize("case", ["a_fwd", "b_wgrad"])
def test_three_pieces_indexed_is_split3_indexed(dev, case):
    out, ref = _indexed(dev, 3, case, 300, 130, 77, 1000, lambda *a: gemm(*a, algo="split3"))
    for c, r in zip(out, ref):
        assert torch.equal(c, r)
