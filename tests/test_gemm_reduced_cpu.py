"""CPU: the reduced-precision GEMM modes' definition (fused.round_operand), their names, and the
host side of the C entry points (gnn_gemm_f32_split*): no kernel is launched here."""
import pytest
import torch

from gnn_amd import _lib, fused

from test_abi import _GEMM_WS_SHAPES


def _randn(n, seed):
    g = torch.Generator().manual_seed(seed)
    # a wide exponent range, both signs, some exact zeros
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 31, (n,), generator=g).float())
    x[::97] = 0.0
    return x


def _sig_bits(n, bits, seed):
    """fp32 values with at most `bits` significant bits (an integer below 2^bits times a power of 2)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-(2 ** bits) + 1, 2 ** bits, (n,), generator=g).float()
    return m * torch.exp2(torch.randint(-20, 21, (n,), generator=g).float())


def test_round_operand_bf16_is_torch_bfloat16():
    x = _randn(20000, 1).reshape(100, 200)
    assert torch.equal(fused.round_operand(x, "bf16"), x.bfloat16().float())
    # a tie rounds to even: 1 + 2^-8 lies halfway between the bf16 neighbours 1 and 1 + 2^-7
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    assert fused.round_operand(t, "bf16").tolist() == [1.0, 1.0 + 2.0 ** -6]


def test_round_operand_split2_error_bound():
    x = _randn(20000, 2)
    y = fused.round_operand(x, "split2")
    assert bool(((x.double() - y.double()).abs() <= 2.0 ** -15 * x.double().abs()).all())
    assert bool((y != x).any())  # it does round
    # the definition, element by element: h the top 8 significant bits, m = RNE_bf16(x - h)
    h = (x.view(torch.int32) & -65536).view(torch.float32)
    assert torch.equal(y, h + (x - h).bfloat16().float())
    # strided input (a padded operand view)
    v = _randn(300 * 8, 3).reshape(300, 8)[:, :5]
    assert torch.equal(fused.round_operand(v, "split2"), fused.round_operand(v.contiguous(), "split2"))


@pytest.mark.parametrize("mode", fused.GEMM_REDUCED)
def test_round_operand_idempotent(mode):
    y = fused.round_operand(_randn(20000, 4), mode)
    assert torch.equal(fused.round_operand(y, mode), y)


@pytest.mark.parametrize("mode,bits", [("bf16", 8), ("split2", 16)])
def test_round_operand_identity_on_short_significands(mode, bits):
    x = _sig_bits(20000, bits, 5)
    assert torch.equal(fused.round_operand(x, mode), x)
    if bits == 8:  # and one more bit does not fit
        assert not torch.equal(fused.round_operand(_sig_bits(20000, 9, 6), mode), _sig_bits(20000, 9, 6))


def test_round_operand_full_precision_modes_and_junk():
    x = _randn(100, 7)
    for algo in fused.GEMM_ALGOS:
        assert fused.round_operand(x, algo) is x
    with pytest.raises(ValueError):
        fused.round_operand(x, "fp8")


def test_gemm_algo_names(monkeypatch):
    assert fused.GEMM_ALGOS == ("split3", "f32")
    assert fused.GEMM_REDUCED == ("split2", "bf16")
    monkeypatch.delenv("GNN_GEMM_ALGO", raising=False)
    assert fused.gemm_algo() == "split3"
    for name in fused.GEMM_ALGOS + fused.GEMM_REDUCED:
        monkeypatch.setenv("GNN_GEMM_ALGO", name)
        assert fused.gemm_algo() == name
    for junk in ("tf32", "split1", ""):
        monkeypatch.setenv("GNN_GEMM_ALGO", junk)
        with pytest.raises(RuntimeError, match="GNN_GEMM_ALGO"):
            fused.gemm_algo()


@pytest.mark.parametrize("pieces", [0, 4, -1])
def test_bad_piece_count_is_refused_without_gpu(pieces):
    L = _lib.lib()
    # (M, N > 0 so that the call is not an empty no-op; no pointer is touched before the check)
    rc = L.gnn_gemm_f32_split(pieces, 0, 0, 8, 8, 8, 1, None, 8, None, 8, None, 8, None, 0, None)
    assert rc == -22 and b"pieces" in L.gnn_last_error()
    rc = L.gnn_gemm_f32_split_indexed(pieces, 0, 0, 8, 8, 8, 1, None, 8, None, 0, None, 8, None, 0, None, 8, None, 0,
                                      None)
    assert rc == -22 and b"pieces" in L.gnn_last_error()
    assert L.gnn_gemm_f32_split_workspace_bytes(pieces, 512, 602, 15809, 2) == 0


@pytest.mark.parametrize("pieces", [1, 2, 3])
def test_workspace_query_is_split3s(monkeypatch, pieces):
    L = _lib.lib()
    for k in ("GNN_GEMM_WIDE", "GNN_GEMM_TAIL", "GNN_GEMM_SPLITS"):
        monkeypatch.delenv(k, raising=False)
    for shape in _GEMM_WS_SHAPES:
        assert L.gnn_gemm_f32_split_workspace_bytes(pieces, *shape) == L.gnn_gemm_f32_split3_workspace_bytes(*shape)
    assert L.gnn_gemm_f32_split_workspace_bytes(pieces, *_GEMM_WS_SHAPES[0]) > 0
    if pieces < 3:
        # the reduced modes have no wide tile: their plan stays the 128 x 128 one
        want = [L.gnn_gemm_f32_split3_workspace_bytes(*s) for s in _GEMM_WS_SHAPES]
        monkeypatch.setenv("GNN_GEMM_WIDE", "1")
        assert [L.gnn_gemm_f32_split_workspace_bytes(pieces, *s) for s in _GEMM_WS_SHAPES] == want
