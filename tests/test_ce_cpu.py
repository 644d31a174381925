"""CPU: the softmax cross-entropy loss where no device is needed — GNN.forward_loss with
sigmoid_loss=False off the GPU, and the argument validation of the new entry points
(gnn_head_ce_*, gnn_head_eval_loss_f32) and of the descriptor's loss kind (GNN_SH_LOSS_KIND),
which all answer before any HIP call."""
import numpy as np
import torch

from gnn_amd import _lib
from gnn_amd import executor as E
from gnn_amd.models import build_model, loss


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_forward_loss_ce_on_cpu_is_loss_of_forward(golden):
    z = golden("ladies_tiny.npz")
    adjs = [torch.sparse_coo_tensor(_t(z[f"c0_adj{li}_indices"]), _t(z[f"c0_adj{li}_values"]),
                                    tuple(int(v) for v in z[f"c0_adj{li}_shape"])).coalesce() for li in range(3)]
    sampled = [_t(z[f"c0_sampled{li}"]) for li in range(3)]
    x0 = torch.randn(int(z["c0_nin"]), 602, generator=torch.Generator().manual_seed(5))
    labels = _t(z["c0_labels"]).float()
    onehot = torch.nn.functional.one_hot(labels.argmax(1), labels.shape[1]).float()
    torch.manual_seed(0)
    net = build_model("graphsage", 602, 32, [1, 1, 1], 41, dropout=0.1)
    net.eval()
    with torch.no_grad():
        lo, out = net.forward_loss(x0, adjs, sampled, onehot, sigmoid_loss=False)
        ref_out = net(x0, adjs, sampled)
        ref = loss(ref_out, onehot, False, "cpu")
        bce = net.forward_loss(x0, adjs, sampled, onehot, sigmoid_loss=True)[0]
    assert torch.equal(out, ref_out) and torch.equal(lo, ref)
    rows = torch.logsumexp(ref_out, 1) - (ref_out * onehot).sum(1)
    torch.testing.assert_close(lo, rows.mean(), rtol=1e-5, atol=0.0)
    assert float(lo) != float(bce)


def test_ce_entry_points_validate_without_a_device():
    L = _lib.lib()
    buf = np.zeros(96, np.float32)  # never read: every call below is refused before any HIP call
    p = (buf.ctypes.data + 63) // 64 * 64
    for D, C in ((1022, 9), (2052, 9), (1024, 257), (1024, 0), (0, 9)):
        rc = L.gnn_head_ce_fwd_f32(p, 2056, 3, D, p, p, C, p, 300, 0.1, 1, 0, p, p, p, p, p, p, None)
        assert rc == -22 and b"gnn_head_ce_fwd_f32" in L.gnn_last_error(), (D, C)
        rc = L.gnn_head_ce_bwd_f32(p, 2056, 3, D, p, C, p, 300, None, 0.1, 1, 0, p, p, p, p, 2056, p, None)
        assert rc == -22 and b"gnn_head_ce_bwd_f32" in L.gnn_last_error(), (D, C)
        rc = L.gnn_head_eval_loss_f32(p, 2056, 3, D, p, p, C, p, 300, p, 300, p, p, p, p, 0, 1, None)
        assert rc == -22 and L.gnn_last_error(), (D, C)
    for kind in (2, -1):
        rc = L.gnn_head_eval_loss_f32(p, 2056, 3, 1024, p, p, 9, p, 300, p, 300, p, p, p, p, 1, kind, None)
        assert rc == -22 and b"loss kind" in L.gnn_last_error()
    assert L.gnn_head_eval_loss_f32(p, 2056, 3, 1024, p, p, 9, p, 300, p, 300, p, p, p, p, 2, 1, None) == -22
    assert b"mode" in L.gnn_last_error()
    # the CE pair needs the rows' log-sum-exp buffer
    assert L.gnn_head_ce_fwd_f32(p, 2056, 3, 1024, p, p, 9, p, 300, 0.1, 1, 0, p, p, p, p, p, None, None) == -22
    assert L.gnn_head_ce_bwd_f32(p, 2056, 3, 1024, p, 9, p, 300, None, 0.1, 1, 0, p, p, p, p, 2056, None, None) == -22


def test_descriptor_loss_kind_is_validated_without_a_device():
    """Sizing a descriptor needs no device: both kinds size alike (the training plan always holds
    the rows' log-sum-exp), any other kind is refused by every entry point."""
    L = _lib.lib()
    assert E.H_LOSS_KIND == 23 == E.HEADER - 1
    d = np.zeros(E.HEADER + E.LAYER_SLOTS, dtype=np.int64)
    d[E.H_VERSION], d[E.H_LAYERS], d[E.H_KIND] = E.VERSION, 1, E.GCN
    d[E.H_F0], d[E.H_LDX0], d[E.H_CLASSES], d[E.H_NHID] = 64, 64, 7, 128
    d[E.HEADER + E.L_M], d[E.HEADER + E.L_K], d[E.HEADER + E.L_NNZ] = 50, 80, 300
    sizes = []
    for kind in (0, 1):
        d[E.H_LOSS_KIND] = kind
        sizes.append((L.gnn_train_step_workspace_bytes(d.ctypes.data), L.gnn_eval_step_workspace_bytes(d.ctypes.data)))
        assert 0 < sizes[-1][1] < sizes[-1][0]
    assert sizes[0] == sizes[1]
    out = np.zeros(64, np.float32)
    d[E.H_LABELS], d[E.H_LDL], d[E.H_LOSS] = out.ctypes.data, 7, out.ctypes.data
    for kind in (2, -1, 1 << 32):
        d[E.H_LOSS_KIND] = kind
        assert L.gnn_train_step_workspace_bytes(d.ctypes.data) == 0 and b"loss kind" in L.gnn_last_error()
        assert L.gnn_eval_step_workspace_bytes(d.ctypes.data) == 0 and b"loss kind" in L.gnn_last_error()
        assert L.gnn_train_step_f32(d.ctypes.data, out.ctypes.data, 0, None) == -22
        assert b"loss kind" in L.gnn_last_error()
        assert L.gnn_eval_step_f32(d.ctypes.data, None, 0, out.ctypes.data, 1, out.ctypes.data, 0, None) == -22
        assert b"loss kind" in L.gnn_last_error()
