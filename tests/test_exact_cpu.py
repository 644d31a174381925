"""Exact full-neighbourhood inference, the parts that need no GPU: the block planner, the C ABI
of gnn_spmm_graph_f32 (exports, workspace size, refusals: all host code) and the CPU engine
against a float64 restatement of the reference forward (models.py:6-97) on the full ``lap``."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib, graphs, metrics, models
from gnn_amd.inference import ExactInference, plan_blocks

# ----------------------------------------------------------------------------- shared helpers


def make_world(model_name, N, nfeat, edges_per_node=8, empty=(0, 1, 2, 77), seed=0):
    """(lap, feats) of a Chung-Lu graph with the rows ``empty`` (and the last two) emptied."""
    rng = np.random.default_rng(seed)
    A = graphs.chung_lu(N, edges_per_node * N, 1.3, rng)
    keep = np.ones(N, np.float32)
    keep[list(empty) + [N - 2, N - 1]] = 0
    A = (sp.diags(keep) @ A).tocsr()
    A.eliminate_zeros()
    lap = graphs.lap_matrix(A.astype(np.float32), model_name)
    feats = torch.randn(N, nfeat, generator=torch.Generator().manual_seed(seed + 1))
    return lap, feats


def make_model(model_name, nfeat, nhid, orders, C=7, seed=3):
    torch.manual_seed(seed)
    m = models.build_model(model_name, nfeat, nhid, orders, C, dropout=0.1)
    with torch.no_grad():  # a trained model's scales, offsets and biases are not 1 / 0
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))
    return m


def reference_logits_f64(model, lap, feats) -> torch.Tensor:
    """models.py:6-97 in eval mode on the whole graph, float64 throughout: the operand is lap's
    structure with the weight 1/deg(row) (create_coo_tensor at normfact = 1), dense."""
    lap = sp.csr_matrix(lap)
    deg = np.diff(lap.indptr).astype(np.float64)
    w = np.repeat(1.0 / np.maximum(deg, 1), np.diff(lap.indptr))
    Lap = torch.from_numpy(sp.csr_matrix((w, lap.indices, lap.indptr), shape=lap.shape).toarray())
    d = lambda t: t.detach().double().cpu()
    x = feats.double()
    for gc in model.encoder.gcs:
        if isinstance(gc, models.GraphSageConvolution):
            lin = lambda l, v: v @ d(l.weight).t() + d(l.bias)
            feat = torch.cat([lin(gc.linearB, x), lin(gc.linearW, Lap @ x)], 1) if gc.order > 0 \
                else lin(gc.linearW, x)
        else:
            feat = (Lap @ x if gc.order > 0 else x) @ d(gc.linear.weight).t() + d(gc.linear.bias)
        out = torch.nn.functional.elu(feat)
        mean = out.mean(dim=1, keepdim=True)
        var = out.var(dim=1, unbiased=False, keepdim=True) + 1e-9
        x = (out - mean) * d(gc.scale) * torch.rsqrt(var) + d(gc.offset)
    x = torch.nn.functional.normalize(x, p=2, dim=1)
    return x @ d(model.linear.weight).t() + d(model.linear.bias)


def one_hot_labels(n, C, seed=5):
    cls = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(seed))
    return torch.nn.functional.one_hot(cls, C).float()


# ----------------------------------------------------------------------------- planner


def _check_plan(ip, blocks, max_nnz, max_rows):
    N = len(ip) - 1
    assert [b[0] for b in blocks] == [0] + [b[1] for b in blocks[:-1]] if blocks else N == 0
    assert (blocks[-1][1] if blocks else 0) == N
    for r0, r1 in blocks:
        assert r1 > r0 and r1 - r0 <= max_rows
        nnz = int(ip[r1] - ip[r0])
        assert nnz <= max_nnz or r1 - r0 == 1, (r0, r1, nnz)


def test_plan_blocks_int64_offsets():
    """A row pointer past 2^32 (no index array exists): exact cover, both caps, the over-long row
    alone in its block, a 2^31-entry row refused."""
    rng = np.random.default_rng(0)
    deg = rng.integers(0, 3_000_000, 4000).astype(np.int64)
    deg[100:200] = 0
    deg[1234] = 40_000_000  # longer than max_nnz
    ip = np.concatenate([[0], np.cumsum(deg)])
    assert ip[-1] > 2**32
    max_nnz, max_rows = 1 << 24, 50
    blocks = plan_blocks(ip, max_nnz, max_rows)
    _check_plan(ip, blocks, max_nnz, max_rows)
    assert (1234, 1235) in blocks
    assert any(r1 - r0 == max_rows for r0, r1 in blocks)  # the run of empty rows: the row cap binds
    assert sum(1 for r0, r1 in blocks if int(ip[r1] - ip[r0]) > max_nnz) == 1
    # greedy: no block could have taken the next row as well
    for r0, r1 in blocks:
        if r1 < len(ip) - 1 and r1 - r0 < max_rows:
            assert int(ip[r1 + 1] - ip[r0]) > max_nnz
    deg[2000] = 2**31
    with pytest.raises(ValueError, match="2\\^31"):
        plan_blocks(np.concatenate([[0], np.cumsum(deg)]), max_nnz, max_rows)
    deg[2000] = 2**31 - 2  # the largest row a block can hold
    ip = np.concatenate([[0], np.cumsum(deg)])
    assert (2000, 2001) in plan_blocks(ip, max_nnz, max_rows)


def test_plan_blocks_degenerate():
    assert plan_blocks(np.zeros(1, np.int64), 10, 10) == []
    ip = np.zeros(1001, np.int64)  # all rows empty
    blocks = plan_blocks(ip, 10, 300)
    _check_plan(ip, blocks, 10, 300)
    assert blocks == [(0, 300), (300, 600), (600, 900), (900, 1000)]
    ip = np.concatenate([[0], np.cumsum(np.arange(20) % 4)]).astype(np.int64)
    blocks = plan_blocks(ip, 100, 1)
    assert blocks == [(i, i + 1) for i in range(20)]
    _check_plan(ip, plan_blocks(ip, 1, 7), 1, 7)
    assert plan_blocks(ip) == [(0, 20)]  # the defaults
    with pytest.raises(ValueError):
        plan_blocks(ip, 0, 5)


# ----------------------------------------------------------------------------- C ABI


def test_graph_entry_points_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gnn_spmm_graph_f32", "gnn_spmm_graph_workspace_bytes"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED_SYMBOLS


def test_graph_workspace_bytes():
    L = _lib.lib()
    nnzs = sorted(set(list(range(0, 300_000, 499)) + [10**6, 3 * 10**6, 10**7, 10**8, 2**31 - 2]))
    rowss = sorted(set(list(range(1, 200_000, 997)) + [10**6, 2**31 - 2]))
    al = lambda b: (b + 255) // 256 * 256
    for F in (4, 28, 256, 608):
        for rows in (1, 3, 100, 1000, 5000, 50_000, 10**6):
            prev = 0
            for nnz in nnzs:
                w = L.gnn_spmm_graph_workspace_bytes(rows, nnz, F)
                agg = L.gnn_spmm_workspace_bytes(rows, nnz, F, 0)
                assert w >= prev, (F, rows, nnz)  # monotone in nnz
                assert w >= al(4 * (rows + 1)) + al(4 * nnz) + al(agg)  # the three parts
                prev = w
        for nnz in (0, 7, 1000, 100_000, 10**7):
            prev = 0
            for rows in rowss:
                w = L.gnn_spmm_graph_workspace_bytes(rows, nnz, F)
                assert w >= prev and w >= L.gnn_spmm_workspace_bytes(rows, nnz, F, 0), (F, rows, nnz)
                prev = w


def test_graph_call_refusals_without_gpu():
    """Every refusal comes before any device call: status -22 and the argument's name."""
    L = _lib.lib()
    p = 4096  # a non-NULL, aligned pointer that is never dereferenced
    big = 1 << 40

    def call(num_nodes=100, row0=10, rows=20, e0=0, nnz=50, ldx=8, kind=0, ldy=8, F=8, ws=p, wsb=big, X=p, Y=p):
        return L.gnn_spmm_graph_f32(p, p, p, num_nodes, row0, rows, e0, nnz, X, ldx, kind, Y, ldy, F, ws, wsb, None)

    cases = [
        (dict(rows=-1), b"negative"), (dict(nnz=-1), b"negative"), (dict(num_nodes=-1), b"negative"),
        (dict(F=-4), b"negative"), (dict(row0=-1), b"negative"), (dict(e0=-1), b"negative"),
        (dict(nnz=2**31 - 1), b"2^31"), (dict(rows=2**31 - 1, num_nodes=2**40), b"2^31"),
        (dict(num_nodes=2**31 - 1), b"2^31"),
        (dict(row0=90, rows=11), b"num_nodes"), (dict(row0=101, rows=0), b"num_nodes"),
        (dict(F=12), b"ldx"), (dict(F=12, ldx=12), b"ldy"),
        (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"),
        (dict(wsb=L.gnn_spmm_graph_workspace_bytes(20, 50, 8) - 1), b"workspace too small"),
        (dict(ws=None), b"workspace too small"),
        (dict(ws=p + 8), b"16-byte aligned"),
        (dict(kind=1, F=6), b"multiples of 4"), (dict(kind=2, ldx=10), b"multiples of 4"),
        (dict(kind=1, ldy=10), b"multiples of 4"), (dict(kind=1, X=p + 4), b"X not 8-byte aligned"),
        (dict(kind=2, Y=p + 8), b"Y not 16-byte aligned"),
    ]
    for kw, word in cases:
        assert call(**kw) == -22, kw
        assert word in L.gnn_last_error(), (kw, L.gnn_last_error())
    # nothing to do: accepted without a device call
    assert call(rows=0, nnz=0) == 0 and call(F=0) == 0


# ----------------------------------------------------------------------------- CPU engine

CASES = [("graphsage", [1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1])]
IDS = ["sage11", "sage101", "gcn11"]


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def world(request):
    name, orders = request.param
    N, nfeat, C = 600, 20, 7
    lap, feats = make_world(name, N, nfeat)
    model = make_model(name, nfeat, 12, orders, C).eval()
    return model, lap, feats, reference_logits_f64(model, lap, feats), C


def test_cpu_engine_matches_float64_reference(world):
    model, lap, feats, ref, C = world
    eng = ExactInference(model, lap, "cpu", max_rows=97)
    assert len(eng.blocks) == 7 and eng.blocks[-1] == (582, 600)  # a partial last block
    z = eng.logits(feats)
    assert z.dtype == torch.float32 and z.shape == (600, C)
    assert torch.allclose(z.double(), ref, rtol=1e-5, atol=1e-6), float((z.double() - ref).abs().max())
    nodes = np.array([5, 0, 599, 77, 300, 301, 5])  # unordered, an empty row, a repeat
    assert torch.equal(eng.logits(feats, nodes), z[torch.from_numpy(nodes)])
    one = ExactInference(model, lap, "cpu", max_rows=10**6).logits(feats)  # a single block
    assert len(ExactInference(model, lap, "cpu", max_rows=10**6).blocks) == 1
    assert torch.allclose(one, z, rtol=1e-5, atol=1e-6)
    assert not model.training


def test_cpu_engine_evaluate_counts(world):
    model, lap, feats, _, C = world
    eng = ExactInference(model, lap, "cpu", max_rows=97)
    nodes = np.arange(40, 560, 3)
    z = eng.logits(feats, nodes)
    labels = one_hot_labels(len(nodes), C)
    for sigmoid_loss, mode in ((True, 0), (False, 1), (True, 1)):
        res = eng.evaluate(feats, nodes, labels, sigmoid_loss=sigmoid_loss, mode=mode)
        want = metrics.prediction_counts(z, labels, mode).numpy().astype(np.int64)
        assert np.array_equal(eng.last_counts, want)
        micro, macro = metrics.f1_from_counts(want[0], want[1], want[2], mode)
        assert res["micro_f1"] == micro and res["macro_f1"] == macro
        assert res["rows"] == len(nodes) and res["batches"] == 1
        assert res["loss"] == pytest.approx(float(models.loss(z, labels, sigmoid_loss, "cpu")), rel=1e-6)
        assert set(res) == {"micro_f1", "macro_f1", "loss", "batches", "rows", "ref_batch_weighted_micro_f1"}


def test_cpu_engine_16bit_table_and_trainer(world):
    from gnn_amd.train import Trainer

    model, lap, feats, _, C = world
    eng = ExactInference(model, lap, "cpu", max_rows=97)
    h = feats.half()
    assert torch.equal(eng.logits(h), eng.logits(h.float()))
    nodes = np.arange(0, 600, 5)
    labels = one_hot_labels(len(nodes), C)
    tr = Trainer(model, 1e-3, "cpu")
    for training in (True, False):
        model.train(training)
        res = tr.evaluate_exact(lap, feats, nodes, labels)
        assert model.training == training
        assert res == ExactInference(model.eval(), lap, "cpu").evaluate(feats, nodes, labels)
        model.train(training)
    assert tr._exact[1] is not None and tr.evaluate_exact(lap, feats, nodes, labels) == res  # the cached engine
    with pytest.raises(ValueError, match="rows"):
        eng.logits(feats[:-1])
