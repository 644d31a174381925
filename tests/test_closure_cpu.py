"""Exact inference restricted to a query set's k-hop closure, the parts that need no GPU: the C ABI
of gnn_closure_* and gnn_spmm_rows_f32 (exports, sizes, refusals: all host code), the closure's
node sets against an np.unique chain, and the CPU engine in closure scope against the float64
reference forward and against the full-graph scope."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib, metrics, models
from gnn_amd.inference import Closure, ExactInference
from test_exact_cpu import make_model, make_world, one_hot_labels, reference_logits_f64

NEW_SYMBOLS = ("gnn_closure_table_bytes", "gnn_closure_workspace_bytes", "gnn_closure_mark", "gnn_closure_list",
               "gnn_closure_rank", "gnn_spmm_rows_workspace_bytes", "gnn_spmm_rows_f32")


# ----------------------------------------------------------------------------- C ABI


def test_closure_entry_points_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED_SYMBOLS


def test_closure_sizes():
    L = _lib.lib()
    prev_t = prev_w = 0
    for n in (0, 1, 31, 32, 33, 2000, 2**18, 2**18 + 1, 2**20 + 37, 10**8, 2**31 - 2):
        t, w = L.gnn_closure_table_bytes(n), L.gnn_closure_workspace_bytes(n)
        words = (n + 31) // 32
        assert t % 256 == 0 and t >= 8 * (words + 1)  # one word per 32 ids and the trailing total
        assert w % 256 == 0 and w >= 2 * 4 * ((words + 8191) // 8192 + 1)
        assert t >= prev_t and w >= prev_w
        prev_t, prev_w = t, w


def test_rows_workspace_bytes():
    """The sweep of test_graph_workspace_bytes: monotone in rows and in nnz, never below the row
    pointer, the columns, the weights and the aggregation's own size."""
    L = _lib.lib()
    nnzs = sorted(set(list(range(0, 300_000, 499)) + [10**6, 3 * 10**6, 10**7, 10**8, 2**31 - 2]))
    rowss = sorted(set(list(range(1, 200_000, 997)) + [10**6, 2**31 - 2]))
    al = lambda b: (b + 255) // 256 * 256
    for F in (4, 28, 256, 608):
        for rows in (1, 3, 100, 1000, 5000, 50_000, 10**6):
            prev = 0
            for nnz in nnzs:
                w = L.gnn_spmm_rows_workspace_bytes(rows, nnz, F)
                agg = L.gnn_spmm_workspace_bytes(rows, nnz, F, 0)
                assert w >= prev, (F, rows, nnz)  # monotone in nnz
                assert w >= al(4 * (rows + 1)) + 2 * al(4 * nnz) + al(agg)  # the four parts
                prev = w
        for nnz in (0, 7, 1000, 100_000, 10**7):
            prev = 0
            for rows in rowss:
                w = L.gnn_spmm_rows_workspace_bytes(rows, nnz, F)
                assert w >= prev and w >= L.gnn_spmm_workspace_bytes(rows, nnz, F, 0), (F, rows, nnz)
                prev = w
    # a few rows of a small closure do not pay the large blocks' floor
    assert L.gnn_spmm_rows_workspace_bytes(9, 18, 16) < 4096


def test_closure_call_refusals_without_gpu():
    """Every refusal comes before any device call: status -22 and the argument's name."""
    L = _lib.lib()
    p = 4096  # a non-NULL, aligned pointer that is never dereferenced
    big = 1 << 40

    def mark(num_nodes=100, n=5, expand=1, indptr=p, indices=p, seeds=p, table=p, count=p, ws=p, wsb=big):
        return L.gnn_closure_mark(indptr, indices, num_nodes, seeds, n, expand, table, count, ws, wsb, None)

    def lst(table=p, num_nodes=100, out=p, cap=10):
        return L.gnn_closure_list(table, num_nodes, out, cap, None)

    def rank(table=p, num_nodes=100, ids=p, n=5, pos=p, err=p):
        return L.gnn_closure_rank(table, num_nodes, ids, n, pos, err, None)

    cases = [
        (mark, dict(num_nodes=-1), b"negative"), (mark, dict(n=-1), b"negative"),
        (mark, dict(num_nodes=2**31 - 1), b"2^31"), (mark, dict(num_nodes=2**40), b"2^31"),
        (mark, dict(n=2**31 - 1), b"2^31"),
        (mark, dict(table=None), b"table"), (mark, dict(table=p + 4), b"table"), (mark, dict(count=None), b"count"),
        (mark, dict(ws=None), b"workspace too small"),
        (mark, dict(wsb=L.gnn_closure_workspace_bytes(100) - 1), b"workspace too small"),
        (mark, dict(num_nodes=2**20 + 37, wsb=L.gnn_closure_workspace_bytes(2**20 + 37) - 1), b"workspace too small"),
        (mark, dict(ws=p + 8), b"16-byte aligned"),
        (mark, dict(seeds=None), b"seeds"), (mark, dict(indptr=None), b"indptr"), (mark, dict(indices=None), b"indices"),
        (lst, dict(num_nodes=-1), b"negative"), (lst, dict(cap=-1), b"negative"), (lst, dict(num_nodes=2**31 - 1), b"2^31"),
        (lst, dict(table=None), b"table"), (lst, dict(out=None), b"out"),
        (rank, dict(num_nodes=-1), b"negative"), (rank, dict(n=-1), b"negative"),
        (rank, dict(num_nodes=2**31 - 1), b"2^31"), (rank, dict(table=None), b"table"),
        (rank, dict(ids=None), b"ids"), (rank, dict(pos=None), b"pos"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == -22, (fn.__name__, kw)
        assert word in L.gnn_last_error(), (fn.__name__, kw, L.gnn_last_error())
    # nothing to do: accepted without a device call
    assert lst(cap=0) == 0 and lst(num_nodes=0) == 0 and rank(n=0, ids=None, pos=None) == 0


def test_rows_call_refusals_without_gpu():
    L = _lib.lib()
    p = 4096
    big = 1 << 40

    def call(num_nodes=100, M=20, nnz=50, K=60, ldx=8, kind=0, ldy=8, F=8, ws=p, wsb=big, X=p, Y=p, table=p, rows=p,
             rowseg=p):
        return L.gnn_spmm_rows_f32(p, p, p, num_nodes, rows, M, rowseg, nnz, table, K, X, ldx, kind, Y, ldy, F, ws, wsb,
                                   None, None)

    cases = [
        (dict(M=-1), b"negative"), (dict(nnz=-1), b"negative"), (dict(num_nodes=-1), b"negative"),
        (dict(F=-4), b"negative"), (dict(K=-1), b"negative"),
        (dict(nnz=2**31 - 1), b"2^31"), (dict(M=2**31 - 1), b"2^31"), (dict(num_nodes=2**31 - 1), b"2^31"),
        (dict(K=2**31 - 1, num_nodes=2**40), b"2^31"), (dict(K=2**31), b"2^31"),
        (dict(K=101), b"num_nodes"),
        (dict(F=12), b"ldx"), (dict(F=12, ldx=12), b"ldy"),
        (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"),
        (dict(wsb=L.gnn_spmm_rows_workspace_bytes(20, 50, 8) - 1), b"workspace too small"),
        (dict(ws=None), b"workspace too small"),
        (dict(ws=p + 8), b"16-byte aligned"),
        (dict(kind=1, F=6), b"multiples of 4"), (dict(kind=2, ldx=10), b"multiples of 4"),
        (dict(kind=1, ldy=10), b"multiples of 4"), (dict(kind=1, X=p + 4), b"X not 8-byte aligned"),
        (dict(kind=2, Y=p + 8), b"Y not 16-byte aligned"),
        (dict(table=None), b"table"), (dict(table=p + 4), b"table"), (dict(rows=None), b"rows"),
        (dict(rowseg=None), b"rowseg"), (dict(Y=None), b"NULL"), (dict(X=None), b"NULL indices/X"),
    ]
    for kw, word in cases:
        assert call(**kw) == -22, kw
        assert word in L.gnn_last_error(), (kw, L.gnn_last_error())
    assert call(M=0, nnz=0) == 0 and call(F=0) == 0


# ----------------------------------------------------------------------------- closure sets

CASES = [("graphsage", [1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1])]
IDS = ["sage11", "sage101", "gcn11"]
N = 600


def reference_levels(lap, orders, nodes):
    """The closure's sets bottom to top by np.unique over the rows' concatenated columns."""
    lap = sp.csr_matrix(lap)
    levels = [np.unique(np.asarray(nodes, dtype=np.int64))]
    for o in reversed(orders):
        top = levels[0]
        if o == 0:
            levels.insert(0, top)
            continue
        cols = np.concatenate([lap.indices[lap.indptr[r]:lap.indptr[r + 1]] for r in top] + [np.zeros(0, np.int32)])
        levels.insert(0, np.unique(np.concatenate([top, cols.astype(np.int64)])))
    return levels


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def world(request):
    name, orders = request.param
    nfeat, C = 20, 7
    lap, feats = make_world(name, N, nfeat)
    model = make_model(name, nfeat, 12, orders, C).eval()
    return model, lap, feats, reference_logits_f64(model, lap, feats), C, orders


QUERIES = {
    "unsorted_dups": np.array([301, 5, 599, 300, 5, 44, 301, 17, 5]),
    "emptied_rows": np.array([0, 77, N - 1]),
    "all": np.arange(N),
    "none": np.zeros(0, np.int64),
}


@pytest.mark.parametrize("qname", list(QUERIES))
def test_closure_sets_equal_numpy_chain(world, qname):
    model, lap, feats, _, C, orders = world
    nodes = QUERIES[qname]
    eng = ExactInference(model, lap, "cpu", max_rows=97)
    c = eng.closure(nodes)
    assert isinstance(c, Closure)
    want = reference_levels(lap, orders, nodes)
    assert c.sizes == [w.size for w in want]
    for l, (got, w) in enumerate(zip(c.sets, want)):
        assert np.array_equal(got, w), (qname, l)
    L = len(orders)
    assert np.array_equal(c.sets[L][c.query_pos.numpy()], nodes)  # caller order, duplicates kept
    ip = sp.csr_matrix(lap).indptr.astype(np.int64)
    for l, o in enumerate(orders):
        if o == 0:  # an order-0 layer repeats its set
            assert c.sets[l] is c.sets[l + 1] and c.self_pos[l] is None and c.blocks[l] is None
            continue
        rows = c.sets[l + 1].astype(np.int64)
        assert np.array_equal(c.sets[l][c.self_pos[l].numpy()], c.sets[l + 1])
        assert np.array_equal(c.scans[l], np.concatenate([[0], np.cumsum(ip[rows + 1] - ip[rows])]))
        blocks = c.blocks[l]
        assert [b[0] for b in blocks] == [0] + [b[1] for b in blocks[:-1]] if blocks else rows.size == 0
        assert all(b - a <= 97 for a, b in blocks) and (blocks[-1][1] if blocks else 0) == rows.size
    if qname == "emptied_rows":  # rows without entries reach nothing: every level is the query set
        assert all(np.array_equal(s, [0, 77, N - 1]) for s in c.sets)
    if qname == "all":
        assert all(np.array_equal(s, np.arange(N)) for s in c.sets)
    if qname == "none":
        z = eng.logits(feats, nodes, scope="closure")
        assert z.shape == (0, C) and eng.embed(feats, closure=c).shape[0] == 0
    with pytest.raises(ValueError, match="nodes"):
        eng.closure([0, N])


def test_ring_closure_is_small():
    """A ring of 5,000 nodes (row i holds i - 1 and i + 1), a 2-layer GraphSAGE and 3 far-apart query
    nodes: levels of exactly 3 / 9 / 15 nodes, 3 embedded rows, and a memory need that follows the
    closure, not the graph."""
    n, nfeat, nhid = 5000, 32, 16
    i = np.arange(n)
    lap = sp.csr_matrix((np.ones(2 * n, np.float32), (np.repeat(i, 2), np.stack([(i - 1) % n, (i + 1) % n], 1).ravel())),
                        shape=(n, n))
    feats = torch.randn(n, nfeat, generator=torch.Generator().manual_seed(2))
    model = make_model("graphsage", nfeat, nhid, [1, 1]).eval()
    eng = ExactInference(model, lap, "cpu")
    nodes = np.array([4000, 100, 2500])
    c = eng.closure(nodes)
    assert c.sizes == [15, 9, 3]
    assert np.array_equal(c.sets[1], np.sort(np.concatenate([nodes - 1, nodes, nodes + 1])))
    full, part = eng.memory_needed(feats), eng.memory_needed(feats, closure=c)
    print(f"ring: memory_needed graph {full} closure {part}")
    assert 0 < part < 0.01 * full
    emb = eng.embed(feats, closure=c)
    assert emb.shape == (3, 2 * nhid)
    z = eng.logits(feats, nodes, scope=c)
    ref = reference_logits_f64(model, lap, feats)[torch.from_numpy(nodes)]
    assert float((z.double() - ref).norm() / ref.norm()) <= 1e-4
    assert torch.equal(z, eng.logits(feats, None, scope=c))  # the closure's own nodes
    # one of its nodes: the same embedded row (the head's product of 1 row against 3 may round apart)
    assert torch.allclose(z[[1]], eng.logits(feats, [100], scope=c), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError, match="outside"):
        eng.logits(feats, [101], scope=c)
    with pytest.raises(ValueError, match="scope"):
        eng.logits(feats, nodes, scope="auto")


# ----------------------------------------------------------------------------- CPU engine


def _rel(z, ref):
    return float((z.double() - ref).norm() / ref.norm())


def test_closure_logits_accuracy(world):
    """err_c <= 1e-4 (the project's whole-forward criterion) and err_c <= 2 err_g + 1e-6: both
    scopes sum the same terms under different blocking, neither order is privileged."""
    model, lap, feats, ref, C, orders = world
    eng = ExactInference(model, lap, "cpu", max_rows=97)
    nodes = np.concatenate([np.arange(40, 560, 3)[::-1], [5, 0, 599, 77, 300, 301, 5, 43]])
    z = eng.logits(feats, nodes, scope="closure")
    assert z.dtype == torch.float32 and z.shape == (len(nodes), C)
    assert eng.orders_taken == ["dense" if o == 0 else "aggregate" for o in orders]
    idx = torch.from_numpy(nodes)
    err_c, err_g = _rel(z, ref[idx]), _rel(eng.logits(feats, nodes), ref[idx])
    print(f"closure cpu {orders}: err_c {err_c:.3e} err_g {err_g:.3e}")
    assert err_c <= 1e-4
    assert err_c <= 2 * err_g + 1e-6
    first, second = [int(np.flatnonzero(nodes == 5)[k]) for k in (0, 1)]
    assert torch.equal(z[first], z[second])  # duplicate queries: equal rows
    c = eng.closure(nodes)
    assert len(c.blocks[0]) >= 2  # more than one block of rows
    assert torch.equal(eng.logits(feats, nodes, scope=c), z)
    assert torch.equal(eng.logits(feats, nodes), eng.logits(feats, nodes, scope="graph"))
    assert not model.training


def test_closure_16bit_table_and_trainer(world):
    from gnn_amd.train import Trainer

    model, lap, feats, _, C, _ = world
    eng = ExactInference(model, lap, "cpu", max_rows=97)
    nodes = np.arange(0, 600, 5)
    h = feats.half()
    assert torch.equal(eng.logits(h, nodes, scope="closure"), eng.logits(h.float(), nodes, scope="closure"))
    labels = one_hot_labels(len(nodes), C)
    tr = Trainer(model, 1e-3, "cpu")
    for training in (True, False):
        model.train(training)
        res = tr.evaluate_exact(lap, feats, nodes, labels, scope="closure")
        assert model.training == training
        assert set(res) == set(tr.evaluate_exact(lap, feats, nodes, labels, scope="graph"))
        assert res == ExactInference(model.eval(), lap, "cpu").evaluate(feats, nodes, labels, scope="closure")
        model.train(training)
    model.eval()


def test_closure_evaluate_counts(world):
    model, lap, feats, _, C, _ = world
    eng = ExactInference(model, lap, "cpu", max_rows=97)
    nodes = np.arange(40, 560, 3)
    z = eng.logits(feats, nodes, scope="closure")
    labels = one_hot_labels(len(nodes), C)
    for sigmoid_loss, mode in ((True, 0), (False, 1)):
        res = eng.evaluate(feats, nodes, labels, sigmoid_loss=sigmoid_loss, mode=mode, scope="closure")
        want = metrics.prediction_counts(z, labels, mode).numpy().astype(np.int64)
        assert np.array_equal(eng.last_counts, want)
        assert res["rows"] == len(nodes)
        assert res["loss"] == pytest.approx(float(models.loss(z, labels, sigmoid_loss, "cpu")), rel=1e-5)
        assert set(res) == {"micro_f1", "macro_f1", "loss", "batches", "rows", "ref_batch_weighted_micro_f1"}
