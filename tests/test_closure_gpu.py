"""Closure-scope inference on the GPU: the set kernels (gnn_closure_mark / list / rank) against
numpy, gnn_spmm_rows_f32's operand against its np.searchsorted materialisation and against
gnn_ladies_extract_f32, its sums against spmm_csr on that operand, the guard, refusals, capture;
then the engine in closure scope against the CPU engine's sets and the float64 reference."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle as O
from gnn_amd import _lib, metrics, models
from gnn_amd import custom_sparse_ops as cso
from gnn_amd.inference import ExactInference
from gnn_amd.sampler import NativeGraph, device_graph
from test_exact_cpu import make_model, make_world, one_hot_labels, reference_logits_f64
from test_exact_gpu import _hand_graph

pytestmark = pytest.mark.gpu

N = 2000
WIDTHS = [(4, 4), (26, 26), (256, 256), (602, 608)]  # (F, row stride)


@pytest.fixture(scope="module")
def graph(dev):
    g = NativeGraph(_hand_graph())
    return g, device_graph(g, dev)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _entries(g, rows):
    """(concatenated columns, degrees) of the graph rows ``rows`` on the host."""
    rows = np.asarray(rows, dtype=np.int64)
    deg = (g.indptr[rows + 1] - g.indptr[rows]).astype(np.int64)
    ent = np.concatenate([g.indices[g.indptr[r]:g.indptr[r + 1]] for r in rows] + [np.zeros(0, np.int32)])
    return ent.astype(np.int64), deg


def _table_words(S, n):
    """The membership table of the ascending set S over n nodes as int32 [words + 1, 2]."""
    words = (n + 31) // 32
    x = np.zeros(words + 1, np.uint32)
    np.bitwise_or.at(x, S >> 5, (np.uint32(1) << (S & 31).astype(np.uint32)))
    pop = np.array([bin(int(v)).count("1") for v in x], np.int64)
    y = np.concatenate([[0], np.cumsum(pop)[:-1]]).astype(np.uint32)
    y[words] = S.size
    return np.stack([x, y], 1).view(np.int32)


def _read_table(table, n):
    words = (n + 31) // 32
    return table[: (words + 1) * 8].view(torch.int32).view(-1, 2).cpu().numpy()


def _check_set(dgraph, n, seeds, expand, S, dev):
    """mark / list / rank of one seed list against the ascending numpy set S."""
    L = _lib.lib()
    ds = _t(np.asarray(seeds, dtype=np.int32), dev)
    table, count = cso.closure_mark(dgraph, ds, expand)
    assert int(count.item()) == S.size
    got = _read_table(table, n)
    assert np.array_equal(got, _table_words(S, n))
    table2, count2 = cso.closure_mark(dgraph, ds, expand)  # two calls: equal bits
    assert int(count2.item()) == S.size and np.array_equal(_read_table(table2, n), got)
    assert np.array_equal(cso.closure_list(table, n, S.size).cpu().numpy(), S.astype(np.int32))
    if S.size >= 3:  # a short list: nothing at or past cap
        out = torch.full((S.size,), -7, dtype=torch.int32, device=dev)
        _lib.check(L.gnn_closure_list(table.data_ptr(), n, out.data_ptr(), S.size - 3, _lib.stream_of(dev)), "list")
        out = out.cpu().numpy()
        assert np.array_equal(out[: S.size - 3], S[: S.size - 3]) and np.all(out[S.size - 3:] == -7)
    ids = np.random.default_rng(1).permutation(n).astype(np.int32)  # a shuffled superset
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    pos = cso.closure_rank(table, n, _t(ids, dev), err).cpu().numpy()
    member = np.isin(ids, S)
    want = np.where(member, np.searchsorted(S, ids), 0)
    assert pos.dtype == np.int64 and np.array_equal(pos, want)
    assert int(err.item()) == (0 if member.all() else 1)
    if S.size:  # members only: the flag stays clear
        err.zero_()
        assert np.array_equal(cso.closure_rank(table, n, _t(S[::-1].astype(np.int32), dev), err).cpu().numpy(),
                              np.arange(S.size)[::-1])
        assert int(err.item()) == 0


SEEDS = {
    "word_edges": [0, 31, 32, 63, 64, 1999],
    "degree0": [2],
    "degree1500": [15, 800, 1500],
    "repeats": np.random.default_rng(3).integers(0, N, 300).tolist(),
    "all": list(range(N)),
    "none": [],
}


@pytest.mark.parametrize("expand", [0, 1])
@pytest.mark.parametrize("name", list(SEEDS))
def test_mark_list_rank_hand_graph(graph, dev, name, expand):
    g, dg = graph
    seeds = np.asarray(SEEDS[name], dtype=np.int64)
    if name == "repeats":
        assert np.unique(seeds).size < seeds.size
    if name == "degree0":
        assert g.indptr[3] == g.indptr[2]
    if name == "degree1500":
        assert all(g.indptr[s + 1] - g.indptr[s] == 1500 for s in seeds)
    ent, _ = _entries(g, seeds)
    S = np.unique(np.concatenate([seeds, ent])) if expand else np.unique(seeds)
    _check_set(dg, N, seeds, expand, S, dev)


def test_mark_multi_chunk_scan(dev):
    """2^20 + 37 nodes: 32,770 table words, five chunks of the 8,192-word scan workgroups (the
    chunk-sum scan and the chunk add both matter), two random entries per row, 50,000 seeds."""
    n = 2**20 + 37
    assert (n + 31) // 32 > 4 * 8192
    rng = np.random.default_rng(11)
    indices = np.sort(rng.integers(0, n, (n, 2)), axis=1).astype(np.int32).ravel()
    indptr = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    dg = SimpleNamespace(indptr=_t(indptr, dev), indices=_t(indices, dev), num_nodes=n,
                         device=_t(indptr[:1], dev).device)
    seeds = rng.integers(0, n, 50_000)
    S = np.unique(np.concatenate([seeds, indices.reshape(n, 2)[seeds].ravel().astype(np.int64)]))
    _check_set(dg, n, seeds, 1, S, dev)


# ----------------------------------------------------------------------------- gnn_spmm_rows_f32

ROWS_CUT = np.unique(np.concatenate([np.arange(0, N, 3), np.arange(10, 16), [800, 801, 1500]]))
ROWS_SHORT = np.arange(1700, N)


def _al(b):
    return (b + 255) // 256 * 256


def _operand(g, rows, S):
    """lap[rows, :][:, S] as spmm_csr reads it, by np.searchsorted: (rowptr, col, val); a column
    outside S becomes column 0 with value 0."""
    ent, deg = _entries(g, rows)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    pos = np.searchsorted(S, ent)
    inside = (pos < S.size) & (S[np.minimum(pos, S.size - 1)] == ent)
    with np.errstate(divide="ignore"):
        w = (1.0 / deg.astype(np.float64)).astype(np.float32)
    col = np.where(inside, pos, 0).astype(np.int32)
    val = np.where(inside, np.repeat(w, deg), np.float32(0)).astype(np.float32)
    return rowptr, col, val


def _rows_call(dg, rows_d, rowseg_d, nnz, table, K, X, F, dev, err=None, Y=None):
    """gnn_spmm_rows_f32 with a workspace of the test's own: (Y, rowptr, col, val) of the block."""
    L = _lib.lib()
    M = rows_d.numel()
    ld = X.stride(0)
    Y = torch.empty((M, F), dtype=torch.float32, device=dev) if Y is None else Y
    wsb = L.gnn_spmm_rows_workspace_bytes(M, nnz, F)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.gnn_spmm_rows_f32(dg.indptr.data_ptr(), dg.indices.data_ptr(), dg.degree.data_ptr(), N,
                                   rows_d.data_ptr(), M, rowseg_d.data_ptr(), nnz, table.data_ptr(), K, X.data_ptr(), ld,
                                   cso.FEAT_KIND[X.dtype], Y.data_ptr(), Y.stride(0), F, ws.data_ptr(), wsb,
                                   None if err is None else err.data_ptr(), _lib.stream_of(dev)), "gnn_spmm_rows_f32")
    o1 = _al(4 * (M + 1))
    o2 = o1 + _al(4 * nnz)
    rowptr = ws[: 4 * (M + 1)].view(torch.int32)
    col = ws[o1: o1 + 4 * nnz].view(torch.int32)
    val = ws[o2: o2 + 4 * nnz].view(torch.float32)
    return Y, rowptr, col, val


@pytest.fixture(scope="module", params=["cut", "short"])
def block(request, graph, dev):
    """A row list, its closure as the column set (table, K, S) and the materialised operand."""
    g, dg = graph
    rows = ROWS_CUT if request.param == "cut" else ROWS_SHORT
    ent, deg = _entries(g, rows)
    S = np.unique(np.concatenate([rows, ent]))
    rows_d = _t(rows.astype(np.int32), dev)
    table, count = cso.closure_mark(dg, rows_d, True)
    K = int(count.item())
    assert K == S.size
    if request.param == "short":
        assert K < N  # the columns are positions in the set, not node ids
    rowptr, col, val = _operand(g, rows, S)
    op = cso.CsrOperand(_t(rowptr, dev), _t(col, dev), _t(val, dev), (rows.size, K))
    return SimpleNamespace(name=request.param, rows=rows, rows_d=rows_d, rowseg=_t(rowptr, dev), nnz=int(rowptr[-1]),
                           table=table, K=K, S=S, op=op, host=(rowptr, col, val), deg=deg)


def test_rows_operand_equals_materialisation_and_extract(graph, dev, block):
    g, dg = graph
    b = block
    if b.name == "cut":  # empty rows at both ends, rows of 1,500 entries cut across units
        assert b.deg[0] == 0 and b.deg[-1] == 0 and (b.deg == 1500).sum() == 3
    X = torch.randn(b.K, 8, device=dev)
    _, rowptr, col, val = _rows_call(dg, b.rows_d, b.rowseg, b.nnz, b.table, b.K, X, 8, dev)
    assert torch.equal(rowptr, b.op.rowptr) and torch.equal(col, b.op.col) and torch.equal(val, b.op.val)
    assert int(col.max()) < b.K
    ex = cso.extract_operand(dg, b.rows_d, _t(b.S.astype(np.int32), dev), torch.ones(b.K, device=dev), b.nnz, b.rowseg,
                             rowseg_total=b.nnz)
    assert torch.equal(rowptr, ex.rowptr) and torch.equal(col, ex.col) and torch.equal(val, ex.val)
    dg.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("F,ld", WIDTHS)
def test_rows_sums_equal_spmm_csr(graph, dev, block, F, ld, dtype):
    g, dg = graph
    b = block
    X = torch.randn(b.K, ld, generator=torch.Generator().manual_seed(F)).to(dtype).to(dev)[:, :F]
    want = cso.spmm_csr(b.op, X)
    got = cso.spmm_rows(dg, b.rows_d, b.rowseg, b.nnz, b.table, b.K, X)
    assert got.dtype == torch.float32 and got.shape == want.shape and got.stride() == want.stride()
    assert torch.equal(got, want), (b.name, F, dtype)
    if dtype == torch.float32:
        Fk = (F + 3) & ~3 if ld != F else F
        kernel = cso.spmm_config(b.rows.size, b.nnz, Fk, ld, ld if Fk != F else F, K=b.K)["kernel"]
        assert kernel.startswith("spmm_row_kernel" if b.name == "short" else "spmm_unit_kernel"), kernel
        if b.name == "cut" and F == 256:  # fp64: err <= 1e-5 |A| |X| + 1e-6, no exception budget
            rowptr, col, val = b.host
            Xh = X.cpu().numpy()
            y64, yabs = O.spmm_f64(rowptr, col, val, Xh), O.spmm_abs(rowptr, col, val, Xh)
            err = np.abs(got.cpu().numpy().astype(np.float64) - y64)
            assert np.all(err <= 1e-5 * yabs + 1e-6), float((err - 1e-5 * yabs).max())
            assert not got[0].any() and not got[-1].any()  # the empty rows at both ends
    dg.check()


def test_rows_guard_column_outside_the_set(graph, dev):
    """A table built without one neighbour of one row: the flag reads 1, every stored column is
    below K, that row sums the remaining terms and the other rows are unchanged. The call is in
    bounds by construction — the missing column is stored as column 0 with weight 0."""
    g, dg = graph
    rows = ROWS_SHORT
    ent, deg = _entries(g, rows)
    S = np.unique(np.concatenate([rows, ent]))
    cnt = np.bincount(ent, minlength=N)
    cnt[rows] = 0  # not a row of the list: its self position stays out of the picture
    gone = int(np.flatnonzero(cnt == 1)[0])  # a column that exactly one entry of the list names
    row_hit = int(np.searchsorted(np.cumsum(deg), int(np.flatnonzero(ent == gone)[0]), side="right"))
    S1 = S[S != gone]
    rows_d = _t(rows.astype(np.int32), dev)
    table, _ = cso.closure_mark(dg, rows_d, True)
    table1, count1 = cso.closure_mark(dg, _t(S1.astype(np.int32), dev), False)
    K, K1 = S.size, int(count1.item())
    assert K1 == K - 1
    rowptr, col, val = _operand(g, rows, S1)
    assert (val == 0).sum() == 1
    rowseg, nnz = _t(rowptr, dev), int(rowptr[-1])
    X = torch.randn(K, 26, device=dev)
    X1 = X[_t(np.flatnonzero(S != gone), dev)].contiguous()
    full, *_ = _rows_call(dg, rows_d, rowseg, nnz, table, K, X, 26, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    got, rp, cl, vl = _rows_call(dg, rows_d, rowseg, nnz, table1, K1, X1, 26, dev, err=err)
    assert int(err.item()) == 1
    assert int(cl.max()) < K1 and torch.equal(cl, _t(col, dev)) and torch.equal(vl, _t(val, dev))
    others = np.arange(rows.size) != row_hit
    assert torch.equal(got[_t(others, dev)], full[_t(others, dev)])
    y64 = O.spmm_f64(rowptr, col, val, X1.cpu().numpy())
    assert np.allclose(got.cpu().numpy(), y64, rtol=1e-5, atol=1e-6)
    assert not torch.equal(got[row_hit], full[row_hit])
    assert int(dg.err.item()) == 0  # the test's own flag took it


def test_rows_refusals_launch_nothing_and_capture(graph, dev, block):
    g, dg = graph
    b = block
    L = _lib.lib()
    M = b.rows.size
    X = torch.randn(b.K, 608, device=dev).half()
    Y = torch.full((M, 608), -7.0, device=dev)
    wsb = L.gnn_spmm_rows_workspace_bytes(M, b.nnz, 608)
    ws = torch.empty(wsb + 64, dtype=torch.uint8, device=dev)

    def call(**kw):
        a = dict(num_nodes=N, M=M, nnz=b.nnz, K=b.K, X=X.data_ptr(), ldx=608, kind=1, Y=Y.data_ptr(), ldy=608, F=608,
                 ws=ws.data_ptr(), wsb=wsb, table=b.table.data_ptr())
        a.update(kw)
        return L.gnn_spmm_rows_f32(dg.indptr.data_ptr(), dg.indices.data_ptr(), dg.degree.data_ptr(), a["num_nodes"],
                                   b.rows_d.data_ptr(), a["M"], b.rowseg.data_ptr(), a["nnz"], a["table"], a["K"], a["X"],
                                   a["ldx"], a["kind"], a["Y"], a["ldy"], a["F"], a["ws"], a["wsb"], None,
                                   _lib.stream_of(dev))

    cases = [(dict(kind=3), b"kind"), (dict(X=X.data_ptr() + 2), b"X not 8-byte aligned"),
             (dict(Y=Y.data_ptr() + 8), b"Y not 16-byte aligned"), (dict(F=602), b"multiples of 4"),
             (dict(ldx=606, F=604), b"multiples of 4"), (dict(ldy=610), b"multiples of 4"),
             (dict(F=612), b"ldx"), (dict(ldy=604), b"ldy"),
             (dict(wsb=wsb - 1), b"workspace too small"), (dict(ws=ws.data_ptr() + 8), b"16-byte aligned"),
             (dict(K=N + 1), b"num_nodes"), (dict(K=2**31), b"2^31"), (dict(nnz=2**31), b"2^31"),
             (dict(M=-1), b"negative"), (dict(table=None), b"table")]
    for kw, word in cases:
        assert call(**kw) == -22, kw
        assert word in L.gnn_last_error(), (kw, L.gnn_last_error())
    torch.cuda.synchronize()
    assert bool((Y == -7.0).all())  # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    direct = cso.spmm_rows(dg, b.rows_d, b.rowseg, b.nnz, b.table, b.K, X)
    assert torch.equal(Y, direct)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):  # one stream, no parallel branches
        y = cso.spmm_rows(dg, b.rows_d, b.rowseg, b.nnz, b.table, b.K, X)
    y.fill_(-7.0)
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, direct)
    dg.check()


# ----------------------------------------------------------------------------- the engine

ENGINE = [("graphsage", [1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1])]


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


@pytest.mark.parametrize("name,orders", ENGINE, ids=["sage11", "sage101", "gcn11"])
def test_engine_closure_scope(dev, monkeypatch, name, orders):
    NN, C, nfeat, nhid = 600, 7, 48, 16
    lap, feats = make_world(name, NN, nfeat)
    cpu_model = make_model(name, nfeat, nhid, orders, C).eval()
    ref = reference_logits_f64(cpu_model, lap, feats)
    model = models.build_model(name, nfeat, nhid, orders, C, dropout=0.1, fused=True)
    model.load_state_dict(cpu_model.state_dict())
    model = model.to(dev).eval()
    nodes = np.concatenate([np.arange(40, 560, 3), [43, 40, 556, 43]])  # duplicates appended

    eng = ExactInference(model, lap, dev, max_rows=97)
    c = eng.closure(nodes)
    c_cpu = ExactInference(cpu_model, lap, "cpu", max_rows=97).closure(nodes)
    assert c.sizes == c_cpu.sizes and len(c.blocks[0]) >= 2
    for l in range(len(orders) + 1):
        assert np.array_equal(c.sets[l], c_cpu.sets[l]) and np.array_equal(c.dsets[l].cpu().numpy(), c.sets[l])
    for l, o in enumerate(orders):
        if o == 0:
            assert c.sets[l] is c.sets[l + 1] and c.self_pos[l] is None
        else:
            assert np.array_equal(c.self_pos[l].cpu().numpy(), c_cpu.self_pos[l].numpy())
            assert np.array_equal(c.scans[l], c_cpu.scans[l]) and c.blocks[l] == c_cpu.blocks[l]
    assert np.array_equal(c.query_pos.cpu().numpy(), c_cpu.query_pos.numpy())

    z = eng.logits(feats, nodes, scope="closure")
    assert eng.orders_taken[0] == "project"  # 48 -> 16: the shape rule of the full-graph scope
    z_g = eng.logits(feats, nodes)
    idx = torch.from_numpy(nodes)
    err_c, err_g = _rel(z, ref[idx]), _rel(z_g, ref[idx])
    print(f"closure gpu {name} {orders}: err_c {err_c:.3e} err_g {err_g:.3e}")
    assert z.shape == (len(nodes), C) and err_c <= 1e-4
    assert err_c <= 2 * err_g + 1e-6
    assert torch.equal(z[-1], z[1]) and torch.equal(z[-3], z[0])  # duplicates: equal rows
    assert torch.equal(eng.logits(feats, nodes, scope=c), z)
    assert torch.equal(eng.logits(feats.to(dev), nodes, scope=c), z)  # a device table: gathered there
    assert eng.logits(feats, [], scope="closure").shape == (0, C)

    # 16-bit tables equal their widened runs, from the host and from the device
    for dt in (torch.float16, torch.bfloat16):
        h = feats.to(dt)
        zh = eng.logits(h.float(), nodes, scope=c)
        assert torch.equal(eng.logits(h, nodes, scope=c), zh)
        assert torch.equal(eng.logits(h.to(dev), nodes, scope=c), zh)

    # evaluate: counts and loss of its own closure logits
    labels = one_hot_labels(len(nodes), C)
    res = eng.evaluate(feats, nodes, labels, scope="closure")
    want = metrics.prediction_counts(z, labels.to(dev), 0).cpu().numpy().astype(np.int64)
    assert np.array_equal(eng.last_counts, want)
    assert res["loss"] == pytest.approx(float(models.loss(z, labels.to(dev), True, dev)), rel=1e-5)
    assert res["rows"] == len(nodes)

    # an aggregate-first layer 0 (12 -> 32) through the same blocks
    lap2, feats2 = make_world(name, NN, 12)
    cpu2 = make_model(name, 12, 32, orders, C).eval()
    m2 = models.build_model(name, 12, 32, orders, C, dropout=0.1, fused=True)
    m2.load_state_dict(cpu2.state_dict())
    eng2 = ExactInference(m2.to(dev).eval(), lap2, dev, max_rows=97)
    ref2 = reference_logits_f64(cpu2, lap2, feats2)[idx]
    z2, z2g = eng2.logits(feats2, nodes, scope="closure"), eng2.logits(feats2, nodes)
    assert eng2.orders_taken[0] == "aggregate"
    e_c, e_g = _rel(z2, ref2), _rel(z2g, ref2)
    print(f"closure gpu {name} {orders} aggregate: err_c {e_c:.3e} err_g {e_g:.3e}")
    assert e_c <= 1e-4 and e_c <= 2 * e_g + 1e-6

    # the memory check comes before any allocation
    need = eng.memory_needed(feats, closure=c)
    assert need < eng.memory_needed(feats)
    monkeypatch.setattr(ExactInference, "_free_bytes", lambda self: need - 1)
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(RuntimeError, match=str(need)):
        eng.embed(feats, closure=c)
    assert torch.cuda.memory_allocated(dev) == before
