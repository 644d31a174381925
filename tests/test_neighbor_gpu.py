"""Node-wise neighbour sampling on the GPU: gnn_nbr_rowptr / draw / relabel against the numpy
restatement bit for bit, the guards, refusals and capture; then NeighborSampler against
neighbor_sample_host array for array, through the native training step against the Python
autograd path, and at full fanout against the float64 reference.

The hand-built graph has 1,400 nodes, not "about 400": a row of 1,000 distinct columns needs at
least 1,000 of them. The degrees, fanouts, seeds and layer indices are the ones asked for."""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib, models
from gnn_amd import custom_sparse_ops as cso
from gnn_amd import executor as E
from gnn_amd.inference import ExactInference
from gnn_amd.neighbor import NeighborSampler, neighbor_sample_host
from gnn_amd.sampler import NativeGraph, device_graph
from gnn_amd.train import Evaluator, Trainer
from test_exact_cpu import make_model, make_world, reference_logits_f64
from test_neighbor_cpu import BATCH, CASES, IDS, NN, _labels, small_degree_world

pytestmark = pytest.mark.gpu

N = 1400
DEGREES = [0, 1, 2, 5, 63, 64, 65, 130, 1000]
SEEDS = [3, (0x9ABCDEF1 << 32) | 0x12345678]


def _hand_lap():
    """Row i has DEGREES[i % 9] distinct columns, ascending; the last row (1,000 entries) ends at
    column N - 1 and row 10's single entry is column N - 1 too."""
    rng = np.random.default_rng(7)
    deg = np.array([DEGREES[i % 9] for i in range(N)])
    deg[N - 1] = 1000
    cols = []
    for i in range(N):
        c = np.sort(rng.choice(N, deg[i], replace=False))
        if i in (10, N - 1) and c.size and c[-1] != N - 1:
            c[-1] = N - 1
        cols.append(c)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    data = np.repeat(1.0 / np.maximum(deg, 1), deg).astype(np.float32)
    return sp.csr_matrix((data, np.concatenate(cols).astype(np.int32), indptr), shape=(N, N))


@pytest.fixture(scope="module")
def graph(dev):
    g = NativeGraph(_hand_lap())
    assert g.data is None and sorted(set(np.diff(g.indptr))) == DEGREES and g.indices.max() == N - 1
    return g, device_graph(g, dev)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# out of order, with repeats, every degree, the first and the last node
ROWS = np.concatenate([np.random.default_rng(5).permutation(N)[:300], [N - 1, 0, 8, 17, 8, N - 1, 7, 7]])
TAIL = 64  # sentinel entries behind every output


def _draw(indptr, indices, rows, f, seed, layer, dev, cap=None, n_nodes=N, n_entries=None):
    """gnn_nbr_rowptr + gnn_nbr_draw with sentinel-filled outputs: (rowptr, total, ids, val, err)."""
    L = _lib.lib()
    M = rows.numel()
    cap = M * f if cap is None else cap
    E_ = int(indices.numel()) if n_entries is None else n_entries
    rowptr = torch.full((M + 1 + TAIL,), -7, dtype=torch.int32, device=dev)
    total = torch.full((1 + TAIL,), -7, dtype=torch.int64, device=dev)
    ids = torch.full((cap + TAIL,), -7, dtype=torch.int32, device=dev)
    val = torch.full((cap + TAIL,), -7.0, dtype=torch.float32, device=dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    wsb = L.gnn_nbr_workspace_bytes(M)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = _lib.stream_of(dev)
    _lib.check(L.gnn_nbr_rowptr(indptr.data_ptr(), n_nodes, E_, rows.data_ptr(), M, f, rowptr.data_ptr(),
                                total.data_ptr(), ws.data_ptr(), wsb, err.data_ptr(), st), "gnn_nbr_rowptr")
    _lib.check(L.gnn_nbr_draw(indptr.data_ptr(), indices.data_ptr(), n_nodes, E_, rows.data_ptr(), M, f, seed, layer,
                              rowptr.data_ptr(), ids.data_ptr(), val.data_ptr(), cap, err.data_ptr(), st), "gnn_nbr_draw")
    return rowptr, total, ids, val, err


def _set_and_columns(rows, ids, nnz, dev, err):
    """The layer's input set and relabelled columns: mark(rows ++ ids), list, relabel."""
    L = _lib.lib()
    seeds = torch.cat([rows, ids[:nnz]]).contiguous()
    dg = SimpleNamespace(indptr=None, indices=None, num_nodes=N, device=rows.device)
    table, count = cso.closure_mark(dg, seeds, False)
    K = int(count.item())
    low = cso.closure_list(table, N, K)
    col = torch.full((nnz + TAIL,), -7, dtype=torch.int32, device=dev)
    val0 = torch.full((nnz + TAIL,), -7.0, dtype=torch.float32, device=dev)
    _lib.check(L.gnn_nbr_relabel(table.data_ptr(), N, ids.data_ptr(), nnz, col.data_ptr(), val0.data_ptr(),
                                 err.data_ptr(), _lib.stream_of(dev)), "gnn_nbr_relabel")
    return K, low, col, val0


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("seed", SEEDS, ids=["seed_lo", "seed_hi"])
@pytest.mark.parametrize("f", [1, 5, 64])
def test_draw_is_bit_exact(graph, dev, f, seed, layer):
    g, dg = graph
    rows = _t(ROWS.astype(np.int32), dev)
    M = ROWS.size
    hb = neighbor_sample_host(seed, ROWS, f, g, [1] if layer == 0 else [0, 1])
    w_rowptr, w_col, w_val, (_, K_want) = hb.layers[layer]
    low_want = hb.sets[layer]
    nnz = int(w_rowptr[-1])
    deg = np.diff(g.indptr)[ROWS]
    assert nnz == np.minimum(deg, f).sum() and (f == 64 or nnz < M * f) and set(deg) == set(DEGREES)

    rowptr, total, ids, val, err = _draw(dg.indptr, dg.indices, rows, f, seed, layer, dev)
    assert np.array_equal(rowptr[: M + 1].cpu().numpy(), w_rowptr) and int(total[0]) == nnz
    assert np.array_equal(ids[:nnz].cpu().numpy(), low_want[w_col])
    assert np.array_equal(val[:nnz].cpu().numpy(), w_val)
    K, low, col, val0 = _set_and_columns(rows, ids, nnz, dev, err)
    assert K == K_want and np.array_equal(low.cpu().numpy(), low_want)
    assert col.dtype == torch.int32 and np.array_equal(col[:nnz].cpu().numpy(), w_col)
    assert not err.any()
    # nothing behind the outputs, nothing between nnz and the capacity
    assert bool((rowptr[M + 1:] == -7).all()) and bool((total[1:] == -7).all())
    assert bool((ids[nnz:] == -7).all()) and bool((val[nnz:] == -7.0).all())
    assert bool((col[nnz:] == -7).all()) and bool((val0 == -7.0).all())  # every id is a member: no weight zeroed


def test_rowptr_multi_chunk_scan(graph, dev):
    """20,000 rows: three chunks of the 8,192-row scan workgroups (the chunk add matters)."""
    g, dg = graph
    rows_h = np.random.default_rng(9).integers(0, N, 20_000)
    rows = _t(rows_h.astype(np.int32), dev)
    rowptr, total, ids, val, err = _draw(dg.indptr, dg.indices, rows, 5, 1, 0, dev)
    want = np.concatenate([[0], np.cumsum(np.minimum(np.diff(g.indptr)[rows_h], 5))])
    assert np.array_equal(rowptr[:20_001].cpu().numpy(), want) and int(total[0]) == want[-1] and not err.any()
    hb = neighbor_sample_host(1, rows_h, 5, g, [1])
    assert np.array_equal(ids[: want[-1]].cpu().numpy(), hb.sets[0][hb.layers[0][1]])


def test_guards(graph, dev):
    """Row ids outside the graph, column ids >= N planted in a copy of the graph, a row pointer past
    the index array, an output capacity below the draw: the flag is set each time, every stored
    column is below K, and nothing is written past rowptr[M] or the capacity."""
    g, dg = graph
    f, seed = 5, 3
    deg = np.diff(g.indptr)
    r2, r130 = 11, 16  # rows of degree 2 and 130
    assert deg[r2] == 2 and deg[r130] == 130
    indices = g.indices.copy()
    indices[g.indptr[r2] + 1] = N + 3  # kept: the whole row is
    indices[g.indptr[r130]:g.indptr[r130 + 1]] = N + np.arange(130)  # whichever five are kept
    base = ROWS[:100][~np.isin(ROWS[:100], [r2, r130])]  # rows the planted columns do not touch
    rows_h = np.concatenate([base, [N + 5, -3, r2, 2**31 - 1, r130]]).astype(np.int64)
    rows = _t(rows_h.astype(np.int32), dev)
    M = rows_h.size
    inside = (rows_h >= 0) & (rows_h < N)
    k = np.where(inside, np.minimum(deg[np.where(inside, rows_h, 0)], f), 0)
    w_rowptr = np.concatenate([[0], np.cumsum(k)])
    nnz = int(w_rowptr[-1])

    rowptr, total, ids, val, err = _draw(dg.indptr, _t(indices, dev), rows, f, seed, 0, dev)
    assert int(err[0]) == 1 and not err[1:].any()
    assert np.array_equal(rowptr[: M + 1].cpu().numpy(), w_rowptr) and int(total[0]) == nnz
    assert bool((ids[nnz:] == -7).all()) and bool((val[nnz:] == -7.0).all()) and bool((rowptr[M + 1:] == -7).all())
    ids_h, val_h = ids[:nnz].cpu().numpy(), val[:nnz].cpu().numpy()
    bad = ids_h == -1
    assert bad.sum() == 6 and np.all(val_h[bad] == 0) and np.all(val_h[~bad] > 0)
    assert np.all((ids_h[~bad] >= 0) & (ids_h[~bad] < N))
    # the valid rows are the undisturbed graph's draw
    hb = neighbor_sample_host(seed, base, f, g, [1])
    n100 = int(hb.layers[0][0][-1])
    assert np.array_equal(ids_h[:n100], hb.sets[0][hb.layers[0][1]])
    err2 = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    K, low, col, val0 = _set_and_columns(_t(rows_h[inside].astype(np.int32), dev), ids, nnz, dev, err2)
    col_h = col[:nnz].cpu().numpy()
    assert int(err2[0]) == 1 and K == low.numel() and col_h.max() < K and np.all(col_h[bad] == 0)
    assert np.array_equal(low.cpu().numpy()[col_h[~bad]], ids_h[~bad])
    assert np.all(val0[:nnz].cpu().numpy()[bad] == 0) and bool((val0[:nnz][_t(~bad, dev)] == -7.0).all())
    assert bool((col[nnz:] == -7).all()) and bool((val0[nnz:] == -7.0).all())

    # a row pointer that ends past the index array: the last row keeps nothing
    indptr = g.indptr.copy()
    indptr[N] += 50
    rows3 = _t(np.array([N - 1, 4, N - 1], np.int32), dev)
    rowptr, total, ids, val, err = _draw(_t(indptr, dev), dg.indices, rows3, f, seed, 0, dev)
    assert int(err[0]) == 1 and rowptr[:4].tolist() == [0, 0, 5, 5] and int(total[0]) == 5
    assert bool((ids[5:] == -7).all()) and bool((ids[:5] >= 0).all())
    # ... and one running backwards
    indptr = g.indptr.copy()
    indptr[5] = indptr[4] - 1
    rowptr, total, ids, val, err = _draw(_t(indptr, dev), dg.indices, _t(np.array([4], np.int32), dev), f, seed, 0, dev)
    assert int(err[0]) == 1 and rowptr[:2].tolist() == [0, 0] and bool((ids == -7).all())

    # a capacity below the draw: the rows that would leave it are skipped
    rows4 = _t(ROWS[:50].astype(np.int32), dev)
    full = _draw(dg.indptr, dg.indices, rows4, f, seed, 0, dev)
    n4 = int(full[1][0])
    short = _draw(dg.indptr, dg.indices, rows4, f, seed, 0, dev, cap=n4 - 7)
    assert int(full[4][0]) == 0 and int(short[4][0]) == 1
    assert bool((short[2][n4 - 7:] == -7).all()) and bool((short[3][n4 - 7:] == -7.0).all())
    rp = full[0][:51].cpu().numpy()
    last = int(np.searchsorted(rp, n4 - 7, side="right")) - 1  # rows [0, last) end inside the capacity
    assert torch.equal(short[2][: rp[last]], full[2][: rp[last]])


def test_refusals_launch_nothing_and_capture(graph, dev):
    g, dg = graph
    L = _lib.lib()
    rows = _t(ROWS.astype(np.int32), dev)
    M, f = ROWS.size, 5
    cap = M * f
    Eg = int(dg.indices.numel())
    rowptr = torch.full((M + 1,), -7, dtype=torch.int32, device=dev)
    total = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ids = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    val = torch.full((cap,), -7.0, dtype=torch.float32, device=dev)
    col = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    wsb = L.gnn_nbr_workspace_bytes(M)
    ws = torch.empty(wsb + 64, dtype=torch.uint8, device=dev)
    table, _ = cso.closure_mark(dg, rows, True)
    good_rowptr = _draw(dg.indptr, dg.indices, rows, f, 3, 0, dev)[0][: M + 1].contiguous()
    torch.cuda.synchronize()
    st = _lib.stream_of(dev)

    def c_rowptr(**kw):
        a = dict(N=N, E=Eg, M=M, f=f, rowptr=rowptr.data_ptr(), total=total.data_ptr(), ws=ws.data_ptr(), wsb=wsb)
        a.update(kw)
        return L.gnn_nbr_rowptr(dg.indptr.data_ptr(), a["N"], a["E"], rows.data_ptr(), a["M"], a["f"], a["rowptr"],
                                a["total"], a["ws"], a["wsb"], None, st)

    def c_draw(**kw):
        a = dict(N=N, E=Eg, M=M, f=f, ids=ids.data_ptr(), val=val.data_ptr(), cap=cap, rp=good_rowptr.data_ptr())
        a.update(kw)
        return L.gnn_nbr_draw(dg.indptr.data_ptr(), dg.indices.data_ptr(), a["N"], a["E"], rows.data_ptr(), a["M"],
                              a["f"], 3, 0, a["rp"], a["ids"], a["val"], a["cap"], None, st)

    def c_relabel(**kw):
        a = dict(table=table.data_ptr(), N=N, n=cap, col=col.data_ptr())
        a.update(kw)
        return L.gnn_nbr_relabel(a["table"], a["N"], rows.data_ptr(), a["n"], a["col"], None, None, st)

    cases = [(c_rowptr, dict(M=-1), b"negative"), (c_rowptr, dict(N=2**31), b"2^31"), (c_rowptr, dict(f=0), b"fanout"),
             (c_rowptr, dict(f=65), b"fanout"), (c_rowptr, dict(M=2**26, f=32), b"M * fanout"),
             (c_rowptr, dict(rowptr=None), b"NULL"), (c_rowptr, dict(total=None), b"NULL"),
             (c_rowptr, dict(wsb=wsb - 1), b"workspace too small"), (c_rowptr, dict(ws=None), b"workspace too small"),
             (c_rowptr, dict(ws=ws.data_ptr() + 8), b"16-byte aligned"),
             (c_draw, dict(cap=-1), b"negative"), (c_draw, dict(M=2**31), b"2^31"), (c_draw, dict(f=0), b"fanout"),
             (c_draw, dict(f=65), b"fanout"), (c_draw, dict(M=2**26, f=32), b"M * fanout"),
             (c_draw, dict(ids=None), b"NULL"), (c_draw, dict(val=None), b"NULL"), (c_draw, dict(rp=None), b"NULL"),
             (c_relabel, dict(n=-1), b"negative"), (c_relabel, dict(n=2**31), b"2^31"),
             (c_relabel, dict(table=None), b"NULL table"), (c_relabel, dict(table=table.data_ptr() + 4), b"8-byte"),
             (c_relabel, dict(col=None), b"NULL")]
    for fn, kw, word in cases:
        assert fn(**kw) == -22, (fn.__name__, kw)
        assert word in L.gnn_last_error(), (fn.__name__, kw, L.gnn_last_error())
    torch.cuda.synchronize()
    for t in (rowptr, total, ids, col):  # nothing ran
        assert bool((t == -7).all())
    assert bool((val == -7.0).all())

    assert c_rowptr() == 0 and c_draw(rp=rowptr.data_ptr()) == 0
    torch.cuda.synchronize()
    nnz = int(total[0])
    assert torch.equal(rowptr, good_rowptr) and nnz == int(good_rowptr[-1])
    want_ids = ids.clone()
    # the entry points record into a graph (capture only: nothing here replays it)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        cst = _lib.stream_of(dev)
        _lib.check(L.gnn_nbr_rowptr(dg.indptr.data_ptr(), N, Eg, rows.data_ptr(), M, f, rowptr.data_ptr(),
                                    total.data_ptr(), ws.data_ptr(), wsb, None, cst), "capture rowptr")
        _lib.check(L.gnn_nbr_draw(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, Eg, rows.data_ptr(), M, f, 3, 0,
                                  rowptr.data_ptr(), ids.data_ptr(), val.data_ptr(), cap, None, cst), "capture draw")
        _lib.check(L.gnn_nbr_relabel(table.data_ptr(), N, ids.data_ptr(), nnz, col.data_ptr(), val.data_ptr(), None,
                                     cst), "capture relabel")
    torch.cuda.synchronize()
    assert torch.equal(ids, want_ids) and bool((col == -7).all())  # recorded, not run


# ----------------------------------------------------------------------------- the sampler


@pytest.fixture(scope="module")
def worlds():
    """(lap, feats, labels) per model name, made once and left unchanged."""
    out = {}
    for name in ("graphsage", "gcn"):
        lap, feats = make_world(name, NN, 48)
        out[name] = (lap, feats, _labels(NN, 7))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_sampler_equals_host_restatement(dev, worlds, name, orders, dtype):
    lap, feats, labels = worlds[name]
    table = feats.to(dtype)
    fan = [25, 10][: sum(orders)]
    ns = NeighborSampler(lap, fan, orders, table, labels, dev)
    b = ns.sample(BATCH, 21)
    hb = neighbor_sample_host(21, BATCH, fan, lap, orders)
    x0, adjs, sampled, lab = b
    assert b.input_nodes.dtype == torch.int64 and np.array_equal(b.input_nodes.cpu().numpy(), hb.input_nodes)
    assert x0.dtype == torch.float32 and x0.stride(1) == 1 and x0.stride(0) % 32 == 0
    assert torch.equal(x0.cpu(), table[torch.from_numpy(hb.input_nodes)].float())  # widened exactly
    assert torch.equal(lab.cpu(), torch.from_numpy(np.asarray(labels[BATCH].todense(), dtype=np.float32)))
    for l, o in enumerate(orders):
        if o == 0:
            assert adjs[l] is None and sampled[l].numel() == 0 and sampled[l].dtype == torch.int64
            continue
        rowptr, col, val, shape = hb.layers[l]
        op = adjs[l]
        assert isinstance(op, cso.CsrOperand) and op.shape == shape and op.nnz == col.size
        assert np.array_equal(op.rowptr.cpu().numpy(), rowptr) and np.array_equal(op.col.cpu().numpy(), col)
        assert np.array_equal(op.val.cpu().numpy(), val)
        assert sampled[l].dtype == torch.int64 and np.array_equal(sampled[l].cpu().numpy(), hb.sampled_nodes[l])
        if l >= 1:
            want_t = sp.csr_matrix((val, col, rowptr), shape=shape).T.tocsr()
            want_t.sort_indices()
            assert op._t is not None and np.array_equal(op._t.rowptr.cpu().numpy(), want_t.indptr)
            assert np.array_equal(op._t.col.cpu().numpy(), want_t.indices)
            assert np.array_equal(op._t.val.cpu().numpy(), want_t.data)
            if l == len(orders) - 1:  # BATCH repeats two nodes: no row map, the step's fused residual needs one
                assert getattr(sampled[l], "_gnn_rmap", None) is None
    # a table already on the device, and the same rows drawn in a batch of unique nodes
    ns_d = NeighborSampler(lap, fan, orders, table.to(dev), labels, dev)
    b2 = ns_d.sample(BATCH, 21)
    assert torch.equal(b2.x0, x0) and all(torch.equal(p, q) for p, q in zip(b2.sampled_nodes, sampled))
    uniq = ns_d.sample(BATCH[:-2], 21)
    top = len(orders) - 1
    rm = uniq.sampled_nodes[top]._gnn_rmap.cpu().numpy()
    sn = uniq.sampled_nodes[top].cpu().numpy()
    assert rm.dtype == np.int32 and np.array_equal(rm[sn], np.arange(sn.size)) and (rm >= 0).sum() == sn.size


def test_sampler_refuses_a_table_that_does_not_fit(dev, worlds, monkeypatch):
    lap, feats, labels = worlds["graphsage"]
    need = NN * 64 * 4  # 48 floats in whole-line rows of 64
    monkeypatch.setattr(NeighborSampler, "_free_bytes", lambda self: need - 1)
    with pytest.raises(RuntimeError, match=str(need)):
        NeighborSampler(lap, 5, [1, 1], feats, labels, dev)
    NeighborSampler(lap, 5, [1, 1], feats.to(dev), labels, dev)  # a resident table takes nothing more


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _grads(tr):
    return [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in tr.params]


@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_native_step_takes_the_batch_and_matches_python_path(dev, worlds, name, orders):
    """One training step (dropout 0.1, the same seeds) on the native executor against the Python
    autograd path: tests/test_orders_gpu.py's bounds for that comparison — loss within
    1e-6 |loss| + 1e-7, every gradient within 1e-5 in relative L2."""
    lap, feats, labels = worlds[name]
    ns = NeighborSampler(lap, [25, 10][: sum(orders)], orders, feats, labels, dev)
    batch = ns.sample(np.arange(40, 560, 2), 9)
    args = tuple(batch)

    def trainer(native):
        torch.manual_seed(0)
        m = models.build_model(name, feats.shape[1], 128, list(orders), 7, 0.1, fused=True).to(dev)
        tr = Trainer(m, 0.01, dev)
        assert tr.executor is not None
        if not native:
            tr.executor = None  # what GNN_NATIVE_STEP=0 leaves: the Python autograd path
        return tr

    ta, tb = trainer(False), trainer(True)
    assert isinstance(tb.executor, E.NativeStep) and tb.executor.supports(*args)
    assert tb.executor.supports(*args, inference=True)
    torch.manual_seed(100)
    la = ta.step(*args)
    unused = [p.grad is None for p in ta.params]
    ga = _grads(ta)
    torch.manual_seed(100)
    lb = tb.step(*args)
    gb = _grads(tb)
    torch.cuda.synchronize()
    print(f"neighbor {name} {orders}: loss {float(la):.8f} / {float(lb):.8f}, max gradient error "
          f"{max(_rel(x, y) for x, y, u in zip(gb, ga, unused) if not u):.2e}")
    assert np.isfinite(float(lb)) and abs(float(la) - float(lb)) <= 1e-6 * abs(float(la)) + 1e-7
    for i, (x, y, u) in enumerate(zip(gb, ga, unused)):
        if u:
            assert not bool(x.any()), i
        else:
            assert _rel(x, y) <= 1e-5, (i, _rel(x, y))


@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_full_fanout_scores_the_full_neighbourhood(dev, name, orders):
    """f >= the largest degree: the sampled batch is lap itself, so Evaluator.predict gives the
    exact logits — test_engine_closure_scope's bounds: relative L2 error against the float64
    reference <= 1e-4, and <= 2 x the closure engine's error + 1e-6."""
    C, nfeat, nhid = 7, 48, 128
    lap, feats = small_degree_world(name, NN, nfeat)
    cpu_model = make_model(name, nfeat, nhid, orders, C).eval()
    ref = reference_logits_f64(cpu_model, lap, feats)[torch.from_numpy(BATCH)]
    model = models.build_model(name, nfeat, nhid, orders, C, dropout=0.1, fused=True)
    model.load_state_dict(cpu_model.state_dict())
    model = model.to(dev).eval()
    ns = NeighborSampler(lap, 64, orders, feats, _labels(NN, C), dev)
    batch = ns.sample(BATCH, 1)
    ev = Evaluator(model, dev, executor=E.NativeStep(model))
    z = ev.predict(batch.x0, batch.adjs, batch.sampled_nodes)
    assert ev._native(batch.x0, batch.adjs, batch.sampled_nodes, None)
    z_c = ExactInference(model, lap, dev).logits(feats, BATCH, scope="closure")
    rel = lambda a: float((a.double().cpu() - ref).norm() / ref.norm())
    err, err_c = rel(z), rel(z_c)
    print(f"neighbor full fanout {name} {orders}: err {err:.3e} closure engine {err_c:.3e}")
    assert z.shape == (BATCH.size, C) and err <= 1e-4
    assert err <= 2 * err_c + 1e-6
    assert torch.equal(z[-2], z[int(np.flatnonzero(BATCH == 40)[0])])  # duplicate batch nodes: equal rows
