"""The subgraph sampler on the GPU: gnn_sg_count / gnn_sg_finish against numpy (sentinel tails of 64
behind every output), their guards, refusals and capture; then SubgraphSampler against
subgraph_race_host array for array, against LayerwiseSampler's top operand, and through the native
step against the Python autograd path.

The hand graph (degrees 0, 1, 2, 5, 63, 64, 65, 130, 1000; lap^T != lap) puts a wave's width and
several passes of its lanes under the count; the 300,000-node graph several scan chunks."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib, models, placement, staging
from gnn_amd import custom_sparse_ops as cso
from gnn_amd import executor as E
from gnn_amd.layerwise import LayerwiseSampler
from gnn_amd.placed import PlacedFeatures
from gnn_amd.subgraph import SubgraphSampler, subgraph_race_host
from gnn_amd.train import Trainer
from test_layerwise_gpu import (BATCH, NN, SEEDS, TAIL, _grads, _labels, _no_graph, _rel, _sent, _t, big, graph,  # noqa: F401
                                worlds)
from test_neighbor_gpu import N, ROWS

pytestmark = pytest.mark.gpu


def _scan(v):
    return np.concatenate([[0], np.cumsum(v)])


def _table_of(after_h, n_nodes, dev):
    """(after int32 on the device, its gnn_closure_mark table, K as a device int64[1])."""
    after = _t(after_h.astype(np.int32), dev)
    table, K_t = cso.closure_mark(_no_graph(n_nodes, after), after, False)
    assert int(K_t) == after_h.size
    return after, table, K_t.reshape(1)


def _count(dg, n_nodes, after, K_t, kcap, table, dev):
    """gnn_sg_count into sentinel-filled outputs: (colcnt, err)."""
    colcnt = _sent(kcap, torch.int32, dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().gnn_sg_count(dg.indptr_t.data_ptr(), dg.indices_t.data_ptr(), n_nodes, int(dg.indices_t.numel()),
                                       after.data_ptr(), K_t.data_ptr(), kcap, table.data_ptr(), colcnt.data_ptr(),
                                       err.data_ptr(), _lib.stream_of(dev)), "gnn_sg_count")
    return colcnt, err


def _finish(dg, n_nodes, after, K_t, kcap, colcnt, dev):
    """gnn_sg_finish into sentinel-filled outputs: (colptr_t, rowseg, totals, err)."""
    L = _lib.lib()
    colptr, rowseg, totals = _sent(kcap + 1, torch.int32, dev), _sent(kcap + 1, torch.int32, dev), _sent(2, torch.int64, dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    wsb = L.gnn_sg_finish_workspace_bytes(kcap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.gnn_sg_finish(dg.indptr.data_ptr(), int(dg.indices.numel()), n_nodes, after.data_ptr(), K_t.data_ptr(), kcap,
                               colcnt.data_ptr(), colptr.data_ptr(), rowseg.data_ptr(), totals.data_ptr(), ws.data_ptr(),
                               wsb, err.data_ptr(), _lib.stream_of(dev)), "gnn_sg_finish")
    return colptr, rowseg, totals, err


def _square_counts(g, after_h):
    """(S's column counts, deg(after)) in numpy: S = lap[after][:, after]."""
    S = g.lap[after_h][:, after_h].tocsr()
    return np.bincount(S.indices, minlength=after_h.size), np.diff(g.indptr)[after_h]


def _check_square(g, dg, after_h, dev, slack=7):
    n_nodes, K = g.num_nodes, after_h.size
    kcap = K + slack
    after, table, K_t = _table_of(after_h, n_nodes, dev)
    after = torch.cat([after, torch.full((slack,), 3, dtype=torch.int32, device=dev)])  # past K: never read
    want_cnt, deg = _square_counts(g, after_h)
    colcnt, err = _count(dg, n_nodes, after, K_t, kcap, table, dev)
    assert np.array_equal(colcnt[:K].cpu().numpy(), want_cnt) and bool((colcnt[K:] == -7).all()) and not err.any()
    colptr, rowseg, totals, err = _finish(dg, n_nodes, after, K_t, kcap, colcnt, dev)
    assert not err.any()
    assert np.array_equal(colptr[: K + 1].cpu().numpy(), _scan(want_cnt)) and bool((colptr[K + 1:] == -7).all())
    assert np.array_equal(rowseg[: K + 1].cpu().numpy(), _scan(deg)) and bool((rowseg[K + 1:] == -7).all())
    assert totals[:2].tolist() == [want_cnt.sum(), deg.sum()] and bool((totals[2:] == -7).all())
    return want_cnt


def test_count_and_finish_on_the_hand_graph(graph, dev):
    g, dg = graph
    assert not dg.symmetric and np.diff(g.indptr)[0] == 0
    cnt = _check_square(g, dg, np.arange(N), dev)
    assert np.array_equal(cnt, np.bincount(g.indices, minlength=N)) and cnt.max() > 130  # lap^T's rows, whole
    after = subgraph_race_host(SEEDS[1], ROWS, 40, g, [1, 1]).input_nodes
    assert np.unique(ROWS).size < after.size <= np.unique(ROWS).size + 40
    _check_square(g, dg, after, dev)
    assert _check_square(g, dg, np.array([0]), dev).tolist() == [0]


def test_count_and_finish_over_several_chunks(big, dev):
    g, dg, rows = big
    after = subgraph_race_host(SEEDS[1], rows, 8192, g, [1, 1]).input_nodes
    assert after.size > 3 * 8192
    _check_square(g, dg, after, dev)


def test_guards(graph, dev):
    """Read in layerwise.hip before they run: sg_count_kernel and the chunk scans clamp *K to kcap
    (clamp_size) and write nothing at or past it; a member outside [0, N) fails row_span, which
    gives it no entries, and table_pos refuses an entry outside [0, N) before it indexes the table."""
    g, dg = graph
    after_h = subgraph_race_host(3, ROWS, 40, g, [1, 1]).input_nodes
    K = after_h.size
    want_cnt, deg = _square_counts(g, after_h)
    after, table, K_t = _table_of(after_h, N, dev)
    # *K above kcap: clamped (the finish flags it)
    kcap = K - 5
    huge = _t(np.array([10**6]), dev)
    colcnt, err = _count(dg, N, after, huge, kcap, table, dev)
    assert np.array_equal(colcnt[:kcap].cpu().numpy(), want_cnt[:kcap]) and bool((colcnt[kcap:] == -7).all())
    assert not err.any()
    colptr, rowseg, totals, err = _finish(dg, N, after, huge, kcap, colcnt, dev)
    assert int(err[0]) == 1 and not err[1:].any()
    assert np.array_equal(colptr[: kcap + 1].cpu().numpy(), _scan(want_cnt[:kcap])) and bool((colptr[kcap + 1:] == -7).all())
    assert np.array_equal(rowseg[: kcap + 1].cpu().numpy(), _scan(deg[:kcap])) and bool((rowseg[kcap + 1:] == -7).all())
    assert totals[:2].tolist() == [want_cnt[:kcap].sum(), deg[:kcap].sum()]
    # members outside [0, N): no entries, the flag
    bad_h = after_h.copy()
    where = np.array([4, K // 2, K - 1])
    bad_h[where] = [N + 5, -3, 2**31 - 1]
    ok = np.ones(K, bool)
    ok[where] = False
    bad = _t(bad_h.astype(np.int32), dev)
    colcnt, err = _count(dg, N, bad, K_t, K, table, dev)
    assert int(err[0]) == 1 and not err[1:].any() and bool((colcnt[K:] == -7).all())
    assert np.array_equal(colcnt[:K].cpu().numpy(), np.where(ok, want_cnt, 0))
    colptr, rowseg, totals, err = _finish(dg, N, bad, K_t, K, colcnt, dev)
    assert int(err[0]) == 1 and np.array_equal(rowseg[: K + 1].cpu().numpy(), _scan(np.where(ok, deg, 0)))
    assert np.array_equal(colptr[: K + 1].cpu().numpy(), _scan(np.where(ok, want_cnt, 0)))
    # an entry of lap^T outside [0, N) is no member; a row pointer past the index array gives the row nothing
    Et = int(dg.indices_t.numel())
    ind = dg.indices_t.clone()
    last = K - 1  # the largest member: only its own row ends at the row pointer's entry after it
    hub = int(np.argmax(want_cnt[:last]))
    _, tp, tix = g.transpose_structure
    first = int(tp[after_h[hub]])
    members = np.flatnonzero(np.isin(tix[first: tp[after_h[hub] + 1]], after_h))
    ind[first + int(members[0])] = N + 9
    ptr = dg.indptr_t.clone()
    ptr[after_h[last] + 1] = Et + 50
    colcnt = _sent(K, torch.int32, dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().gnn_sg_count(ptr.data_ptr(), ind.data_ptr(), N, Et, after.data_ptr(), K_t.data_ptr(), K,
                                       table.data_ptr(), colcnt.data_ptr(), err.data_ptr(), _lib.stream_of(dev)), "count")
    want = want_cnt.copy()
    want[hub] -= 1
    want[last] = 0
    assert want_cnt[hub] > 0 and int(err[0]) == 1 and np.array_equal(colcnt[:K].cpu().numpy(), want)
    # totals of 2^31 or more: the flag, zero offsets, 2^31 - 1
    fake = _t(np.arange(5, dtype=np.int64) << 30, dev)
    three = _t(np.array([0, 1, 2], np.int32), dev)
    cnt3 = _t(np.full(3, 2**30, np.int32), dev)
    L = _lib.lib()
    colptr, rowseg, totals = _sent(4, torch.int32, dev), _sent(4, torch.int32, dev), _sent(2, torch.int64, dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    wsb = L.gnn_sg_finish_workspace_bytes(3)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.gnn_sg_finish(fake.data_ptr(), 2**40, 4, three.data_ptr(), _t(np.array([3]), dev).data_ptr(), 3,
                               cnt3.data_ptr(), colptr.data_ptr(), rowseg.data_ptr(), totals.data_ptr(), ws.data_ptr(), wsb,
                               err.data_ptr(), _lib.stream_of(dev)), "gnn_sg_finish")
    assert int(err[0]) == 1 and colptr[:4].tolist() == [0] * 4 and rowseg[:4].tolist() == [0] * 4
    assert totals[:2].tolist() == [2**31 - 1] * 2 and bool((colptr[4:] == -7).all()) and bool((rowseg[4:] == -7).all())


def test_refusals_launch_nothing(graph, dev):
    g, dg = graph
    L = _lib.lib()
    after_h = np.arange(N)
    after, table, K_t = _table_of(after_h, N, dev)
    kcap = N
    colcnt, colptr, rowseg = _sent(kcap, torch.int32, dev), _sent(kcap + 1, torch.int32, dev), _sent(kcap + 1, torch.int32, dev)
    totals = _sent(3, torch.int64, dev)
    wsb = L.gnn_sg_finish_workspace_bytes(kcap)
    ws = torch.full((wsb + 64,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = _lib.stream_of(dev)
    Eg, Et = int(dg.indices.numel()), int(dg.indices_t.numel())

    def c_count(**kw):
        a = dict(indptr=dg.indptr_t.data_ptr(), indices=dg.indices_t.data_ptr(), N=N, E=Et, after=after.data_ptr(),
                 K=K_t.data_ptr(), kcap=kcap, table=table.data_ptr(), colcnt=colcnt.data_ptr())
        a.update(kw)
        return L.gnn_sg_count(a["indptr"], a["indices"], a["N"], a["E"], a["after"], a["K"], a["kcap"], a["table"],
                              a["colcnt"], None, st)

    def c_finish(**kw):
        a = dict(indptr=dg.indptr.data_ptr(), E=Eg, N=N, after=after.data_ptr(), K=K_t.data_ptr(), kcap=kcap,
                 colcnt=colcnt.data_ptr(), colptr=colptr.data_ptr(), rowseg=rowseg.data_ptr(), totals=totals.data_ptr(),
                 ws=ws.data_ptr(), wsb=wsb)
        a.update(kw)
        return L.gnn_sg_finish(a["indptr"], a["E"], a["N"], a["after"], a["K"], a["kcap"], a["colcnt"], a["colptr"],
                               a["rowseg"], a["totals"], a["ws"], a["wsb"], None, st)

    cases = [(c_count, dict(kcap=-1), b"negative"), (c_count, dict(E=-1), b"negative"), (c_count, dict(N=2**31), b"2^31"),
             (c_count, dict(kcap=2**31), b"2^31"), (c_count, dict(K=None), b"NULL K"),
             (c_count, dict(K=K_t.data_ptr() + 4), b"8-byte"), (c_count, dict(table=None), b"NULL table"),
             (c_count, dict(table=table.data_ptr() + 4), b"8-byte"), (c_count, dict(after=None), b"NULL after"),
             (c_count, dict(colcnt=None), b"NULL after"), (c_count, dict(indptr=None), b"NULL after"),
             (c_count, dict(indices=None), b"NULL indices_t"),
             (c_finish, dict(kcap=-1), b"negative"), (c_finish, dict(E=-1), b"negative"), (c_finish, dict(N=2**31), b"2^31"),
             (c_finish, dict(kcap=2**31), b"2^31"), (c_finish, dict(K=None), b"NULL K"), (c_finish, dict(totals=None), b"NULL K"),
             (c_finish, dict(totals=totals.data_ptr() + 4), b"8-byte"), (c_finish, dict(K=K_t.data_ptr() + 4), b"8-byte"),
             (c_finish, dict(colptr=None), b"NULL colptr_t"), (c_finish, dict(rowseg=None), b"NULL colptr_t"),
             (c_finish, dict(after=None), b"NULL after"), (c_finish, dict(colcnt=None), b"NULL after"),
             (c_finish, dict(indptr=None), b"NULL after"), (c_finish, dict(wsb=wsb - 1), b"workspace too small"),
             (c_finish, dict(ws=None), b"workspace too small"), (c_finish, dict(ws=ws.data_ptr() + 8), b"16-byte aligned")]
    for fn, kw, msg in cases:
        assert fn(**kw) == -22, (fn.__name__, kw)
        assert msg in L.gnn_last_error(), (fn.__name__, kw, L.gnn_last_error())
    torch.cuda.synchronize()
    for t_ in (colcnt, colptr, rowseg, totals):  # nothing ran
        assert bool((t_ == -7).all())
    assert bool((ws == 0x5A).all())
    assert c_count() == 0 and c_finish() == 0
    torch.cuda.synchronize()
    assert int(totals[0]) == g.indices.size == int(totals[1]) and bool((ws[wsb:] == 0x5A).all())


def test_capture_replays_bit_identically(graph, dev):
    """The batch's call sequence from the first mark to gnn_sg_finish, captured on one stream (no
    parallel branches)."""
    g, dg = graph
    L = _lib.lib()
    rows = _t(ROWS.astype(np.int32), dev)
    M, samp, seed, layer = ROWS.size, 150, SEEDS[1], 2
    cap = N
    kcap = min(N, M + samp)
    tb = L.gnn_closure_table_bytes(N)
    wsb = max(L.gnn_closure_workspace_bytes(N), L.gnn_lw_select_workspace_bytes(), L.gnn_lw_finish_workspace_bytes(M, kcap),
              L.gnn_sg_finish_workspace_bytes(kcap))
    mk = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    live, table, ws = mk(tb, torch.uint8), mk(tb, torch.uint8), mk(wsb, torch.uint8)
    live_ids, count, key = mk(cap, torch.int32), mk(cap, torch.int32), mk(cap, torch.int64)
    seeds = mk(M + cap, torch.int32)
    seeds[:M] = rows
    after, normfact = mk(kcap, torch.int32), mk(kcap, torch.float32)
    colptr, colseg, rowseg = mk(kcap + 1, torch.int32), mk(kcap + 1, torch.int32), mk(M + 1, torch.int32)
    colcnt, colptr_s, rowseg_s = mk(kcap, torch.int32), mk(kcap + 1, torch.int32), mk(kcap + 1, torch.int32)
    word = mk(11, torch.int64)
    outs = (live, table, live_ids, count, key, seeds, after, normfact, colptr, colseg, rowseg, colcnt, colptr_s, rowseg_s, word)
    Eg, Et = int(dg.indices.numel()), int(dg.indices_t.numel())
    w = lambda i: word[i:].data_ptr()

    def sequence(st):
        ck = _lib.check
        ck(L.gnn_closure_mark(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, rows.data_ptr(), M, 1, live.data_ptr(),
                              w(0), ws.data_ptr(), wsb, st), "mark")
        ck(L.gnn_closure_list(live.data_ptr(), N, live_ids.data_ptr(), cap, st), "list")
        ck(L.gnn_lw_race_skew(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, Eg, rows.data_ptr(), M, live.data_ptr(), seed,
                              layer, count.data_ptr(), key.data_ptr(), cap, w(1), w(8), st, None, 1), "race")
        ck(L.gnn_lw_select(key.data_ptr(), count.data_ptr(), w(0), cap, samp, live_ids.data_ptr(), seeds[M:].data_ptr(),
                           w(2), w(3), ws.data_ptr(), wsb, st), "select")
        ck(L.gnn_closure_mark(None, None, N, seeds.data_ptr(), M + cap, 0, table.data_ptr(), w(4), ws.data_ptr(), wsb,
                              st), "mark")
        ck(L.gnn_closure_list(table.data_ptr(), N, after.data_ptr(), kcap, st), "list")
        ck(L.gnn_lw_finish_skew(dg.indptr.data_ptr(), Eg, dg.indptr_t.data_ptr(), Et, N, rows.data_ptr(), M,
                                after.data_ptr(), w(4), kcap, live.data_ptr(), count.data_ptr(), cap, w(1), w(2),
                                normfact.data_ptr(), colptr.data_ptr(), rowseg.data_ptr(), colseg.data_ptr(), w(5),
                                ws.data_ptr(), wsb, w(8), st, None, 1), "finish")
        ck(L.gnn_sg_count(dg.indptr_t.data_ptr(), dg.indices_t.data_ptr(), N, Et, after.data_ptr(), w(4), kcap,
                          table.data_ptr(), colcnt.data_ptr(), w(8), st), "sg_count")
        ck(L.gnn_sg_finish(dg.indptr.data_ptr(), Eg, N, after.data_ptr(), w(4), kcap, colcnt.data_ptr(),
                           colptr_s.data_ptr(), rowseg_s.data_ptr(), w(9), ws.data_ptr(), wsb, w(8), st), "sg_finish")

    sequence(_lib.stream_of(dev))
    torch.cuda.synchronize()
    direct = [t_.clone() for t_ in outs]
    hb = subgraph_race_host(seed, ROWS, samp, g, [1, 0, 1])
    K = int(word[4])
    want_cnt, deg = _square_counts(g, hb.input_nodes)
    assert np.array_equal(after[:K].cpu().numpy(), hb.input_nodes) and int(word[5]) == hb.layers[2][0][-1]
    assert int(word[8]) == 0 and word[9:].tolist() == [hb.layers[0][0][-1], deg.sum()] and int(word[7]) == deg.sum()
    assert np.array_equal(colptr_s[: K + 1].cpu().numpy(), _scan(want_cnt))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        sequence(_lib.stream_of(dev))
    for t_ in outs[:5] + outs[6:-1]:
        t_.fill_(0x33)
    seeds[M:] = 0x33
    word[:8] = 0x33  # word 8 is the error flag the calls OR into: the caller's to clear
    word[9:] = 0x33
    cg.replay()
    torch.cuda.synchronize()
    ntab, tbl = int(word[0]), ((N + 31) // 32 + 1) * 8  # what the calls write of each output: the rest keeps the fill
    valid = (tbl, tbl, ntab, cap, cap, M + cap, K, K, K + 1, K + 1, M + 1, K, K + 1, K + 1, 11)
    for got, want, n in zip(outs, direct, valid):
        assert torch.equal(got[:n], want[:n])
    del cg


# ----------------------------------------------------------------------------- the sampler

CASES = [(name, orders) for name in ("graphsage", "gcn") for orders in ([1, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1])]
IDS = [("sage" if name == "graphsage" else name) + "".join(map(str, orders)) for name, orders in CASES]


def _transposed(op):
    M, K = op.shape
    L, dev = _lib.lib(), op.device
    tp = torch.empty(K + 1, dtype=torch.int32, device=dev)
    tc = torch.empty(op.nnz, dtype=torch.int32, device=dev)
    tv = torch.empty(op.nnz, dtype=torch.float32, device=dev)
    wsb = L.gnn_csr_transpose_workspace_bytes(M, K, op.nnz)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    _lib.check(L.gnn_csr_transpose(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), M, K, op.nnz, tp.data_ptr(),
                                   tc.data_ptr(), tv.data_ptr(), ws.data_ptr(), wsb, _lib.stream_of(dev)), "gnn_csr_transpose")
    return tp, tc, tv


def _assert_batch(b, hb, table, labels, batch, orders, unique):
    x0, adjs, sampled, lab = b
    assert b.input_nodes.dtype == torch.int64 and np.array_equal(b.input_nodes.cpu().numpy(), hb.input_nodes)
    assert x0.dtype == torch.float32 and x0.stride(1) == 1 and x0.stride(0) % 32 == 0
    assert torch.equal(x0.cpu(), table[torch.from_numpy(hb.input_nodes)].float())  # widened exactly
    assert torch.equal(lab.cpu(), torch.from_numpy(np.asarray(labels[batch].todense(), dtype=np.float32)))
    top = max(l for l, o in enumerate(orders) if o)
    lower = [l for l in range(top) if orders[l]]
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
        if l < top:
            assert op is adjs[lower[0]] and shape[0] == shape[1]  # one operand object for the lower layers
        # the transpose: the top layer's above layer 0; the square one's when one of its layers lies above layer 0
        want_t = l >= 1 if l == top else lower[-1] >= 1
        assert (op._t is not None) == want_t
        if want_t:
            assert op._t.shape == shape[::-1]
            tp, tc, tv = _transposed(op)
            assert torch.equal(op._t.rowptr, tp) and torch.equal(op._t.col, tc) and torch.equal(op._t.val, tv)
        if l >= 1:
            rm = getattr(sampled[l], "_gnn_rmap", None)
            if l == top and not unique:
                assert rm is None  # repeated batch nodes: the fused residual's row map needs unique rows
            else:
                sn = sampled[l].cpu().numpy()
                rm = rm.cpu().numpy()
                assert rm.dtype == np.int32 and np.array_equal(rm[sn], np.arange(sn.size)) and (rm >= 0).sum() == sn.size


def _assert_top_is_layerwise(b, lb, top):
    a, c = b.adjs[top], lb.adjs[top]
    assert a.shape == c.shape and torch.equal(a.rowptr, c.rowptr) and torch.equal(a.col, c.col) and torch.equal(a.val, c.val)
    assert torch.equal(b.sampled_nodes[top], lb.sampled_nodes[top])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_sampler_equals_host_batch(dev, worlds, name, orders, dtype):
    lap, feats, labels = worlds[name]
    table = feats.to(dtype)
    top = len(orders) - 1
    ss = SubgraphSampler(lap, [90, 70, 50], orders, table, labels, dev)  # the reference's list: 90 is used
    b = ss.sample(BATCH, 21)
    _assert_batch(b, subgraph_race_host(21, BATCH, 90, lap, orders), table, labels, BATCH, orders, False)
    _assert_top_is_layerwise(b, LayerwiseSampler(lap, 90, [0] * top + [1], table, labels, dev).sample(BATCH, 21), top)
    uniq = BATCH[:-2]
    ss_d = SubgraphSampler(lap, 64, orders, table.to(dev), labels, dev)  # a table already on the device
    _assert_batch(ss_d.sample(uniq, SEEDS[1]), subgraph_race_host(SEEDS[1], uniq, 64, lap, orders), table, labels, uniq,
                  orders, True)


def test_sampler_on_the_hand_graph_and_the_large_one(graph, big, dev):
    for (g, dg), rows, samp in ((graph, ROWS, 200), (big[:2], big[2], 8192)):
        Nn = g.num_nodes
        feats = torch.from_numpy(np.random.default_rng(1).standard_normal((Nn, 8)).astype(np.float32)).half()
        labels = _labels(Nn, 3)
        b = SubgraphSampler(g, samp, [1, 1, 1], feats, labels, dev).sample(rows, SEEDS[1])
        _assert_batch(b, subgraph_race_host(SEEDS[1], rows, samp, g, [1, 1, 1]), feats, labels, rows, [1, 1, 1],
                      np.unique(rows).size == rows.size)


def test_sampler_with_a_favoured_set(dev, worlds):
    lap, feats, labels = worlds["graphsage"]
    fav = np.random.default_rng(4).permutation(NN)[: NN // 5]
    orders = [1, 0, 1]
    b = SubgraphSampler(lap, 64, orders, feats, labels, dev, scale_factor=4, skewed_sampling_nodes=fav).sample(BATCH, 21)
    hb = subgraph_race_host(21, BATCH, 64, lap, orders, fav, 4)
    assert not np.array_equal(hb.input_nodes, subgraph_race_host(21, BATCH, 64, lap, orders).input_nodes)
    _assert_batch(b, hb, feats, labels, BATCH, orders, False)
    lb = LayerwiseSampler(lap, 64, [0, 0, 1], feats, labels, dev, scale_factor=4, skewed_sampling_nodes=fav).sample(BATCH, 21)
    _assert_top_is_layerwise(b, lb, 2)
    # scale 1 and an empty set are the plain draw
    plain = subgraph_race_host(21, BATCH, 64, lap, orders)
    for kw in (dict(scale_factor=1, skewed_sampling_nodes=fav), dict(scale_factor=4, skewed_sampling_nodes=np.zeros(0, np.int64))):
        _assert_batch(SubgraphSampler(lap, 64, orders, feats, labels, dev, **kw).sample(BATCH, 21), plain, feats, labels,
                      BATCH, orders, False)


def test_sampler_over_a_placed_store(dev, worlds):
    lap, feats, labels = worlds["graphsage"]
    table = feats.half()
    pl = placement.create_buffer(lap, np.arange(40, 560), NN // 2, [0], 2, alpha=0)
    pf = PlacedFeatures.from_store(staging.FeatureStore(table, pl.gpu_buffer_group[0], dev, 0), pl, 0)
    try:
        own = pf.resident_nodes("own")
        assert NN // 4 < own.size < NN  # half the rows buffered
        orders = [1, 1, 1]
        ss = SubgraphSampler(lap, 64, orders, pf, labels, dev, scale_factor=2, skewed_sampling_nodes=own)
        batches = list(ss.epoch(np.arange(40, 560), 200, seed=3))  # ends with pf.check()
        assert len(batches) == 3
        for b in batches:
            hb = subgraph_race_host(b.seed, b.batch_nodes, 64, lap, orders, own, 2)
            _assert_batch(b, hb, table, labels, b.batch_nodes, orders, True)
        c = pf.counts()
        assert c["total"] == sum(int(b.input_nodes.numel()) for b in batches) and c["own"] > 0 and c["host"] > 0
    finally:
        pf.close()


@pytest.mark.parametrize("name,orders", [("graphsage", [1, 1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1])],
                         ids=["sage111", "sage101", "gcn11"])
def test_native_step_takes_the_batch_and_matches_python_path(dev, worlds, name, orders):
    """One training step (dropout 0.1, the same seeds) and one evaluation on the native executor
    against the Python autograd path, with tests/test_layerwise_gpu.py's bounds for that comparison:
    loss within 1e-6 |loss| + 1e-7, every gradient within 1e-5 in relative L2."""
    lap, feats, labels = worlds[name]
    ss = SubgraphSampler(lap, 128, orders, feats, labels, dev)
    batch = ss.sample(np.arange(40, 560, 2), 9)
    args = tuple(batch)
    lower = [l for l in range(len(orders) - 1) if orders[l]]
    assert lower and all(batch.adjs[l] is batch.adjs[lower[0]] for l in lower)

    def trainer(native):
        torch.manual_seed(0)
        m = models.build_model(name, feats.shape[1], 128, list(orders), 7, 0.1, fused=True).to(dev)
        tr = Trainer(m, 0.01, dev)
        assert tr.executor is not None
        if not native:
            tr.executor = None  # the Python autograd path
        return tr

    ta, tb = trainer(False), trainer(True)
    assert isinstance(tb.executor, E.NativeStep) and tb.executor.supports(*args)
    assert tb.executor.supports(*args, inference=True)
    ea, eb = ta.evaluate([args]), tb.evaluate([args])
    print(f"subgraph {name} {orders}: eval loss {ea['loss']:.8f} / {eb['loss']:.8f}")
    assert eb["rows"] == 260 and abs(ea["loss"] - eb["loss"]) <= 1e-6 * abs(ea["loss"]) + 1e-7
    torch.manual_seed(100)
    la = ta.step(*args)
    unused = [p.grad is None for p in ta.params]
    ga = _grads(ta)
    torch.manual_seed(100)
    lb = tb.step(*args)
    gb = _grads(tb)
    torch.cuda.synchronize()
    print(f"subgraph {name} {orders}: loss {float(la):.8f} / {float(lb):.8f}, max gradient error "
          f"{max(_rel(x, y) for x, y, u in zip(gb, ga, unused) if not u):.2e}")
    assert np.isfinite(float(lb)) and abs(float(la) - float(lb)) <= 1e-6 * abs(float(la)) + 1e-7
    for i, (x, y, u) in enumerate(zip(gb, ga, unused)):
        if u:
            assert not bool(x.any()), i
        else:
            assert _rel(x, y) <= 1e-5, (i, _rel(x, y))
