"""The layer-wise race draw on the GPU: gnn_lw_race / select / finish against the numpy restatement
bit for bit, the radix select on synthetic key arrays, guards, refusals and capture; then
LayerwiseSampler against ladies_race_host array for array and through the native step against the
Python autograd path.

The select's "keys equal in the top 56 bits" cases hold at most 256 keys (the low byte is all that
differs), and "keys differing only in bit 63" exactly two, so those patterns run at the sizes that
fit them; 8,193 keys share their top 48 bits instead."""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib, models
from gnn_amd import custom_sparse_ops as cso
from gnn_amd import executor as E
from gnn_amd.layerwise import LayerwiseSampler, _column_max, _entries, entry_values, ladies_race_host, race_keys
from gnn_amd.sampler import NativeGraph, device_graph
from gnn_amd.train import Trainer
from test_exact_cpu import make_world
from test_neighbor_gpu import DEGREES, N, ROWS, _hand_lap

pytestmark = pytest.mark.gpu

SEEDS = [3, (0x9ABCDEF1 << 32) | 0x12345678]
TAIL = 64
BIG_N = 300_000


@pytest.fixture(scope="module")
def graph(dev):
    g = NativeGraph(_hand_lap())
    assert g.data is None and sorted(set(np.diff(g.indptr))) == DEGREES and g.indices.max() == N - 1
    return g, device_graph(g, dev)


@pytest.fixture(scope="module")
def big(dev):
    """300,000 nodes of degree 3 with a self-loop each, 20,000 rows: (graph, device graph, rows)."""
    rng = np.random.default_rng(11)
    r = np.concatenate([np.repeat(np.arange(BIG_N), 3), np.arange(BIG_N)])
    c = np.concatenate([rng.integers(0, BIG_N, 3 * BIG_N), np.arange(BIG_N)])
    lap = sp.csr_matrix((np.ones(r.size, np.float32), (r, c)), shape=(BIG_N, BIG_N))
    lap.sum_duplicates()
    lap.data[:] = 1.0
    g = NativeGraph(lap)
    return g, device_graph(g, dev), rng.permutation(BIG_N)[:20_000]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sent(n, dtype, dev):
    return torch.full((n + TAIL,), -7, dtype=dtype, device=dev)


def _no_graph(n, like):
    """What closure_mark without expand needs of a graph: the node count and the device."""
    return SimpleNamespace(indptr=None, indices=None, num_nodes=n, device=like.device)


def _race(indptr, indices, n_nodes, rows, live, cap, seed, layer, dev, n_entries=None):
    """gnn_lw_race into sentinel-filled outputs: (count, key, total, err)."""
    L = _lib.lib()
    count, key, total = _sent(cap, torch.int32, dev), _sent(cap, torch.int64, dev), _sent(1, torch.int64, dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    E_ = int(indices.numel()) if n_entries is None else n_entries
    _lib.check(L.gnn_lw_race(indptr.data_ptr(), indices.data_ptr(), n_nodes, E_, rows.data_ptr(), rows.numel(),
                             live.data_ptr(), seed, layer, count.data_ptr(), key.data_ptr(), cap, total.data_ptr(),
                             err.data_ptr(), _lib.stream_of(dev)), "gnn_lw_race")
    return count, key, total, err


def _select(key, count, ntab_t, cap, samp, tab_ids, dev):
    """gnn_lw_select into sentinel-filled outputs: (ids, s_num, tau)."""
    L = _lib.lib()
    ids, s_num, tau = _sent(cap, torch.int32, dev), _sent(1, torch.int64, dev), _sent(1, torch.int64, dev)
    wsb = L.gnn_lw_select_workspace_bytes()
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.gnn_lw_select(key.data_ptr(), count.data_ptr(), ntab_t.data_ptr(), cap, samp, tab_ids.data_ptr(),
                               ids.data_ptr(), s_num.data_ptr(), tau.data_ptr(), ws.data_ptr(), wsb,
                               _lib.stream_of(dev)), "gnn_lw_select")
    return ids, s_num, tau


def _finish(dg, n_nodes, rows, after, K_t, kcap, live, count, cap, total, s_num, dev, indptr=None, n_entries=None):
    """gnn_lw_finish into sentinel-filled outputs: (normfact, colptr_t, rowseg, colseg, totals, err)."""
    L = _lib.lib()
    M = rows.numel()
    normfact = torch.full((kcap + TAIL,), -7.0, dtype=torch.float32, device=dev)
    colptr, colseg, rowseg = _sent(kcap + 1, torch.int32, dev), _sent(kcap + 1, torch.int32, dev), _sent(M + 1, torch.int32, dev)
    totals = _sent(3, torch.int64, dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    wsb = L.gnn_lw_finish_workspace_bytes(M, kcap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ip = dg.indptr if indptr is None else indptr
    E_ = int(dg.indices.numel()) if n_entries is None else n_entries
    Et = int(dg.indices_t.numel()) if n_entries is None else n_entries
    _lib.check(L.gnn_lw_finish(ip.data_ptr(), E_, (dg.indptr_t if indptr is None else indptr).data_ptr(), Et, n_nodes,
                               rows.data_ptr(), M, after.data_ptr(), K_t.data_ptr(), kcap, live.data_ptr(),
                               count.data_ptr(), cap, total.data_ptr(), s_num.data_ptr(), normfact.data_ptr(),
                               colptr.data_ptr(), rowseg.data_ptr(), colseg.data_ptr(), totals.data_ptr(),
                               ws.data_ptr(), wsb, err.data_ptr(), _lib.stream_of(dev)), "gnn_lw_finish")
    return normfact, colptr, rowseg, colseg, totals, err


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _layer_on_device(g, dg, rows_h, samp, seed, layer, dev):
    """One layer's device sequence against its numpy restatement, every output and every tail."""
    Nn = g.num_nodes
    rows = _t(rows_h.astype(np.int32), dev)
    M = rows_h.size
    deg = np.diff(g.indptr)
    cap = int(min(Nn, M + deg[rows_h].sum()))
    counts, keys = race_keys(seed, layer, g.indptr, g.indices, rows_h)
    live_h = np.union1d(rows_h, np.flatnonzero(counts))  # the live table: the mark sets its seeds too
    nlive = live_h.size
    is_live = counts[live_h] > 0

    live, nlive_t = cso.closure_mark(dg, rows, True)
    assert int(nlive_t) == nlive <= cap
    live_ids = _sent(cap, torch.int32, dev)
    _lib.check(_lib.lib().gnn_closure_list(live.data_ptr(), Nn, live_ids.data_ptr(), cap, _lib.stream_of(dev)), "list")
    count, key, total, err = _race(dg.indptr, dg.indices, Nn, rows, live, cap, seed, layer, dev)
    assert np.array_equal(count[:nlive].cpu().numpy(), counts[live_h]) and not count[nlive:cap].any()
    assert np.array_equal(_u64(key[:nlive]), keys[live_h]) and not key[nlive:cap].any()
    assert int(total[0]) == counts.sum() and not err.any()
    assert bool((count[cap:] == -7).all()) and bool((key[cap:] == -7).all()) and bool((total[1:] == -7).all())

    ids, s_num, tau = _select(key, count, nlive_t.reshape(1), cap, samp, live_ids, dev)
    lk = keys[live_h][is_live]
    s = min(lk.size, samp)
    want_tau = np.partition(lk, lk.size - s)[lk.size - s] if s else np.uint64(0)
    assert int(s_num[0]) == s and _u64(tau[:1])[0] == want_tau
    want_ids = np.where(is_live & (keys[live_h] >= want_tau), live_h, -1)
    assert np.array_equal(ids[:nlive].cpu().numpy(), want_ids) and bool((ids[nlive:cap] == -1).all())
    assert bool((ids[cap:] == -7).all()) and (want_ids >= 0).sum() == s

    hb = ladies_race_host(seed, rows_h, samp, g, [0] * layer + [1])
    after_h = hb.sets[layer]
    seeds = torch.cat([rows, ids[:cap]]).contiguous()
    table, K_t = cso.closure_mark(_no_graph(Nn, seeds), seeds, False)
    K = int(K_t)
    kcap = min(Nn, M + min(cap, samp))
    assert K == after_h.size <= kcap
    after = _sent(kcap, torch.int32, dev)
    _lib.check(_lib.lib().gnn_closure_list(table.data_ptr(), Nn, after.data_ptr(), kcap, _lib.stream_of(dev)), "list")
    assert np.array_equal(after[:K].cpu().numpy(), after_h)
    normfact, colptr, rowseg, colseg, totals, err = _finish(dg, Nn, rows, after, K_t.reshape(1), kcap, live, count, cap,
                                                           total, s_num, dev)
    assert not err.any()
    assert np.array_equal(normfact[:K].cpu().numpy(), hb.normfact[layer]) and bool((normfact[K:] == -7.0).all())
    scan = lambda v: np.concatenate([[0], np.cumsum(v)])
    deg_t = deg if dg.symmetric else np.diff(g.transpose_structure[1])
    assert np.array_equal(colptr[: K + 1].cpu().numpy(), scan(counts[after_h]))
    assert np.array_equal(rowseg[: M + 1].cpu().numpy(), scan(deg[rows_h]))
    assert np.array_equal(colseg[: K + 1].cpu().numpy(), scan(deg_t[after_h]))
    assert totals[:3].tolist() == [counts[after_h].sum(), deg_t[after_h].sum(), deg[after_h].sum()]
    assert int(totals[0]) == hb.layers[layer][0][-1]  # the operand's nnz
    for t_, n_ in ((colptr, K + 1), (colseg, K + 1), (rowseg, M + 1), (totals, 3)):
        assert bool((t_[n_:] == -7).all())
    return hb, counts, after_h


@pytest.mark.parametrize("layer", [0, 2])
@pytest.mark.parametrize("seed", SEEDS, ids=["seed_lo", "seed_hi"])
def test_layer_is_bit_exact(graph, dev, seed, layer):
    g, dg = graph
    assert set(np.diff(g.indptr)[ROWS]) == set(DEGREES) and np.unique(ROWS).size < ROWS.size
    _layer_on_device(g, dg, ROWS, 200, seed, layer, dev)
    # a few short rows: most row nodes are nobody's column (count 0, normfact 1 / float32(1e-10))
    few = np.array([3, 0, 1, 2, 10, 3, 0, N - 9])
    hb, counts, after = _layer_on_device(g, dg, few, 4, seed, layer, dev)
    zero = counts[after] == 0
    assert zero.any() and np.all(hb.normfact[layer][zero] == np.float32(1) / np.float32(1e-10))
    # every live column drawn, and one
    _layer_on_device(g, dg, few, 1000, seed, layer, dev)
    _layer_on_device(g, dg, few, 1, seed, layer, dev)


def test_layer_large_graph(big, dev):
    """Every chunked scan and every histogram pass over several workgroups and chunks."""
    g, dg, rows = big
    hb, counts, after = _layer_on_device(g, dg, rows, 30_000, SEEDS[1], 1, dev)
    assert (counts > 0).sum() > 8 * 2048 and after.size > 3 * 8192 and rows.size > 2 * 8192


def _key_patterns(n, rng):
    yield "random", rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n).astype(np.uint64)
    if n <= 256:
        yield "top56", np.uint64(0xABCDEF0123456700) | rng.permutation(256)[:n].astype(np.uint64)
    yield "top48", np.uint64(0xFFFF00000000) << np.uint64(16) | rng.permutation(65536)[:n].astype(np.uint64)
    if n == 2:
        yield "bit63", np.array([0x0123456789ABCDEF, 0x8123456789ABCDEF], dtype=np.uint64)


def test_select_on_synthetic_keys(dev):
    rng = np.random.default_rng(6)
    ran = 0
    for nlive in (0, 1, 2, 63, 64, 65, 8193):
        cap = nlive + 5
        live_ids_h = (np.arange(cap) * 3 + 1).astype(np.int32)
        for name, keys in _key_patterns(nlive, rng):
            assert np.unique(keys).size == nlive
            padded = np.concatenate([keys, np.full(cap - nlive, 2**64 - 1, dtype=np.uint64)])  # never read
            key = _t(padded.view(np.int64), dev)
            ones = torch.ones(cap, dtype=torch.int32, device=dev)
            for samp in sorted({1, nlive - 1, nlive, nlive + 1} - {0, -1}):
                ids, s_num, tau = _select(key, ones, _t(np.array([nlive]), dev), cap, samp, _t(live_ids_h, dev), dev)
                s = min(nlive, samp)
                want_tau = np.partition(keys, nlive - s)[nlive - s] if s else np.uint64(0)
                assert int(s_num[0]) == s and _u64(tau[:1])[0] == want_tau, (nlive, name, samp)
                want = np.where(keys >= want_tau, live_ids_h[:nlive], -1)
                got = ids.cpu().numpy()
                assert np.array_equal(got[:nlive], want) and (want >= 0).sum() == s, (nlive, name, samp)
                assert np.all(got[nlive:cap] == -1) and np.all(got[cap:] == -7), (nlive, name, samp)
                assert bool((s_num[1:] == -7).all()) and bool((tau[1:] == -7).all())
                ran += 1
    assert ran >= 50
    # a device nlive beyond the capacity is clamped to it
    keys = next(_key_patterns(64, rng))[1]
    ar = _t(np.arange(64, dtype=np.int32), dev)
    ids, s_num, tau = _select(_t(keys.view(np.int64), dev), ar + 1, _t(np.array([10**6]), dev), 64, 5, ar, dev)
    assert int(s_num[0]) == 5 and int((ids[:64] >= 0).sum()) == 5 and bool((ids[64:] == -7).all())
    # members that are not live (count 0) are never drawn, whatever their key; nlive counts the others
    cnt = (np.arange(64) % 3 != 0).astype(np.int32)
    lk = keys[cnt > 0]
    for samp in (1, 10, lk.size, 64):
        ids, s_num, tau = _select(_t(keys.view(np.int64), dev), _t(cnt, dev), _t(np.array([64]), dev), 64, samp, ar, dev)
        s = min(lk.size, samp)
        want_tau = np.partition(lk, lk.size - s)[lk.size - s]
        assert int(s_num[0]) == s and _u64(tau[:1])[0] == want_tau
        assert np.array_equal(ids[:64].cpu().numpy(), np.where((cnt > 0) & (keys >= want_tau), np.arange(64), -1))


def test_guards(graph, dev):
    """Row ids outside the graph, a row pointer past the index array and one running backwards, a
    column id >= N planted in a copy of the graph, a capacity below the live set, totals past 2^31,
    a set larger than its capacity: the flag each time, in-bounds writes only."""
    g, dg = graph
    seed, layer = 3, 0
    deg = np.diff(g.indptr)
    base = ROWS[:100]
    live, nlive_t = cso.closure_mark(dg, _t(base.astype(np.int32), dev), True)
    nlive = int(nlive_t)
    live_h = np.union1d(base, np.flatnonzero(race_keys(seed, layer, g.indptr, g.indices, base)[0]))
    cap = nlive + 3

    def want(indptr, indices, rows_h):  # the valid entries keep their row positions
        ok = (rows_h >= 0) & (rows_h < N)
        r = np.where(ok, rows_h, 0)  # node 0 has no entries
        i, c, _ = _entries(indptr, indices, r)
        m = (c >= 0) & (c < N)
        return _column_max(N, i[m], c[m], entry_values(seed, layer, i[m], c[m]))

    def check(indptr_h, indices_h, rows_h, **kw):
        count, key, total, err = _race(_t(indptr_h, dev), _t(indices_h, dev), N, _t(rows_h.astype(np.int32), dev), live, cap,
                                       seed, layer, dev, **kw)
        assert int(err[0]) == 1 and not err[1:].any()
        assert bool((count[cap:] == -7).all()) and bool((key[cap:] == -7).all()) and bool((total[1:] == -7).all())
        return count, key, total

    assert deg[0] == 0
    rows_bad = np.concatenate([base[:50], [N + 5, -3, 2**31 - 1], base[50:]]).astype(np.int64)
    counts, keys = want(g.indptr, g.indices, rows_bad)
    count, key, total = check(g.indptr, g.indices, rows_bad)
    assert np.array_equal(count[:nlive].cpu().numpy(), counts[live_h]) and np.array_equal(_u64(key[:nlive]), keys[live_h])
    assert int(total[0]) == counts.sum()

    last = int(np.flatnonzero(base == base.max())[0])
    indptr = g.indptr.copy()
    indptr[base.max() + 1] = g.indptr[-1] + 50  # that row now ends past the index array
    counts, _ = want(g.indptr, g.indices, np.where(np.arange(100) == last, 0, base))
    count, key, total = check(indptr, g.indices, base)
    assert np.array_equal(count[:nlive].cpu().numpy(), counts[live_h]) and int(total[0]) == counts.sum()
    indptr = g.indptr.copy()
    indptr[base[7] + 1] = indptr[base[7]] - 1  # running backwards
    check(indptr, g.indices, base)

    r2 = int(base[deg[base] == 2][0])
    indices = g.indices.copy()
    indices[g.indptr[r2] + 1] = N + 3
    counts, keys = want(g.indptr, indices, base)
    count, key, total = check(g.indptr, indices, base)
    assert np.array_equal(count[:nlive].cpu().numpy(), counts[live_h]) and np.array_equal(_u64(key[:nlive]), keys[live_h])

    # a capacity below the live set: the columns at positions >= cap are dropped
    short = nlive - 9
    count, key, total, err = _race(dg.indptr, dg.indices, N, _t(base.astype(np.int32), dev), live, short, seed, layer, dev)
    counts, keys = race_keys(seed, layer, g.indptr, g.indices, base)
    assert int(err[0]) == 1 and np.array_equal(count[:short].cpu().numpy(), counts[live_h[:short]])
    assert bool((count[short:] == -7).all()) and bool((key[short:] == -7).all())
    assert int(total[0]) == counts[live_h[:short]].sum()

    # finish: degrees of 2^30 in a made-up row pointer (no index array is read): every total >= 2^31
    fake = _t(np.arange(5, dtype=np.int64) << 30, dev)
    rows3 = _t(np.array([0, 0, 0], np.int32), dev)
    after3 = _t(np.array([0, 1, 2], np.int32), dev)
    zero_tab, _ = cso.closure_mark(_no_graph(4, rows3), rows3[:0].contiguous(), False)
    one = _t(np.array([3, 10, 2], np.int64), dev)  # K, total, s_num
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    out = _finish(SimpleNamespace(indptr_t=None, indices=None, indices_t=None), 4, rows3, after3, one[0:], 3, zero_tab, cnt,
                  1, one[1:], one[2:], dev, indptr=fake, n_entries=2**40)
    normfact, colptr, rowseg, colseg, totals, err = out
    assert int(err[0]) == 1 and rowseg[:4].tolist() == [0, 0, 0, 0] and colseg[:4].tolist() == [0, 0, 0, 0]
    assert colptr[:4].tolist() == [0, 0, 0, 0] and totals[:3].tolist() == [0, 2**31 - 1, 2**31 - 1]
    assert bool((normfact[:3] == np.float32(1) / np.float32(1e-10)).all()) and bool((normfact[3:] == -7.0).all())
    # ... and a set that does not fit its capacity: clamped to it
    out = _finish(SimpleNamespace(indptr_t=None, indices=None, indices_t=None), 4, rows3[:1], after3, one[0:], 2, zero_tab,
                  cnt, 1, one[1:], one[2:], dev, indptr=fake, n_entries=2**40)
    normfact, colptr, rowseg, colseg, totals, err = out
    assert int(err[0]) == 1 and bool((colptr[3:] == -7).all()) and bool((normfact[2:] == -7.0).all())
    assert rowseg[:2].tolist() == [0, 2**30] and colseg[:3].tolist() == [0, 0, 0] and bool((colseg[3:] == -7).all())  # 2^31


def test_refusals_launch_nothing(graph, dev):
    g, dg = graph
    L = _lib.lib()
    rows = _t(ROWS.astype(np.int32), dev)
    M = ROWS.size
    cap = N
    kcap = N
    Eg = int(dg.indices.numel())
    live, nlive_t = cso.closure_mark(dg, rows, True)
    nlive_t = nlive_t.reshape(1)
    live_ids = cso.closure_list(live, N, N)
    count, key = _sent(cap, torch.int32, dev), _sent(cap, torch.int64, dev)
    word = _sent(8, torch.int64, dev)
    ids = _sent(cap, torch.int32, dev)
    normfact = torch.full((kcap,), -7.0, dtype=torch.float32, device=dev)
    colptr, colseg, rowseg = _sent(kcap + 1, torch.int32, dev), _sent(kcap + 1, torch.int32, dev), _sent(M + 1, torch.int32, dev)
    wsb = max(L.gnn_lw_select_workspace_bytes(), L.gnn_lw_finish_workspace_bytes(M, kcap))
    ws = torch.full((wsb + 64,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = _lib.stream_of(dev)
    w = lambda i: word[i:].data_ptr()

    def c_race(**kw):
        a = dict(N=N, E=Eg, M=M, live=live.data_ptr(), layer=0, count=count.data_ptr(), key=key.data_ptr(), cap=cap,
                 total=w(1), indptr=dg.indptr.data_ptr(), rows=rows.data_ptr())
        a.update(kw)
        return L.gnn_lw_race(a["indptr"], dg.indices.data_ptr(), a["N"], a["E"], a["rows"], a["M"], a["live"], 3,
                             a["layer"], a["count"], a["key"], a["cap"], a["total"], None, st)

    def c_select(**kw):
        a = dict(key=key.data_ptr(), count=count.data_ptr(), nlive=nlive_t.data_ptr(), cap=cap, samp=5,
                 live_ids=live_ids.data_ptr(), ids=ids.data_ptr(), s_num=w(2), tau=w(3), ws=ws.data_ptr(), wsb=wsb)
        a.update(kw)
        return L.gnn_lw_select(a["key"], a["count"], a["nlive"], a["cap"], a["samp"], a["live_ids"], a["ids"],
                               a["s_num"], a["tau"], a["ws"], a["wsb"], st)

    def c_finish(**kw):
        a = dict(E=Eg, N=N, M=M, K=w(4), kcap=kcap, live=live.data_ptr(), count=count.data_ptr(), cap=cap, total=w(1),
                 s_num=w(2), normfact=normfact.data_ptr(), colptr=colptr.data_ptr(), rowseg=rowseg.data_ptr(),
                 colseg=colseg.data_ptr(), totals=w(5), ws=ws.data_ptr(), wsb=wsb, after=live_ids.data_ptr())
        a.update(kw)
        return L.gnn_lw_finish(dg.indptr.data_ptr(), a["E"], dg.indptr_t.data_ptr(), a["E"], a["N"], rows.data_ptr(),
                               a["M"], a["after"], a["K"], a["kcap"], a["live"], a["count"], a["cap"], a["total"],
                               a["s_num"], a["normfact"], a["colptr"], a["rowseg"], a["colseg"], a["totals"], a["ws"],
                               a["wsb"], None, st)

    cases = [(c_race, dict(M=-1), b"negative"), (c_race, dict(cap=-1), b"negative"), (c_race, dict(N=2**31), b"2^31"),
             (c_race, dict(M=2**31), b"2^31"), (c_race, dict(cap=2**31), b"2^31"), (c_race, dict(layer=-1), b"layer"),
             (c_race, dict(total=None), b"NULL total"), (c_race, dict(live=None), b"NULL live"),
             (c_race, dict(live=live.data_ptr() + 4), b"8-byte"), (c_race, dict(count=None), b"NULL count"),
             (c_race, dict(key=None), b"NULL count"), (c_race, dict(key=key.data_ptr() + 4), b"8-byte"),
             (c_race, dict(indptr=None), b"NULL indptr"), (c_race, dict(rows=None), b"NULL indptr"),
             (c_select, dict(cap=-1), b"negative"), (c_select, dict(cap=2**31), b"2^31"),
             (c_select, dict(samp=0), b"samp_num"), (c_select, dict(nlive=None), b"NULL ntab"),
             (c_select, dict(s_num=None), b"NULL ntab"), (c_select, dict(tau=None), b"NULL ntab"),
             (c_select, dict(key=None), b"NULL key"), (c_select, dict(count=None), b"NULL key"),
             (c_select, dict(live_ids=None), b"NULL key"),
             (c_select, dict(ids=None), b"NULL key"), (c_select, dict(tau=w(3) + 4), b"8-byte"),
             (c_select, dict(wsb=L.gnn_lw_select_workspace_bytes() - 1), b"workspace too small"),
             (c_select, dict(ws=None), b"workspace too small"), (c_select, dict(ws=ws.data_ptr() + 8), b"16-byte aligned"),
             (c_finish, dict(M=-1), b"negative"), (c_finish, dict(kcap=-1), b"negative"), (c_finish, dict(E=-1), b"negative"),
             (c_finish, dict(N=2**31), b"2^31"), (c_finish, dict(kcap=2**31), b"2^31"), (c_finish, dict(K=None), b"NULL K"),
             (c_finish, dict(totals=None), b"NULL K"), (c_finish, dict(totals=w(5) + 4), b"8-byte"),
             (c_finish, dict(live=None), b"NULL live"), (c_finish, dict(colptr=None), b"NULL colptr_t"),
             (c_finish, dict(rowseg=None), b"NULL colptr_t"), (c_finish, dict(colseg=None), b"NULL colptr_t"),
             (c_finish, dict(count=None), b"NULL count"), (c_finish, dict(after=None), b"NULL after"),
             (c_finish, dict(normfact=None), b"NULL after"),
             (c_finish, dict(wsb=L.gnn_lw_finish_workspace_bytes(M, kcap) - 1), b"workspace too small"),
             (c_finish, dict(ws=None), b"workspace too small"), (c_finish, dict(ws=ws.data_ptr() + 8), b"16-byte aligned")]
    for fn, kw, msg in cases:
        assert fn(**kw) == -22, (fn.__name__, kw)
        assert msg in L.gnn_last_error(), (fn.__name__, kw, L.gnn_last_error())
    torch.cuda.synchronize()
    for t_ in (count, key, word, ids, colptr, colseg, rowseg):  # nothing ran
        assert bool((t_ == -7).all())
    assert bool((normfact == -7.0).all()) and bool((ws == 0x5A).all())
    assert c_race() == 0 and c_select() == 0
    torch.cuda.synchronize()
    assert int(word[2]) == 5 and int((ids[:N] >= 0).sum()) == 5


def test_capture_replays_bit_identically(graph, dev):
    """The per-layer call sequence up to the read, captured on one stream (no parallel branches)."""
    g, dg = graph
    L = _lib.lib()
    rows = _t(ROWS.astype(np.int32), dev)
    M, samp, seed, layer = ROWS.size, 150, SEEDS[1], 1
    cap = N
    kcap = min(N, M + samp)
    tb = L.gnn_closure_table_bytes(N)
    wsb = max(L.gnn_closure_workspace_bytes(N), L.gnn_lw_select_workspace_bytes(), L.gnn_lw_finish_workspace_bytes(M, kcap))
    mk = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    live, table, ws = mk(tb, torch.uint8), mk(tb, torch.uint8), mk(wsb, torch.uint8)
    live_ids, count, key = mk(cap, torch.int32), mk(cap, torch.int32), mk(cap, torch.int64)
    seeds = mk(M + cap, torch.int32)
    seeds[:M] = rows
    after, normfact = mk(kcap, torch.int32), mk(kcap, torch.float32)
    colptr, colseg, rowseg = mk(kcap + 1, torch.int32), mk(kcap + 1, torch.int32), mk(M + 1, torch.int32)
    word = mk(9, torch.int64)
    outs = (live, table, live_ids, count, key, seeds, after, normfact, colptr, colseg, rowseg, word)
    Eg, Et = int(dg.indices.numel()), int(dg.indices_t.numel())
    w = lambda i: word[i:].data_ptr()

    def sequence(st):
        ck = _lib.check
        ck(L.gnn_closure_mark(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, rows.data_ptr(), M, 1, live.data_ptr(),
                              w(0), ws.data_ptr(), wsb, st), "mark")
        ck(L.gnn_closure_list(live.data_ptr(), N, live_ids.data_ptr(), cap, st), "list")
        ck(L.gnn_lw_race(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, Eg, rows.data_ptr(), M, live.data_ptr(), seed,
                         layer, count.data_ptr(), key.data_ptr(), cap, w(1), w(8), st), "race")
        ck(L.gnn_lw_select(key.data_ptr(), count.data_ptr(), w(0), cap, samp, live_ids.data_ptr(), seeds[M:].data_ptr(),
                           w(2), w(3), ws.data_ptr(), wsb, st), "select")
        ck(L.gnn_closure_mark(None, None, N, seeds.data_ptr(), M + cap, 0, table.data_ptr(), w(4), ws.data_ptr(), wsb,
                              st), "mark")
        ck(L.gnn_closure_list(table.data_ptr(), N, after.data_ptr(), kcap, st), "list")
        ck(L.gnn_lw_finish(dg.indptr.data_ptr(), Eg, dg.indptr_t.data_ptr(), Et, N, rows.data_ptr(), M, after.data_ptr(),
                           w(4), kcap, live.data_ptr(), count.data_ptr(), cap, w(1), w(2), normfact.data_ptr(),
                           colptr.data_ptr(), rowseg.data_ptr(), colseg.data_ptr(), w(5), ws.data_ptr(), wsb, w(8), st),
           "finish")

    sequence(_lib.stream_of(dev))
    torch.cuda.synchronize()
    direct = [t_.clone() for t_ in outs]
    hb = ladies_race_host(seed, ROWS, samp, g, [0, 1])
    K = int(word[4])
    assert np.array_equal(after[:K].cpu().numpy(), hb.sets[1]) and int(word[5]) == hb.layers[1][0][-1]
    assert int(word[8]) == 0
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        sequence(_lib.stream_of(dev))
    for t_ in outs[:5] + outs[6:-1]:
        t_.fill_(0x33)
    seeds[M:] = 0x33
    word[:8] = 0x33  # word 8 is the error flag the calls OR into: the caller's to clear
    cg.replay()
    torch.cuda.synchronize()
    ntab, tbl = int(word[0]), ((N + 31) // 32 + 1) * 8  # what the calls write of each output: the rest keeps the fill
    valid = (tbl, tbl, ntab, cap, cap, M + cap, K, K, K + 1, K + 1, M + 1, 9)
    for got, want, n in zip(outs, direct, valid):
        assert torch.equal(got[:n], want[:n])


# ----------------------------------------------------------------------------- the sampler

CASES = [("graphsage", [1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1]), ("gcn", [1, 0, 1])]
IDS = ["sage11", "sage101", "gcn11", "gcn101"]
NN = 600
BATCH = np.concatenate([np.arange(40, 560, 7)[::-1], [0, 77, 40, 47]])


def _labels(n, C):
    cls = np.random.default_rng(2).integers(0, C, n)
    return sp.csr_matrix((np.ones(n, np.int32), (np.arange(n), cls)), shape=(n, C))


@pytest.fixture(scope="module")
def worlds():
    """(lap, feats, labels) per model name, made once and left unchanged."""
    out = {}
    for name in ("graphsage", "gcn"):
        lap, feats = make_world(name, NN, 48)
        out[name] = (lap, feats, _labels(NN, 7))
    return out


def _assert_batch(b, hb, table, labels, batch, orders, unique):
    x0, adjs, sampled, lab = b
    assert b.input_nodes.dtype == torch.int64 and np.array_equal(b.input_nodes.cpu().numpy(), hb.input_nodes)
    assert x0.dtype == torch.float32 and x0.stride(1) == 1 and x0.stride(0) % 32 == 0
    assert torch.equal(x0.cpu(), table[torch.from_numpy(hb.input_nodes)].float())  # widened exactly
    assert torch.equal(lab.cpu(), torch.from_numpy(np.asarray(labels[batch].todense(), dtype=np.float32)))
    top = max(l for l, o in enumerate(orders) if o)
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
            M, K = shape
            assert op._t is not None and op._t.shape == (K, M)
            L = _lib.lib()
            dev = op.device
            tp = torch.empty(K + 1, dtype=torch.int32, device=dev)
            tc = torch.empty(op.nnz, dtype=torch.int32, device=dev)
            tv = torch.empty(op.nnz, dtype=torch.float32, device=dev)
            wsb = L.gnn_csr_transpose_workspace_bytes(M, K, op.nnz)
            ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
            _lib.check(L.gnn_csr_transpose(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), M, K, op.nnz,
                                           tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), ws.data_ptr(), wsb,
                                           _lib.stream_of(dev)), "gnn_csr_transpose")
            assert torch.equal(op._t.rowptr, tp) and torch.equal(op._t.col, tc) and torch.equal(op._t.val, tv)
            rm = getattr(sampled[l], "_gnn_rmap", None)
            if l == top and not unique:
                assert rm is None  # repeated batch nodes: the fused residual's row map needs unique rows
            else:
                sn = sampled[l].cpu().numpy()
                rm = rm.cpu().numpy()
                assert rm.dtype == np.int32 and np.array_equal(rm[sn], np.arange(sn.size)) and (rm >= 0).sum() == sn.size
        else:
            assert op._t is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_sampler_equals_host_batch(dev, worlds, name, orders, dtype):
    lap, feats, labels = worlds[name]
    table = feats.to(dtype)
    samp = [90, 70, 50][: len(orders)]
    ls = LayerwiseSampler(lap, samp, orders, table, labels, dev)
    _assert_batch(ls.sample(BATCH, 21), ladies_race_host(21, BATCH, samp, lap, orders), table, labels, BATCH, orders, False)
    uniq = BATCH[:-2]
    ls_d = LayerwiseSampler(lap, 64, orders, table.to(dev), labels, dev)  # a table already on the device
    _assert_batch(ls_d.sample(uniq, SEEDS[1]), ladies_race_host(SEEDS[1], uniq, 64, lap, orders), table, labels, uniq,
                  orders, True)


def test_sampler_on_the_hand_graph_and_the_large_one(graph, big, dev):
    for (g, dg), rows, samp in ((graph, ROWS, 200), (big[:2], big[2], 30_000)):
        Nn = g.num_nodes
        feats = torch.from_numpy(np.random.default_rng(1).standard_normal((Nn, 8)).astype(np.float32)).half()
        labels = _labels(Nn, 3)
        ls = LayerwiseSampler(g, samp, [1, 1], feats, labels, dev)
        b = ls.sample(rows, SEEDS[1])
        _assert_batch(b, ladies_race_host(SEEDS[1], rows, samp, g, [1, 1]), feats, labels, rows, [1, 1],
                      np.unique(rows).size == rows.size)


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _grads(tr):
    return [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in tr.params]


@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_native_step_takes_the_batch_and_matches_python_path(dev, worlds, name, orders):
    """One training step (dropout 0.1, the same seeds) and one evaluation on the native executor
    against the Python autograd path: tests/test_neighbor_gpu.py's bounds for that comparison —
    loss within 1e-6 |loss| + 1e-7, every gradient within 1e-5 in relative L2."""
    lap, feats, labels = worlds[name]
    ls = LayerwiseSampler(lap, 128, orders, feats, labels, dev)
    batch = ls.sample(np.arange(40, 560, 2), 9)
    args = tuple(batch)

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
    print(f"layerwise {name} {orders}: eval loss {ea['loss']:.8f} / {eb['loss']:.8f}")
    assert eb["rows"] == 260 and abs(ea["loss"] - eb["loss"]) <= 1e-6 * abs(ea["loss"]) + 1e-7
    torch.manual_seed(100)
    la = ta.step(*args)
    unused = [p.grad is None for p in ta.params]
    ga = _grads(ta)
    torch.manual_seed(100)
    lb = tb.step(*args)
    gb = _grads(tb)
    torch.cuda.synchronize()
    print(f"layerwise {name} {orders}: loss {float(la):.8f} / {float(lb):.8f}, max gradient error "
          f"{max(_rel(x, y) for x, y, u in zip(gb, ga, unused) if not u):.2e}")
    assert np.isfinite(float(lb)) and abs(float(la) - float(lb)) <= 1e-6 * abs(float(la)) + 1e-7
    for i, (x, y, u) in enumerate(zip(gb, ga, unused)):
        if u:
            assert not bool(x.any()), i
        else:
            assert _rel(x, y) <= 1e-5, (i, _rel(x, y))
