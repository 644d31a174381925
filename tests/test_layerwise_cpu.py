"""The layer-wise race draw on the host: its law against the exact inclusion probabilities of
successive sampling, the distinctness of its keys, ``ladies_race_host`` against a restatement of the
reference sampler's layer (sampler.py:113-139) given the drawn set, and LayerwiseSampler on the CPU."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import custom_sparse_ops as cso
from gnn_amd import models
from gnn_amd.layerwise import (LayerwiseSampler, batch_seed, entry_values, ladies_race_host, mix64, race_key, race_keys,
                               race_select)
from gnn_amd.layerwise import _column_max, _entries
from gnn_amd.train import Trainer
from test_exact_cpu import make_world

LAW_CASES = [([3, 1, 1, 2, 1], 2), ([5, 1, 1, 1], 1), ([2, 2, 1, 1, 4, 1], 3), ([7, 3, 1, 1, 1, 1, 1], 4)]
T = 20_000


def _inclusion(w, s):
    """Exact inclusion probabilities of s successive draws without replacement proportional to w."""
    n = len(w)
    p = np.zeros(n)
    for order in itertools.permutations(range(n), s):
        pr, left = 1.0, float(sum(w))
        for j in order:
            pr *= w[j] / left
            left -= w[j]
        p[list(order)] += pr
    return p


def _tiny_u(w):
    """Column j in rows 0 .. w[j]-1: (row positions, column slots) of a U with those column counts."""
    i = np.concatenate([np.arange(x) for x in w])
    j = np.repeat(np.arange(len(w)), w)
    return i, j


def _tiny_graph(w, ids, N):
    """The graph whose rows 0 .. max(w)-1 are that U with column slot j at node ids[j]."""
    i, j = _tiny_u(w)
    return sp.csr_matrix((np.ones(i.size, np.float32), (i, np.asarray(ids)[j])), shape=(N, N))


def _included(w, s, K, cols):
    """Inclusion counts per column slot over T draws: keys K uint64[T], column ids cols int64[T, n]."""
    i, j = _tiny_u(w)
    with np.errstate(over="ignore"):
        h = mix64(((cols[:, j].astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)[None, :]) + K[:, None])
    first = np.concatenate([[0], np.cumsum(w)[:-1]])
    key = np.maximum.reduceat(h, first, axis=1)  # [T, n]
    top = np.argsort(key, axis=1)[:, len(w) - s:]
    return np.bincount(top.reshape(-1), minlength=len(w))


def _assert_law(w, s, got, what):
    p = _inclusion(w, s)
    assert abs(p.sum() - s) < 1e-9
    sigma = np.sqrt(T * p * (1 - p))
    z = (got - T * p) / sigma
    print(f"law {what} w={w} s={s}: worst {np.abs(z).max():.2f} sigma")
    assert got.sum() == T * s and np.all(np.abs(z) <= 5.0), (w, s, z)


@pytest.mark.parametrize("w,s", LAW_CASES)
def test_law_over_seeds(w, s):
    seeds = 12345 + 7919 * np.arange(T)
    cols = np.broadcast_to(np.arange(len(w), dtype=np.int64), (T, len(w)))
    got = _included(w, s, race_key(seeds, 0), cols)
    _assert_law(w, s, got, "seeds")
    # the vectorised count is the sampler's own draw: the first seeds through race_keys / race_select
    g = _tiny_graph(w, np.arange(len(w)), max(max(w), len(w)))
    rows = np.arange(max(w))
    for t in range(50):
        counts, keys = race_keys(int(seeds[t]), 0, g.indptr, g.indices, rows)
        assert np.array_equal(counts[: len(w)], w)
        s_num, sel = race_select(counts, keys, s)
        one = _included(w, s, race_key(seeds[t: t + 1], 0), cols[:1])
        assert s_num == s and np.array_equal(np.flatnonzero(one), sel)


@pytest.mark.parametrize("w,s", LAW_CASES)
def test_law_over_column_ids(w, s):
    """The seed fixed, the columns at 20,000 different places in the id space."""
    n = len(w)
    cols = (1000 + 13 * np.arange(T))[:, None] + np.arange(n, dtype=np.int64)[None, :] * 3
    got = _included(w, s, np.broadcast_to(race_key(777, 0), (T,)), cols)
    _assert_law(w, s, got, "column ids")
    N = int(cols.max()) + 1
    for t in (0, 1, T - 1):
        g = _tiny_graph(w, cols[t], N)
        counts, keys = race_keys(777, 0, g.indptr, g.indices, np.arange(max(w)))
        one = _included(w, s, race_key(np.array([777]), 0), cols[t: t + 1])
        assert np.array_equal(cols[t][np.flatnonzero(one)], race_select(counts, keys, s)[1])


def _random_graph(N, deg, seed, self_loops=False):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(N), deg)
    c = rng.integers(0, N, r.size)
    if self_loops:
        r, c = np.concatenate([r, np.arange(N)]), np.concatenate([c, np.arange(N)])
    m = sp.csr_matrix((np.ones(r.size, np.float32), (r, c)), shape=(N, N))
    m.sum_duplicates()
    m.data[:] = 1.0
    return m


def test_entry_values_are_distinct_and_order_free():
    g = _random_graph(4000, 30, 1)
    rows = np.random.default_rng(2).integers(0, 4000, 3500)  # repeats: a repeated row counts again
    i, c, deg = _entries(g.indptr.astype(np.int64), g.indices, rows)
    assert i.size >= 100_000 and np.unique(rows).size < rows.size
    for seed, layer in ((3, 0), ((0x9ABCDEF1 << 32) | 0x12345678, 2)):
        h = entry_values(seed, layer, i, c)
        assert np.unique(h).size == h.size
        counts, keys = race_keys(seed, layer, g.indptr, g.indices, rows)
        assert counts.sum() == h.size and np.unique(keys[counts > 0]).size == (counts > 0).sum()
        assert not keys[counts == 0].any()
        perm = np.random.default_rng(5).permutation(h.size)
        c2, k2 = _column_max(4000, i[perm], c[perm], h[perm])
        assert np.array_equal(c2, counts) and np.array_equal(k2, keys)
        assert np.array_equal(keys, np.array([h[c == v].max() if counts[v] else 0 for v in range(200)] +
                                             list(keys[200:]), dtype=np.uint64))
    assert race_key(3, 0) != race_key(3, 1) and race_key(3, 0) != race_key(4, 0)
    assert int(mix64(0x9E3779B97F4A7C15)) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0
    assert int(race_key(0, 0)) == 0xE220A8397B1DCDAF


def _reference_layer(lap, rows, after, samp, counts_want=None):
    """sampler.py:113-139 given the drawn set: U, pi, p, s_num, U[:, after], normfact and
    create_coo_tensor's CPU branch. Returns (rowptr, col, val, s_num, pi)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    U = lap[rows, :]
    pi = np.asarray(sp.linalg.norm(U, ord=0, axis=0)).reshape(-1)
    p = pi / np.sum(pi)
    s_num = np.min([np.sum(p > 0), samp])
    adj = U[:, after]
    normfact = 1 / np.clip(s_num * p[after], 1e-10, 1).astype(np.float32)
    coo = cso.create_coo_tensor(t(U.indptr.astype(np.int32)), t(adj.indptr.astype(np.int32)),
                                t(adj.indices.astype(np.int32)), t(normfact), adj.shape[0], adj.shape[1])
    r, c = coo.indices().numpy()
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=adj.shape[0]))])
    return rowptr, c, coo.values().numpy(), int(s_num), pi, normfact


def _check_batch(lap, batch, samp, orders, seed):
    hb = ladies_race_host(seed, batch, samp, lap, orders)
    L = len(orders)
    rows = np.asarray(batch, dtype=np.int64)
    assert np.array_equal(hb.sets[L], rows) and np.array_equal(hb.input_nodes, hb.sets[0])
    samp_l = [samp] * L if np.ndim(samp) == 0 else [samp[L - 1 - l] for l in range(L)]
    for l in range(L - 1, -1, -1):
        if orders[l] == 0:
            assert hb.layers[l] is None and hb.sampled_nodes[l].size == 0 and hb.sets[l] is hb.sets[l + 1]
            continue
        after = hb.sets[l]
        rowptr, col, val, s_num, pi, normfact = _reference_layer(lap, rows, after, samp_l[l])
        # the set: the s_num live columns with the largest keys, joined by the rows
        counts, keys = race_keys(seed, l, lap.indptr, lap.indices, rows)
        assert np.array_equal(counts, pi.astype(np.int64))
        live = np.flatnonzero(pi)
        sel = live[np.argsort(keys[live])[live.size - s_num:]]
        assert np.array_equal(after, np.unique(np.concatenate([sel, rows]))) and s_num == hb.s_num[l]
        g_rowptr, g_col, g_val, shape = hb.layers[l]
        assert shape == (rows.size, after.size) and g_rowptr.dtype == np.int32 and g_col.dtype == np.int32
        assert np.array_equal(g_rowptr, rowptr) and np.array_equal(g_col, col)
        assert g_val.dtype == np.float32 and np.array_equal(g_val, val)
        assert np.array_equal(hb.normfact[l], normfact)
        assert np.array_equal(after[hb.sampled_nodes[l]], rows)
        if np.unique(rows).size == rows.size and np.all(np.diff(rows) > 0):
            assert np.array_equal(hb.sampled_nodes[l], np.where(np.isin(after, rows))[0])
        rows = after
    return hb


@pytest.mark.parametrize("orders", [[1], [1, 1], [1, 0, 1], [0, 1, 1, 0]])
def test_host_batch_equals_reference_layer(orders):
    lap = _random_graph(900, 6, 3, self_loops=True)
    batch = np.random.default_rng(4).permutation(900)[:64]
    _check_batch(lap, batch, 100, orders, 21)
    _check_batch(lap, batch, [100, 50, 75, 60][: len(orders)], orders, (0x9ABCDEF1 << 32) | 5)


def test_host_batch_edge_cases():
    """No self-loops: a batch node that is nobody's column (normfact 1 / float32(1e-10), an empty
    column); samp_num >= the live columns; samp_num = 1; repeated batch nodes; a degree-0 node."""
    lap = _random_graph(300, 4, 8).tolil()
    lap[:, 5] = 0   # node 5 is nobody's column
    lap[9, :] = 0   # node 9 has no entries
    lap = lap.tocsr()
    lap.eliminate_zeros()
    lap.data[:] = 1.0
    batch = np.array([40, 5, 9, 40, 299, 0, 17, 5])
    hb = _check_batch(lap, batch, 10_000, [1, 1], 2)  # everything live is drawn
    top = hb.layers[1]
    k5 = int(np.searchsorted(hb.sets[1], 5))
    assert hb.sets[1][k5] == 5 and hb.normfact[1][k5] == np.float32(1) / np.float32(1e-10)
    assert not (top[1] == k5).any()  # its column is empty
    assert top[0][3] - top[0][2] == 0 and top[0][1] - top[0][0] == top[0][4] - top[0][3] > 0  # node 9; 40 twice
    counts, _ = race_keys(2, 1, lap.indptr, lap.indices, batch)
    assert hb.s_num[1] == (counts > 0).sum()
    one = _check_batch(lap, batch, 1, [1, 1], 2)
    assert one.s_num == [1, 1] and one.sets[1].size <= np.unique(batch).size + 1
    _check_batch(lap, batch, 7, [1, 0, 1], 11)
    with pytest.raises(ValueError, match="orders"):
        ladies_race_host(1, batch, 5, lap, [1, 2])
    with pytest.raises(ValueError, match="sample sizes"):
        ladies_race_host(1, batch, [5], lap, [1, 1])
    with pytest.raises(ValueError, match="sample sizes"):
        ladies_race_host(1, batch, 0, lap, [1, 1])
    with pytest.raises(ValueError, match=r"ids in \[0, 300\)"):
        ladies_race_host(1, [300], 5, lap, [1])
    weighted = lap.copy()
    weighted.data[3] = 0.0
    with pytest.raises(ValueError, match="stores values"):
        ladies_race_host(1, batch, 5, weighted, [1])


def _labels(N, C):
    cls = np.random.default_rng(2).integers(0, C, N)
    return sp.csr_matrix((np.ones(N, np.int32), (np.arange(N), cls)), shape=(N, C))


@pytest.mark.parametrize("name,orders", [("graphsage", [1, 0, 1]), ("gcn", [1, 1])], ids=["sage101", "gcn11"])
def test_cpu_sampler_equals_host_batch_and_trains(name, orders):
    C, nfeat, NN = 7, 12, 600
    lap, feats = make_world(name, NN, nfeat)
    labels = _labels(NN, C)
    batch = np.concatenate([np.arange(40, 560, 7)[::-1], [0, 77, 40, 47]])
    ls = LayerwiseSampler(lap, 64, orders, feats.to(torch.bfloat16), labels, "cpu")
    b = ls.sample(batch, 21)
    hb = ladies_race_host(21, batch, 64, lap, orders)
    x0, adjs, sampled, lab = b
    assert np.array_equal(b.input_nodes.numpy(), hb.input_nodes)
    assert x0.dtype == torch.float32 and torch.equal(x0, feats.to(torch.bfloat16)[b.input_nodes].float())
    assert torch.equal(lab, torch.from_numpy(np.asarray(labels[batch].todense(), dtype=np.float32)))
    for l, o in enumerate(orders):
        if o == 0:
            assert adjs[l] is None and sampled[l].numel() == 0
            continue
        rowptr, col, val, shape = hb.layers[l]
        a = adjs[l]
        assert a.is_coalesced() and tuple(a.shape) == shape
        assert np.array_equal(a.indices()[0].numpy(), np.repeat(np.arange(shape[0]), np.diff(rowptr)))
        assert np.array_equal(a.indices()[1].numpy(), col) and np.array_equal(a.values().numpy(), val)
        assert np.array_equal(sampled[l].numpy(), hb.sampled_nodes[l])

    torch.manual_seed(0)
    model = models.build_model(name, nfeat, 16, orders, C, dropout=0.1)
    tr = Trainer(model, 0.01, "cpu")
    before = [p.detach().clone() for p in tr.params]
    train = LayerwiseSampler(lap, 64, orders, feats, labels, "cpu")
    nodes = np.arange(40, 560)
    first = next(iter(train.epoch(nodes, 200, seed=3)))
    assert first.seed == batch_seed(3, 0) and np.unique(first.batch_nodes).size == 200
    assert np.isfinite(float(tr.step(*first)))
    assert any(not torch.equal(p.detach(), q) for p, q in zip(tr.params, before))
    assert np.array_equal(np.concatenate([b.batch_nodes for b in train.sequential(nodes, 200)]), nodes)
    res = tr.evaluate(train.sequential(nodes[:300], 128))
    assert res["rows"] == 300 and res["batches"] == 3 and np.isfinite(res["loss"])
    with pytest.raises(ValueError, match="scale_factor"):
        LayerwiseSampler(lap, 64, orders, feats, labels, "cpu", scale_factor=2.0)
    with pytest.raises(ValueError, match="feats"):
        LayerwiseSampler(lap, 64, orders, feats.double(), labels, "cpu")
