"""The locality-skewed layer-wise draw on the host: the law of the replica race against the exact
inclusion probabilities of successive sampling proportional to w = count * s, the distinctness of
all replica values, its reduction to the plain draw, ``ladies_race_host`` against a restatement of
the reference's layer (sampler.py:113-139 with pi[F] *= scale) given the drawn set, the skew's
effect on the drawn columns, and LayerwiseSampler / PlacedFeatures.resident_nodes on the CPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import custom_sparse_ops as cso
from gnn_amd import models
from gnn_amd.layerwise import (LayerwiseSampler, _column_max, _entries, favoured_bits, ladies_race_host, mix64,
                               race_key, race_keys, race_normfact, race_select, replica_max)
from gnn_amd.placed import PLACE_HOST, PLACE_SHIFT, PlacedFeatures, pack_placement
from gnn_amd.train import Trainer
from test_exact_cpu import make_world
from test_layerwise_cpu import T, _inclusion, _labels, _random_graph, _tiny_graph, _tiny_u

# (counts, favoured flags, scale, s)
LAW_CASES = [([3, 1, 1, 2, 1], [0, 1, 0, 1, 0], 3, 2), ([2, 2, 1, 1, 4, 1], [1, 0, 0, 1, 0, 1], 2, 3),
             ([5, 1, 1, 1], [0, 1, 1, 0], 16, 1), ([1, 1, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0], 64, 2),
             ([7, 3, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 0, 0], 5, 4), ([3, 1, 1, 2, 1], [1, 1, 1, 1, 1], 4, 2)]
NN = 600


def _weights(counts, fav, scale):
    return [c * (scale if f else 1) for c, f in zip(counts, fav)]


def _included(counts, fav, scale, s, K, cols):
    """Inclusion counts per column slot over T draws of the replica race: keys K uint64[T], column
    ids cols int64[T, n]. Replica r of the entry (i, j): mix64((col_j << 32 | r << 26 | i) + K)."""
    i, j = _tiny_u(counts)
    rep = np.array([scale if fav[x] else 1 for x in j])
    ii, jj = np.repeat(i, rep), np.repeat(j, rep)  # replicas, grouped by column slot
    rr = np.concatenate([np.arange(x) for x in rep])
    with np.errstate(over="ignore"):
        h = mix64(((cols[:, jj].astype(np.uint64) << np.uint64(32)) | (rr.astype(np.uint64) << np.uint64(26))[None, :]
                   | ii.astype(np.uint64)[None, :]) + K[:, None])
    w = _weights(counts, fav, scale)
    first = np.concatenate([[0], np.cumsum(w)[:-1]])
    key = np.maximum.reduceat(h, first, axis=1)  # [T, n]
    top = np.argsort(key, axis=1)[:, len(counts) - s:]
    return np.bincount(top.reshape(-1), minlength=len(counts))


def _assert_law(w, s, got, what):
    p = _inclusion(w, s)
    assert abs(p.sum() - s) < 1e-9
    sigma = np.sqrt(T * p * (1 - p))
    z = (got - T * p) / sigma
    print(f"skewed law {what} w={w} s={s}: worst {np.abs(z).max():.2f} sigma")
    assert got.sum() == T * s and np.all(np.abs(z) <= 5.0), (w, s, z)


@pytest.mark.parametrize("counts,fav,scale,s", LAW_CASES)
def test_law_over_seeds(counts, fav, scale, s):
    n = len(counts)
    seeds = 12345 + 7919 * np.arange(T)
    cols = np.broadcast_to(np.arange(n, dtype=np.int64), (T, n))
    got = _included(counts, fav, scale, s, race_key(seeds, 0), cols)
    _assert_law(_weights(counts, fav, scale), s, got, "seeds")
    # the vectorised count is the sampler's own draw: the first seeds through race_keys / race_select
    g = _tiny_graph(counts, np.arange(n), max(max(counts), n))
    rows = np.arange(max(counts))
    for t in range(50):
        c_, keys = race_keys(int(seeds[t]), 0, g.indptr, g.indices, rows, np.flatnonzero(fav), scale)
        assert np.array_equal(c_[:n], counts)
        s_num, sel = race_select(c_, keys, s)
        one = _included(counts, fav, scale, s, race_key(seeds[t: t + 1], 0), cols[:1])
        assert s_num == s and np.array_equal(np.flatnonzero(one), sel)


@pytest.mark.parametrize("counts,fav,scale,s", LAW_CASES)
def test_law_over_column_ids(counts, fav, scale, s):
    """The seed fixed, the columns at 20,000 different places in the id space."""
    n = len(counts)
    cols = (1000 + 13 * np.arange(T))[:, None] + np.arange(n, dtype=np.int64)[None, :] * 3
    got = _included(counts, fav, scale, s, np.broadcast_to(race_key(777, 0), (T,)), cols)
    _assert_law(_weights(counts, fav, scale), s, got, "column ids")
    N = int(cols.max()) + 1
    for t in (0, 1, T - 1):
        g = _tiny_graph(counts, cols[t], N)
        c_, keys = race_keys(777, 0, g.indptr, g.indices, np.arange(max(counts)), cols[t][np.flatnonzero(fav)], scale)
        one = _included(counts, fav, scale, s, race_key(np.array([777]), 0), cols[t: t + 1])
        assert np.array_equal(cols[t][np.flatnonzero(one)], race_select(c_, keys, s)[1])


def test_replica_values_are_distinct_and_order_free():
    N = 2000
    g = _random_graph(N, 12, 1)
    rows = np.random.default_rng(2).integers(0, N, 1500)  # repeats: a repeated row counts again
    i, c, _ = _entries(g.indptr.astype(np.int64), g.indices, rows)
    assert np.unique(rows).size < rows.size and i.size > 15_000
    for seed, layer in ((3, 0), ((0x9ABCDEF1 << 32) | 0x12345678, 2)):
        K = race_key(seed, layer)
        with np.errstate(over="ignore"):
            h = np.stack([mix64(((c.astype(np.uint64) << np.uint64(32)) | np.uint64(r << 26) | i.astype(np.uint64)) + K)
                          for r in range(64)])  # [64, entries]: every replica of every entry
        assert np.unique(h).size == h.size
        counts, keys = race_keys(seed, layer, g.indptr, g.indices, rows, np.arange(N), 64)
        plain_counts, plain_keys = race_keys(seed, layer, g.indptr, g.indices, rows)
        assert np.array_equal(counts, plain_counts) and counts.sum() == i.size
        assert np.unique(keys[counts > 0]).size == (counts > 0).sum() and not keys[counts == 0].any()
        best = h.max(axis=0)
        assert np.array_equal(best, replica_max(seed, layer, i, c, np.full(i.size, 64)))
        want = np.array([best[c == v].max() if counts[v] else 0 for v in range(N)], dtype=np.uint64)
        assert np.array_equal(keys, want) and np.all(keys >= plain_keys) and np.any(keys > plain_keys)
        perm = np.random.default_rng(5).permutation(i.size)
        c2, k2 = _column_max(N, i[perm], c[perm], best[perm])
        assert np.array_equal(c2, counts) and np.array_equal(k2, keys)


def _same_batch(a, b):
    assert len(a.layers) == len(b.layers) and np.array_equal(a.input_nodes, b.input_nodes)
    for x, y in zip(a.layers, b.layers):
        assert (x is None) == (y is None)
        if x is not None:
            assert all(np.array_equal(u, v) for u, v in zip(x[:3], y[:3])) and x[3] == y[3]
    for xs, ys in ((a.sampled_nodes, b.sampled_nodes), (a.sets, b.sets), (a.normfact, b.normfact)):
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(xs, ys))
    assert a.s_num == b.s_num


@pytest.fixture(scope="module")
def world():
    lap, feats = make_world("graphsage", NN, 12)
    return lap, feats, _labels(NN, 7)


BATCH = np.concatenate([np.arange(40, 560, 7)[::-1], [0, 77, 40, 47]])


def _favoured(seed, n=NN, share=0.2):
    return np.sort(np.random.default_rng(seed).permutation(n)[: int(share * n)])


@pytest.mark.parametrize("orders", [[1, 1], [1, 0, 1]])
def test_reduces_to_the_plain_draw(world, orders):
    lap = world[0]
    plain = ladies_race_host(21, BATCH, 64, lap, orders)
    fav = [_favoured(l) for l in range(len(orders))]
    _same_batch(plain, ladies_race_host(21, BATCH, 64, lap, orders, fav, 1))
    _same_batch(plain, ladies_race_host(21, BATCH, 64, lap, orders, fav, 1.0))
    _same_batch(plain, ladies_race_host(21, BATCH, 64, lap, orders, np.zeros(0, np.int64), 8))
    _same_batch(plain, ladies_race_host(21, BATCH, 64, lap, orders, [np.zeros(0, np.int64)] * len(orders), 8))
    _same_batch(plain, ladies_race_host(21, BATCH, 64, lap, orders, None, 8))
    _same_batch(plain, ladies_race_host(21, BATCH, 64, lap, orders, [None] * len(orders), 8))
    counts, keys = race_keys(21, 1, lap.indptr, lap.indices, BATCH)
    for kw in (dict(favoured=fav[0], scale=1), dict(favoured=np.zeros(0, np.int64), scale=8), dict(favoured=None, scale=8)):
        c2, k2 = race_keys(21, 1, lap.indptr, lap.indices, BATCH, **kw)
        assert np.array_equal(c2, counts) and np.array_equal(k2, keys)
    after = np.flatnonzero(counts)[:50]
    assert np.array_equal(race_normfact(counts, after, 40), race_normfact(counts, after, 40, weights=counts))


def _reference_layer(lap, rows, after, samp, fav, scale):
    """sampler.py:113-139 given the drawn set, with :119-121's pi[F] *= scale: U, pi, p, s_num,
    U[:, after], normfact and create_coo_tensor's CPU branch."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    U = lap[rows, :]
    pi = np.asarray(sp.linalg.norm(U, ord=0, axis=0)).reshape(-1)
    raw = pi.astype(np.int64)
    pi[fav] = pi[fav] * scale
    p = pi / np.sum(pi)
    s_num = np.min([np.sum(p > 0), samp])
    adj = U[:, after]
    normfact = 1 / np.clip(s_num * p[after], 1e-10, 1).astype(np.float32)
    coo = cso.create_coo_tensor(t(U.indptr.astype(np.int32)), t(adj.indptr.astype(np.int32)),
                                t(adj.indices.astype(np.int32)), t(normfact), adj.shape[0], adj.shape[1])
    r, c = coo.indices().numpy()
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=adj.shape[0]))])
    return rowptr, c, coo.values().numpy(), int(s_num), raw, normfact


@pytest.mark.parametrize("orders", [[1], [1, 1], [1, 0, 1]])
def test_host_batch_equals_reference_layer(world, orders):
    lap = world[0]
    L, scale, seed = len(orders), 3, 21
    samp = [100, 50, 75][:L]  # top-down
    fav = [_favoured(10 + l) for l in range(L)]
    hb = ladies_race_host(seed, BATCH, samp, lap, orders, fav, scale)
    rows = BATCH.astype(np.int64)
    assert np.array_equal(hb.sets[L], rows) and np.array_equal(hb.input_nodes, hb.sets[0])
    differs = False
    plain = ladies_race_host(seed, BATCH, samp, lap, orders)
    for l in range(L - 1, -1, -1):
        if orders[l] == 0:
            assert hb.layers[l] is None and hb.sampled_nodes[l].size == 0 and hb.sets[l] is hb.sets[l + 1]
            continue
        after = hb.sets[l]
        rowptr, col, val, s_num, pi, normfact = _reference_layer(lap, rows, after, samp[L - 1 - l], fav[l], scale)
        counts, keys = race_keys(seed, l, lap.indptr, lap.indices, rows, fav[l], scale)
        assert np.array_equal(counts, pi)  # the raw entry counts
        live = np.flatnonzero(pi)
        sel = live[np.argsort(keys[live])[live.size - s_num:]]
        assert np.array_equal(after, np.unique(np.concatenate([sel, rows]))) and s_num == hb.s_num[l]
        g_rowptr, g_col, g_val, shape = hb.layers[l]
        assert shape == (rows.size, after.size) and g_rowptr.dtype == np.int32 and g_col.dtype == np.int32
        assert np.array_equal(g_rowptr, rowptr) and np.array_equal(g_col, col)
        assert g_val.dtype == np.float32 and np.array_equal(g_val, val)
        assert hb.normfact[l].dtype == np.float32 and np.array_equal(hb.normfact[l], normfact)
        assert np.array_equal(after[hb.sampled_nodes[l]], rows)
        differs |= not np.array_equal(after, plain.sets[l])
        rows = after
    assert differs  # the skew moved the draw


def test_skew_favours_the_favoured():
    """Bottom layer only, 64 columns drawn, 20 % of the nodes favoured, 20 fixed seeds pooled: the
    favoured share among the drawn columns (``after`` minus the rows) at scale 8 exceeds scale 1's.
    By the law the favoured share of the weight moves from f to 8 f / (1 + 7 f)."""
    lap, _ = make_world("graphsage", NN, 4)
    fav = _favoured(7)
    rows = np.arange(100, 400, 5)
    share = {}
    for scale in (1, 8):
        n_fav = n_all = 0
        for seed in range(100, 120):
            hb = ladies_race_host(seed, rows, 64, lap, [1], fav, scale)
            drawn = np.setdiff1d(hb.sets[0], rows)
            n_fav += int(np.isin(drawn, fav).sum())
            n_all += drawn.size
        share[scale] = n_fav / n_all
    print(f"favoured share of the drawn columns: scale 1 {share[1]:.3f}, scale 8 {share[8]:.3f}")
    assert share[8] > share[1]


def test_favoured_bits():
    N = 77
    ids = np.array([0, 31, 32, 63, 64, 76, 31])
    bits = favoured_bits(ids, N)
    assert bits.dtype == np.uint32 and bits.shape == (3,)
    assert bits.tolist() == [1 | (1 << 31), 1 | (1 << 31), 1 | (1 << 12)]
    assert favoured_bits(np.zeros(0, np.int64), 64).tolist() == [0, 0] and favoured_bits([], 65).shape == (3,)
    got = np.flatnonzero(np.unpackbits(favoured_bits(_favoured(3), NN).view(np.uint8), bitorder="little"))
    assert np.array_equal(got, _favoured(3))
    for bad in ([N], [-1], np.array([0.5])):
        with pytest.raises(ValueError, match=r"ids in \[0, 77\)"):
            favoured_bits(bad, N)


@pytest.mark.parametrize("name,orders", [("graphsage", [1, 0, 1]), ("gcn", [1, 1])], ids=["sage101", "gcn11"])
def test_cpu_sampler_equals_host_batch_and_trains(name, orders):
    C, nfeat = 7, 12
    lap, feats = make_world(name, NN, nfeat)
    labels = _labels(NN, C)
    L = len(orders)
    fav = [_favoured(20 + l) for l in range(L)]
    fav[0] = None if L == 3 else fav[0]  # no skew at that layer
    ls = LayerwiseSampler(lap, 64, orders, feats, labels, "cpu", scale_factor=2, skewed_sampling_nodes=fav)
    b = ls.sample(BATCH, 21)
    hb = ladies_race_host(21, BATCH, 64, lap, orders, fav, 2)
    assert not np.array_equal(hb.input_nodes, ladies_race_host(21, BATCH, 64, lap, orders).input_nodes)
    x0, adjs, sampled, lab = b
    assert np.array_equal(b.input_nodes.numpy(), hb.input_nodes) and torch.equal(x0, feats[b.input_nodes].float())
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
    # one id array: every aggregating layer; 2.0 is an integer
    one = LayerwiseSampler(lap, 64, orders, feats, labels, "cpu", scale_factor=2.0, skewed_sampling_nodes=fav[-1])
    hb1 = ladies_race_host(21, BATCH, 64, lap, orders, [fav[-1]] * L, 2)
    assert np.array_equal(one.sample(BATCH, 21).input_nodes.numpy(), hb1.input_nodes)

    torch.manual_seed(0)
    model = models.build_model(name, nfeat, 16, orders, C, dropout=0.1)
    tr = Trainer(model, 0.01, "cpu")
    before = [p.detach().clone() for p in tr.params]
    first = next(iter(ls.epoch(np.arange(40, 560), 200, seed=3)))
    assert np.isfinite(float(tr.step(*first)))
    assert any(not torch.equal(p.detach(), q) for p, q in zip(tr.params, before))

    make = lambda **kw: LayerwiseSampler(lap, 64, orders, feats, labels, "cpu", **kw)
    with pytest.raises(ValueError, match="scale_factor 2.5 is not an integer.*fractional weight"):
        make(scale_factor=2.5, skewed_sampling_nodes=fav)
    for bad in (65, 0):
        with pytest.raises(ValueError, match=r"scale_factor must lie in \[1, 64\]"):
            make(scale_factor=bad, skewed_sampling_nodes=fav)
    with pytest.raises(ValueError, match="scale_factor"):
        make(scale_factor=2)  # nothing to favour
    with pytest.raises(ValueError, match=rf"ids in \[0, {NN}\)"):
        make(scale_factor=2, skewed_sampling_nodes=np.array([3, NN]))
    with pytest.raises(ValueError, match=f"{L + 1} favoured sets for {L} layers"):
        make(scale_factor=2, skewed_sampling_nodes=fav + [fav[-1]])
    with pytest.raises(ValueError, match="not an integer"):
        ladies_race_host(1, BATCH, 5, lap, orders, fav, 1.5)


def test_resident_nodes():
    N = 40
    dev = np.full(N, -1)
    idx = np.zeros(N, np.int64)
    own, peer = np.array([3, 9, 31, 32, 39]), np.array([0, 10, 33])
    dev[own], dev[peer] = 5, 2
    idx[own], idx[peer] = np.arange(own.size), np.arange(peer.size)
    place = pack_placement(dev, idx, [2, 5], 1)  # rank 1 is device 5: source 0
    assert np.array_equal(np.flatnonzero(place == PLACE_HOST), np.setdiff1d(np.arange(N), np.union1d(own, peer)))
    assert np.array_equal(np.flatnonzero((place != PLACE_HOST) & ((place >> PLACE_SHIFT) == 0)), own)
    table = torch.randn(N, 4)
    pf = PlacedFeatures(table, place, [table[torch.from_numpy(own)], table[torch.from_numpy(peer)]], "cpu")
    got = pf.resident_nodes()
    assert got.dtype == np.int64 and np.array_equal(got, own) and np.array_equal(pf.resident_nodes("own"), own)
    assert np.array_equal(pf.resident_nodes("device"), np.union1d(own, peer))
    with pytest.raises(ValueError, match="'own' or 'device'"):
        pf.resident_nodes("host")
    # the other rank's view: its own buffer is the first one's peer
    pf0 = PlacedFeatures(table, pack_placement(dev, idx, [2, 5], 0),
                         [table[torch.from_numpy(peer)], table[torch.from_numpy(own)]], "cpu")
    assert np.array_equal(pf0.resident_nodes("own"), peer)
    assert np.array_equal(pf0.resident_nodes("device"), np.union1d(own, peer))
