"""CPU: the subgraph sampler's batch in numpy (gnn_amd/subgraph.py). Its top layer is the layer-wise
draw's, its square operand scipy's lap[after][:, after] with create_coo_tensor's values, its
operand builder reproduces the reference-pinned host sampler's layers, the skew changes normfact as
``race_normfact(weights=)`` says, the refusals carry their reasons, and ``device="cpu"`` trains."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import models, sampler
from gnn_amd.layerwise import ladies_race_host, race_keys, race_normfact
from gnn_amd.subgraph import SubgraphSampler, subgraph_operand, subgraph_race_host
from gnn_amd.train import Trainer
from test_exact_cpu import make_world
from test_neighbor_gpu import ROWS, _hand_lap

NN = 600
BATCH = np.concatenate([np.arange(40, 560, 7)[::-1], [0, 77, 40, 47]])  # repeats, empty rows, not ascending
ORDERS = [[1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 0]]
OIDS = ["111", "101", "011", "110"]


def _labels(n, C):
    cls = np.random.default_rng(2).integers(0, C, n)
    return sp.csr_matrix((np.ones(n, np.int32), (np.arange(n), cls)), shape=(n, C))


def _graphs():
    yield "hand", sp.csr_matrix(_hand_lap()), ROWS, 40
    for name in ("graphsage", "gcn"):
        yield name, sp.csr_matrix(make_world(name, NN, 4)[0]), BATCH, 64


def _assert_square(lap, after, nf, layer):
    """S against scipy's lap[after][:, after]: the structure, and the values rule."""
    rowptr, col, val, shape = layer
    K = after.size
    S = sp.csr_matrix(lap)[after][:, after].tocsr()
    S.sort_indices()
    assert shape == (K, K) and rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32
    assert np.array_equal(rowptr, S.indptr) and np.array_equal(col, S.indices)
    deg = np.diff(sp.csr_matrix(lap).indptr)[after].astype(np.float64)
    r = np.repeat(np.arange(K), np.diff(rowptr))
    with np.errstate(divide="ignore"):  # an empty row has no entry to weigh
        assert np.array_equal(val, ((1.0 / deg)[r] * nf.astype(np.float64)[col]).astype(np.float32))


@pytest.mark.parametrize("orders", ORDERS + [[1], [0, 1], [1, 1]], ids=OIDS + ["1", "01", "11"])
def test_top_layer_is_the_layerwise_one_and_square_is_scipys(orders):
    L = len(orders)
    t = max(l for l, o in enumerate(orders) if o)
    for gname, lap, rows, samp in _graphs():
        assert gname != "hand" or (lap != lap.T).nnz  # not symmetric
        for seed in (3, (0x9ABCDEF1 << 32) | 0x12345678):
            hb = subgraph_race_host(seed, rows, [samp, 1, 2], lap, orders)  # the reference's list: [0] is used
            lw = ladies_race_host(seed, rows, samp, lap, [0] * t + [1])
            after = lw.sets[t]
            for a, b in zip(hb.layers[t][:3], lw.layers[t][:3]):
                assert a.dtype == b.dtype and np.array_equal(a, b)
            assert hb.layers[t][3] == lw.layers[t][3] == (rows.size, after.size)
            assert np.array_equal(hb.sampled_nodes[t], lw.sampled_nodes[t]) and hb.sampled_nodes[t].dtype == np.int64
            assert np.array_equal(after[hb.sampled_nodes[t]], rows)
            assert hb.s_num[t] == lw.s_num[t] and np.array_equal(hb.normfact[t], lw.normfact[t])
            assert np.array_equal(hb.input_nodes, after) and hb.input_nodes.dtype == np.int64
            assert all(np.array_equal(hb.sets[l], after) for l in range(t + 1))
            assert all(np.array_equal(hb.sets[l], rows) for l in range(t + 1, L + 1))
            lower = [l for l in range(t) if orders[l]]
            for l in range(L):
                if not orders[l]:
                    assert hb.layers[l] is None and hb.sampled_nodes[l].size == 0 and hb.normfact[l] is None
            for l in lower:
                assert hb.layers[l] is hb.layers[lower[0]]  # built once
                assert np.array_equal(hb.sampled_nodes[l], np.arange(after.size))
                assert hb.normfact[l] is hb.normfact[t] and hb.s_num[l] == hb.s_num[t]
            if lower:
                _assert_square(lap, after, hb.normfact[t], hb.layers[lower[0]])
    # one int is the list's element [0]
    a, b = subgraph_race_host(5, BATCH, 64, lap, orders), subgraph_race_host(5, BATCH, np.array([64, 9, 9]), lap, orders)
    assert np.array_equal(a.input_nodes, b.input_nodes) and np.array_equal(a.layers[t][2], b.layers[t][2])


def _tiny(golden):
    g = golden("graph_tiny.npz")
    N = int(g["N"])
    lap = sp.csr_matrix((g["lap_data"], g["lap_indices"], g["lap_indptr"]), shape=(N, N))
    labels = sp.csr_matrix((np.ones(N, np.int32), (np.arange(N), g["labels_cls"])), shape=(N, int(g["num_classes"])))
    return lap, labels, N


@pytest.mark.parametrize("orders", ORDERS, ids=OIDS)
def test_operand_builder_reproduces_the_reference_pinned_layers(golden, orders):
    """sampler.subgraph_sample_host(native=False) is pinned to the reference's recorded outputs
    (tests/test_sampler_placement.py); its after, rows and normfact through the new operand builder
    give its layers: rowptr, normfact, shape and sampled_nodes exactly, the columns per row as sets
    (below its first layer the reference slices an unsorted lap). The square layers' sampled_nodes
    match exactly. The drawn layer's are the positions of the rows in after IN ROW ORDER here, as the
    layer-wise device draw hands them (x[sampled_nodes] lines up with the labels); the reference's
    np.where(np.isin(after, batch)) lists the same positions ascending, so for the goldens' unsorted
    batches the two agree as sets, and exactly on a sorted batch. The reference hands an order-0 layer
    below the drawn one the square operand too; the device batch hands None there."""
    lap, labels, N = _tiny(golden)
    z = golden("subgraph_tiny.npz")
    pl = golden("placement_tiny.npz")
    t = max(l for l, o in enumerate(orders) if o)
    for c in range(4):
        samp, bs, seed, ndev = (int(v) for v in z[f"c{c}_cfg"])
        batch = np.asarray(z[f"c{c}_batch"])
        hb = sampler.subgraph_sample_host(seed, batch, np.array([samp] * 5), N, lap, labels, orders, pl[f"n{ndev}_dev0"],
                                          pl[f"n{ndev}_idx"], None, 1.0, list(range(ndev)), native=False)
        after = np.asarray(hb.input_nodes)
        assert np.array_equal(after, np.unique(after)) and np.isin(batch, after).all()
        checked = 0
        for l in range(t + 1):
            HL = hb.layers[l]
            assert HL is not None
            rows = batch if l == t else after
            rowptr, col, val, shape = subgraph_operand(lap, rows, after, HL.normfact)
            assert shape == tuple(HL.shape) and np.array_equal(rowptr, HL.rowptr) and rowptr.dtype == HL.rowptr.dtype
            for r in range(shape[0]):
                s, e = rowptr[r], rowptr[r + 1]
                assert np.array_equal(col[s:e], np.sort(HL.colidx[s:e]))
            deg = np.diff(HL.fullrowptr).astype(np.float64)
            rr = np.repeat(np.arange(shape[0]), np.diff(rowptr))
            assert np.array_equal(val, ((1.0 / deg[rr]) * HL.normfact[col].astype(np.float64)).astype(np.float32))
            want = np.asarray(hb.sampled_nodes[l], np.int64)
            if l < t:
                assert np.array_equal(np.arange(after.size), want)
                checked += 1
            else:
                assert np.array_equal(np.unique(np.searchsorted(after, batch)), want)
                assert np.array_equal(np.searchsorted(after, np.sort(batch)), want)  # a sorted batch: exactly
        assert checked == t
        for l in range(t + 1, len(orders)):
            assert hb.layers[l] is None


def _favoured(k):
    return np.random.default_rng(k).permutation(NN)[: NN // 5]


def test_skew():
    """Scale 1, no set or an empty set: the plain batch bit for bit. Scale 4: normfact is
    race_normfact's with the weights count * s, over the skewed draw's own after."""
    lap = sp.csr_matrix(make_world("graphsage", NN, 4)[0])
    orders, seed, samp = [1, 0, 1], 21, 64
    fav = _favoured(4)
    plain = subgraph_race_host(seed, BATCH, samp, lap, orders)
    for kw in (dict(skewed_sampling_nodes=fav, scale_factor=1), dict(skewed_sampling_nodes=np.zeros(0, np.int64), scale_factor=4),
               dict(skewed_sampling_nodes=None, scale_factor=1.0)):
        same = subgraph_race_host(seed, BATCH, samp, lap, orders, **kw)
        assert np.array_equal(same.input_nodes, plain.input_nodes)
        for l in (0, 2):
            for a, b in zip(same.layers[l][:3], plain.layers[l][:3]):
                assert np.array_equal(a, b)
            assert np.array_equal(same.normfact[l], plain.normfact[l])
    hb = subgraph_race_host(seed, BATCH, samp, lap, orders, fav, 4)
    after = hb.input_nodes
    counts, keys = race_keys(seed, 2, lap.indptr, lap.indices, BATCH, fav, 4)
    s = np.ones(NN, np.int64)
    s[fav] = 4
    live = np.flatnonzero(counts)
    sel = live[np.argsort(keys[live])[live.size - hb.s_num[2]:]]
    assert np.array_equal(after, np.unique(np.concatenate([sel, BATCH])))
    nf = race_normfact(counts, after, hb.s_num[2], weights=counts * s)
    assert np.array_equal(hb.normfact[2], nf) and hb.normfact[0] is hb.normfact[2]
    assert not np.array_equal(nf, race_normfact(counts, after, hb.s_num[2]))
    assert not np.array_equal(after, plain.input_nodes)  # the skew moved the draw
    _assert_square(lap, after, nf, hb.layers[0])
    # a list of ids is one id array
    again = subgraph_race_host(seed, BATCH, samp, lap, orders, fav.tolist(), 4)
    assert np.array_equal(again.input_nodes, after)


def test_refusals():
    lap, feats = make_world("graphsage", NN, 4)
    labels = _labels(NN, 7)
    fav = _favoured(1)
    make = lambda orders=(1, 1), **kw: SubgraphSampler(lap, 64, list(orders), feats, labels, "cpu", **kw)
    host = lambda orders=(1, 1), **kw: subgraph_race_host(1, BATCH, 64, lap, list(orders), **kw)
    for fn in (make, host):
        with pytest.raises(ValueError, match="scale_factor 2.5 is not an integer.*fractional weight"):
            fn(scale_factor=2.5, skewed_sampling_nodes=fav)
        for bad in (65, 0):
            with pytest.raises(ValueError, match=r"scale_factor must lie in \[1, 64\]"):
                fn(scale_factor=bad, skewed_sampling_nodes=fav)
        with pytest.raises(ValueError, match="per-layer list of favoured sets.*draws once"):
            fn(scale_factor=2, skewed_sampling_nodes=[fav, fav])
        with pytest.raises(ValueError, match="per-layer list of favoured sets"):
            fn(scale_factor=2, skewed_sampling_nodes=[None, fav])
        with pytest.raises(ValueError, match=rf"ids in \[0, {NN}\)"):
            fn(scale_factor=2, skewed_sampling_nodes=np.array([3, NN]))
        with pytest.raises(ValueError, match="no aggregating layer"):
            fn(orders=(0, 0))
        with pytest.raises(ValueError, match="non-empty list of 0 / 1"):
            fn(orders=(1, 2))
    with pytest.raises(ValueError, match="scale_factor 2 without skewed_sampling_nodes.*nothing to favour"):
        make(scale_factor=2)
    with pytest.raises(ValueError, match=r"sample sizes must lie in \[1, 2\^31\)"):
        SubgraphSampler(lap, [0, 5], [1, 1], feats, labels, "cpu")
    weighted = sp.csr_matrix(lap).copy()
    weighted.data[3] = 0.0  # an explicit zero: a graph with values of its own
    for fn in (lambda: SubgraphSampler(weighted, 64, [1, 1], feats, labels, "cpu"),
               lambda: subgraph_race_host(1, BATCH, 64, weighted, [1, 1])):
        with pytest.raises(ValueError, match="weighted graphs are out of scope"):
            fn()


@pytest.mark.parametrize("name,orders", [("graphsage", [1, 1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1])],
                         ids=["sage111", "sage101", "gcn11"])
def test_cpu_sampler_equals_host_batch_and_trains(name, orders):
    C, nfeat = 7, 12
    lap, feats = make_world(name, NN, nfeat)
    labels = _labels(NN, C)
    fav = _favoured(20)
    ss = SubgraphSampler(lap, 64, orders, feats, labels, "cpu", scale_factor=2.0, skewed_sampling_nodes=fav)
    b = ss.sample(BATCH, 21)
    hb = subgraph_race_host(21, BATCH, 64, lap, orders, fav, 2)
    x0, adjs, sampled, lab = b
    assert np.array_equal(b.input_nodes.numpy(), hb.input_nodes) and torch.equal(x0, feats[b.input_nodes].float())
    assert torch.equal(lab, torch.from_numpy(np.asarray(labels[BATCH].todense(), dtype=np.float32)))
    lower = [l for l in range(len(orders) - 1) if orders[l]]
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
    assert all(adjs[l] is adjs[lower[0]] for l in lower)  # one operand object
    plain = SubgraphSampler(lap, [64, 3], orders, feats, labels, "cpu")
    assert np.array_equal(plain.sample(BATCH, 21).input_nodes.numpy(), subgraph_race_host(21, BATCH, 64, lap, orders).input_nodes)

    torch.manual_seed(0)
    model = models.build_model(name, nfeat, 16, orders, C, dropout=0.1)
    tr = Trainer(model, 0.01, "cpu")
    before = [p.detach().clone() for p in tr.params]
    first = next(iter(ss.epoch(np.arange(40, 560), 200, seed=3)))
    assert np.isfinite(float(tr.step(*first)))
    assert any(not torch.equal(p.detach(), q) for p, q in zip(tr.params, before))
    assert len(list(ss.sequential(np.arange(100), 40))) == 3
