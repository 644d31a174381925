"""Node-wise neighbour sampling, the parts that need no GPU: the draw's numpy restatement
(``neighbor_keep``: shape, determinism, uniformity), the whole batch in numpy
(``neighbor_sample_host``), the full-fanout case against ``lap`` itself and the closure of
ExactInference, the CPU sampler through ``Trainer.step``, the refusals (Python and C ABI)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib, graphs, models
from gnn_amd.inference import ExactInference
from gnn_amd.neighbor import NeighborSampler, batch_seed, neighbor_keep, neighbor_sample_host
from gnn_amd.train import Trainer
from test_exact_cpu import make_model, make_world, one_hot_labels

CASES = [("graphsage", [1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1])]
IDS = ["sage11", "sage101", "gcn11"]
NN = 600
# out of order, two repeats at the end (40 and 47), two rows of degree 0 (0 and 77; none for GCN)
BATCH = np.concatenate([np.arange(40, 560, 7)[::-1], [0, 77, 40, 47]])


def small_degree_world(name, N, nfeat, seed=0):
    """(lap, feats): a Chung-Lu graph with a light tail (every degree <= 64, GCN's self loop
    included), the rows 0, 1, 2, 77 and the last two emptied."""
    rng = np.random.default_rng(seed)
    A = graphs.chung_lu(N, 4 * N, 0.5, rng)
    keep = np.ones(N, np.float32)
    keep[[0, 1, 2, 77, N - 2, N - 1]] = 0
    A = (sp.diags(keep) @ A).tocsr()
    A.eliminate_zeros()
    lap = graphs.lap_matrix(A.astype(np.float32), name)
    assert 8 <= np.diff(lap.indptr).max() <= 64
    return lap, torch.randn(N, nfeat, generator=torch.Generator().manual_seed(seed + 1))


# ----------------------------------------------------------------------------- the draw


@pytest.mark.parametrize("d,f", [(0, 3), (1, 1), (2, 1), (5, 5), (5, 64), (6, 5), (63, 64), (64, 64), (65, 64),
                                 (130, 64), (1000, 1), (1000, 5), (1000, 64), (2**31 - 2, 64)])
def test_keep_is_k_distinct_ascending_positions(d, f):
    k = min(d, f)
    for seed, layer, node in [(0, 0, 0), (3, 1, 399), (2**63 + 11, 2, 2**31 - 2)]:
        S = neighbor_keep(seed, layer, node, d, f)
        assert S.dtype == np.int64 and S.shape == (k,)
        assert np.all(S[1:] > S[:-1]) and (k == 0 or (S[0] >= 0 and S[-1] < d))
        assert np.array_equal(S, neighbor_keep(seed, layer, node, d, f))  # deterministic
        if d <= f:
            assert np.array_equal(S, np.arange(d))
    # arrays of seeds / nodes: the scalar draw, row for row
    many = neighbor_keep(np.arange(5), 1, 7, d, f)
    assert many.shape == (5, k)
    for s in range(5):
        assert np.array_equal(many[s], neighbor_keep(s, 1, 7, d, f))
    many = neighbor_keep(9, 0, np.arange(4), d, f)
    for n in range(4):
        assert np.array_equal(many[n], neighbor_keep(9, 0, n, d, f))


def test_keep_differs_across_seeds_layers_nodes():
    d, f, T = 1000, 5, 64
    base = neighbor_keep(1, 0, 10, d, f)
    by_seed = neighbor_keep(np.arange(2, 2 + T), 0, 10, d, f)
    by_hi = neighbor_keep((np.arange(1, 1 + T).astype(np.uint64) << np.uint64(32)) + np.uint64(1), 0, 10, d, f)
    by_node = neighbor_keep(1, 0, np.arange(11, 11 + T), d, f)
    by_layer = np.stack([neighbor_keep(1, l, 10, d, f) for l in range(1, 1 + T)])
    for other in (by_seed, by_hi, by_node, by_layer):
        # C(1000, 5) subsets: an equal draw is a defect, not chance
        assert not (other == base[None, :]).all(axis=1).any()
        assert np.unique(other, axis=0).shape[0] == T
    assert len({batch_seed(5, b) for b in range(1000)} | {5}) == 1001
    assert batch_seed(5, 3) != batch_seed(6, 3)


@pytest.mark.parametrize("d,f", [(3, 2), (10, 3), (65, 64), (130, 64)])
def test_keep_is_uniform(d, f):
    """20,000 seeds at a fixed node, and 20,000 nodes at a fixed seed: every entry's inclusion count
    within 5 sigma of T k / d, sigma^2 = T (k/d)(1 - k/d) (a binomial count; 5 sigma over 130 entries
    and 8 runs fails a correct draw once in ~10^4 changes of a constant — the draw is a fixed
    function, so a pass stays a pass)."""
    T, k = 20_000, min(d, f)
    sigma = np.sqrt(T * (k / d) * (1 - k / d))
    for what, S in (("seeds", neighbor_keep(np.arange(T), 0, 5, d, f)),
                    ("nodes", neighbor_keep(7, 1, np.arange(T), d, f))):
        count = np.bincount(S.reshape(-1), minlength=d)
        dev = np.abs(count - T * k / d).max() / sigma
        print(f"neighbor_keep d {d} f {f} over {what}: worst inclusion deviation {dev:.2f} sigma")
        assert dev <= 5.0, (what, dev)


def test_keep_subsets_of_five_are_uniform():
    """The ten 2-subsets of d = 5 over 20,000 seeds: each within 5 sigma of 2,000 (sigma = 42.4)."""
    S = neighbor_keep(np.arange(20_000), 0, 5, 5, 2)
    count = np.bincount(S[:, 0] * 5 + S[:, 1], minlength=25)
    pairs = [a * 5 + b for a in range(5) for b in range(a + 1, 5)]
    assert count.sum() == count[pairs].sum()
    assert np.abs(count[pairs] - 2000).max() <= 5 * np.sqrt(20_000 * 0.1 * 0.9)


# ----------------------------------------------------------------------------- the whole batch


def _dense(layer):
    rowptr, col, val, shape = layer
    return sp.csr_matrix((val, col, rowptr), shape=shape)


@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_sample_host_whole_batch(name, orders):
    lap, _ = make_world(name, NN, 8)
    deg = np.diff(lap.indptr)
    assert deg.max() > 64  # rows above every fanout, rows below
    fan = [5, 3][: sum(orders)]
    hb = neighbor_sample_host(11, BATCH, fan, lap, orders)
    layers, sampled, input_nodes = hb
    L = len(orders)
    assert len(layers) == len(sampled) == L and len(hb.sets) == L + 1
    assert np.array_equal(hb.sets[L], BATCH) and input_nodes is hb.sets[0]
    fl = iter(fan)
    for l in range(L):
        up, low = hb.sets[l + 1], hb.sets[l]
        if orders[l] == 0:
            assert layers[l] is None and sampled[l].size == 0 and low is up
            continue
        f = next(fl)
        rowptr, col, val, shape = layers[l]
        assert shape == (up.size, low.size)
        assert rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32
        assert np.array_equal(np.diff(rowptr), np.minimum(deg[up], f))
        assert low.dtype == np.int64 and np.all(low[1:] > low[:-1])  # ascending, unique
        assert np.isin(up, low).all()  # set[l] contains set[l + 1]
        assert np.array_equal(low[sampled[l]], up)  # rows map to themselves
        assert np.array_equal(np.unique(np.concatenate([up, low[col]])), low)
        k = np.diff(rowptr)
        for i in range(up.size):
            c = col[rowptr[i]:rowptr[i + 1]]
            assert np.all(c[1:] > c[:-1])  # ascending per row, as CsrOperand requires
            row = lap.indices[lap.indptr[up[i]]:lap.indptr[up[i] + 1]]
            assert np.array_equal(low[c], row[neighbor_keep(11, l, up[i], deg[up[i]], f)])
        assert np.all(val == np.repeat((1.0 / np.maximum(k, 1)).astype(np.float32), k))
        sums = np.asarray(_dense(layers[l]).sum(axis=1)).ravel()
        assert np.allclose(sums, (k > 0).astype(np.float32), rtol=0, atol=4e-6)  # k <= 64 terms of float32(1/k)
    top = _dense(layers[L - 1]).toarray()
    assert np.array_equal(top[-2], top[np.flatnonzero(BATCH == 40)[0]])  # duplicate batch nodes: equal rows
    assert np.array_equal(top[-1], top[np.flatnonzero(BATCH == 47)[0]])
    if name == "graphsage":
        assert not top[np.flatnonzero(BATCH == 77)[0]].any()  # a row of degree 0
    # a row's entries do not depend on the batch: the same node drawn alone
    one = neighbor_sample_host(11, [BATCH[3]], fan, lap, orders)
    a, b = layers[L - 1], one.layers[L - 1]
    assert np.array_equal(hb.sets[L - 1][a[1][a[0][3]:a[0][4]]], one.sets[L - 1][b[1]])
    # another seed: another batch
    other = neighbor_sample_host(12, BATCH, fan, lap, orders)
    assert not np.array_equal(other.input_nodes, input_nodes)


@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_full_fanout_is_lap_itself(name, orders):
    """f >= the largest degree: the operands are lap[rows][:, set] with float32(1 / deg), exactly,
    and the sets are the closure's."""
    lap, feats = small_degree_world(name, NN, 8)
    hb = neighbor_sample_host(5, BATCH, 64, lap, orders)
    model = make_model(name, 8, 4, orders, 3).eval()
    c = ExactInference(model, lap, "cpu").closure(BATCH)
    L = len(orders)
    assert np.array_equal(np.unique(hb.sets[L]), c.sets[L])
    for l in range(L):
        assert np.array_equal(hb.sets[l], c.sets[l])
        if orders[l] == 0:
            continue
        up, low = hb.sets[l + 1], hb.sets[l]
        deg = np.diff(lap.indptr)[up]
        w = sp.csr_matrix((np.repeat((1.0 / np.maximum(np.diff(lap.indptr), 1).astype(np.float64)).astype(np.float32),
                                     np.diff(lap.indptr)), lap.indices, lap.indptr), shape=lap.shape)
        want = w[up][:, low]
        want.sort_indices()
        rowptr, col, val, _ = hb.layers[l]
        assert np.array_equal(rowptr, want.indptr) and np.array_equal(col, want.indices)
        assert np.array_equal(val, want.data) and np.array_equal(np.diff(rowptr), deg)


# ----------------------------------------------------------------------------- the CPU sampler


def _labels(N, C):
    cls = np.random.default_rng(2).integers(0, C, N)
    return sp.csr_matrix((np.ones(N, np.int32), (np.arange(N), cls)), shape=(N, C))


@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_cpu_sampler_equals_host_restatement_and_trains(name, orders):
    C, nfeat = 7, 12
    lap, feats = make_world(name, NN, nfeat)
    labels = _labels(NN, C)
    ns = NeighborSampler(lap, 4, orders, feats.to(torch.bfloat16), labels, "cpu")
    b = ns.sample(BATCH, 21)
    hb = neighbor_sample_host(21, BATCH, 4, lap, orders)
    x0, adjs, sampled, lab = b
    assert np.array_equal(b.input_nodes.numpy(), hb.input_nodes)
    assert x0.dtype == torch.float32 and torch.equal(x0, feats.to(torch.bfloat16)[b.input_nodes].float())
    assert torch.equal(lab, torch.from_numpy(np.asarray(labels[BATCH].todense(), dtype=np.float32)))
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
    # dense labels and a dense numpy table of labels give the same rows
    dense = np.asarray(labels.todense(), dtype=np.float32)
    for lf in (dense, torch.from_numpy(dense)):
        assert torch.equal(NeighborSampler(lap, 4, orders, feats, lf, "cpu").sample(BATCH, 21).labels, lab)

    torch.manual_seed(0)
    model = models.build_model(name, nfeat, 16, orders, C, dropout=0.1)
    tr = Trainer(model, 0.01, "cpu")
    before = [p.detach().clone() for p in tr.params]
    train = NeighborSampler(lap, 4, orders, feats, labels, "cpu")
    nodes = np.arange(40, 560)
    losses = []
    for it, batch in enumerate(train.epoch(nodes, 200, seed=3)):
        assert batch.seed == batch_seed(3, it) and np.unique(batch.batch_nodes).size == batch.batch_nodes.size
        losses.append(float(tr.step(*batch)))
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert all(not torch.equal(p.detach(), q) for p, q in zip(tr.params, before)
               if p.grad is not None and bool(p.grad.any()))
    assert sum(1 for p, q in zip(tr.params, before) if not torch.equal(p.detach(), q)) >= len(before) - 2 * orders.count(0)
    # epoch: a permutation of the nodes, the same one for the same seed; sequential: in order
    seen = np.concatenate([b.batch_nodes for b in train.epoch(nodes, 200, seed=3)])
    assert np.array_equal(np.sort(seen), nodes) and not np.array_equal(seen, nodes)
    assert np.array_equal(seen, np.concatenate([b.batch_nodes for b in train.epoch(nodes, 200, seed=3)]))
    assert np.array_equal(np.concatenate([b.batch_nodes for b in train.sequential(nodes, 200)]), nodes)
    res = tr.evaluate(train.sequential(nodes[:300], 128))
    assert res["rows"] == 300 and res["batches"] == 3 and np.isfinite(res["loss"])


# ----------------------------------------------------------------------------- refusals


def test_sampler_refusals():
    lap, feats = make_world("graphsage", NN, 6)
    labels = one_hot_labels(NN, 3)
    ok = lambda **kw: NeighborSampler(**{**dict(lap=lap, fanouts=4, orders=[1, 1], feats=feats, labels_full=labels,
                                                device="cpu"), **kw})
    ok()
    zeros = lap.copy().tocsr()
    zeros.data[3] = 0.0  # an entry that stores a value of its own
    with pytest.raises(ValueError, match="stores values"):
        ok(lap=zeros)
    for f in (0, 65, -1, [4, 65], [0, 4]):
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            ok(fanouts=f)
    for o in ([1, 2], [], [1, -1]):
        with pytest.raises(ValueError, match="orders"):
            ok(orders=o)
    for f, o in (([4], [1, 1]), ([4, 4, 4], [1, 1]), ([4, 4], [1, 0, 0])):
        with pytest.raises(ValueError, match="fanouts for"):
            ok(fanouts=f, orders=o)
    with pytest.raises(ValueError, match="feats"):
        ok(feats=feats.double())
    with pytest.raises(ValueError, match="rows"):
        ok(feats=feats[:-1])
    with pytest.raises(ValueError, match="rows"):
        ok(labels_full=labels[:-1])
    with pytest.raises(ValueError, match=r"ids in \[0, 600\)"):
        ok().sample([3, NN], 0)
    with pytest.raises(ValueError, match=r"ids in \[0, 600\)"):
        ok().sample(np.array([0.5]), 0)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        neighbor_keep(0, 0, 0, 10, 65)
    with pytest.raises(ValueError, match="orders"):
        neighbor_sample_host(0, [1], 4, lap, [3])


def test_c_abi_refusals_without_gpu():
    """Every refusal is decided on the host before a launch: status -22 and a text, no GPU needed."""
    L = _lib.lib()
    P = 4096  # a non-NULL, 16-byte aligned stand-in: refused calls never touch it
    ws = L.gnn_nbr_workspace_bytes(100)
    assert ws >= 2 * 4 * 2 and ws % 256 == 0
    assert L.gnn_nbr_workspace_bytes(8192 * 3 + 1) >= 2 * 4 * 5
    assert L.gnn_nbr_workspace_bytes(-5) == L.gnn_nbr_workspace_bytes(0)

    def rowptr(**kw):
        a = dict(indptr=P, N=1000, E=5000, rows=P, M=100, f=10, rowptr=P, total=P, ws=P, wsb=ws, err=None)
        a.update(kw)
        return L.gnn_nbr_rowptr(a["indptr"], a["N"], a["E"], a["rows"], a["M"], a["f"], a["rowptr"], a["total"],
                                a["ws"], a["wsb"], a["err"], None)

    def draw(**kw):
        a = dict(indptr=P, indices=P, N=1000, E=5000, rows=P, M=100, f=10, rowptr=P, ids=P, val=P, cap=1000)
        a.update(kw)
        return L.gnn_nbr_draw(a["indptr"], a["indices"], a["N"], a["E"], a["rows"], a["M"], a["f"], 1, 0, a["rowptr"],
                              a["ids"], a["val"], a["cap"], None, None)

    def relabel(**kw):
        a = dict(table=P, N=1000, ids=P, n=100, col=P)
        a.update(kw)
        return L.gnn_nbr_relabel(a["table"], a["N"], a["ids"], a["n"], a["col"], None, None, None)

    big = 2**31 - 1
    cases = [(rowptr, dict(M=-1), b"negative"), (rowptr, dict(N=-1), b"negative"), (rowptr, dict(E=-1), b"negative"),
             (rowptr, dict(N=big), b"2^31"), (rowptr, dict(M=big, wsb=2**40), b"2^31"),
             (rowptr, dict(M=2**26, f=32, wsb=2**40), b"M * fanout"), (rowptr, dict(f=0), b"fanout"),
             (rowptr, dict(f=65), b"fanout"), (rowptr, dict(rowptr=None), b"NULL"), (rowptr, dict(total=None), b"NULL"),
             (rowptr, dict(rows=None), b"NULL"), (rowptr, dict(indptr=None), b"NULL"),
             (rowptr, dict(ws=None), b"workspace too small"), (rowptr, dict(wsb=ws - 1), b"workspace too small"),
             (rowptr, dict(ws=P + 8), b"16-byte aligned"),
             (draw, dict(M=-1), b"negative"), (draw, dict(cap=-1), b"negative"), (draw, dict(N=big), b"2^31"),
             (draw, dict(M=big), b"2^31"), (draw, dict(M=2**26, f=32), b"M * fanout"), (draw, dict(f=0), b"fanout"),
             (draw, dict(f=65), b"fanout"), (draw, dict(rows=None), b"NULL"), (draw, dict(rowptr=None), b"NULL"),
             (draw, dict(indptr=None), b"NULL"), (draw, dict(indices=None), b"NULL"), (draw, dict(ids=None), b"NULL"),
             (draw, dict(val=None), b"NULL"),
             (relabel, dict(n=-1), b"negative"), (relabel, dict(N=big), b"2^31"), (relabel, dict(n=big), b"2^31"),
             (relabel, dict(table=None), b"NULL table"), (relabel, dict(table=P + 4), b"8-byte aligned"),
             (relabel, dict(ids=None), b"NULL"), (relabel, dict(col=None), b"NULL")]
    for fn, kw, word in cases:
        assert fn(**kw) == -22, (fn.__name__, kw)
        assert word in L.gnn_last_error(), (fn.__name__, kw, L.gnn_last_error())
    assert draw(M=0) == 0 and relabel(n=0) == 0  # empty: nothing to launch
