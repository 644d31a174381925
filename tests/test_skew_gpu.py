"""The locality-skewed layer-wise draw on the GPU: gnn_lw_race_skew / gnn_lw_finish_skew against the
numpy restatement bit for bit on a hand-made graph (a hub row, a repeated row, an empty row, favoured
sets on the bit table's word boundaries), their reduction to the plain entry points, their refusals,
then LayerwiseSampler with a skew against ladies_race_host array for array, through the native
step, and over a placed feature store, where the skew moves the buffer's hit count to exactly what
the oracle predicts."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib, models, placement, staging
from gnn_amd import custom_sparse_ops as cso
from gnn_amd import executor as E
from gnn_amd.layerwise import LayerwiseSampler, favoured_bits, ladies_race_host, race_keys, race_normfact
from gnn_amd.placed import PlacedFeatures
from gnn_amd.sampler import NativeGraph, device_graph
from gnn_amd.train import Trainer
from test_exact_cpu import make_world
from test_layerwise_gpu import BATCH, NN, SEEDS, TAIL, _assert_batch, _labels, _no_graph, _select, _sent, _t, _u64

pytestmark = pytest.mark.gpu

N = 301  # 9 words of the favoured table and 13 bits of a tenth
HUB, EMPTY = 5, 6
ROWS = np.array([HUB, 17, 40, EMPTY, 17, 299, 0, 123, 64, 31, 200, 250, N - 1, 77, 78, 79])
SCALES = [2, 3, 64]
FAVOURED = {"none": np.zeros(0, np.int64), "all": np.arange(N), "every_other": np.arange(0, N, 2),
            "word_edges": np.array([0, 31, 32, 63, 64, N - 1])}


def _hand_lap():
    """Row HUB has 220 columns or more (the favoured table's word edges among them), row EMPTY none,
    the others 1 .. 12."""
    rng = np.random.default_rng(9)
    deg = 1 + np.arange(N) % 12
    deg[HUB], deg[EMPTY] = 220, 0
    cols = [np.sort(rng.choice(N, d, replace=False)) for d in deg]
    cols[HUB] = np.union1d(cols[HUB], FAVOURED["word_edges"])
    deg[HUB] = cols[HUB].size
    indptr = np.concatenate([[0], np.cumsum(deg)])
    return sp.csr_matrix((np.ones(indptr[-1], np.float32), np.concatenate(cols).astype(np.int32), indptr), shape=(N, N))


@pytest.fixture(scope="module")
def graph(dev):
    g = NativeGraph(_hand_lap())
    deg = np.diff(g.indptr)
    assert g.data is None and N % 32 and deg[HUB] >= 200 and deg[EMPTY] == 0 and np.unique(ROWS).size < ROWS.size
    return g, device_graph(g, dev)


def _table(ids, dev, n=N):
    return torch.from_numpy(favoured_bits(ids, n).view(np.int32)).to(dev)


def _race_skew(dg, rows, live, cap, seed, layer, dev, fav_p, scale, M=None):
    """gnn_lw_race_skew into sentinel-filled outputs: (count, key, total, err)."""
    L = _lib.lib()
    count, key, total = _sent(cap, torch.int32, dev), _sent(cap, torch.int64, dev), _sent(1, torch.int64, dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    _lib.check(L.gnn_lw_race_skew(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, int(dg.indices.numel()),
                                  rows.data_ptr(), rows.numel() if M is None else M, live.data_ptr(), seed, layer,
                                  count.data_ptr(), key.data_ptr(), cap, total.data_ptr(), err.data_ptr(),
                                  _lib.stream_of(dev), fav_p, scale), "gnn_lw_race_skew")
    return count, key, total, err


def _finish_skew(dg, rows, after, K_t, kcap, live, count, cap, total, s_num, dev, fav_p, scale):
    """gnn_lw_finish_skew into sentinel-filled outputs: (normfact, colptr_t, rowseg, colseg, totals, err)."""
    L = _lib.lib()
    M = rows.numel()
    normfact = torch.full((kcap + TAIL,), -7.0, dtype=torch.float32, device=dev)
    colptr, colseg, rowseg = _sent(kcap + 1, torch.int32, dev), _sent(kcap + 1, torch.int32, dev), _sent(M + 1, torch.int32, dev)
    totals = _sent(3, torch.int64, dev)
    err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
    wsb = L.gnn_lw_finish_workspace_bytes(M, kcap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.gnn_lw_finish_skew(dg.indptr.data_ptr(), int(dg.indices.numel()), dg.indptr_t.data_ptr(),
                                    int(dg.indices_t.numel()), N, rows.data_ptr(), M, after.data_ptr(), K_t.data_ptr(),
                                    kcap, live.data_ptr(), count.data_ptr(), cap, total.data_ptr(), s_num.data_ptr(),
                                    normfact.data_ptr(), colptr.data_ptr(), rowseg.data_ptr(), colseg.data_ptr(),
                                    totals.data_ptr(), ws.data_ptr(), wsb, err.data_ptr(), _lib.stream_of(dev), fav_p,
                                    scale), "gnn_lw_finish_skew")
    return normfact, colptr, rowseg, colseg, totals, err


def _skewed_layer(g, dg, fav_h, scale, samp, seed, layer, dev):
    """One layer's device sequence with a skew against its numpy restatement, every output and every tail."""
    rows_h = ROWS
    rows = _t(rows_h.astype(np.int32), dev)
    M = rows_h.size
    deg = np.diff(g.indptr)
    cap = int(min(N, M + deg[rows_h].sum()))
    counts, keys = race_keys(seed, layer, g.indptr, g.indices, rows_h, fav_h, scale)
    s_of = np.ones(N, np.int64)
    s_of[fav_h] = scale
    w = counts * s_of
    live_h = np.union1d(rows_h, np.flatnonzero(counts))
    nlive = live_h.size
    fav = _table(fav_h, dev)

    live, nlive_t = cso.closure_mark(dg, rows, True)
    assert int(nlive_t) == nlive <= cap
    live_ids = cso.closure_list(live, N, nlive)
    live_ids = torch.cat([live_ids, torch.full((cap - nlive,), -7, dtype=torch.int32, device=dev)])
    count, key, total, err = _race_skew(dg, rows, live, cap, seed, layer, dev, fav.data_ptr(), scale)
    assert np.array_equal(count[:nlive].cpu().numpy(), counts[live_h]) and not count[nlive:cap].any()  # raw counts
    assert np.array_equal(_u64(key[:nlive]), keys[live_h]) and not key[nlive:cap].any()
    assert int(total[0]) == w.sum() and not err.any()
    assert bool((count[cap:] == -7).all()) and bool((key[cap:] == -7).all()) and bool((total[1:] == -7).all())

    ids, s_num, tau = _select(key, count, nlive_t.reshape(1), cap, samp, live_ids, dev)
    hb = ladies_race_host(seed, rows_h, samp, g, [0] * layer + [1], [None] * layer + [fav_h], scale)
    after_h = hb.sets[layer]
    assert int(s_num[0]) == hb.s_num[layer]
    seeds = torch.cat([rows, ids[:cap]]).contiguous()
    table, K_t = cso.closure_mark(_no_graph(N, seeds), seeds, False)
    K = int(K_t)
    kcap = min(N, M + min(cap, samp))
    assert K == after_h.size <= kcap
    after = _sent(kcap, torch.int32, dev)
    _lib.check(_lib.lib().gnn_closure_list(table.data_ptr(), N, after.data_ptr(), kcap, _lib.stream_of(dev)), "list")
    assert np.array_equal(after[:K].cpu().numpy(), after_h)
    normfact, colptr, rowseg, colseg, totals, err = _finish_skew(dg, rows, after, K_t.reshape(1), kcap, live, count, cap,
                                                                total, s_num, dev, fav.data_ptr(), scale)
    assert not err.any()
    want_nf = race_normfact(counts, after_h, hb.s_num[layer], weights=w)
    assert np.array_equal(normfact[:K].cpu().numpy(), want_nf) and np.array_equal(want_nf, hb.normfact[layer])
    assert bool((normfact[K:] == -7.0).all())
    scan = lambda v: np.concatenate([[0], np.cumsum(v)])
    deg_t = deg if dg.symmetric else np.diff(g.transpose_structure[1])
    assert np.array_equal(colptr[: K + 1].cpu().numpy(), scan(counts[after_h]))  # the raw counts' scan
    assert np.array_equal(rowseg[: M + 1].cpu().numpy(), scan(deg[rows_h]))
    assert np.array_equal(colseg[: K + 1].cpu().numpy(), scan(deg_t[after_h]))
    assert totals[:3].tolist() == [counts[after_h].sum(), deg_t[after_h].sum(), deg[after_h].sum()]
    assert int(totals[0]) == hb.layers[layer][0][-1]  # the operand's nnz
    for t_, n_ in ((colptr, K + 1), (colseg, K + 1), (rowseg, M + 1), (totals, 3)):
        assert bool((t_[n_:] == -7).all())
    return after_h


@pytest.mark.parametrize("layer", [0, 2])
@pytest.mark.parametrize("seed", SEEDS, ids=["seed_lo", "seed_hi"])
def test_kernels_are_bit_exact(graph, dev, seed, layer):
    g, dg = graph
    plain = ladies_race_host(seed, ROWS, 40, g, [0] * layer + [1]).sets[layer]
    moved = 0
    for name, fav_h in FAVOURED.items():
        for scale in SCALES:
            after = _skewed_layer(g, dg, fav_h, scale, 40, seed, layer, dev)
            if name == "none":
                assert np.array_equal(after, plain)
            moved += not np.array_equal(after, plain)
    assert moved  # the skew changes the draw somewhere
    _skewed_layer(g, dg, FAVOURED["word_edges"], 64, 1000, seed, layer, dev)  # every live column drawn
    _skewed_layer(g, dg, FAVOURED["every_other"], 3, 1, seed, layer, dev)    # and one


def test_null_skew_is_the_plain_race(graph, dev):
    g, dg = graph
    L = _lib.lib()
    rows = _t(ROWS.astype(np.int32), dev)
    cap = N
    live, _ = cso.closure_mark(dg, rows, True)
    fav = _table(FAVOURED["every_other"], dev)
    for seed in SEEDS:
        count, key, total = _sent(cap, torch.int32, dev), _sent(cap, torch.int64, dev), _sent(1, torch.int64, dev)
        err = torch.zeros(1 + TAIL, dtype=torch.int32, device=dev)
        _lib.check(L.gnn_lw_race(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, int(dg.indices.numel()), rows.data_ptr(),
                                 rows.numel(), live.data_ptr(), seed, 1, count.data_ptr(), key.data_ptr(), cap,
                                 total.data_ptr(), err.data_ptr(), _lib.stream_of(dev)), "gnn_lw_race")
        counts, keys = race_keys(seed, 1, g.indptr, g.indices, ROWS)
        assert int(total[0]) == counts.sum() and int(count[:cap].sum()) == counts.sum()
        for fav_p, scale in ((None, 7), (fav.data_ptr(), 1), (None, 1)):
            got = _race_skew(dg, rows, live, cap, seed, 1, dev, fav_p, scale)
            for a, b in zip(got, (count, key, total, err)):
                assert torch.equal(a, b)


def test_refusals_launch_nothing(graph, dev):
    g, dg = graph
    L = _lib.lib()
    rows = _t(ROWS.astype(np.int32), dev)
    M, cap, kcap = ROWS.size, N, N
    Eg = int(dg.indices.numel())
    live, nlive_t = cso.closure_mark(dg, rows, True)
    live_ids = cso.closure_list(live, N, N)
    fav = _table(FAVOURED["all"], dev)
    count, key = _sent(cap, torch.int32, dev), _sent(cap, torch.int64, dev)
    word = _sent(8, torch.int64, dev)
    normfact = torch.full((kcap,), -7.0, dtype=torch.float32, device=dev)
    colptr, colseg, rowseg = _sent(kcap + 1, torch.int32, dev), _sent(kcap + 1, torch.int32, dev), _sent(M + 1, torch.int32, dev)
    wsb = L.gnn_lw_finish_workspace_bytes(M, kcap)
    ws = torch.full((wsb + 64,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = _lib.stream_of(dev)
    w = lambda i: word[i:].data_ptr()

    def c_race(M=M, fav_p=fav.data_ptr(), scale=2):
        return L.gnn_lw_race_skew(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, Eg, rows.data_ptr(), M, live.data_ptr(), 3,
                                  0, count.data_ptr(), key.data_ptr(), cap, w(1), None, st, fav_p, scale)

    def c_finish(M=M, fav_p=fav.data_ptr(), scale=2):
        return L.gnn_lw_finish_skew(dg.indptr.data_ptr(), Eg, dg.indptr_t.data_ptr(), Eg, N, rows.data_ptr(), M,
                                    live_ids.data_ptr(), w(4), kcap, live.data_ptr(), count.data_ptr(), cap, w(1), w(2),
                                    normfact.data_ptr(), colptr.data_ptr(), rowseg.data_ptr(), colseg.data_ptr(), w(5),
                                    ws.data_ptr(), wsb, None, st, fav_p, scale)

    for fn in (c_race, c_finish):
        for kw, msg in ((dict(scale=0), b"outside [1, 64]"), (dict(scale=65), b"outside [1, 64]"),
                        (dict(scale=-3), b"outside [1, 64]"), (dict(scale=65, fav_p=None), b"outside [1, 64]"),
                        (dict(fav_p=fav.data_ptr() + 1), b"4-byte aligned"), (dict(fav_p=fav.data_ptr() + 2), b"4-byte aligned"),
                        (dict(M=2**26), b"M < 2^26"), (dict(M=2**26, scale=64), b"M < 2^26")):
            assert fn(**kw) == -22, (fn.__name__, kw)
            assert msg in L.gnn_last_error(), (fn.__name__, kw, L.gnn_last_error())
    torch.cuda.synchronize()
    for t_ in (count, key, word, colptr, colseg, rowseg):  # nothing ran
        assert bool((t_ == -7).all())
    assert bool((normfact == -7.0).all()) and bool((ws == 0x5A).all())
    assert c_race() == 0  # the same arguments, accepted
    torch.cuda.synchronize()
    counts, _ = race_keys(3, 0, g.indptr, g.indices, ROWS)
    assert int(word[1]) == 2 * counts.sum() and int(count[:cap].sum()) == counts.sum()


# ----------------------------------------------------------------------------- the sampler

CASES = [("graphsage", [1, 1]), ("graphsage", [1, 0, 1]), ("gcn", [1, 1])]
IDS = ["sage11", "sage101", "gcn11"]


@pytest.fixture(scope="module")
def worlds():
    """(lap, feats, labels) per model name, made once and left unchanged."""
    out = {}
    for name in ("graphsage", "gcn"):
        lap, feats = make_world(name, NN, 48)
        out[name] = (lap, feats, _labels(NN, 7))
    return out


def _favoured(seed, share=0.2):
    return np.sort(np.random.default_rng(seed).permutation(NN)[: int(share * NN)])


@pytest.mark.parametrize("name,orders", CASES, ids=IDS)
def test_sampler_equals_host_batch_and_steps(dev, worlds, name, orders):
    lap, feats, labels = worlds[name]
    samp = [90, 70, 50][: len(orders)]
    fav = [_favoured(30 + l) for l in range(len(orders))]
    ls = LayerwiseSampler(lap, samp, orders, feats, labels, dev, scale_factor=4, skewed_sampling_nodes=fav)
    hb = ladies_race_host(21, BATCH, samp, lap, orders, fav, 4)
    assert not np.array_equal(hb.input_nodes, ladies_race_host(21, BATCH, samp, lap, orders).input_nodes)
    _assert_batch(ls.sample(BATCH, 21), hb, feats, labels, BATCH, orders, False)
    uniq = BATCH[:-2]
    one = LayerwiseSampler(lap, 64, orders, feats.half(), labels, dev, scale_factor=4.0, skewed_sampling_nodes=fav[0])
    _assert_batch(one.sample(uniq, SEEDS[1]), ladies_race_host(SEEDS[1], uniq, 64, lap, orders, fav[0], 4), feats.half(),
                  labels, uniq, orders, True)

    # the native step takes the batch: the Python autograd path's loss, test_layerwise_gpu.py's bound
    args = tuple(ls.sample(np.arange(40, 560, 2), 9))

    def trainer(native):
        torch.manual_seed(0)
        m = models.build_model(name, feats.shape[1], 128, list(orders), 7, 0.1, fused=True).to(dev)
        tr = Trainer(m, 0.01, dev)
        assert tr.executor is not None
        if not native:
            tr.executor = None
        return tr

    ta, tb = trainer(False), trainer(True)
    assert isinstance(tb.executor, E.NativeStep) and tb.executor.supports(*args)
    torch.manual_seed(100)
    la = float(ta.step(*args))
    torch.manual_seed(100)
    lb = float(tb.step(*args))
    print(f"skewed layerwise {name} {orders}: loss {la:.8f} / {lb:.8f}")
    assert np.isfinite(lb) and abs(la - lb) <= 1e-6 * abs(la) + 1e-7


def test_skew_over_a_placed_store(dev, worlds):
    """Buffer fraction 0.2, the bottom layer favouring the rank's own buffer: X0 bit-equal to the
    table's rows, a clean check(), and the buffer's hit count over 10 fixed seeds at scale 8 and at
    scale 1 exactly the oracle's — the former the larger."""
    lap, feats, labels = worlds["graphsage"]
    orders = [1, 1]
    train = np.arange(40, 560)
    pl = placement.create_buffer(lap, train, int(0.2 * NN), [0], 2, alpha=0)
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
    pf = PlacedFeatures.from_store(store, pl, 0)
    try:
        own = pf.resident_nodes("own")
        assert np.array_equal(own, np.sort(pl.gpu_buffer_group[0])) and own.size == int(0.2 * NN)
        hits = {}
        for scale in (8, 1):
            ls = LayerwiseSampler(lap, 64, orders, pf, labels, dev, scale_factor=scale, skewed_sampling_nodes=[own, None])
            pf.reset_counts()
            want_own = want_all = 0
            for seed in range(50, 60):
                b = ls.sample(BATCH, seed)
                hb = ladies_race_host(seed, BATCH, 64, lap, orders, [own, None], scale)
                assert np.array_equal(b.input_nodes.cpu().numpy(), hb.input_nodes)
                assert torch.equal(b.x0.cpu(), feats.float()[torch.from_numpy(hb.input_nodes)])
                want_own += int(np.isin(hb.input_nodes, own).sum())
                want_all += hb.input_nodes.size
            pf.check()
            c = pf.counts()
            print(f"placed store, scale {scale}: own {c['own']} host {c['host']} of {c['total']} rows (oracle {want_own})")
            assert c["own"] == want_own and c["total"] == want_all and c["host"] == want_all - want_own
            hits[scale] = c["own"]
        assert hits[8] > hits[1]
    finally:
        pf.close()
