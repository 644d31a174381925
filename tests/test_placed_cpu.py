"""CPU: the placement map (pack_placement), the numpy restatement of the placed gather, the
device="cpu" samplers over a PlacedFeatures, epoch's rank splitting, and gnn_gather_placed_f32's
refusals through the library without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gnn_amd import _lib, placement, staging
from gnn_amd.layerwise import LayerwiseSampler
from gnn_amd.neighbor import NeighborSampler, batch_seed
from gnn_amd.placed import (MAX_SOURCES, PLACE_HOST, PLACE_SHIFT, PlacedFeatures, pack_placement,
                            placed_gather_host)
from gnn_amd.sampler import rank_batches
from test_exact_cpu import make_world

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN, NFEAT, C = 600, 12, 7
TRAIN = np.arange(40, 560)
PLACEMENTS = [(1, 150), (2, 90), (4, 60)]  # (ndev, rows buffered per device)


def _labels(N, n_cls):
    cls = np.random.default_rng(2).integers(0, n_cls, N)
    return sp.csr_matrix((np.ones(N, np.int32), (np.arange(N), cls)), shape=(N, n_cls))


@pytest.fixture(scope="module")
def world():
    lap, feats = make_world("graphsage", NN, NFEAT)
    return lap, feats, _labels(NN, C)


def _placement(lap, ndev, k, devices=None):
    devices = list(range(ndev)) if devices is None else devices
    return placement.create_buffer(lap, TRAIN, k, devices, 2, alpha=0)


def _loop_pack(dev_ids, idx, devices, rank):
    """pack_placement by a direct loop."""
    others = [d for j, d in enumerate(devices) if j != rank]
    out = np.empty(len(dev_ids), np.int32)
    for v in range(len(dev_ids)):
        d = int(dev_ids[v])
        if d == -1:
            out[v] = PLACE_HOST
        else:
            src = 0 if d == devices[rank] else 1 + others.index(d)
            out[v] = (src << PLACE_SHIFT) | int(idx[v])
    return out


@pytest.mark.parametrize("ndev,k", PLACEMENTS)
def test_pack_placement_equals_a_direct_loop(world, ndev, k):
    lap = world[0]
    devices = [3, 5, 0, 9][:ndev]  # device ids need not be 0 .. ndev-1
    pl = _placement(lap, ndev, k, devices)
    for rank in range(ndev):
        got = pack_placement(pl.device_id_of_nodes_group[rank], pl.idx_of_nodes_on_device_group[rank], devices, rank)
        assert got.dtype == np.int32 and got.shape == (NN,)
        assert np.array_equal(got, _loop_pack(pl.device_id_of_nodes_group[rank],
                                              pl.idx_of_nodes_on_device_group[rank], devices, rank))
        own = pl.gpu_buffer_group[rank]
        assert np.array_equal(got[own], np.arange(len(own), dtype=np.int32))  # source 0, slot = position
        assert (got == PLACE_HOST).sum() == (pl.device_id_of_nodes_group[rank] == -1).sum() > 0


def test_pack_placement_refusals():
    dev = np.array([0, -1, 1, 0])
    idx = np.array([0, 1, 0, 1])
    with pytest.raises(ValueError, match="slot"):
        pack_placement(dev, np.array([0, 1, 0, 1 << PLACE_SHIFT]), [0, 1], 0)
    pack_placement(dev, np.array([0, 1 << 40, 0, (1 << PLACE_SHIFT) - 1]), [0, 1], 0)  # a host node's slot is not read
    with pytest.raises(ValueError, match="at most 16"):
        pack_placement(dev, idx, list(range(MAX_SOURCES + 1)), 0)
    with pytest.raises(ValueError, match="device id 1 is not among"):
        pack_placement(dev, idx, [0, 2], 0)
    got = pack_placement(dev, idx, list(range(MAX_SOURCES)), 15)  # 16 devices: sources 0 .. 15
    assert got.tolist() == [(1 << PLACE_SHIFT) | 0, PLACE_HOST, (2 << PLACE_SHIFT) | 0, (1 << PLACE_SHIFT) | 1]


def _sources(feats, pl, rank, ndev):
    """The rank's source list (own buffer first, the peers in device order) as CPU tensors."""
    order = [rank] + [j for j in range(ndev) if j != rank]
    return [feats[torch.from_numpy(np.asarray(pl.gpu_buffer_group[j], np.int64))] for j in order]


NODES = np.concatenate([np.random.default_rng(4).integers(0, NN, 400), [0, NN - 1, 5, 5, NN - 1]])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("ndev,k", PLACEMENTS)
def test_host_restatement_is_the_table(world, ndev, k, dtype):
    lap, feats, _ = world
    feats = feats.to(dtype)
    pl = _placement(lap, ndev, k)
    want = feats.float()[torch.from_numpy(NODES)]
    for rank in range(ndev):
        place = pack_placement(pl.device_id_of_nodes_group[rank], pl.idx_of_nodes_on_device_group[rank],
                               list(range(ndev)), rank)
        srcs = _sources(feats, pl, rank, ndev)
        got, counts, flag = placed_gather_host(place, srcs, feats, NODES, info=True)
        assert got.dtype == torch.float32 and torch.equal(got, want) and flag == 0
        p = place[NODES].astype(np.int64)
        want_counts = np.bincount(np.where(p == PLACE_HOST, ndev, p >> PLACE_SHIFT), minlength=ndev + 1)
        assert np.array_equal(counts, want_counts) and counts.sum() == NODES.size
        # every source is really read: poison one at a time and the rows it serves change
        for s in range(ndev):
            bad = list(srcs)
            bad[s] = torch.full_like(srcs[s], 7.0)
            other = placed_gather_host(place, bad, feats, NODES)
            assert int((other != want).any(dim=1).sum()) == int(counts[s]) > 0
    # guards: zeros and the flag, every other row exact
    place = pack_placement(pl.device_id_of_nodes_group[0], pl.idx_of_nodes_on_device_group[0], list(range(ndev)), 0)
    srcs = _sources(feats, pl, 0, ndev)
    nodes = np.concatenate([NODES, [-1, NN]])
    got, _, flag = placed_gather_host(place, srcs, feats, nodes, info=True)
    assert flag == 1 and torch.equal(got[:-2], want) and not got[-2:].any()
    got, counts, flag = placed_gather_host(place, srcs, None, NODES, F=NFEAT, info=True)
    host = place[NODES] == PLACE_HOST
    assert flag == 1 and counts[-1] == 0 and not got[host].any() and torch.equal(got[~host], want[~host])


def _placed_cpu(feats, pl, rank, ndev, peers=True):
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[rank], "cpu", rank)
    if not peers:
        return PlacedFeatures.from_store(store, pl, rank)
    place = pack_placement(pl.device_id_of_nodes_group[rank], pl.idx_of_nodes_on_device_group[rank],
                           list(range(ndev)), rank)
    return PlacedFeatures(feats, place, _sources(feats, pl, rank, ndev), "cpu")


def _same_batch(a, b):
    assert torch.equal(a.x0, b.x0) and torch.equal(a.labels, b.labels) and torch.equal(a.input_nodes, b.input_nodes)
    for p, q in zip(a.adjs, b.adjs):
        assert (p is None) == (q is None)
        if p is not None:
            assert torch.equal(p.indices(), q.indices()) and torch.equal(p.values(), q.values())
    assert all(torch.equal(p, q) for p, q in zip(a.sampled_nodes, b.sampled_nodes))


@pytest.mark.parametrize("peers", [True, False], ids=["peers", "host_for_peers"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cpu_samplers_over_a_placed_store(world, dtype, peers):
    lap, feats, labels = world
    feats = feats.to(dtype)
    pl = _placement(lap, 2, 90)
    batch = np.arange(40, 560, 5)
    for rank in range(2):
        for make in (lambda f: NeighborSampler(lap, 4, [1, 1], f, labels, "cpu"),
                     lambda f: LayerwiseSampler(lap, 64, [1, 0, 1], f, labels, "cpu")):
            pf = _placed_cpu(feats, pl, rank, 2, peers)
            assert (pf.N, pf.F, pf.dtype) == (NN, NFEAT, dtype)
            plain, placed = make(feats), make(pf)
            _same_batch(plain.sample(batch, 11), placed.sample(batch, 11))
            c = pf.counts()
            assert c["total"] == placed.sample(batch, 11).input_nodes.numel() and c["own"] > 0 and c["host"] > 0
            assert (sum(c["peers"]) > 0) == peers
            pf.reset_counts()
            assert pf.counts()["total"] == 0
            for a, b in zip(plain.epoch(TRAIN, 200, seed=3), placed.epoch(TRAIN, 200, seed=3)):
                _same_batch(a, b)
            pf.check()
    with pytest.raises(ValueError, match="PlacedFeatures"):
        NeighborSampler(lap, 4, [1, 1], [feats], labels, "cpu")
    with pytest.raises(ValueError, match="rows"):
        NeighborSampler(lap, 4, [1, 1], PlacedFeatures(feats[:-1], np.full(NN - 1, PLACE_HOST, np.int32),
                                                       [None], "cpu"), labels, "cpu")


def test_placed_features_refuses_a_map_its_sources_do_not_hold(world):
    _, feats, _ = world
    place = np.full(NN, PLACE_HOST, np.int32)
    place[3] = (1 << PLACE_SHIFT) | 2
    with pytest.raises(ValueError, match="source or a slot"):
        PlacedFeatures(feats, place, [feats[:4]], "cpu")
    place[3] = 4
    with pytest.raises(ValueError, match="source or a slot"):
        PlacedFeatures(feats, place, [feats[:4]], "cpu")
    with pytest.raises(ValueError, match="no host table"):
        PlacedFeatures(None, place, [feats[:5]], "cpu")
    pf = PlacedFeatures(feats, place, [feats[:4]], "cpu", validate=False)  # the gather's own guard
    got = pf.gather(torch.tensor([3, 9]))
    assert not got[0].any() and torch.equal(got[1], feats[9])
    with pytest.raises(RuntimeError, match="could not serve|outside the placement map"):
        pf.check()


@pytest.mark.parametrize("n,world_size,bs", [(523, 4, 50), (10, 4, 3), (7, 3, 2), (520, 2, 200)])
def test_epoch_splits_the_permuted_list_by_rank(world, n, world_size, bs):
    lap, feats, labels = world
    ns = NeighborSampler(lap, 2, [1], feats, labels, "cpu")
    nodes = np.arange(30, 30 + n)
    whole = [b.batch_nodes for b in ns.epoch(nodes, n, seed=9)]
    assert len(whole) == 1
    perm = whole[0]  # the permuted list: world size 1, one batch
    chunk = -(-n // world_size)
    seen = []
    for rank in range(world_size):
        got = list(ns.epoch(nodes, bs, seed=9, rank=rank, world_size=world_size))
        mine = perm[rank * chunk: min((rank + 1) * chunk, n)]
        # rank_batches' chunk rule: the same batch count and sizes for this n, world and batch size
        ref = rank_batches(nodes, bs, rank, world_size, 0)
        assert [len(b.batch_nodes) for b in got] == [len(r) for r in ref]
        assert np.array_equal(np.concatenate([b.batch_nodes for b in got] + [np.zeros(0, np.int64)]), mine)
        assert all(b.seed == batch_seed(9, i) for i, b in enumerate(got))
        seen.append(mine)
    assert np.array_equal(np.concatenate(seen), perm) and np.array_equal(np.sort(perm), nodes)
    # the defaults are today's batches
    a = [b.batch_nodes for b in ns.epoch(nodes, bs, seed=9)]
    b = [b.batch_nodes for b in ns.epoch(nodes, bs, seed=9, rank=0, world_size=1)]
    assert len(a) == -(-n // bs) and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(np.concatenate(a), perm)
    with pytest.raises(ValueError, match="rank"):
        next(ns.epoch(nodes, bs, seed=9, rank=world_size, world_size=world_size))


# ----------------------------------------------------------------------------- the C ABI, no GPU

_P = 0x10000  # "some 16-byte aligned address": every call below returns before a pointer is read
_ARGS = dict(place=_P, N=100, srcs=_P, nsrc=2, host=_P, ld_host=16, kind=0, nodes=_P, n=5, dst=_P, ld_dst=16, F=12,
             counts=None, flag=_P)


def _call(L, **kw):
    a = dict(_ARGS, **kw)
    return L.gnn_gather_placed_f32(a["place"], a["N"], a["srcs"], a["nsrc"], a["host"], a["ld_host"], a["kind"],
                                   a["nodes"], a["n"], a["dst"], a["ld_dst"], a["F"], a["counts"], a["flag"], None)


@pytest.mark.parametrize("kw,words", [
    (dict(place=None), "NULL"), (dict(srcs=None), "NULL"), (dict(nodes=None), "NULL"), (dict(dst=None), "NULL"),
    (dict(flag=None), "NULL"),
    (dict(n=-1), "negative"), (dict(F=-1), "negative"), (dict(N=-1), "negative"), (dict(ld_dst=-16), "negative"),
    (dict(ld_host=-16), "negative"),
    (dict(n=1 << 31), "2\\^31"), (dict(N=1 << 31), "2\\^31"), (dict(F=1 << 31, ld_dst=1 << 32, ld_host=1 << 32), "2\\^31"),
    (dict(nsrc=0), "nsrc"), (dict(nsrc=17), "nsrc"), (dict(nsrc=-1), "nsrc"),
    (dict(kind=3), "kind"), (dict(kind=-1), "kind"),
    (dict(F=17), "stride"), (dict(ld_host=11), "stride"), (dict(ld_dst=11), "stride"),
    (dict(dst=_P + 2), "misaligned"), (dict(host=_P + 2), "misaligned"), (dict(host=_P + 1, kind=1), "misaligned"),
])
def test_gather_placed_refusals_without_gpu(kw, words):
    L = _lib.lib()
    rc = _call(L, **kw)
    assert rc == -22 and re.search(words, L.gnn_last_error().decode()), (rc, L.gnn_last_error())
    with pytest.raises(RuntimeError, match="gnn_gather_placed_f32"):
        _lib.check(rc, "gather_placed")


def test_gather_placed_empty_calls_return_before_null_checks():
    L = _lib.lib()
    none = dict(place=None, srcs=None, host=None, nodes=None, dst=None, flag=None)
    assert _call(L, n=0, **none) == 0
    assert _call(L, F=0, **none) == 0
    assert _call(L, n=0, F=0, N=0, **none) == 0
    assert _call(L, n=0, F=17) == -22  # a width past the stride is refused first, as the other gathers do
    assert _call(L, host=None, ld_host=0, n=0) == 0  # no host table: its stride is not looked at


def test_symbol_is_exported_and_declared():
    assert "gnn_gather_placed_f32" in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.lib(), "gnn_gather_placed_f32")
    with open(os.path.join(REPO, "include", "gnn_spmm.h")) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+gnn_gather_placed_f32\s*\(", txt)
    assert re.search(r"#define\s+GNN_PLACE_HOST\s+\(-1\)", txt) and re.search(r"#define\s+GNN_PLACE_SHIFT\s+27\b", txt)
    assert re.search(r"typedef\s+struct\s+gnn_place_src\s*\{\s*const\s+void\s*\*\s*base;\s*int64_t\s+ld;\s*int64_t\s+rows;", txt)
    assert (PLACE_HOST, PLACE_SHIFT, MAX_SOURCES) == (-1, 27, 16)
