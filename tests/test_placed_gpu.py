"""GPU: gnn_gather_placed_f32 through PlacedFeatures against ``feats.float()[nodes]`` bit for bit —
every kind, widths on both sides of a register pass, row counts around the walkers' 64-position
loads and uneven ranges, every source mix, strides and bases that force every load width — then
the counters, the guards, capture and replay, and the device samplers over a placed store."""
import numpy as np
import pytest
import torch

from gnn_amd import models, placement, staging
from gnn_amd.layerwise import LayerwiseSampler
from gnn_amd.neighbor import NeighborSampler
from gnn_amd.placed import PLACE_HOST, PLACE_SHIFT, PlacedFeatures, placed_gather_host
from gnn_amd.train import Trainer
from test_exact_cpu import make_world
from test_placed_cpu import C, NN, TRAIN, _labels

pytestmark = pytest.mark.gpu

N = 1100
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
WIDTHS = [1, 26, 602, 608, 1030, 2056]  # 1030 > 768 (an fp32 pass), 2056 > 1024 (a 16-bit pass)
ROWS = [0, 1, 3, 64, 65, 1027]
MIXES = ["own", "host", "nohost", "three", "zero_rows"]
_TABLES = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _table(dtype, F):
    """(table [N, F] of ``dtype``, its ``.float()``): computed once per (dtype, F) and left unchanged.
    16-bit tables run through all 65,536 patterns (N * F >= 65,536 from F = 60 up)."""
    key = (dtype, F)
    if key not in _TABLES:
        if dtype == torch.float32:
            t = torch.randn(N, F, generator=torch.Generator().manual_seed(F))
        else:
            pat = (np.arange(N * F, dtype=np.int64) * 40503 + 17) & 0xFFFF  # odd multiplier: a bijection mod 2^16
            assert F < 60 or np.unique(pat).size == 65536
            t = torch.from_numpy(pat.astype(np.uint16).view(np.int16)).view(dtype).view(N, F)
        _TABLES[key] = (t, _widened(t))
    return _TABLES[key]


def _widened(t):
    """The reference, ``t.float()``. Its NaN words alone are set by integer arithmetic to the IEEE
    conversion's (sign, quiet NaN, payload moved up): torch's CPU conversion of an fp16 NaN gives
    that word in the vector body of a copy and 0x7fffffff in its scalar tail, so which one
    ``feats.float()[nodes]`` holds depends on where the element falls; every other word is the CPU
    conversion's, and NaNs are compared as bits like the rest."""
    x = t.float()
    if t.dtype == torch.float32:
        return x
    nan = torch.isnan(x)
    assert int(nan.sum()) > 0 or t.numel() < 65536
    b = t.view(torch.int16).to(torch.int64) & 0xFFFF
    w = (b << 16) if t.dtype == torch.bfloat16 else (((b & 0x8000) << 16) | 0x7FC00000 | ((b & 0x3FF) << 13))
    w = torch.where(w >= 2**31, w - 2**32, w).to(torch.int32)
    agree = int((x.view(torch.int32)[nan] == w[nan]).sum())
    assert 2 * agree >= int(nan.sum()), "the CPU conversion's own NaN words are mostly the IEEE ones"
    x.view(torch.int32)[nan] = w[nan]
    return x


def _rows_view(rows: torch.Tensor, ld: int, offset: int, device) -> torch.Tensor:
    """``rows`` copied into rows of stride ``ld`` whose base is ``offset`` elements into a buffer."""
    r, F = rows.shape
    flat = torch.zeros(max(r, 1) * ld + offset + 8, dtype=rows.dtype, device=device)
    v = flat.as_strided((r, F), (ld, 1), offset)
    v.copy_(rows)
    return v


def _mix(mix, seed):
    """(source of every node: -1 host or 0..2, nsrc)."""
    rng = np.random.default_rng(seed)
    if mix == "own":
        return np.zeros(N, np.int64), 1
    if mix == "host":
        return np.full(N, -1, np.int64), 1
    if mix == "nohost":
        return rng.integers(0, 3, N), 3
    if mix == "three":
        return rng.integers(-1, 3, N), 3
    src = rng.integers(-1, 2, N)  # zero_rows: source 1 buffers nothing
    return np.where(src == 1, 2, src), 3


def _parts(dtype, F, mix, padded, dev):
    """(host table or None, place, source tensors on ``dev``, src of every node, want =
    table.float()) of one source mix. ``padded``: the host table and the buffers of sources 1 and 2
    in rows of whole lines plus 3 elements with their bases off by one element (scalar loads) while
    source 0 keeps whole-line rows (16-byte loads), all in one launch; else stride F for the table
    and the buffers."""
    table, want = _table(dtype, F)
    src, nsrc = _mix(mix, F + len(mix))
    rng = np.random.default_rng(F)
    place = np.full(N, PLACE_HOST, np.int32)
    sources = []
    for s in range(nsrc):
        ids = rng.permutation(np.flatnonzero(src == s))
        place[ids] = (s << PLACE_SHIFT) | np.arange(ids.size)
        if padded and s >= 1:  # the "peers": an odd stride and a base off by one element, as the host table
            sources.append(_rows_view(table[torch.from_numpy(ids)], staging.padded_ld(F, 64) + 3, 1, dev))
        else:
            sources.append(_rows_view(table[torch.from_numpy(ids)], staging.padded_ld(F, 64) if padded else F, 0, dev))
    host = None
    if mix != "nohost":
        host = _rows_view(table, staging.padded_ld(F, 64) + 3, 1, "cpu") if padded else _rows_view(table, F, 0, "cpu")
    return host, place, sources, src, want


def _case(dtype, F, mix, padded, dev):
    host, place, sources, src, want = _parts(dtype, F, mix, padded, dev)
    return PlacedFeatures(host, place, sources, dev, F=F), src, want


def _nodes(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, N, n)
    if n >= 3:
        q[[0, n // 2, n - 1]] = [N - 1, 0, N - 1]  # the first and the last node; a repeat at the odd last place
    if n >= 64:
        q[10:14] = q[9]  # repeats
    return q


def _assert_rows(got, want, what):
    got = got.cpu()
    same = _bits(got) == _bits(want)
    print(f"{what}: {int((~same).sum())} of {same.numel()} words differ")
    assert got.shape == want.shape and bool(same.all()), what  # bits: NaN patterns included


@pytest.mark.parametrize("padded", [False, True], ids=["ldF", "padded_off1"])
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_is_the_table(dev, dtype, F, padded):
    for mix in MIXES:
        pf, src, want = _case(dtype, F, mix, padded, dev)
        nsrc = pf.nsrc
        assert (pf._host_ptr is None) == (mix in ("own", "nohost"))  # no host-placed node: nothing registered
        total = np.zeros(nsrc + 1, np.int64)
        for n in ROWS:
            q = _nodes(n, n + F)
            for idt in (torch.int64, torch.int32):
                got = pf.gather(torch.from_numpy(q).to(dev).to(idt))
                assert got.dtype == torch.float32 and got.shape == (n, F) and (n == 0 or got.stride(0) % 32 == 0)
                _assert_rows(got, want[torch.from_numpy(q)], f"{mix} n={n} {idt}")
                total += np.bincount(np.where(src[q] < 0, nsrc, src[q]), minlength=nsrc + 1)
        # a destination of the caller's: an odd stride (scalar stores), everything else untouched
        q = _nodes(65, 3)
        buf = torch.full((65, F + 5), float("nan"), device=dev)
        pf.gather(torch.from_numpy(q).to(dev), out=buf[:, 1: F + 1])
        total += np.bincount(np.where(src[q] < 0, nsrc, src[q]), minlength=nsrc + 1)
        _assert_rows(buf[:, 1: F + 1], want[torch.from_numpy(q)], f"{mix} out=")
        assert bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, F + 1:]).all())
        c = pf.counts()
        assert [c["own"]] + c["peers"] + [c["host"]] == total.tolist() and c["total"] == total.sum()
        if mix == "zero_rows":
            assert pf.sources[1] == (0, 0, 0) or pf.sources[1][2] == 0
            assert c["peers"][0] == 0 and c["peers"][1] > 0 and c["own"] > 0 and c["host"] > 0
        pf.reset_counts()
        assert pf.counts()["total"] == 0
        pf.check()
        pf.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_second_run_is_bit_identical_and_equals_the_restatement(dev, dtype):
    F = 602
    host, place, sources, src, want = _parts(dtype, F, "three", True, dev)
    pf = PlacedFeatures(host, place, sources, dev)
    q = _nodes(1027, 5)
    qd = torch.from_numpy(q).to(dev)
    a, b = pf.gather(qd), pf.gather(qd)
    assert torch.equal(_bits(a), _bits(b))
    ref, counts, flag = placed_gather_host(place, [t.cpu() for t in sources], host, q, info=True)
    _assert_rows(a, ref, "restatement")
    c = pf.counts()
    assert flag == 0 and [c["own"]] + c["peers"] + [c["host"]] == (2 * counts).tolist()
    pf.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_guards_zero_the_row_and_raise_the_flag(dev, dtype):
    """Every row the map cannot serve is zeros, every other row exact, the flag is up and check()
    raises; the same inputs through the restatement give the same rows."""
    F = 70
    host, good, sources, src, want = _parts(dtype, F, "three", False, dev)
    rng = np.random.default_rng(1)
    pick = lambda s, k: rng.choice(np.flatnonzero(src == s), k, replace=False)
    rows1 = int(sources[1].shape[0])
    top = (1 << PLACE_SHIFT) - 1
    broken = {
        "source index >= nsrc": (pick(0, 3), [(3 << PLACE_SHIFT) | 1, (15 << PLACE_SHIFT) | 0, (7 << PLACE_SHIFT) | 5]),
        "slot >= rows": (pick(1, 3), [(1 << PLACE_SHIFT) | rows1, (1 << PLACE_SHIFT) | top,
                                      (1 << PLACE_SHIFT) | (rows1 + 1000)]),
        "a negative word that is not -1": (pick(2, 2), [-2, -(1 << 31)]),
    }
    q = np.concatenate([np.arange(N), np.arange(N)[::-1][:131]])
    qd = torch.from_numpy(q).to(dev)

    def run(place, srcs, table, nodes, bad_positions, what):
        pf = PlacedFeatures(table, place, srcs, dev, F=F, validate=False)
        pf.check()  # nothing gathered yet
        got = pf.gather(nodes).cpu()
        ids = nodes.cpu().numpy().astype(np.int64)
        ref = want[torch.from_numpy(np.clip(ids, 0, N - 1))].clone()
        ref[torch.from_numpy(bad_positions)] = 0
        assert bad_positions.size > 0
        _assert_rows(got, ref, what)  # the bad rows zeros, every other row exact
        cpu_srcs = [None if t is None else (t.cpu() if isinstance(t, torch.Tensor) else None) for t in srcs]
        if all(t is None or isinstance(t, torch.Tensor) for t in srcs):
            rows, _, flag = placed_gather_host(place, cpu_srcs, table, ids, F=F, info=True)
            assert flag == 1 and torch.equal(_bits(rows), _bits(ref)), what
        with pytest.raises(RuntimeError, match="PlacedFeatures"):
            pf.check()
        pf.close()

    # the map's own faults, one kind at a time and all at once
    everything = good.copy()
    for name, (nodes_bad, words) in broken.items():
        place = good.copy()
        place[nodes_bad] = words
        everything[nodes_bad] = words
        run(place, sources, host, qd, np.flatnonzero(np.isin(q, nodes_bad)), name)
    bad_all = np.concatenate([b for b, _ in broken.values()])
    run(everything, sources, host, qd, np.flatnonzero(np.isin(q, bad_all)), "all at once")
    with pytest.raises(ValueError, match="source or a slot"):
        PlacedFeatures(host, everything, sources, dev)  # what validate=True says of that map
    # nodes outside the map
    out = torch.tensor([5, -1, N, 2**31 - 1, -(2**31), N - 1, 0], dtype=torch.int64)
    run(good, sources, host, out.to(torch.int32).to(dev), np.array([1, 2, 3, 4]), "nodes outside the map")
    # a source in use without a buffer, and one whose rows are narrower than F
    run(good, [sources[0], None, sources[2]], host, qd, np.flatnonzero(src[q] == 1), "a NULL base")
    narrow = (sources[2].data_ptr(), int(sources[2].shape[0]), F - 1)
    run(good, [sources[0], sources[1], narrow], host, qd, np.flatnonzero(src[q] == 2), "ld < F")
    # host-placed nodes and no host table
    run(good, sources, None, qd, np.flatnonzero(src[q] < 0), "a NULL host table")


def test_captured_gather_replays_bit_exact(dev):
    F = 602
    pf, src, want = _case(torch.float16, F, "three", True, dev)
    q1, q2 = _nodes(1027, 8), _nodes(1027, 9)
    nodes = torch.from_numpy(q1).to(torch.int32).to(dev)
    out = torch.zeros((1027, staging.padded_ld(F, 32)), device=dev)[:, :F]
    pf.gather(nodes, out=out)  # warm-up: the library is loaded and the table mapped
    torch.cuda.synchronize()
    out.zero_()
    pf.reset_counts()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):  # one stream, no parallel branches
        pf.gather(nodes, out=out)
    cg.replay()
    _assert_rows(out, want[torch.from_numpy(q1)], "replay 1")
    nodes.copy_(torch.from_numpy(q2).to(torch.int32))
    out.zero_()
    cg.replay()
    _assert_rows(out, want[torch.from_numpy(q2)], "replay 2")
    assert pf.counts()["total"] == 2 * 1027
    pf.check()
    del cg
    pf.close()


# ----------------------------------------------------------------------------- the samplers


@pytest.fixture(scope="module")
def world():
    lap, feats = make_world("graphsage", NN, 48)
    return lap, feats, _labels(NN, C)


def _same_operands(a, b):
    assert torch.equal(a.input_nodes, b.input_nodes) and torch.equal(a.labels, b.labels)
    for p, q in zip(a.adjs, b.adjs):
        assert (p is None) == (q is None)
        if p is not None:
            assert p.shape == q.shape and torch.equal(p.rowptr, q.rowptr) and torch.equal(p.col, q.col)
            assert torch.equal(p.val, q.val)
    assert all(torch.equal(p, q) for p, q in zip(a.sampled_nodes, b.sampled_nodes))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("fraction", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("kind", ["neighbor", "layerwise"])
def test_samplers_over_a_placed_store(dev, world, kind, fraction, dtype):
    lap, feats, labels = world
    feats = feats.to(dtype)
    orders = [1, 1]
    pl = placement.create_buffer(lap, TRAIN, int(fraction * NN), [0], 2, alpha=0)
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
    pf = PlacedFeatures.from_store(store, pl, 0)
    try:
        _sampler_checks(dev, lap, feats, labels, orders, kind, fraction, pf)
    finally:
        pf.close()  # the table's registration goes, whatever the checks said


def _sampler_checks(dev, lap, feats, labels, orders, kind, fraction, pf):
    assert (pf._host_ptr is None) == (fraction == 1.0)
    make = ((lambda f: NeighborSampler(lap, [10, 5], orders, f, labels, dev)) if kind == "neighbor" else
            (lambda f: LayerwiseSampler(lap, 64, orders, f, labels, dev)))
    plain, placed = make(feats), make(pf)
    nodes = np.arange(40, 560)
    pa = list(plain.epoch(nodes, 200, seed=3))
    pb = list(placed.epoch(nodes, 200, seed=3))  # ends with pf.check()
    assert len(pa) == len(pb) == 3
    for a, b in zip(pa, pb):
        _same_operands(a, b)
        assert b.x0.stride() == a.x0.stride() and torch.equal(a.x0, b.x0)
        assert torch.equal(a.x0.cpu(), feats.float()[a.input_nodes.cpu()])
    c = pf.counts()
    assert c["total"] == sum(int(b.input_nodes.numel()) for b in pb)
    assert (c["own"] > 0) == (fraction > 0) and (c["host"] > 0) == (fraction < 1)

    def train(batches):
        torch.manual_seed(0)
        m = models.build_model("graphsage", feats.shape[1], 128, orders, C, 0.1, fused=True).to(dev)
        tr = Trainer(m, 0.01, dev)
        torch.manual_seed(100)
        losses = [float(tr.step(*b)) for b in batches[:2]]  # fp32 losses: exact as Python floats
        return losses, [p.detach().clone() for p in tr.params]

    (la, wa), (lb, wb) = train(pa), train(pb)
    assert np.isfinite(la).all() and la == lb and all(torch.equal(x, y) for x, y in zip(wa, wb))


def test_sampler_refusals_over_a_placed_store(dev, world, monkeypatch):
    lap, feats, labels = world
    pl = placement.create_buffer(lap, TRAIN, 60, [0], 2, alpha=0)
    cpu = PlacedFeatures.from_store(staging.FeatureStore(feats, pl.gpu_buffer_group[0], "cpu", 0), pl, 0)
    with pytest.raises(ValueError, match="is on cpu"):
        NeighborSampler(lap, 5, [1, 1], cpu, labels, dev)
    need = NN * 64 * 4
    monkeypatch.setattr(NeighborSampler, "_free_bytes", lambda self: need - 1)
    with pytest.raises(RuntimeError, match=f"{need} bytes of device memory, {need - 1} free: a partially buffered "
                                           "feature store is out of scope.*PlacedFeatures"):
        NeighborSampler(lap, 5, [1, 1], feats, labels, dev)
