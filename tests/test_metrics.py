"""CPU: F1 from prediction counts (gnn_amd.metrics) against the reference's utils.calc_f1 — the
goldens of tests/golden/make_f1_golden.py: sklearn's f1_score through the reference's own code —
the Evaluator's pooling over batches on a CPU model, and the loaders' sequential stream.

Tolerance: micro and macro are float64 ratios of the same integers sklearn divides, so 1e-12.
"""
import numpy as np
import pytest
import torch

from gnn_amd import graphs, loader, metrics
from gnn_amd.models import build_model
from gnn_amd.train import Evaluator


def _cases(z):
    return [str(n) for n in z["names"]]


def _counts(z, name):
    mode = 0 if bool(z[name + "_is_sigmoid"]) else 1
    logits, labels = torch.from_numpy(z[name + "_logits"]), torch.from_numpy(z[name + "_labels"])
    return metrics.prediction_counts(logits, labels, mode), mode, logits, labels


def test_golden_covers_the_cases(golden):
    z = golden("f1_cases.npz")
    names = _cases(z)
    assert len(names) >= 8
    C = {z[n + "_logits"].shape[1] for n in names}
    assert {1, 41, 172} <= C
    assert any(z[n + "_logits"].shape[0] == 1 for n in names)
    modes = {bool(z[n + "_is_sigmoid"]) for n in names}
    assert modes == {True, False}
    for n in names:  # the generator's condition on the inputs: z > 0 and sigmoid(z) > 0.5 agree
        assert np.all(np.abs(z[n + "_logits"]) >= 1e-3)
    ties = z["arg_c172_ties_logits"]
    assert np.all((ties == ties.max(axis=1, keepdims=True)).sum(axis=1) == 2)
    empty = z["sig_c172_empty_class_logits"], z["sig_c172_empty_class_labels"]
    assert not (empty[0][:, 5] > 0).any() and not empty[1][:, 5].any()
    assert z["sig_all_wrong_micro"] == 0.0 and z["arg_all_wrong_micro"] == 0.0


def test_f1_matches_reference_calc_f1(golden):
    z = golden("f1_cases.npz")
    for name in _cases(z):
        counts, mode, _, _ = _counts(z, name)
        assert counts.dtype == torch.int32 and counts.shape[0] == 3
        micro, macro = metrics.f1_from_counts(counts[0], counts[1], counts[2], mode)
        assert abs(micro - float(z[name + "_micro"])) <= 1e-12, (name, micro, float(z[name + "_micro"]))
        assert abs(macro - float(z[name + "_macro"])) <= 1e-12, (name, macro, float(z[name + "_macro"]))


def test_count_identities(golden):
    z = golden("f1_cases.npz")
    for name in _cases(z):
        counts, mode, logits, labels = _counts(z, name)
        tp, fp, fn = (int(c.sum()) for c in counts)
        if mode == 1:
            assert tp + fn == logits.shape[0] and fp == fn, name
            pred = np.argmax(logits.numpy(), axis=1)  # np.argmax: the first index wins ties
            assert np.array_equal(np.bincount(pred, minlength=logits.shape[1]), (counts[0] + counts[1]).numpy())
        else:
            assert tp + fn == int((labels > 0.5).sum()), name
            assert tp + fp == int((logits > 0).sum()), name


def test_f1_from_counts_conventions():
    assert metrics.f1_from_counts([0, 0], [0, 0], [0, 0], 0) == (0.0, 0.0)
    assert metrics.f1_from_counts([0, 0], [0, 0], [0, 0], 1) == (0.0, 0.0)
    # mode 0 averages over all classes, mode 1 over the classes that occur
    assert metrics.f1_from_counts([2, 0], [0, 0], [0, 0], 0) == (1.0, 0.5)
    assert metrics.f1_from_counts([2, 0], [0, 0], [0, 0], 1) == (1.0, 1.0)
    with pytest.raises(ValueError):
        metrics.prediction_counts(torch.zeros(2, 3), torch.zeros(2, 3), 2)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _golden_batch(z, case, seed):
    p = f"c{case}_"
    adjs = [torch.sparse_coo_tensor(_t(z[f"{p}adj{li}_indices"]), _t(z[f"{p}adj{li}_values"]),
                                    tuple(int(v) for v in z[f"{p}adj{li}_shape"])).coalesce() for li in range(3)]
    sampled = [_t(z[f"{p}sampled{li}"]) for li in range(3)]
    x0 = torch.randn(int(z[p + "nin"]), 602, generator=torch.Generator().manual_seed(seed))
    return x0, adjs, sampled, _t(z[p + "labels"])


@pytest.mark.parametrize("mode", [0, 1])
def test_evaluator_pools_batches_on_cpu(golden, mode):
    """Two batches of different sizes (the reference sampler's 128- and 16-node batches on the
    tiny graph) through a CPU model: the pooled scores are those of the concatenated logits, the
    reference's batch-weighted micro-F1 is the hand-computed mean, nothing leaves train mode."""
    z = golden("ladies_tiny.npz")
    batches = [_golden_batch(z, 0, 5), _golden_batch(z, 2, 6)]
    assert batches[0][3].shape[0] == 128 and batches[1][3].shape[0] == 16
    torch.manual_seed(0)
    net = build_model("graphsage", 602, 32, [1, 1, 1], 41, dropout=0.1)
    net.train()
    ev = Evaluator(net, "cpu", sigmoid_loss=True, mode=mode)
    for b in batches:
        loss, counts = ev.add(*b)
        assert isinstance(loss, torch.Tensor) and counts.shape == (3, 41) and counts.dtype == torch.int32
        assert net.training  # restored after every batch
    res = ev.result()
    assert net.training
    net.eval()
    with torch.no_grad():
        outs = [net(b[0], b[1], b[2]) for b in batches]
        losses = [float(net.forward_loss(*b)[0]) for b in batches]
    net.train()
    assert torch.equal(ev.predict(*batches[1][:3]), outs[1]) and net.training
    labels = [b[3] for b in batches]
    pooled = metrics.prediction_counts(torch.cat(outs), torch.cat(labels), mode)
    micro, macro = metrics.f1_from_counts(pooled[0], pooled[1], pooled[2], mode)
    assert res["micro_f1"] == micro and res["macro_f1"] == macro
    assert res["batches"] == 2 and res["rows"] == 144
    per = [metrics.f1_from_counts(*metrics.prediction_counts(o, y, mode), mode)[0] for o, y in zip(outs, labels)]
    assert abs(res["ref_batch_weighted_micro_f1"] - (per[0] * 128 + per[1] * 16) / 144) <= 1e-15
    assert abs(res["loss"] - (losses[0] * 128 + losses[1] * 16) / 144) <= 1e-6 * abs(res["loss"])
    assert Evaluator(net, "cpu").result()["batches"] == 0


def _tiny_loader(cls=loader.BatchLoader, **kw):
    A, labels, _, ncls, train, valid, test = graphs.make_dataset(graphs.TINY, seed=1, with_features=False)
    lap = graphs.lap_matrix(A, "graphsage")
    N = A.shape[0]
    ld = cls(lap, labels, train, 64, 16, [1, 1, 1], np.full(N, -1), np.zeros(N, np.int64), workers=2, seed=5, **kw)
    return ld, train, valid


def _same_batches(a, b):
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert np.array_equal(x.host.batch_nodes, y.host.batch_nodes)
        assert np.array_equal(x.host.input_nodes, y.host.input_nodes)
        for la, lb in zip(x.host.layers, y.host.layers):
            assert np.array_equal(la.colidx, lb.colidx) and np.array_equal(la.normfact, lb.normfact)


def test_batch_loader_sequential():
    ld, train, valid = _tiny_loader()
    bs = 48
    assert len(valid) % bs != 0 and len(valid) > 2 * bs  # the last chunk is short
    got = list(ld.sequential(valid, bs))
    nodes = [np.asarray(b.host.batch_nodes) for b in got]
    assert len(got) == -(-len(valid) // bs)
    assert all(len(n) == bs for n in nodes[:-1]) and len(nodes[-1]) == len(valid) % bs
    assert np.array_equal(np.concatenate(nodes), np.asarray(valid))  # consecutive, each node once
    assert [len(n) for n in (np.asarray(b.host.batch_nodes) for b in ld.sequential(valid[:20]))] == [16, 4]
    _same_batches(got, list(ld.sequential(valid, bs)))  # a pass is repeatable
    # the training stream's seeds are untouched by the evaluation passes
    after = list(ld.epoch(1))
    ld.close()
    fresh, _, _ = _tiny_loader()
    ref = list(fresh.epoch(1))
    fresh.close()
    _same_batches(after, ref)


def test_native_loader_sequential_matches_batch_loader():
    nat, train, valid = _tiny_loader(loader.NativeLoader, pinned=False)
    py, _, _ = _tiny_loader()
    a = list(nat.sequential(valid, 48))
    b = list(py.sequential(valid, 48))
    assert len(a) == len(b) == -(-len(valid) // 48)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x.host.input_nodes), np.asarray(y.host.input_nodes))
        assert np.array_equal(np.asarray(x.host.sampled_nodes[-1]), np.asarray(y.host.sampled_nodes[-1]))
        assert np.array_equal(np.asarray(x.host.labels), np.asarray(y.host.labels))
    after = [np.asarray(lb.host.input_nodes).copy() for lb in nat.epoch(1)]
    ref = [np.asarray(lb.host.input_nodes) for lb in py.epoch(1)]
    assert len(after) == len(ref) and all(np.array_equal(p, q) for p, q in zip(after, ref))
    py.close()
    nat.close()
