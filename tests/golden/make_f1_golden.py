"""Generate tests/golden/f1_cases.npz from the reference's own utils.calc_f1 (utils.py:142-149,
sklearn.metrics.f1_score underneath), driven as its validation block drives it (main.py:193-195:
pred = Sigmoid()(output) or softmax(output, 1), then calc_f1(labels, pred, sigmoid_loss)).

Runs ONLY where the reference is present (make_golden.py's import recipe); the committed .npz is
data: per case the logits, the labels, is_sigmoid and the micro / macro F1 the reference returned.

Inputs are drawn so that the two thresholds of gnn_amd.metrics agree with the reference's by
construction, and this is asserted, not assumed:
  * every logit is a non-zero multiple of 1/64 (|z| >= 1e-3), so `z > 0` and the fp32
    `sigmoid(z) > 0.5` cannot disagree (they do only for 0 < z < ~1.2e-7);
  * distinct logits differ by >= 1/64, so the fp32 softmax keeps them distinct and keeps exact
    ties exact: argmax(softmax(z)) == argmax(z), the first index winning.

C = 1 appears in argmax mode only: given a one-column multi-label target sklearn takes it for a
binary one and scores both values of the column (micro becomes the accuracy), which is not the
per-class F1 the counts describe.

Usage: python tests/golden/make_f1_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import install_stubs  # noqa: E402


def _logits(rng, M, C):
    """Non-zero multiples of 1/64 in [-4, 4]."""
    k = rng.integers(1, 257, size=(M, C)) * rng.choice([-1, 1], size=(M, C))
    return (k / 64.0).astype(np.float32)


def _onehot(cls, C):
    y = np.zeros((len(cls), C), np.float32)
    y[np.arange(len(cls)), cls] = 1.0
    return y


def cases():
    rng = np.random.default_rng(2024)
    out = []
    # ---- multi-label (is_sigmoid = True)
    z = _logits(rng, 37, 41)
    out.append(("sig_c41", z, (rng.random((37, 41)) < 0.3).astype(np.float32), True))
    z = _logits(rng, 20, 172)
    y = (rng.random((20, 172)) < 0.1).astype(np.float32)
    z[:, 5], y[:, 5] = -np.abs(z[:, 5]), 0.0  # a class with no positives and no predictions
    z[:, 9], y[:, 9] = np.abs(z[:, 9]), 0.0  # predicted, never true
    z[:, 11], y[:, 11] = -np.abs(z[:, 11]), 1.0  # true, never predicted
    out.append(("sig_c172_empty_class", z, y, True))
    z = _logits(rng, 5, 7)
    out.append(("sig_all_wrong", z, (z <= 0).astype(np.float32), True))
    z = _logits(rng, 1, 41)
    out.append(("sig_single_row", z, (rng.random((1, 41)) < 0.4).astype(np.float32), True))
    # ---- single-label (is_sigmoid = False)
    z = _logits(rng, 50, 41)
    out.append(("arg_c41", z, _onehot(rng.integers(0, 41, 50), 41), False))
    z = _logits(rng, 30, 172)
    top = z.max(axis=1) + 0.5
    a, b = rng.integers(0, 86, 30), rng.integers(86, 172, 30)
    z[np.arange(30), a] = top  # two exactly tied maxima per row: the first index must win
    z[np.arange(30), b] = top
    true = np.where(rng.random(30) < 0.5, a, b)
    out.append(("arg_c172_ties", z, _onehot(true, 172), False))
    z = _logits(rng, 4, 1)
    out.append(("arg_c1", z, np.ones((4, 1), np.float32), False))
    z = _logits(rng, 6, 7)
    out.append(("arg_all_wrong", z, _onehot((z.argmax(axis=1) + 1 + rng.integers(0, 6, 6)) % 7, 7), False))
    z = _logits(rng, 1, 41)
    out.append(("arg_single_row", z, _onehot(z.argmax(axis=1), 41), False))
    return out


def main():
    install_stubs()
    import utils as ref_utils  # noqa: E402

    fx = {}
    names = []
    for name, z, y, is_sigmoid in cases():
        assert np.all(np.abs(z) >= 1e-3), name
        zt = torch.from_numpy(z)
        pred = torch.nn.Sigmoid()(zt) if is_sigmoid else torch.nn.functional.softmax(zt, dim=1)
        pred = pred.numpy().copy()
        if is_sigmoid:
            assert np.array_equal(pred > 0.5, z > 0), name
        else:
            assert np.array_equal(pred.argmax(axis=1), z.argmax(axis=1)), name
        micro, macro = ref_utils.calc_f1(y.copy(), pred, is_sigmoid)  # thresholds pred in place
        names.append(name)
        fx[name + "_logits"], fx[name + "_labels"] = z, y
        fx[name + "_is_sigmoid"] = np.array(is_sigmoid)
        fx[name + "_micro"], fx[name + "_macro"] = np.float64(micro), np.float64(macro)
        print(f"{name}: M {z.shape[0]} C {z.shape[1]} micro {micro:.6f} macro {macro:.6f}")
    fx["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "f1_cases.npz"), **fx)


if __name__ == "__main__":
    main()
