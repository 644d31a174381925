"""F1 scores from per-class prediction counts.

Reference: utils.calc_f1 (utils.py:142-149) thresholds (is_sigmoid) or argmaxes the predictions
on the host and calls sklearn.metrics.f1_score twice (micro, macro). Here the counts tp / fp / fn
per class are all a score needs: the evaluation head (gnn_head_eval_f32, include/gnn_layers.h)
produces them on the device, ``prediction_counts`` with torch ops anywhere else, and
``f1_from_counts`` turns them into sklearn's numbers (checked against sklearn 1.7.2 through the
reference's calc_f1: tests/golden/f1_cases.npz). Counts add over batches, so a whole validation
pass needs one device-to-host copy. numpy and torch only.
"""
from __future__ import annotations

import numpy as np
import torch

SIGMOID, ARGMAX = 0, 1  # mode: calc_f1(is_sigmoid=True) / calc_f1(is_sigmoid=False)


def prediction_counts(logits: torch.Tensor, labels: torch.Tensor, mode: int) -> torch.Tensor:
    """int32 [3, C] = (tp, fp, fn) per class, on the inputs' device.

    mode 0 (multi-label): pred_j = z_j > 0, true_j = y_j > 0.5. The reference thresholds
    sigmoid(z) > 0.5 in fp32, which differs only for 0 < z < ~1.2e-7 (the fp32 sigmoid rounds to
    exactly 0.5 there). mode 1 (single-label): pred = argmax z, true = argmax y, the first index
    winning ties as np.argmax; tp[c] = #(pred = c = true), fp[c] = #(pred = c != true),
    fn[c] = #(true = c != pred)."""
    if logits.dim() != 2 or logits.shape != labels.shape:
        raise ValueError(f"prediction_counts: logits {tuple(logits.shape)} vs labels {tuple(labels.shape)}")
    C = logits.shape[1]
    if mode == SIGMOID:
        pred, true = logits > 0, labels > 0.5
    elif mode == ARGMAX:
        # the first maximum, whatever torch.argmax does with ties: the smallest index at the maximum
        idx = torch.arange(C, device=logits.device).expand_as(logits)

        def first_max(t):
            at = t == t.max(dim=1, keepdim=True).values
            return torch.where(at, idx, C).min(dim=1).values

        cls = torch.arange(C, device=logits.device)
        pred, true = first_max(logits)[:, None] == cls, first_max(labels)[:, None] == cls
    else:
        raise ValueError(f"prediction_counts: mode {mode} (0 sigmoid, 1 argmax)")
    return torch.stack([(pred & true).sum(0), (pred & ~true).sum(0), (true & ~pred).sum(0)]).to(torch.int32)


def f1_from_counts(tp, fp, fn, mode: int):
    """(micro, macro) F1 in float64 with sklearn's conventions: micro = 2Σtp / (2Σtp + Σfp + Σfn),
    0 when nothing was predicted or true; per-class F1 = 2tp / (2tp + fp + fn), 0 for an empty
    class; macro = their mean over all C classes (mode 0) or over the classes that occur in
    y_true ∪ y_pred (mode 1: sklearn infers the label set from the class indices it sees)."""
    tp, fp, fn = (np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a).astype(np.int64).ravel()
                  for a in (tp, fp, fn))
    den = 2 * tp + fp + fn
    total = int(den.sum())
    micro = 2.0 * float(tp.sum()) / float(total) if total else 0.0
    per_class = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    if mode == ARGMAX:
        per_class = per_class[den > 0]
    macro = float(per_class.mean()) if per_class.size else 0.0
    return micro, macro
