"""What the reduced-precision GEMM modes cost in training quality (MI355X; needs the GPU).

The layer GEMMs run on the split kernel at three bf16 pieces per operand by default ("split3":
fp32-level accuracy). ``Trainer(..., gemm="split2" | "bf16")`` keeps two pieces or one
(fused.round_operand: |x - x'| <= 2^-15 |x| or 2^-8 |x| on every operand of a split-kernel product,
fp32 accumulation). This probe trains the same seeded model on the same seeded batches under each
mode and reports how far the reduced modes drift from split3.

Geometry: config 2 (Reddit-shaped synthetic graph, GraphSAGE orders 1,1, nhid 512, LADIES samp
8192, batch 512, buffer 0.1 N). ``--train-batches`` distinct batches are staged once through the
native loader and the native staging call and cycled for ``--steps`` Adam steps (dropout 0.1, the
same dropout seeds under every mode); the loss is recorded every ``--every`` steps; at the end
``Trainer.evaluate`` runs over ``--eval-batches`` further batches the run never trained on
(argmax micro / macro F1, mean loss). The synthetic graph's labels are drawn independently of its
random features, so nothing could be learnt from them as they are: the probe plants a class
prototype in the features (``--signal`` times a unit-variance random vector per class, added to
the unit-variance noise; the default 0.25 puts two classes 8.7 noise deviations apart), the same
table under every mode. The gaps against split3 are the result, not the absolute scores — and on
this synthetic graph they are gaps between runs that do not learn: measured at signal 0, 0.08 and
0.25, the loss reaches the label prior's 4.70 within ~60 steps and stays there, and the held-out F1
stays at chance (1 / 41 classes) under every mode, so the F1 gap carries no information here and a
verdict on model quality needs a real dataset. One JSON line; no threshold.

    python scripts/gemm_precision_probe.py [--steps 300] [--every 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_amd import graphs, loader, placement, staging  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402

MODES = ("split3", "split2", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--train-batches", type=int, default=24)
    ap.add_argument("--eval-batches", type=int, default=8)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "tiny"])
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--signal", type=float, default=0.25, help="size of the planted class prototypes (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gemm_precision_probe: no GPU visible; this probe measures on the device and has no fallback")
    os.environ.pop("GNN_GEMM_ALGO", None)  # the modes go through the descriptor, not the environment
    dev = torch.device("cuda", 0)
    spec = graphs.REDDIT if args.graph == "reddit" else graphs.TINY
    samp, bs = (8192, 512) if args.graph == "reddit" else (256, 64)
    orders = [1, 1]
    A, labels, feats, ncls, train, *_ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    if args.signal:
        cls = torch.from_numpy(np.asarray(labels.argmax(axis=1)).reshape(-1))
        proto = torch.randn(ncls, feats.shape[1], generator=torch.Generator().manual_seed(1))
        feats = feats + args.signal * proto[cls]
    N, F = A.shape[0], int(feats.shape[1])
    pl = placement.create_buffer(lap, train, int(0.1 * N), [0], 3, alpha=0)
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
    ld = loader.NativeLoader(lap, labels, train, samp, bs, orders, pl.device_id_of_nodes_group[0],
                             pl.idx_of_nodes_on_device_group[0], store=store, workers=args.workers, seed=0,
                             device_extract=True)
    try:
        stager = staging.Stager(store)
        items = []
        for _, lb in zip(range(args.train_batches + args.eval_batches), ld.epoch(1)):
            staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
            items.append((lb, staged, staged.wait()))
        torch.cuda.synchronize()
    finally:
        ld.close()
    batch = lambda it: (it[2], it[1].adjs, it[1].batch.sampled_nodes, it[1].batch.labels)  # noqa: E731
    train_items, eval_items = items[:args.train_batches], items[args.train_batches:]
    out = {"probe": "gemm_precision", "graph": spec.name, "samp": samp, "batch": bs, "nhid": args.nhid, "F": F,
           "orders": orders, "signal": args.signal, "f1": "argmax (mode 1)", "steps": args.steps, "every": args.every,
           "train_batches": len(train_items), "eval_batches": len(eval_items), "device": torch.cuda.get_device_name(0), "modes": {}}
    for mode in MODES:
        torch.manual_seed(0)
        net = build_model("graphsage", F, args.nhid, orders, ncls, 0.1, fused=True).to(dev)
        tr = Trainer(net, 0.01, dev, gemm=mode)
        assert all(tr.executor.supports(*batch(it)) for it in items), "the native step refused a batch"
        losses = []
        for s in range(args.steps):
            torch.manual_seed(1000 + s)  # the dropout seeds: the same under every mode
            loss = tr.step(*batch(train_items[s % len(train_items)]))
            if s % args.every == 0 or s == args.steps - 1:
                losses.append((s, loss))
        ev = tr.evaluate([batch(it) for it in eval_items], mode=1)
        torch.cuda.synchronize()
        out["modes"][mode] = {"loss": [[s, round(float(v), 6)] for s, v in losses],
                              "eval": {k: round(float(ev[k]), 6) for k in ("micro_f1", "macro_f1", "loss")}}
    ref = out["modes"]["split3"]
    for mode in MODES[1:]:
        m = out["modes"][mode]
        rel = [abs(a[1] - b[1]) / max(abs(b[1]), 1e-30) for a, b in zip(m["loss"], ref["loss"])]
        m["vs_split3"] = {"max_rel_loss_gap": float(f"{max(rel):.3e}"), "final_rel_loss_gap": float(f"{rel[-1]:.3e}"),
                          **{f"eval_{k}_gap": round(m["eval"][k] - ref["eval"][k], 6)
                             for k in ("micro_f1", "macro_f1", "loss")}}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
