"""What a neighbour-sampled batch costs to draw on the device, and how fast the training step
runs over such batches (MI355X; needs the GPU, no fallback).

Geometry: the Reddit-shaped synthetic graph of ``bench.py`` (233 k nodes, 602 features), GraphSAGE,
batch 512, the feature table resident on the device; fanouts (25, 10) with two aggregating layers
and (10, 10, 10) with three. Per case, over ``--batches`` batches of one shuffled pass after one
warm-up batch: the time of ``NeighborSampler.sample`` (a host clock around work that ends in a
device synchronisation; median, min, max), the batch's shapes, then ``Trainer.step`` over the
batches already drawn (steps per second, one synchronisation at the end) and drawing and stepping
in turn on the one stream (nothing overlaps: the sampler has no producer thread).

Beside it, on the same box: one host thread's LADIES draw (``ladies_sample_host``, samp 8192, the
same batch nodes), the producer cost DESIGN §8 quotes per thread. The two samplers make different
batches, so this is a record, not a race.

    python scripts/neighbor_probe.py [--batches 20] [--graph reddit] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_amd import graphs, sampler  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.neighbor import NeighborSampler  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402

CASES = [((25, 10), [1, 1]), ((10, 10, 10), [1, 1, 1])]


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def median_shape(shapes, k):
    """[M, K, nnz] of layer k, each the median over the batches (None for an order-0 layer)."""
    if shapes[0][k] is None:
        return None
    return [int(statistics.median(s[k][i] for s in shapes)) for i in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "tiny"])
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--samp-num", type=int, default=8192, help="the LADIES draw's layer size")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("neighbor_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    spec = {"reddit": graphs.REDDIT, "tiny": graphs.TINY}[args.graph]
    A, labels, feats, ncls, train, _, _ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N, F = A.shape[0], int(feats.shape[1])
    print(f"graph {spec.name}: N={N} nnz={lap.nnz}", file=sys.stderr, flush=True)
    out = {"probe": "neighbor", "label": args.label, "graph": spec.name, "N": N, "nnz": int(lap.nnz), "F": F,
           "nhid": args.nhid, "batch_size": args.batch_size, "batches": args.batches,
           "device": torch.cuda.get_device_name(0), "cases": []}
    feats_dev = None
    for fan, orders in CASES:
        ns = NeighborSampler(lap, list(fan), orders, feats if feats_dev is None else feats_dev, labels, dev)
        feats_dev = ns.feats  # one upload serves both cases
        torch.manual_seed(0)
        model = build_model("graphsage", F, args.nhid, orders, ncls, 0.1, fused=True).to(dev)
        tr = Trainer(model, 0.01, dev)
        rng = np.random.default_rng(0)
        chunks = [rng.choice(train, args.batch_size, replace=False) for _ in range(args.batches + 1)]
        ms, batches = [], []
        for b, q in enumerate(chunks):
            t, batch = wall_ms(lambda: ns.sample(q, 1000 + b))
            if b:
                ms.append(t)
                batches.append(batch)
        native = all(tr.executor is not None and tr.executor.supports(*b) for b in batches)
        tr.step(*batches[0])  # warm-up: workspaces, the GEMM plans
        t_steps, _ = wall_ms(lambda: [tr.step(*b) for b in batches])

        def both():
            for b, q in enumerate(chunks[1:]):
                tr.step(*ns.sample(q, 2000 + b))

        t_both, _ = wall_ms(both)
        shapes = [[None if a is None else [a.shape[0], a.shape[1], a.nnz] for a in b.adjs] for b in batches]
        case = {"fanouts": list(fan), "orders": orders, "native_step": bool(native), "sample_ms": spread(ms),
                "median_layer_shapes_M_K_nnz_bottom_up": [median_shape(shapes, k) for k in range(len(orders))],
                "median_input_nodes": int(statistics.median(int(b.input_nodes.numel()) for b in batches)),
                "step_only_per_s": round(len(batches) / (t_steps * 1e-3), 1),
                "step_only_ms": round(t_steps / len(batches), 3),
                "sample_then_step_per_s": round(len(batches) / (t_both * 1e-3), 1)}
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)
        del tr, model, batches
    # one host thread's LADIES draw over the same kind of batch, for the record
    lad = []
    none, zero = np.full(N, -1), np.zeros(N, np.int64)
    for b in range(min(args.batches, 10) + 1):
        q = np.sort(np.random.default_rng(100 + b).choice(train, args.batch_size, replace=False))
        t0 = time.perf_counter()
        sampler.ladies_sample_host(3 + b, q, np.array([args.samp_num] * 5), N, lap, labels, [1, 1], none, zero, None,
                                   1.0, [0])
        if b:
            lad.append((time.perf_counter() - t0) * 1e3)
    out["ladies_host_draw_ms_one_thread"] = dict(spread(lad), samp_num=args.samp_num, orders=[1, 1])
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
