"""What the device-side LADIES draw (gnn_amd.layerwise, the hashed race) costs per batch, stage by
stage, how fast the training step runs over its batches, and — in the same run on the same box —
what one host producer thread pays for the native host draw (MI355X; needs the GPU, no fallback).

Geometry: BASELINE config 2 (the Reddit-shaped graph, GraphSAGE, orders [1, 1, 1], samp 8192,
batch 512) and the products-shaped graph of ``gnn_amd.graphs`` with the same sampler settings; the
feature table resident on the device. Per graph, over ``--batches`` distinct batches after
``--warmup`` warm-up batches: the GPU time of every stage of every layer's draw between HIP events
on the stream (medians; the stages' sum is the draw's GPU time, host gaps excluded), the wall time of
``LayerwiseSampler.sample`` (host clock around work that ends synchronised; it includes the one
read per layer, the allocations and the Python between launches), ``Trainer.step`` over the batches
already drawn, drawing and stepping in turn on one stream (no producer thread: nothing overlaps),
and ``ladies_sample_host``'s native path over the same batch nodes on one thread. The two samplers
draw different random streams of the same law, so the batch shapes agree in distribution only.

    python scripts/layerwise_probe.py [--graphs reddit,products] [--batches 20] [--out FILE]
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
from gnn_amd.layerwise import LayerwiseSampler  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402

SPECS = {"reddit": graphs.REDDIT, "products": graphs.PRODUCTS, "tiny": graphs.TINY}
ORDERS = [1, 1, 1]


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stage_ms(trace):
    """{(layer, stage): ms} of one batch's trace: the time from the previous mark of the layer."""
    out, prev = {}, {}
    for layer, stage, ev in trace:
        if stage != "begin":
            out[(layer, stage)] = prev[layer].elapsed_time(ev)
        prev[layer] = ev
    return out


def probe(name, args, dev):
    spec = SPECS[name]
    t0 = time.perf_counter()
    A, labels, feats, ncls, train, _, _ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N, F = A.shape[0], int(feats.shape[1])
    print(f"graph {spec.name}: N={N} nnz={lap.nnz} ({time.perf_counter() - t0:.0f} s)", file=sys.stderr, flush=True)
    ls = LayerwiseSampler(lap, args.samp_num, ORDERS, feats, labels, dev)
    torch.manual_seed(0)
    model = build_model("graphsage", F, args.nhid, ORDERS, ncls, 0.1, fused=True).to(dev)
    tr = Trainer(model, 0.01, dev)
    rng = np.random.default_rng(0)
    chunks = [rng.choice(train, args.batch_size, replace=False) for _ in range(args.warmup + args.batches)]
    wall, stages, batches = [], [], []
    for b, q in enumerate(chunks):
        ls.trace = []
        t, batch = wall_ms(lambda: ls.sample(q, 1000 + b))
        if b >= args.warmup:
            wall.append(t)
            stages.append(stage_ms(ls.trace))
            batches.append(batch)
    ls.trace = None
    keys = list(stages[0])
    per_stage = {f"layer{l}/{s}": round(statistics.median(st[(l, s)] for st in stages), 4) for l, s in keys}
    draw = [sum(v for (l, s), v in st.items() if s != "read+extract+rank+maps") for st in stages]
    whole = [sum(st.values()) for st in stages]
    native = all(tr.executor is not None and tr.executor.supports(*b) for b in batches)
    tr.step(*batches[0])  # warm-up: workspaces, the GEMM plans
    t_steps, _ = wall_ms(lambda: [tr.step(*b) for b in batches])

    def both():
        for b, q in enumerate(chunks[args.warmup:]):
            tr.step(*ls.sample(q, 2000 + b))

    t_both, _ = wall_ms(both)
    shapes = [[[a.shape[0], a.shape[1], a.nnz] for a in b.adjs] for b in batches]
    med_shape = [[int(statistics.median(s[k][i] for s in shapes)) for i in range(3)] for k in range(len(ORDERS))]
    # the native host draw, one thread, the same batch nodes
    host = []
    none, zero = np.full(N, -1), np.zeros(N, np.int64)
    for b, q in enumerate(chunks[: args.warmup + min(args.batches, 10)]):
        t0 = time.perf_counter()
        sampler.ladies_sample_host(3 + b, np.sort(q), np.array([args.samp_num] * 5), N, lap, labels, ORDERS, none, zero,
                                   None, 1.0, [0])
        if b >= args.warmup:
            host.append((time.perf_counter() - t0) * 1e3)
    case = {"graph": spec.name, "N": N, "nnz": int(lap.nnz), "F": F, "orders": ORDERS, "samp_num": args.samp_num,
            "batch_size": args.batch_size, "native_step": bool(native),
            "stage_gpu_ms_median": per_stage,
            "draw_gpu_ms": spread(draw), "draw_and_extract_gpu_ms": spread(whole), "sample_wall_ms": spread(wall),
            "median_layer_shapes_M_K_nnz_bottom_up": med_shape,
            "step_only_ms": round(t_steps / len(batches), 3),
            "step_only_per_s": round(len(batches) / (t_steps * 1e-3), 1),
            "sample_then_step_per_s": round(len(batches) / (t_both * 1e-3), 1),
            "host_native_draw_ms_one_thread": spread(host)}
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="reddit,products")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--samp-num", type=int, default=8192)
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("layerwise_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    out = {"probe": "layerwise", "label": args.label, "device": torch.cuda.get_device_name(0), "batches": args.batches,
           "warmup": args.warmup, "cases": []}
    for name in args.graphs.split(","):
        out["cases"].append(probe(name, args, dev))
        line = json.dumps(out)
        if args.out:  # after every graph: a later one running out of time loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
