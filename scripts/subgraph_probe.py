"""What a device-drawn subgraph-sampler batch (gnn_amd.subgraph: one race over the batch rows, one
square operand for every layer below) costs, stage by stage, how fast the training step runs over
its batches, and — in the same run on the same box — the device LADIES draw (gnn_amd.layerwise) of
the same batch nodes beside it (MI355X; needs the GPU, no fallback).

Geometry: BASELINE config 2 (the Reddit-shaped graph, GraphSAGE, orders [1, 1, 1], samp 8192,
batch 512) and the products-shaped graph of ``gnn_amd.graphs`` with the same sampler settings; the
feature table resident on the device. Per graph, over ``--batches`` distinct batches after
``--warmup`` warm-up batches: the GPU time of every stage between HIP events on the stream (medians;
``sg_count`` is gnn_sg_count on its own), the wall time of ``sample`` (host clock around work that
ends synchronised; it includes the one read per batch, the allocations and the Python between
launches), ``Trainer.step`` over the batches already drawn, and drawing and stepping in turn on one
stream (no producer thread: nothing overlaps). The two samplers are different estimators — LADIES
draws anew at every layer, the subgraph sampler once — so their batch shapes differ by design.

    python scripts/subgraph_probe.py [--graphs reddit,products] [--batches 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_amd import graphs  # noqa: E402
from gnn_amd.layerwise import LayerwiseSampler  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.subgraph import SubgraphSampler  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402
from layerwise_probe import ORDERS, SPECS, spread, stage_ms, wall_ms  # noqa: E402

EXTRACT = ("read+extract+rank+maps", "read+extract_top+rank+maps", "extract_square")


def measure(smp, tr, chunks, args):
    """One sampler over the chunks: stage medians, draw / whole GPU time, wall time, step rates, shapes."""
    wall, stages, batches = [], [], []
    for b, q in enumerate(chunks):
        smp.trace = []
        t, batch = wall_ms(lambda: smp.sample(q, 1000 + b))
        if b >= args.warmup:
            wall.append(t)
            stages.append(stage_ms(smp.trace))
            batches.append(batch)
    smp.trace = None
    per_stage = {f"layer{l}/{s}": round(statistics.median(st[(l, s)] for st in stages), 4) for l, s in stages[0]}
    draw = [sum(v for (l, s), v in st.items() if s not in EXTRACT) for st in stages]
    whole = [sum(st.values()) for st in stages]
    native = all(tr.executor is not None and tr.executor.supports(*b) for b in batches)
    tr.step(*batches[0])  # warm-up: workspaces, the GEMM plans
    t_steps, _ = wall_ms(lambda: [tr.step(*b) for b in batches])

    def both():
        for b, q in enumerate(chunks[args.warmup:]):
            tr.step(*smp.sample(q, 2000 + b))

    t_both, _ = wall_ms(both)
    shapes = [[[a.shape[0], a.shape[1], a.nnz] for a in b.adjs] for b in batches]
    med_shape = [[int(statistics.median(s[k][i] for s in shapes)) for i in range(3)] for k in range(len(ORDERS))]
    return {"native_step": bool(native), "stage_gpu_ms_median": per_stage, "draw_gpu_ms": spread(draw),
            "draw_and_extract_gpu_ms": spread(whole), "sample_wall_ms": spread(wall),
            "median_layer_shapes_M_K_nnz_bottom_up": med_shape,
            "median_input_rows": int(statistics.median(int(b.input_nodes.numel()) for b in batches)),
            "step_only_ms": round(t_steps / len(batches), 3), "step_only_per_s": round(len(batches) / (t_steps * 1e-3), 1),
            "sample_then_step_per_s": round(len(batches) / (t_both * 1e-3), 1)}


def probe(name, args, dev):
    spec = SPECS[name]
    A, labels, feats, ncls, train, _, _ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N, F = A.shape[0], int(feats.shape[1])
    print(f"graph {spec.name}: N={N} nnz={lap.nnz}", file=sys.stderr, flush=True)
    ss = SubgraphSampler(lap, args.samp_num, ORDERS, feats, labels, dev)
    ls = LayerwiseSampler(ss.graph, args.samp_num, ORDERS, ss.feats, labels, dev)  # the same resident graph and table
    rng = np.random.default_rng(0)
    chunks = [rng.choice(train, args.batch_size, replace=False) for _ in range(args.warmup + args.batches)]
    case = {"graph": spec.name, "N": N, "nnz": int(lap.nnz), "F": F, "orders": ORDERS, "samp_num": args.samp_num,
            "batch_size": args.batch_size}
    for key, smp in (("subgraph", ss), ("ladies", ls), ("subgraph_again", ss)):
        torch.manual_seed(0)
        model = build_model("graphsage", F, args.nhid, ORDERS, ncls, 0.1, fused=True).to(dev)
        case[key] = measure(smp, Trainer(model, 0.01, dev), chunks, args)
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
        sys.exit("subgraph_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    out = {"probe": "subgraph", "label": args.label, "device": torch.cuda.get_device_name(0), "batches": args.batches,
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
