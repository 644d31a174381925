"""What the locality-skewed LADIES draw (gnn_lw_race_skew, scale_factor > 1) buys over a placed feature
store and what it costs in the race (MI355X; needs the GPU, no fallback).

Geometry: the Reddit-shaped synthetic graph of ``bench.py``, GraphSAGE, orders [1, 1, 1], samp 8192,
batches of 512, the fp32 table placed by ``placement.create_buffer`` at buffer fractions 0.1 and
0.5 (this GPU's buffer and the registered host table). The favoured sets are
``placement.get_skewed_sampled_nodes`` of that placement, one per layer, as the reference hands
them to its sampler. Scales 1, 2, 4, 8 and 16, one ``LayerwiseSampler`` each over the one store,
interleaved batch by batch in this one process; scale 1 is the plain race of the same run, the
figure every other scale is read beside. Per fraction and scale, over ``--batches`` batches after
``--warmup``:

* ``counts()``'s own / host rows per batch (the buffer's hit rate of X0);
* the race's time per layer, between the HIP events of ``LayerwiseSampler.trace``;
* the X0 gather (``PlacedFeatures.gather`` on the batch's input nodes) between HIP events;
* then drawing and stepping in turn on the one stream (``Trainer.step``), the scales alternating
  twice: batches per second.

    python scripts/skew_probe.py [--batches 12] [--fractions 0.1,0.5] [--out profiles/skew/skew_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_amd import graphs, placement, staging  # noqa: E402
from gnn_amd.layerwise import LayerwiseSampler  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.placed import PlacedFeatures  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402

SPECS = {"reddit": graphs.REDDIT, "tiny": graphs.TINY}
ORDERS = [1, 1, 1]
SCALES = [1, 2, 4, 8, 16]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def race_ms(trace):
    """{layer: ms} of one batch's trace: from the mark before the race to the mark after it."""
    out, prev = {}, {}
    for layer, stage, ev in trace:
        if stage == "race":
            out[layer] = prev[layer].elapsed_time(ev)
        prev[layer] = ev
    return out


def probe(frac, args, lap, A, feats, labels, ncls, train, dev):
    N, F = lap.shape[0], int(feats.shape[1])
    pl = placement.create_buffer(lap, train, int(frac * N), [0], len(ORDERS), alpha=0)
    skew = placement.get_skewed_sampled_nodes(A + sp.eye(N, dtype=A.dtype, format="csr"), pl.gpu_buffer_group, ORDERS)
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
    pf = PlacedFeatures.from_store(store, pl, 0)
    samplers = {s: LayerwiseSampler(lap, args.samp_num, ORDERS, pf, labels, dev, scale_factor=s,
                                    skewed_sampling_nodes=skew) for s in SCALES}
    rng = np.random.default_rng(0)
    chunks = [rng.choice(train, args.batch_size, replace=False) for _ in range(args.warmup + args.batches)]
    rows = {s: {"own": [], "host": [], "input": []} for s in SCALES}
    race = {s: {l: [] for l in range(len(ORDERS))} for s in SCALES}
    gather = {s: [] for s in SCALES}
    for b, q in enumerate(chunks):
        for s, ls in samplers.items():
            pf.reset_counts()
            ls.trace = []
            batch = ls.sample(q, 1000 + b)
            c = pf.counts()  # one read: the batch's kernels have ended
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pf.gather(batch.input_nodes, out=batch.x0, count=False)
            e1.record()
            torch.cuda.synchronize()
            if b >= args.warmup:
                rows[s]["own"].append(c["own"])
                rows[s]["host"].append(c["host"])
                rows[s]["input"].append(c["total"])
                for l, ms in race_ms(ls.trace).items():
                    race[s][l].append(ms)
                gather[s].append(e0.elapsed_time(e1))
            ls.trace = None
    pf.check()
    torch.manual_seed(0)
    model = build_model("graphsage", F, args.nhid, ORDERS, ncls, 0.1, fused=True).to(dev)
    tr = Trainer(model, 0.01, dev)
    qs = chunks[args.warmup:]
    for ls in samplers.values():
        tr.step(*ls.sample(qs[0], 1))  # warm-up: workspaces, the GEMM plans
    rates = {s: [] for s in SCALES}
    for _ in range(2):
        for s, ls in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b, q in enumerate(qs):
                tr.step(*ls.sample(q, 2000 + b))
            torch.cuda.synchronize()
            rates[s].append(round(len(qs) / (time.perf_counter() - t0), 1))
    pf.check()
    pf.close()
    case = {"fraction": frac, "buffer_rows": int(frac * N), "favoured_per_layer": [int(len(x)) for x in skew], "scales": []}
    for s in SCALES:
        own, host = statistics.mean(rows[s]["own"]), statistics.mean(rows[s]["host"])
        rec = {"scale": s, "input_rows_mean": round(statistics.mean(rows[s]["input"]), 1), "own_rows_mean": round(own, 1),
               "host_rows_mean": round(host, 1), "own_share": round(own / max(own + host, 1), 4),
               "race_ms_by_layer": {f"layer{l}": spread(v) for l, v in race[s].items()},
               "race_ms_sum_of_medians": round(sum(statistics.median(v) for v in race[s].values()), 4),
               "x0_gather_ms": spread(gather[s]), "draw_then_step_per_s": rates[s]}
        print(json.dumps(rec), file=sys.stderr, flush=True)
        case["scales"].append(rec)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="reddit", choices=list(SPECS))
    ap.add_argument("--fractions", default="0.1,0.5")
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--samp-num", type=int, default=8192)
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("skew_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    spec = SPECS[args.graph]
    t0 = time.perf_counter()
    A, labels, feats, ncls, train, _, _ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    print(f"graph {spec.name}: N={A.shape[0]} nnz={lap.nnz} ({time.perf_counter() - t0:.0f} s)", file=sys.stderr, flush=True)
    out = {"probe": "skew", "label": args.label, "graph": spec.name, "N": int(A.shape[0]), "nnz": int(lap.nnz),
           "F": int(feats.shape[1]), "orders": ORDERS, "samp_num": args.samp_num, "batch_size": args.batch_size,
           "batches": args.batches, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "cases": []}
    for frac in (float(x) for x in args.fractions.split(",")):
        out["cases"].append(probe(frac, args, lap, A, feats, labels, ncls, train, dev))
        line = json.dumps(out)
        if args.out:  # after every fraction: a later one running out of time loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
