"""What X0 costs when the device draw's feature table is placed, not resident (MI355X; needs the
GPU, no fallback).

Geometry: the Reddit-shaped synthetic graph of ``bench.py`` (233 k nodes, 602 features), the input
nodes of neighbour-sampled batches of 512 at fanouts (25, 10) and (10, 10, 10), as
``scripts/neighbor_probe.py`` draws them. Per case, per table dtype (fp32, fp16) and per buffer
fraction (1.0, 0.5, 0.1, 0: the hottest rows of ``placement.create_buffer`` in this GPU's buffer,
the rest in the registered host table):

* ``PlacedFeatures.gather`` (gnn_gather_placed_f32) on the batches' input nodes, timed by HIP
  events around the call, against ``gnn_gather_rows_f32`` / ``_h16_f32`` on the same ids from the
  whole table resident on the device — the two interleaved, ``--rounds`` rounds over ``--batches``
  batches in this one process (a third call in the same rounds leaves the per-source tally out);
  medians, minima and the ratio of the medians;
* rows and bytes per source (``counts()``), and the host share's bytes over the gather's time.

Then, at fraction 0.1 and fp32: drawing and stepping in turn on the one stream over the placed
store and over the resident table (``Trainer.step``, GraphSAGE, 512 outputs per linear).

    python scripts/placed_probe.py [--batches 5] [--rounds 7] [--graph reddit] [--out FILE]
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
from gnn_amd import custom_sparse_ops as cso  # noqa: E402
from gnn_amd import graphs, placement, staging  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.neighbor import NeighborSampler  # noqa: E402
from gnn_amd.placed import PlacedFeatures  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402

CASES = [((25, 10), [1, 1]), ((10, 10, 10), [1, 1, 1])]
FRACTIONS = [1.0, 0.5, 0.1, 0.0]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20, help="draw-then-step pairs at fraction 0.1")
    ap.add_argument("--graph", default="reddit", choices=["reddit", "tiny"])
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("placed_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    spec = {"reddit": graphs.REDDIT, "tiny": graphs.TINY}[args.graph]
    A, labels, feats, ncls, train, _, _ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N, F = A.shape[0], int(feats.shape[1])
    print(f"graph {spec.name}: N={N} nnz={lap.nnz}", file=sys.stderr, flush=True)
    out = {"probe": "placed", "label": args.label, "graph": spec.name, "N": N, "nnz": int(lap.nnz), "F": F,
           "batch_size": args.batch_size, "batches": args.batches, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "cases": []}
    tables = {"fp32": feats, "fp16": feats.to(torch.float16)}
    resident = {}
    for fan, orders in CASES:
        ns = NeighborSampler(lap, list(fan), orders, resident.get("fp32", feats), labels, dev)
        resident["fp32"] = ns.feats
        if "fp16" not in resident:
            resident["fp16"] = NeighborSampler(lap, list(fan), orders, tables["fp16"], labels, dev).feats
        rng = np.random.default_rng(0)
        chunks = [rng.choice(train, args.batch_size, replace=False) for _ in range(max(args.batches, args.steps))]
        ids = [ns.sample(q, 1000 + b).input_nodes for b, q in enumerate(chunks[: args.batches])]
        rows = [int(i.numel()) for i in ids]
        case = {"fanouts": list(fan), "orders": orders, "input_rows": rows, "gathers": []}
        # the hottest rows first: create_buffer's order on one device is argsort(-sample_prob)
        hot = placement.create_buffer(lap, train, N, [0], len(orders), alpha=0).gpu_buffer_group[0]
        for name, table in tables.items():
            esz = table.element_size()
            res = resident[name]
            for frac in FRACTIONS:
                k = int(frac * N)
                pl = placement.Placement([np.where(np.isin(np.arange(N), hot[:k]), 0, -1)], [_slots(N, hot[:k])],
                                         [hot[:k]], 0, np.zeros(1))
                store = staging.FeatureStore(table, pl.gpu_buffer_group[0], dev, 0)
                pf = PlacedFeatures.from_store(store, pl, 0)
                x0 = [torch.empty((n, staging.padded_ld(F, 32)), dtype=torch.float32, device=dev)[:, :F] for n in rows]
                ids32 = [i.to(torch.int32) for i in ids]
                for i, x in zip(ids, x0):  # warm-up, and the rows are the resident gather's
                    ref = torch.empty_like(x)
                    cso.gather_rows(res, i, ref, None)
                    if not torch.equal(pf.gather(i, out=x), ref):
                        sys.exit(f"placed_probe: {name} fraction {frac}: rows differ from the resident table's")
                pf.check()
                pf.reset_counts()
                ev_p, ev_r, ev_n = [], [], []
                for _ in range(args.rounds):
                    for i, i32, x in zip(ids, ids32, x0):
                        ev_p.append(timed(lambda: pf.gather(i32, out=x)))
                        ev_r.append(timed(lambda: cso.gather_rows(res, i, x, None)))
                        ev_n.append(timed(lambda: pf.gather(i32, out=x, count=False)))  # without the tally
                torch.cuda.synchronize()
                tp = [a.elapsed_time(b) for a, b in ev_p]
                tr_ = [a.elapsed_time(b) for a, b in ev_r]
                tn = [a.elapsed_time(b) for a, b in ev_n]
                c = pf.counts()
                per = args.rounds
                host_bytes = c["host"] // per * F * esz
                rec = {"dtype": name, "fraction": frac, "buffer_rows": k,
                       "rows_per_pass": {"own": c["own"] // per, "host": c["host"] // per},
                       "bytes_per_pass": {"own": c["own"] // per * F * esz, "host": host_bytes},
                       "placed_ms": spread(tp), "resident_ms": spread(tr_), "placed_uncounted_ms": spread(tn),
                       "ratio_of_medians": round(statistics.median(tp) / statistics.median(tr_), 3),
                       # per batch: the host rows' bytes over the whole gather's time
                       "host_GBps": round(host_bytes / len(ids) / (statistics.median(tp) * 1e-3) / 1e9, 2)}
                print(json.dumps(rec), file=sys.stderr, flush=True)
                case["gathers"].append(rec)
                if name == "fp32" and frac == 0.1:
                    case["draw_then_step"] = draw_then_step(args, lap, fan, orders, pf, res, labels, ncls, F, chunks, dev)
                    print(json.dumps(case["draw_then_step"]), file=sys.stderr, flush=True)
                pf.close()
                del pf, store, x0
        out["cases"].append(case)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _slots(N, nodes):
    idx = np.arange(N)
    idx[nodes] = np.arange(len(nodes))
    return idx


def draw_then_step(args, lap, fan, orders, pf, res, labels, ncls, F, chunks, dev):
    """Steps per second of sample-then-step on the one stream, over the placed store and over the
    resident table, the two alternating twice in this process."""
    out = {}
    samplers = {"placed": NeighborSampler(lap, list(fan), orders, pf, labels, dev),
                "resident": NeighborSampler(lap, list(fan), orders, res, labels, dev)}
    torch.manual_seed(0)
    model = build_model("graphsage", F, args.nhid, orders, ncls, 0.1, fused=True).to(dev)
    tr = Trainer(model, 0.01, dev)
    qs = chunks[: args.steps]
    for name, ns in samplers.items():
        tr.step(*ns.sample(qs[0], 1))  # warm-up: workspaces, the GEMM plans
    rates = {"placed": [], "resident": []}
    for _ in range(2):
        for name, ns in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b, q in enumerate(qs):
                tr.step(*ns.sample(q, 2000 + b))
            torch.cuda.synchronize()
            rates[name].append(round(len(qs) / (time.perf_counter() - t0), 1))
    pf.check()
    out["fraction"] = 0.1
    out["steps"] = len(qs)
    out["per_s"] = rates
    return out


if __name__ == "__main__":
    main()
