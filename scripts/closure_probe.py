"""What closure-scope exact inference costs against the full-graph scope (MI355X; needs the GPU,
no fallback).

Geometry: the products-shaped synthetic graph of ``bench.py --graph products`` (2.4 M nodes, ~50
entries a row), GraphSAGE with 3 aggregating layers (nhid 256 per half), the feature table
resident on the device in whole-line rows. For each query-set size |Q| in {512, 8192, 65536}
(random nodes): the sizes of the closure's levels, the time to build the closure
(ExactInference.closure: the set kernels, the host copies, the plan), the time of
``embed(feats, closure)`` and, interleaved with it on the same box, the time of the full-graph
``embed(feats)``. One warm-up round is dropped; every time is a host clock around work that ends
in a device synchronisation; median, min and max over the rounds (the machine is shared). The
crossover between the scopes is recorded, not acted on: there is no scope="auto".

    python scripts/closure_probe.py [--rounds 4] [--graph products] [--out FILE]
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
from gnn_amd import graphs, staging  # noqa: E402
from gnn_amd.inference import ExactInference  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--graph", default="products", choices=["products", "reddit", "tiny"])
    ap.add_argument("--nhid", type=int, default=256)
    ap.add_argument("--queries", type=int, nargs="+", default=[512, 8192, 65536])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("closure_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    spec = {"products": graphs.PRODUCTS, "reddit": graphs.REDDIT, "tiny": graphs.TINY}[args.graph]
    A, _, feats, ncls, _, _, _ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N, F = A.shape[0], int(feats.shape[1])
    orders = [1, 1, 1]
    torch.manual_seed(0)
    model = build_model("graphsage", F, args.nhid, orders, ncls, 0.1, fused=True).to(dev).eval()
    print(f"graph {spec.name}: N={N} nnz={lap.nnz}", file=sys.stderr, flush=True)
    eng = ExactInference(model, lap, dev)
    x_dev = torch.zeros((N, staging.padded_ld(F)), device=dev)[:, :F]  # whole-line rows, resident
    x_dev.copy_(feats)
    out = {"probe": "closure", "label": args.label, "graph": spec.name, "N": N, "nnz": int(lap.nnz), "F": F,
           "nhid": args.nhid, "orders": orders, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "order": "per round and |Q|: closure build, closure embed, full-graph embed; 1 warm-up round dropped",
           "memory_needed_graph_bytes": eng.memory_needed(x_dev), "cases": []}
    rng = np.random.default_rng(0)
    queries = [rng.choice(N, min(q, N), replace=False) for q in args.queries]
    times = [{"build": [], "closure": [], "graph": []} for _ in queries]
    closures = [None] * len(queries)
    for r in range(args.rounds + 1):
        for i, q in enumerate(queries):
            ms_b, c = wall_ms(lambda: eng.closure(q))
            ms_c, emb = wall_ms(lambda: eng.embed(x_dev, closure=c))
            assert emb.shape[0] == c.sizes[-1]
            del emb
            ms_g, full = wall_ms(lambda: eng.embed(x_dev))
            del full
            closures[i] = c
            print(f"round {r} |Q|={len(q)}: levels {c.sizes} build {ms_b:.1f} closure {ms_c:.1f} graph {ms_g:.1f} ms",
                  file=sys.stderr, flush=True)
            if r:
                times[i]["build"].append(ms_b)
                times[i]["closure"].append(ms_c)
                times[i]["graph"].append(ms_g)
    for q, c, t in zip(queries, closures, times):
        out["cases"].append({"queries": int(len(q)), "level_sizes_bottom_to_top": c.sizes,
                             "level_entries": [None if s is None else int(s[-1]) for s in c.scans],
                             "blocks": [None if b is None else len(b) for b in c.blocks],
                             "memory_needed_closure_bytes": eng.memory_needed(x_dev, closure=c),
                             "closure_build_ms": spread(t["build"]), "closure_embed_ms": spread(t["closure"]),
                             "graph_embed_ms": spread(t["graph"])})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
