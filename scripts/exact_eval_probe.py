"""What exact full-neighbourhood evaluation costs (MI355X; needs the GPU, no fallback).

Geometry: config 2 (Reddit-shaped graph, GraphSAGE nhid 256 per half, orders 1,1). One model, one
box, the variants interleaved per round after a warm-up round; every time is a host clock around
work that ends in a device synchronisation, the per-phase times HIP events around the engine's own
phases (ExactInference.timing). The machine is shared: median, min and max over the rounds.

  (a) exact      Trainer.evaluate_exact scoring the validation nodes (the engine runs over ALL
                 nodes whatever is scored) from the host table, upload included, and
                 exact_resident from a table already on the device in whole-line rows; per layer
                 the time in products / aggregation / tails (resident table)
  (b) one_shot   the same model scored by model.forward_loss on the one-shot full operand (a
                 CsrOperand of the whole lap, x[arange(N)]), where it fits
  (c) sampled    Trainer.evaluate over loader.sequential LADIES batches of the same nodes, producer
                 included (the route every reported number takes today)
  (d) sweep      embed() under max_nnz x max_rows: where the defaults come from
  (e) order      layer 0 forced project-first / aggregate-first (602 -> 256): its phase times

    python scripts/exact_eval_probe.py [--rounds 5] [--graph reddit] [--out FILE]
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
from gnn_amd import graphs, loader, placement, staging  # noqa: E402
from gnn_amd.inference import ExactInference  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def phases(eng, feats):
    """One embed with the engine's phase events on: {layer: {phase: ms}} and the total."""
    eng.timing = []
    ms, _ = wall_ms(lambda: eng.embed(feats))
    out = {}
    for li, name, e0, e1 in eng.timing:
        d = out.setdefault(str(li), {})
        d[name] = d.get(name, 0.0) + e0.elapsed_time(e1)
    eng.timing = None
    return ms, {k: {p: round(v, 3) for p, v in d.items()} for k, d in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "tiny"])
    ap.add_argument("--nhid", type=int, default=256)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exact_eval_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    spec = graphs.REDDIT if args.graph == "reddit" else graphs.TINY
    samp, bs = (8192, 512) if args.graph == "reddit" else (256, 64)
    A, labels, feats, ncls, train, valid, _ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N, F = A.shape[0], int(feats.shape[1])
    orders = [1, 1]
    torch.manual_seed(0)
    model = build_model("graphsage", F, args.nhid, orders, ncls, 0.1, fused=True).to(dev)
    tr = Trainer(model, 0.01, dev)
    y_valid = torch.from_numpy(np.asarray(labels[valid].todense(), dtype=np.float32))
    out = {"probe": "exact_eval", "label": args.label, "graph": spec.name, "N": N, "nnz": int(lap.nnz), "F": F,
           "nhid": args.nhid, "orders": orders, "scored_nodes": int(len(valid)), "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "order": "exact, one_shot, sampled per round; 1 warm-up round dropped"}

    # (b) the one-shot full operand
    deg = np.diff(lap.indptr)
    with np.errstate(divide="ignore"):
        val = np.repeat((1.0 / deg.astype(np.float64)).astype(np.float32), deg)
    t = lambda a: torch.from_numpy(a).to(dev)
    full = cso.CsrOperand(t(lap.indptr.astype(np.int32)), t(lap.indices.astype(np.int32)), t(val), (N, N))
    x_dev = torch.zeros((N, staging.padded_ld(F)), device=dev)[:, :F]  # whole-line rows, resident
    x_dev.copy_(feats)
    ar = torch.arange(N, device=dev)
    vidx = t(np.asarray(valid, dtype=np.int64))
    y_dev = y_valid.to(dev)

    def one_shot():
        model.eval()
        with torch.no_grad():
            z = model(x_dev, [full] * len(orders), [ar] * len(orders))[vidx]
            return float(torch.nn.functional.binary_cross_entropy_with_logits(z, y_dev, reduction="sum") / len(valid))

    # (c) the sampled route
    pl = placement.create_buffer(lap, train, int(0.1 * N), [0], 3, alpha=0)
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
    ld = loader.NativeLoader(lap, labels, train, samp, bs, orders, pl.device_id_of_nodes_group[0],
                             pl.idx_of_nodes_on_device_group[0], store=store, workers=args.workers, seed=0,
                             device_extract=True)
    stager = staging.Stager(store)

    def sampled():
        def batches():
            for lb in ld.sequential(valid):
                staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
                x0 = staged.wait()
                yield x0, staged.adjs, staged.batch.sampled_nodes, staged.batch.labels
        return tr.evaluate(batches())

    res = {"exact": [], "exact_resident": [], "one_shot": [], "sampled": []}
    last = {}
    try:
        for r in range(args.rounds + 1):
            for name, fn in (("exact", lambda: tr.evaluate_exact(lap, feats, valid, y_valid)),
                             ("exact_resident", lambda: tr.evaluate_exact(lap, x_dev, valid, y_valid)),
                             ("one_shot", one_shot), ("sampled", sampled)):
                try:
                    ms, v = wall_ms(fn)
                except torch.cuda.OutOfMemoryError:
                    last[name] = "does not fit"
                    continue
                if r:
                    res[name].append(ms)
                last[name] = v
    finally:
        ld.close()
    out["wall_ms"] = {k: spread(v) for k, v in res.items() if v}
    out["results"] = {k: (v if not isinstance(v, dict) else {a: round(b, 6) if isinstance(b, float) else b
                                                             for a, b in v.items()}) for k, v in last.items()}
    eng = tr._exact[1]
    out["blocks_default"] = len(eng.blocks)
    out["orders_taken"] = eng.orders_taken
    out["memory_needed_bytes"] = eng.memory_needed(feats)
    phases(eng, x_dev)  # warm
    out["exact_phases_ms"] = [phases(eng, x_dev) for _ in range(3)]

    # (d) block-size sweep, interleaved
    grid = [(mn, mr) for mn in (1 << 20, 1 << 22, 1 << 24, 1 << 26) for mr in (1 << 12, 1 << 14, 1 << 16, 1 << 18)]
    engines = {g: ExactInference(model, lap, dev, max_nnz=g[0], max_rows=g[1]) for g in grid}
    sweep = {g: [] for g in grid}
    for r in range(args.rounds + 1):
        for g, e in engines.items():
            ms, _ = wall_ms(lambda: e.embed(x_dev))
            if r:
                sweep[g].append(ms)
    out["sweep_embed_ms"] = [{"max_nnz": g[0], "max_rows": g[1], "blocks": len(engines[g].blocks), **spread(v)}
                             for g, v in sweep.items()]

    # (e) layer 0 either way
    order = {"project": [], "aggregate": []}
    for r in range(args.rounds + 1):
        for name in order:
            eng.force_order = name
            ms, ph = phases(eng, x_dev)
            if r:
                order[name].append({"embed_ms": round(ms, 3), "layer0": ph["0"]})
    eng.force_order = None
    out["layer0_order"] = {k: {"layer0_total_ms": spread([sum(x["layer0"].values()) for x in v]), "last": v[-1]}
                           for k, v in order.items()}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
