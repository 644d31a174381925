"""What the native step buys for models with order-0 (dense) layers (MI355X; needs the GPU).

The reference's ``--orders`` (main.py:41) with zeros, e.g. 1,0,1,0 — a common way to run LADIES —
builds layers without an aggregation (models.py:17-21, 59-60). Trainer runs such a model through
the native step executor (gnn_train_step_f32, GNN_SL_DENSE) when the library takes it, and through
the Python autograd path otherwise; a tree whose executor refuses order-0 layers falls back on its
own, so THE SAME SCRIPT run there is the baseline.

Geometry: config 2 (Reddit-shaped graph, GraphSAGE nhid 512, LADIES samp 8192, batch 512, buffer
0.1 N). Per orders (default 1,0,1,0 and 1,1,0) the same seeded batches are staged once through the
native loader and the native staging call, then Trainer.step is driven over them, window by
window:

  ms_per_step        HIP events around a window of back-to-back steps / its steps
  host_issue_ms      host wall time of one Trainer.step call issued onto an idle device (a
                     synchronisation before each call, none inside it), mean over the batches:
                     what the host spends issuing a step, free of queue back-pressure

Where the executor takes the model, each window is run twice, alternating: through the executor
("native") and with ``tr.executor = None`` ("python", the autograd path of this same tree), on two
trainers with the same initial weights. The machine is shared, so a difference means something
only against the spread of the windows: median, min and max are reported, after two warm-up
rounds. One JSON line; no threshold.

    python scripts/orders_probe.py [--orders 1,0,1,0 1,1,0] [--windows 7] [--batches 8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_amd import graphs, loader, placement, staging  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", nargs="+", default=["1,0,1,0", "1,1,0"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batches", type=int, default=8, help="distinct pre-staged batches per window")
    ap.add_argument("--rounds", type=int, default=4, help="passes over the batches per window")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "tiny"])
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--label", default="", help="free text kept in the record (which tree this is)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("orders_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    spec = graphs.REDDIT if args.graph == "reddit" else graphs.TINY
    samp, bs = (8192, 512) if args.graph == "reddit" else (256, 64)
    A, labels, feats, ncls, train, *_ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N, F = A.shape[0], int(feats.shape[1])
    pl = placement.create_buffer(lap, train, int(0.1 * N), [0], 3, alpha=0)
    store = staging.FeatureStore(feats, pl.gpu_buffer_group[0], dev, 0)
    out = {"probe": "orders", "label": args.label, "graph": spec.name, "samp": samp, "batch": bs, "nhid": args.nhid,
           "F": F, "windows": args.windows, "batches": args.batches, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "order": "native, python alternating per window where both exist; 2 warm-up rounds dropped",
           "results": {}}
    for spec_orders in args.orders:
        orders = [int(o) for o in spec_orders.split(",")]
        ld = loader.NativeLoader(lap, labels, train, samp, bs, orders, pl.device_id_of_nodes_group[0],
                                 pl.idx_of_nodes_on_device_group[0], store=store, workers=args.workers, seed=0,
                                 device_extract=True)
        try:
            stager = staging.Stager(store)
            items = []
            for _, lb in zip(range(args.batches), ld.epoch(1)):
                staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
                x0 = staged.wait()
                items.append((lb, staged, x0))
            torch.cuda.synchronize()
        finally:
            ld.close()
        trainers = {}
        for path in ("native", "python"):
            torch.manual_seed(0)
            net = build_model("graphsage", F, args.nhid, orders, ncls, 0.1, fused=True).to(dev)
            tr = Trainer(net, 0.01, dev)
            if path == "python":
                tr.executor = None
            elif tr.executor is None or not all(
                    tr.executor.supports(x0, st.adjs, st.batch.sampled_nodes, st.batch.labels) for _, st, x0 in items):
                continue  # this tree's executor does not take the model: only its Python path exists
            trainers[path] = tr
        res = {p: {"ms_per_step": [], "host_issue_ms": []} for p in trainers}
        losses = {}
        for w in range(args.windows + 2):  # two warm-up rounds
            for path, tr in trainers.items():
                torch.manual_seed(1000 + w)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                n = 0
                e0.record()
                for _ in range(args.rounds):
                    for _, staged, x0 in items:
                        db = staged.batch
                        loss = tr.step(x0, staged.adjs, db.sampled_nodes, db.labels)
                        n += 1
                e1.record()
                torch.cuda.synchronize()
                losses[path] = float(loss)
                host = 0.0
                for _, staged, x0 in items:
                    db = staged.batch
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.step(x0, staged.adjs, db.sampled_nodes, db.labels)
                    host += time.perf_counter() - t0
                torch.cuda.synchronize()
                if w >= 2:
                    res[path]["ms_per_step"].append(e0.elapsed_time(e1) / n)
                    res[path]["host_issue_ms"].append(host * 1e3 / len(items))
        rows = [int(x0.shape[0]) for _, _, x0 in items]
        r = {"paths": list(trainers), "input_rows_median": int(statistics.median(rows)),
             "layers": [None if a is None else [int(a.shape[0]), int(a.shape[1]), int(a.nnz)] for a in items[0][1].adjs],
             "last_loss": {p: round(v, 6) for p, v in losses.items()},
             **{k: {p: spread(res[p][k]) for p in trainers} for k in ("ms_per_step", "host_issue_ms")}}
        if len(trainers) == 2:
            r["native_over_python_median"] = {
                k: round(r[k]["native"]["median"] / r[k]["python"]["median"], 4) for k in ("ms_per_step", "host_issue_ms")}
        out["results"][spec_orders] = r
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
