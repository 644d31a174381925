"""What a 16-bit feature store changes on the staging path (MI355X; needs the GPU).

The same seeded Reddit-shaped LADIES batches (samp 8192, batch 512, buffer 0.1 N) are produced by
the native loader and staged from an fp32 FeatureStore and from the ``.half()`` of the same
table. One JSON line reports, for each store:

  blob_bytes_per_batch / host_rows_bytes_per_batch   what the producer writes and the H2D moves
  producer_cpu_ms_per_batch                          process CPU time over a window in which only
                                                     the loader's workers run (the training thread
                                                     blocks in gnn_loader_next), per batch
  x0_gather_us                                       HIP-event time of the X0 gather
                                                     (gnn_gather_rows2_f32 / _h16_f32), per batch
  x0_gather_gbs                                      bytes read + written by it over that time

The two stores alternate window by window in one process (the machine is shared: a difference
means something only against the spread of the repeats, so median, min and max are reported). No
threshold: the fp32 store of the same build is the comparison.

    python scripts/feat16_probe.py [--workers 14] [--windows 7] [--producer-batches 48]
                                   [--gather-batches 12] [--out FILE]
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


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=14)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--producer-batches", type=int, default=48, help="batches per producer window")
    ap.add_argument("--gather-batches", type=int, default=12, help="distinct batches per gather window")
    ap.add_argument("--graph", default="reddit", choices=["reddit", "tiny"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("feat16_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    spec = graphs.REDDIT if args.graph == "reddit" else graphs.TINY
    samp, bs = (8192, 512) if args.graph == "reddit" else (256, 64)
    A, labels, feats, _, train, *_ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N = A.shape[0]
    pl = placement.create_buffer(lap, train, int(0.1 * N), [0], 3, alpha=0)
    tables = {"fp32": feats, "fp16": feats.half()}
    stores = {k: staging.FeatureStore(t, pl.gpu_buffer_group[0], dev, 0) for k, t in tables.items()}

    def make_loader(name):
        return loader.NativeLoader(lap, labels, train, samp, bs, [1, 1, 1], pl.device_id_of_nodes_group[0],
                                   pl.idx_of_nodes_on_device_group[0], store=stores[name], workers=args.workers,
                                   prefetch=args.workers, seed=0, device_extract=True)

    # ---- the producers: blob bytes and CPU per batch -------------------------------------
    loaders = {k: make_loader(k) for k in stores}
    its = {k: ld.forever() for k, ld in loaders.items()}
    blob, rows_b, cpu_ms, wall_ms = ({k: [] for k in stores} for _ in range(4))
    try:
        for k in stores:  # warm-up: every worker has produced, the blob pools are at their size
            for _ in range(3 * args.workers):
                next(its[k])
        for _ in range(args.windows):
            for k in stores:  # the other loader's queue is full: its workers sleep
                c0, t0 = time.process_time(), time.perf_counter()
                for _ in range(args.producer_batches):
                    nb = next(its[k]).host
                    blob[k].append(nb.nbytes)
                    rows_b[k].append(nb._count(nb._bb + loader.B_HOST_ROWS) * (2 if nb.desc[loader.H_FEAT_KIND] else 4))
                    del nb
                cpu_ms[k].append((time.process_time() - c0) / args.producer_batches * 1e3)
                wall_ms[k].append((time.perf_counter() - t0) / args.producer_batches * 1e3)
    finally:
        for ld in loaders.values():
            ld.close()

    # ---- the X0 gather: HIP-event time per batch ----------------------------------------
    gathers, checked = {}, {}
    for k, store in stores.items():
        ld = make_loader(k)  # same seed: the same batches for both stores
        try:
            nbs = [lb.host for _, lb in zip(range(args.gather_batches), ld.epoch(1))]
        finally:
            ld.close()
        items, moved = [], 0
        for nb in nbs:
            own_pos, own_src, host_pos, host_dev = nb.stage_views(dev)
            x0 = torch.empty((nb.num_input_nodes, store.ld), dtype=torch.float32, device=dev)
            items.append((own_src, own_pos, int(own_pos.numel()), host_dev, host_pos, int(host_pos.numel()), x0))
            n = int(own_pos.numel()) + int(host_pos.numel())
            moved += n * (store.ld * store.gpu_buffer.element_size() + store.ld * 4 + 16)
        gathers[k] = (store, nbs, items, moved / len(nbs))
        # the staged X0 is the table widened, bit for bit (first batch)
        own_src, own_pos, n_own, host_dev, host_pos, nh, x0 = items[0]
        cso.gather_rows2(store.gpu_buffer, own_src, own_pos, n_own, host_dev, None, host_pos, nh, x0)
        nodes = torch.from_numpy(np.asarray(nbs[0].input_nodes, np.int64))
        checked[k] = bool(torch.equal(x0[:, :store.F].cpu(), tables[k].float()[nodes]))
    gather_us = {k: [] for k in stores}
    for w in range(args.windows + 2):  # two warm-up rounds
        for k, (store, _, items, _) in gathers.items():
            evs = []
            for own_src, own_pos, n_own, host_dev, host_pos, nh, x0 in items:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                cso.gather_rows2(store.gpu_buffer, own_src, own_pos, n_own, host_dev, None, host_pos, nh, x0)
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            if w >= 2:
                gather_us[k].append(sum(a.elapsed_time(b) for a, b in evs) / len(evs) * 1e3)

    out = {
        "probe": "feat16", "graph": spec.name, "samp": samp, "batch": bs, "workers": args.workers,
        "windows": args.windows, "producer_batches": args.producer_batches, "gather_batches": args.gather_batches,
        "device": torch.cuda.get_device_name(0),
        "x0_bit_equal_to_table": checked,
        "ld_x0": stores["fp32"].ld, "ld_rows": {k: s.ld_rows for k, s in stores.items()},
        "blob_bytes_per_batch": {k: int(statistics.mean(v)) for k, v in blob.items()},
        "host_rows_bytes_per_batch": {k: int(statistics.mean(v)) for k, v in rows_b.items()},
        "producer_cpu_ms_per_batch": {k: spread(v) for k, v in cpu_ms.items()},
        "producer_wall_ms_per_batch": {k: spread(v) for k, v in wall_ms.items()},
        "x0_gather_us": {k: spread(v) for k, v in gather_us.items()},
        "x0_gather_bytes_per_batch": {k: int(g[3]) for k, g in gathers.items()},
        "x0_gather_gbs": {k: round(gathers[k][3] / (statistics.median(v) * 1e-6) / 1e9, 1)
                          for k, v in gather_us.items()},
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
