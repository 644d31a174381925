"""What aggregating layer 0 straight from 16-bit rows buys on the step (MI355X; needs the GPU).

The same seeded Reddit-shaped LADIES batches (samp 8192, batch 512, buffer 0.1 N: the config-2
shape) are staged from ONE fp16 feature table, drawn once, in two modes:

  widened   FeatureStore(fp16 table): X0 is fp32, widened by the X0 gather (what the store did
            before keep16); the step's layer 0 gathers 4-byte elements
  keep16    FeatureStore(fp16 table, keep16=True): X0 stays fp16, copied by the X0 gather; the
            step's layer 0 aggregates from the 16-bit rows (gnn_spmm_csr_h16_f32) and widens
            x[sampled] into its own buffer

and, per mode and batch, these are timed:

  x0_gather_us     HIP events around the X0 gather (own-buffer + host rows, one launch)
  agg_l0_us        the layer-0 forward aggregation's main kernel by its dispatch's own timestamps
                   (the library's timing hook, as rocprofv3 reports the kernel)
  xs_gather_us     HIP events around the layer-0 x[sampled] gather
  gpu_step_us      HIP events around one native training step (forward + backward), back to back
                   over the batches

The modes alternate window by window in one process (widened, keep16, widened, ...): the machine
is shared, so a difference means something only against the spread of the repeats — median, min
and max over the windows are reported, after two warm-up rounds. The baseline is the widened mode
of the same run, never a figure from a document. One JSON line; no threshold.

    python scripts/agg16_probe.py [--windows 7] [--batches 8] [--graph reddit] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_amd import custom_sparse_ops as cso  # noqa: E402
from gnn_amd import graphs, loader, placement, staging  # noqa: E402
from gnn_amd.models import build_model  # noqa: E402
from gnn_amd.train import Trainer  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batches", type=int, default=8, help="distinct pre-sampled batches per window")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "tiny"])
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("agg16_probe: no GPU visible; this probe measures on the device and has no fallback")
    dev = torch.device("cuda", 0)
    spec = graphs.REDDIT if args.graph == "reddit" else graphs.TINY
    samp, bs = (8192, 512) if args.graph == "reddit" else (256, 64)
    A, labels, feats, ncls, train, *_ = graphs.make_dataset(spec, seed=0)
    lap = graphs.lap_matrix(A, "graphsage")
    N, F = A.shape[0], int(feats.shape[1])
    pl = placement.create_buffer(lap, train, int(0.1 * N), [0], 3, alpha=0)
    table = feats.half()  # the features, drawn once in fp16
    modes = ("widened", "keep16")
    stores = {m: staging.FeatureStore(table, pl.gpu_buffer_group[0], dev, 0, keep16=(m == "keep16")) for m in modes}

    # ---- the same pre-sampled batches, staged once per mode through the real staging path ----
    state = {}
    for m, store in stores.items():
        ld = loader.NativeLoader(lap, labels, train, samp, bs, [1, 1, 1], pl.device_id_of_nodes_group[0],
                                 pl.idx_of_nodes_on_device_group[0], store=store, workers=args.workers, seed=0,
                                 device_extract=True)
        try:
            stager = staging.Stager(store)
            items = []
            for _, lb in zip(range(args.batches), ld.epoch(1)):
                staged = stager.issue(lb.plan, loader.ToDevice(lb.host, dev))
                x0 = staged.wait()
                items.append((lb, staged, x0, lb.host.stage_views(dev)))
            torch.cuda.synchronize()
        finally:
            ld.close()
        torch.manual_seed(0)
        net = build_model("graphsage", F, args.nhid, [1, 1, 1], ncls, 0.1, fused=True).to(dev)
        tr = Trainer(net, 0.01, dev)
        if tr.executor is None:
            sys.exit("agg16_probe: the native step executor is off (GNN_NATIVE_STEP=0)")
        for _, staged, x0, _ in items:
            if not tr.executor.supports(x0, staged.adjs, staged.batch.sampled_nodes, staged.batch.labels):
                sys.exit(f"agg16_probe: the executor does not take the {m} batches")
        state[m] = (store, items, tr)
    # the two modes computed the same thing: X0 is the table (widened or not), bit for bit
    checked = {}
    for m, (store, items, _) in state.items():
        lb, _, x0, _ = items[0]
        nodes = torch.from_numpy(np.asarray(lb.host.input_nodes, np.int64))
        want = table[nodes] if m == "keep16" else table[nodes].float()
        checked[m] = bool(x0.dtype == want.dtype and torch.equal(x0.cpu(), want))
    a0 = cso.spmm_csr(state["widened"][1][0][1].adjs[0], state["widened"][1][0][2])
    b0 = cso.spmm_csr(state["keep16"][1][0][1].adjs[0], state["keep16"][1][0][2])
    checked["agg_l0_bit_identical"] = bool(torch.equal(a0.view(torch.int32), b0.view(torch.int32)))

    keys = ("x0_gather_us", "agg_l0_us", "xs_gather_us", "gpu_step_us")
    res = {m: {k: [] for k in keys} for m in modes}
    kernels = {}
    for w in range(args.windows + 2):  # two warm-up rounds
        for m in modes:
            store, items, tr = state[m]
            buf = staging.word_rows(store.gpu_buffer) if store.keep16 else store.gpu_buffer
            g_ev, x_ev, s_ev = [], [], []
            cso.take_timing_records()
            for lb, staged, x0, (own_pos, own_src, host_pos, host_dev) in items:
                full = x0.as_strided((x0.shape[0], x0.stride(0)), (x0.stride(0), 1))
                dst = staging.word_rows(full) if store.keep16 else full
                hrows = dst  # a placeholder when the batch has no host rows
                if host_pos.numel():
                    hrows = staging.word_rows(host_dev) if store.keep16 else host_dev
                g_ev.append(timed(lambda: cso.gather_rows2(buf, own_src, own_pos, int(own_pos.numel()), hrows, None,
                                                           host_pos, int(host_pos.numel()), dst)))
                op0, sampled = staged.adjs[0], staged.batch.sampled_nodes[0]
                cso.enable_timing(True)
                feat = cso.spmm_csr(op0, x0)
                cso.enable_timing(False)
                xs = torch.empty((sampled.numel(), feat.stride(0)), dtype=torch.float32, device=dev)[:, :F]
                x_ev.append(timed(lambda: cso.gather_rows(x0, sampled, xs, None, n=sampled.numel())))
            for lb, staged, x0, _ in items:
                db = staged.batch
                s_ev.append(timed(lambda: tr.step(x0, staged.adjs, db.sampled_nodes, db.labels)))
            torch.cuda.synchronize()
            recs = cso.take_timing_records()
            kernels[m] = recs[0][3]
            if w >= 2:
                r = res[m]
                r["x0_gather_us"].append(sum(a.elapsed_time(b) for a, b in g_ev) / len(g_ev) * 1e3)
                r["agg_l0_us"].append(sum(x[1] for x in recs) / len(recs) * 1e3)
                r["xs_gather_us"].append(sum(a.elapsed_time(b) for a, b in x_ev) / len(x_ev) * 1e3)
                r["gpu_step_us"].append(sum(a.elapsed_time(b) for a, b in s_ev) / len(s_ev) * 1e3)

    op0 = state["widened"][1][0][1].adjs[0]
    out = {
        "probe": "agg16", "graph": spec.name, "samp": samp, "batch": bs, "nhid": args.nhid, "F": F,
        "windows": args.windows, "batches": args.batches, "device": torch.cuda.get_device_name(0),
        "order": "widened, keep16 alternating per window; 2 warm-up rounds dropped",
        "checks": checked,
        "layer0": {"M": op0.shape[0], "K": op0.shape[1], "nnz": op0.nnz},
        "x0_bytes_per_batch": {m: int(state[m][1][0][2].shape[0] * state[m][1][0][2].stride(0)
                                      * state[m][1][0][2].element_size()) for m in modes},
        "agg_l0_kernel": kernels,
        **{k: {m: spread(res[m][k]) for m in modes} for k in keys},
    }
    out["keep16_over_widened_median"] = {
        k: round(out[k]["keep16"]["median"] / out[k]["widened"]["median"], 4) for k in keys}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
