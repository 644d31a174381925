"""Exact full-neighbourhood inference: the trained model run layer by layer over every node.

Reference: the sampled layers of sampler.py:113-139 draw ``adj = lap[rows, :][:, after] / (s·p)``,
an estimate of ``lap[rows, :]`` — every number main.py reports goes through such a draw. Here the
estimated quantity itself is computed: for each layer, ``H' = layer(lap · H, H)`` over all N nodes,
with the weights 1/deg(row) of create_coo_tensor at normfact = 1. No sampler, no importance
weights, eval semantics (no dropout).

On the GPU the graph stays where ``sampler.DeviceGraph`` keeps it and is read in place, a block of
rows at a time (custom_sparse_ops.spmm_graph: gnn_spmm_graph_f32); the layer products are
fused.gemm / fused.linear_pair, the tail fused.sage_norm, the head gnn_head_eval_loss_f32. The
input table (in its own dtype), two ping-pong activation buffers and the projection buffers all
stay resident on the device: a graph whose activations do not fit (papers-scale) is out of scope —
``embed`` raises with the figure before it allocates. On the CPU (config 1, and the tests) the
same planner and block loop drive the layer modules' own pieces through torch sparse blocks of
``lap`` with the same weights; nothing native runs there.

Order of operations of an aggregating layer, chosen from its shapes: *project first* when
n_out < n_in — lap · (H · Wᵀ): the aggregation, the byte-bound part, runs at the narrower width
(config 2: 602 -> 256 and 512 -> 256) and the bias is added after it, so a row of degree 0 gives
linearW(0) = b as the model does — else *aggregate first*, the model's own order.
"""
from __future__ import annotations

import contextlib
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import custom_sparse_ops as cso
from . import models
from .sampler import device_graph, native_graph

# Defaults of plan_blocks, from the sweep of scripts/exact_eval_probe.py: on the
# Reddit-shaped graph a block costs ~0.09 ms beyond its sums, and these caps run within 2.5 % of
# one single block while a block's temporaries (4 bytes of weights per entry, the output rows)
# stay bounded on larger graphs.
DEFAULT_MAX_NNZ = 1 << 24
DEFAULT_MAX_ROWS = 1 << 16
# rows per chunk of the dense passes (products over all nodes, order-0 layers, the head)
ROW_CHUNK = 1 << 16


def plan_blocks(indptr, max_nnz: Optional[int] = None, max_rows: Optional[int] = None) -> List[Tuple[int, int]]:
    """Contiguous row blocks [(row0, row1)] covering [0, N) exactly, each of at most ``max_rows``
    rows and ``max_nnz`` entries — except that a single row longer than ``max_nnz`` gets a block of
    its own (ValueError if it holds 2^31 entries or more: a block's offsets are int32). Host only;
    ``indptr`` is the graph's int64 row pointer (N + 1 entries)."""
    ip = np.asarray(indptr, dtype=np.int64)
    if ip.ndim != 1 or ip.size < 1:
        raise ValueError("plan_blocks: indptr must be a 1-D array of N + 1 entries")
    max_nnz = DEFAULT_MAX_NNZ if max_nnz is None else int(max_nnz)
    max_rows = DEFAULT_MAX_ROWS if max_rows is None else int(max_rows)
    if max_nnz < 1 or max_rows < 1:
        raise ValueError("plan_blocks: max_nnz and max_rows must be >= 1")
    max_nnz, max_rows = min(max_nnz, 2**31 - 2), min(max_rows, 2**31 - 2)
    N = ip.size - 1
    blocks = []
    r0 = 0
    while r0 < N:
        # the last row pointer within the entry cap, then the row cap
        r1 = int(np.searchsorted(ip, ip[r0] + max_nnz, side="right")) - 1
        r1 = min(r1, r0 + max_rows, N)
        if r1 <= r0:  # one row longer than max_nnz
            r1 = r0 + 1
            if int(ip[r1] - ip[r0]) >= 2**31 - 1:
                raise ValueError(f"plan_blocks: row {r0} holds {int(ip[r1] - ip[r0])} entries (>= 2^31)")
        blocks.append((r0, r1))
        r0 = r1
    return blocks


def _chunks(n: int, size: int):
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def _layer_parts(gc):
    """(sage, W_B or None, b_B or None, W_W, b_W) of a GraphSageConvolution / GraphConvolution."""
    if isinstance(gc, models.GraphSageConvolution):
        if gc.order > 0:
            return True, gc.linearB.weight, gc.linearB.bias, gc.linearW.weight, gc.linearW.bias
        return True, None, None, gc.linearW.weight, gc.linearW.bias
    if isinstance(gc, models.GraphConvolution):
        return False, None, None, gc.linear.weight, gc.linear.bias
    raise ValueError(f"ExactInference: unsupported layer {type(gc).__name__}")


def _tail_torch(feat, gc):
    """ELU and the row standardisation of models.py:22-25 / 61-64."""
    out = F.elu(feat)
    mean = out.mean(dim=1, keepdim=True)
    var = out.var(dim=1, unbiased=False, keepdim=True) + 1e-9
    return (out - mean) * gc.scale * torch.rsqrt(var) + gc.offset


class ExactInference:
    """The model (a models.GNN over a GraphSage or GCN encoder, orders in {0, 1}, fused or not) over
    all nodes of ``graph`` (a lap matrix or a sampler.NativeGraph) on ``device``."""

    def __init__(self, model, graph, device, max_nnz: Optional[int] = None, max_rows: Optional[int] = None):
        enc = getattr(model, "encoder", None)
        if not isinstance(model, models.GNN) or not isinstance(enc, (models.GraphSage, models.GCN)):
            raise ValueError("ExactInference: model must be a models.GNN over a GraphSage or GCN encoder")
        for gc in enc.gcs:
            _layer_parts(gc)
            if gc.order not in (0, 1):
                raise ValueError(f"ExactInference: layer order {gc.order} (0 or 1)")
            if gc.spmm_fn is not models._default_spmm and torch.device(device).type == "cuda":
                raise ValueError("ExactInference: a model with its own spmm_fn runs on the CPU only")
        self.model = model
        self.graph = native_graph(graph)
        self.device = torch.device(device)
        self.N = self.graph.num_nodes
        self.blocks = plan_blocks(self.graph.indptr, max_nnz, max_rows)
        self.native = self.device.type == "cuda"
        self.dgraph = device_graph(self.graph, self.device) if self.native else None
        # per layer, set by embed(): "project" / "aggregate" / "dense" (diagnostics, the probe)
        self.orders_taken: List[str] = []
        # measurements only (scripts/exact_eval_probe.py): layer 0's order forced to "project" /
        # "aggregate", and, when a list, (layer, phase, start event, end event) of every phase
        self.force_order: Optional[str] = None
        self.timing: Optional[list] = None
        self.last_counts = None  # evaluate(): the pooled (tp, fp, fn) counts, int64 [3, C] on the host

    # ------------------------------------------------------------------ shared helpers
    def _table(self, feats) -> torch.Tensor:
        host = getattr(feats, "host", None)
        if host is not None and hasattr(feats, "F"):  # a staging.FeatureStore: its host table
            feats = host[:, : feats.F]
        if not isinstance(feats, torch.Tensor) or feats.dim() != 2 or feats.dtype not in cso.FEAT_KIND:
            raise ValueError("ExactInference: feats must be a 2-D float32 / float16 / bfloat16 table "
                             "or a staging.FeatureStore")
        if feats.shape[0] != self.N:
            raise ValueError(f"ExactInference: feats has {feats.shape[0]} rows, the graph {self.N} nodes")
        n_in = self.model.encoder.gcs[0].n_in
        if feats.shape[1] != n_in:
            raise ValueError(f"ExactInference: feats has {feats.shape[1]} columns, the model reads {n_in}")
        return feats

    def _project_first(self, li: int, n_in: int, n_out: int) -> bool:
        if self.force_order is not None and li == 0:
            return self.force_order == "project"
        return n_out < n_in

    @contextlib.contextmanager
    def _phase(self, li: int, name: str):
        """Device events around one phase (products / aggregation / tail) when ``timing`` is a list."""
        if self.timing is None:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        self.timing.append((li, name, e0, e1))

    def _free_bytes(self) -> int:
        """Device memory this process can still take: the driver's free figure plus what torch's
        allocator holds unused."""
        free, _ = torch.cuda.mem_get_info(self.device)
        return int(free) + int(torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device))

    # ------------------------------------------------------------------ embed
    def embed(self, feats) -> torch.Tensor:
        """The top layer's output [N, encoder.nhid] for all nodes, on the device, without dropout."""
        table = self._table(feats)
        with torch.no_grad():
            out = self._embed_native(table) if self.native else self._embed_cpu(table)
        return out

    def _embed_cpu(self, table: torch.Tensor) -> torch.Tensor:
        g = self.graph
        ip = g.indptr
        deg = np.diff(ip)
        H = table.to(self.device)
        self.orders_taken = []
        for gc in self.model.encoder.gcs:
            sage, _, _, W, _ = _layer_parts(gc)
            if gc.order == 0:
                self.orders_taken.append("dense")
                outs = [_tail_torch((gc.linearW if sage else gc.linear)(models._f32(H[a:b])), gc)
                        for a, b in _chunks(self.N, ROW_CHUNK)]
            else:
                self.orders_taken.append("aggregate")
                outs = []
                for r0, r1 in self.blocks:
                    e0, e1 = int(ip[r0]), int(ip[r1])
                    crow = torch.from_numpy(ip[r0:r1 + 1] - e0)
                    col = torch.from_numpy(g.indices[e0:e1].astype(np.int64))
                    with np.errstate(divide="ignore"):
                        w = (1.0 / deg[r0:r1].astype(np.float64)).astype(np.float32)
                    val = torch.from_numpy(np.repeat(w, deg[r0:r1]))
                    rows = torch.repeat_interleave(torch.arange(r1 - r0, dtype=torch.int64), crow[1:] - crow[:-1])
                    adj = torch.sparse_coo_tensor(torch.stack([rows, col]), val, (r1 - r0, self.N),
                                                  is_coalesced=True)
                    agg = gc.spmm_fn(adj, H)  # custom_sparse_ops.spmm's CPU branch: torch.sparse.mm
                    if sage:
                        feat = torch.cat([gc.linearB(models._f32(H[r0:r1])), gc.linearW(agg)], 1)
                    else:
                        feat = gc.linear(agg)
                    outs.append(_tail_torch(feat, gc))
            width = W.shape[0] * (2 if sage and gc.order else 1)
            H = torch.cat(outs, 0) if outs else torch.zeros((0, width), dtype=torch.float32, device=self.device)
        return H

    def _layer_plan(self, table: torch.Tensor):
        """Per layer (kind, n_in, n_out, width) and the bytes embed keeps resident."""
        plan = []
        n_in = table.shape[1]
        for li, gc in enumerate(self.model.encoder.gcs):
            sage, _, _, W, _ = _layer_parts(gc)
            n_out = W.shape[0]
            width = n_out * (2 if (sage and gc.order > 0) else 1)
            kind = "dense" if gc.order == 0 else ("project" if self._project_first(li, n_in, n_out) else "aggregate")
            plan.append((kind, n_in, n_out, width, sage))
            n_in = width
        return plan

    def memory_needed(self, feats) -> int:
        """Bytes of device memory ``embed`` needs for this table: the resident table (if it is not
        on the device already), two ping-pong activation buffers, the projection buffers and the
        largest block's temporaries."""
        table = self._table(feats)
        plan = self._layer_plan(table)
        N = self.N
        esz = table.element_size()
        need = 0
        if not table.is_cuda:
            from .staging import padded_ld

            need += N * padded_ld(table.shape[1], 128 // esz) * esz
        act = max(p[3] for p in plan)
        need += 2 * N * act * 4
        proj = max([p[2] * (2 if p[4] else 1) for p in plan if p[0] == "project"], default=0)
        need += N * proj * 4
        L = None
        tmp = 0
        ip = self.graph.indptr
        for r0, r1 in self.blocks:
            rows, nnz = r1 - r0, int(ip[r1] - ip[r0])
            for kind, n_in, n_out, width, sage in plan:
                if kind == "dense":
                    continue
                if L is None:
                    from . import _lib

                    L = _lib.lib()
                Fa = n_out if kind == "project" else n_in
                Fa4 = (Fa + 3) & ~3
                # the workspace, the aggregate, the pair of products and the tail's output
                t = L.gnn_spmm_graph_workspace_bytes(rows, nnz, Fa4) + rows * 4 * (2 * Fa4 + 3 * width)
                tmp = max(tmp, t)
        chunk = min(ROW_CHUNK, N)
        tmp = max(tmp, chunk * 4 * (max(p[1] for p in plan) + 3 * act))
        return int(need + tmp)

    def _rows_f32(self, H: torch.Tensor, r0: int, r1: int, ld: Optional[int] = None) -> torch.Tensor:
        """Rows [r0, r1) of H as fp32 rows of stride ld (default: H's own width): the view itself
        when H is fp32 in that layout, else a copy — 16-bit rows widened (gnn_gather_rows_h16_f32)."""
        Fw = H.shape[1]
        if H.dtype == torch.float32 and (ld is None or H.stride(0) == ld or r1 - r0 <= 1):
            return H[r0:r1]
        ld = Fw + (Fw & 1) if ld is None else ld  # even rows: the GEMM's operand contract
        dst = torch.empty((r1 - r0, ld), dtype=torch.float32, device=H.device)[:, :Fw]
        if r1 > r0:
            cso.gather_rows(H[r0:r1], None, dst, None, n=r1 - r0)
        return dst

    @staticmethod
    def _products(x: torch.Tensor, Ws) -> list:
        """x · Wᵀ for each W over one row chunk: fused.gemm (one batched launch) on operands inside
        its contract, torch.mm otherwise, as fused.LinearPairFn routes them."""
        from . import fused

        M, K = x.shape
        if M and fused._gemm_ok(x, *Ws) and fused._same_layout(Ws):
            return fused.gemm(False, False, [x] * len(Ws), list(Ws), M, Ws[0].shape[0], K)
        return [torch.mm(x, W.t()) for W in Ws]

    def _embed_native(self, table: torch.Tensor) -> torch.Tensor:
        from . import _lib, fused
        from .staging import padded_ld

        dev = self.device
        N = self.N
        need = self.memory_needed(table)
        free = self._free_bytes()
        if need > free:
            raise RuntimeError(f"ExactInference: {need} bytes of device memory needed ({N} nodes), {free} free: "
                               "activations resident on the host are out of scope")
        plan = self._layer_plan(table)
        self.orders_taken = [p[0] for p in plan]
        ip = self.graph.indptr
        with _lib.on_device(dev):
            if table.is_cuda:
                if table.device != dev:
                    raise ValueError("ExactInference: feats is on another device")
                H = table if table.stride(1) == 1 else table.contiguous()
            else:  # whole-line rows in the table's own dtype
                ld = padded_ld(table.shape[1], 128 // table.element_size())
                H = torch.zeros((N, ld), dtype=table.dtype, device=dev)[:, : table.shape[1]]
                H.copy_(table, non_blocking=False)
            act = max(p[3] for p in plan)
            pingpong = [torch.empty((N, act), dtype=torch.float32, device=dev) for _ in range(2)]
            nproj = max([p[2] * (2 if p[4] else 1) for p in plan if p[0] == "project"], default=0)
            proj = torch.empty((N, nproj), dtype=torch.float32, device=dev) if nproj else None
            for li, (gc, (kind, n_in, n_out, width, sage)) in enumerate(zip(self.model.encoder.gcs, plan)):
                _, WB, bB, WW, bW = _layer_parts(gc)
                out = pingpong[li & 1].view(-1)[: N * width].view(N, width)  # contiguous rows of its own width
                if kind == "dense":
                    for a, b in _chunks(N, ROW_CHUNK):
                        with self._phase(li, "products"):
                            (hW,) = fused.linear_pair([self._rows_f32(H, a, b)], [WW])
                        with self._phase(li, "tail"):
                            out[a:b] = fused.sage_norm(None, hW, gc.scale, gc.offset, 0.0, False, None, bW)
                elif kind == "project":
                    PW = proj.view(-1)[: N * n_out].view(N, n_out)
                    PB = proj.view(-1)[N * n_out: 2 * N * n_out].view(N, n_out) if sage else None
                    for a, b in _chunks(N, ROW_CHUNK):
                        with self._phase(li, "products"):
                            ps = self._products(self._rows_f32(H, a, b), [WB, WW] if sage else [WW])
                            PW[a:b] = ps[-1]
                            if sage:
                                PB[a:b] = ps[0]
                    for r0, r1 in self.blocks:
                        with self._phase(li, "aggregation"):
                            Z = cso.spmm_graph(self.dgraph, r0, r1 - r0, PW, int(ip[r0]), int(ip[r1] - ip[r0]))
                        with self._phase(li, "tail"):
                            out[r0:r1] = fused.sage_norm(PB[r0:r1] if sage else None, Z, gc.scale, gc.offset, 0.0,
                                                         False, bB if sage else None, bW)
                else:
                    for r0, r1 in self.blocks:
                        with self._phase(li, "aggregation"):
                            agg = cso.spmm_graph(self.dgraph, r0, r1 - r0, H, int(ip[r0]), int(ip[r1] - ip[r0]))
                        with self._phase(li, "products"):
                            if sage:
                                ld = agg.stride(0) if r1 - r0 > 1 else None
                                hB, hW = fused.linear_pair([self._rows_f32(H, r0, r1, ld), agg], [WB, WW])
                            else:
                                hB = None
                                (hW,) = fused.linear_pair([agg], [WW])
                        with self._phase(li, "tail"):
                            out[r0:r1] = fused.sage_norm(hB, hW, gc.scale, gc.offset, 0.0, False,
                                                         bB if sage else None, bW)
                H = out
        return H

    # ------------------------------------------------------------------ head
    def _head(self, x: torch.Tensor, labels: Optional[torch.Tensor], mode: int, sigmoid_loss: bool):
        """(logits, loss, counts) of one chunk of embedded rows: L2-normalise, linear (models.py:
        90-97 in eval mode) and, with labels, the mean loss and the (tp, fp, fn) counts [3, C]."""
        lin = self.model.linear
        C = lin.weight.shape[0]
        if self.native:
            from . import _lib, fused

            M, D = x.shape
            shape_of = labels if labels is not None else torch.empty((M, C), device="meta")
            if fused.head_supported(x, lin.weight, shape_of) and lin.bias is not None:
                dev = x.device
                W = lin.weight.contiguous()
                z = torch.empty((M, C), dtype=torch.float32, device=dev)
                if labels is None:
                    args = (None, 0, z.data_ptr(), C, None, None, None, None)
                    loss = counts = None
                else:
                    labels = labels if labels.dtype == torch.float32 else labels.float()
                    labels = labels if labels.stride(1) == 1 else labels.contiguous()
                    rowloss = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
                    rowmask = torch.empty(max(M, 1) * 8, dtype=torch.int64, device=dev)
                    loss = torch.empty((), dtype=torch.float32, device=dev)
                    counts = torch.empty((3, C), dtype=torch.int32, device=dev)
                    args = (labels.data_ptr(), labels.stride(0), z.data_ptr(), C, rowloss.data_ptr(),
                            rowmask.data_ptr(), loss.data_ptr(), counts.data_ptr())
                with _lib.on_device(dev):
                    _lib.check(_lib.lib().gnn_head_eval_loss_f32(
                        x.data_ptr(), x.stride(0), M, D, W.data_ptr(), lin.bias.data_ptr(), C, *args, int(mode),
                        0 if sigmoid_loss else 1, _lib.stream_of(dev)), "gnn_head_eval_loss_f32")
                return z, loss, counts
        z = lin(F.normalize(x, p=2, dim=1))
        if labels is None:
            return z, None, None
        from . import metrics

        labels = labels.float()
        return z, models.loss(z, labels, sigmoid_loss, z.device).to(torch.float32), \
            metrics.prediction_counts(z, labels, mode)

    def _node_index(self, nodes) -> Optional[torch.Tensor]:
        if nodes is None:
            return None
        idx = torch.as_tensor(np.asarray(nodes) if not isinstance(nodes, torch.Tensor) else nodes)
        return idx.to(device=self.device, dtype=torch.int64).contiguous()

    def _take(self, emb: torch.Tensor, idx: Optional[torch.Tensor], a: int, b: int) -> torch.Tensor:
        if idx is None:
            return emb[a:b]
        if self.native:
            out = torch.empty((b - a, emb.shape[1]), dtype=torch.float32, device=emb.device)
            cso.gather_rows(emb, idx[a:b], out, None, n=b - a)
            return out
        return emb[idx[a:b]]

    def logits(self, feats, nodes=None) -> torch.Tensor:
        """The model's logits [len(nodes), C] (all N nodes when ``nodes`` is None), on the device."""
        emb = self.embed(feats)
        idx = self._node_index(nodes)
        n = self.N if idx is None else int(idx.numel())
        C = self.model.linear.weight.shape[0]
        out = torch.empty((n, C), dtype=torch.float32, device=self.device)
        with torch.no_grad():
            for a, b in _chunks(n, ROW_CHUNK):
                out[a:b] = self._head(self._take(emb, idx, a, b), None, 0, True)[0]
        return out

    def evaluate(self, feats, nodes, labels, sigmoid_loss: bool = True, mode: Optional[int] = None) -> dict:
        """Loss and F1 of ``nodes`` (None: all) against ``labels`` (one float row of C entries per
        node of ``nodes``, host or device): chunks of nodes through the evaluation head, accumulated
        in train.Evaluator's buffer, one host copy at the end. Returns ``Evaluator.result()``'s keys;
        the pooled (tp, fp, fn) counts stay in ``self.last_counts``."""
        from .train import Evaluator

        emb = self.embed(feats)
        idx = self._node_index(nodes)
        n = self.N if idx is None else int(idx.numel())
        if not isinstance(labels, torch.Tensor):
            labels = torch.as_tensor(np.asarray(labels))
        if labels.dim() != 2 or labels.shape[0] != n:
            raise ValueError(f"ExactInference.evaluate: labels {tuple(labels.shape)} for {n} nodes")
        labels = labels.to(self.device)
        ev = Evaluator(self.model, self.device, sigmoid_loss, mode=mode)
        with torch.no_grad():
            for a, b in _chunks(n, ROW_CHUNK):
                _, loss, counts = self._head(self._take(emb, idx, a, b), labels[a:b], ev.mode, sigmoid_loss)
                ev.add_counts(loss, counts, b - a)
        res = ev.result()
        self.last_counts = ev.counts
        return res
