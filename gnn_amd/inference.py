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
stay resident on the device: a graph whose activations do not fit (papers-scale) is refused in
this scope — ``embed`` raises with the figure before it allocates. Closure scope (``closure``,
``scope="closure"``) runs every layer over the k-hop closure of a query set only — level sets
grown on the device (gnn_closure_mark / list / rank), blocks of their rows aggregated with the
columns relabelled to positions in the level below (custom_sparse_ops.spmm_rows:
gnn_spmm_rows_f32) — the same scores at the closure's cost, whenever the closure fits. On the CPU (config 1, and the tests) the
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


def _row_entries(indptr: np.ndarray, indices: np.ndarray, rows: np.ndarray):
    """(the concatenated columns of the graph rows ``rows``, the rows' degrees), host only."""
    starts = indptr[rows]
    lens = indptr[rows + 1] - starts
    scan = np.cumsum(lens)
    off = np.repeat(starts - (scan - lens), lens) + np.arange(int(scan[-1]) if lens.size else 0, dtype=np.int64)
    return indices[off], lens


class Closure:
    """The node sets a model of L layers reads to score a query set (``ExactInference.closure``).

    ``sets[l]`` (host, ascending node ids) is what layer l reads, ``sets[l + 1]`` what it writes:
    ``sets[L]`` the unique query nodes, ``sets[l] = sets[l + 1] ∪ cols(lap[sets[l + 1], :])`` for an
    aggregating layer and ``sets[l] is sets[l + 1]`` for an order-0 layer. Per aggregating layer l:
    ``scans[l]`` the int64 exclusive scan of the degrees of its rows ``sets[l + 1]``, ``blocks[l]``
    the plan_blocks cover of that scan (positions in ``sets[l + 1]``), ``self_pos[l]`` the positions
    of ``sets[l + 1]`` in ``sets[l]`` (int64, on the engine's device); all three are None for an
    order-0 layer. ``query_pos``: the positions of the caller's nodes in ``sets[L]``, in the caller's
    order, duplicates kept. On the GPU ``dsets`` / ``tables`` hold the sets as int32 device lists
    and as membership tables (gnn_closure_mark), and ``rowsegs[l][b]`` block b's rebased int32 scan."""

    def __init__(self, num_nodes: int, device: torch.device):
        self.num_nodes = num_nodes
        self.device = device
        self.sets: List[np.ndarray] = []
        self.dsets: List[Optional[torch.Tensor]] = []
        self.tables: List[Optional[torch.Tensor]] = []
        self.scans: List[Optional[np.ndarray]] = []
        self.blocks: List[Optional[List[Tuple[int, int]]]] = []
        self.rowsegs: List[Optional[List[torch.Tensor]]] = []
        self.self_pos: List[Optional[torch.Tensor]] = []
        self.query_pos: Optional[torch.Tensor] = None
        self.num_queries = 0

    @property
    def sizes(self) -> List[int]:
        return [int(s.size) for s in self.sets]

    def positions(self, nodes) -> torch.Tensor:
        """Positions of ``nodes`` in the top set (int64, on the closure's device); ValueError if one
        of them is not in it."""
        top = self.sets[-1]
        q = np.asarray(nodes.cpu() if isinstance(nodes, torch.Tensor) else nodes).astype(np.int64).reshape(-1)
        pos = np.searchsorted(top, q)
        if q.size and (top.size == 0 or np.any(top[np.minimum(pos, top.size - 1)] != q)):
            raise ValueError("Closure: a node is outside the closure's query set")
        return torch.from_numpy(pos.astype(np.int64)).to(self.device)


class ExactInference:
    """The model (a models.GNN over a GraphSage or GCN encoder, orders in {0, 1}, fused or not) over
    all nodes of ``graph`` (a lap matrix or a sampler.NativeGraph) on ``device`` — or, in closure
    scope, over the k-hop closure of a query set only (``closure``, ``scope=`` of ``logits`` /
    ``evaluate``)."""

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
        self._caps = (max_nnz, max_rows)  # closure(): the same caps over a closure level's rows
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

    # ------------------------------------------------------------------ closure
    def closure(self, nodes) -> Closure:
        """The k-hop in-closure of ``nodes`` under ``lap``, level by level from the top: the unique
        query nodes, then for every aggregating layer below the set joined by the columns of its
        rows (an order-0 layer repeats its set). Self rows are always members — GraphSAGE's
        linearB(x[rows]) reads them; for GCN they only add rows.

        On the GPU each level is grown on the device over the resident graph (gnn_closure_mark /
        list / rank). Cost on the host: one small device-to-host read per level (the set's size)
        and one copy of every set to the host, where the rows' degree scan is taken from the
        host's row pointer and planned into blocks. On the CPU the same object is built with
        numpy (np.unique over the concatenated rows)."""
        q = np.asarray(nodes.cpu() if isinstance(nodes, torch.Tensor) else nodes).reshape(-1)
        if q.size and (q.dtype.kind not in "iu" or q.min() < 0 or q.max() >= self.N):
            raise ValueError(f"ExactInference.closure: nodes must be integer ids in [0, {self.N})")
        q = q.astype(np.int64)
        gcs = list(self.model.encoder.gcs)
        L = len(gcs)
        c = Closure(self.N, self.device)
        c.num_queries = int(q.size)
        g = self.graph
        levels = [None] * (L + 1)  # (host set, device set, table)
        if self.native:
            dg = self.dgraph
            dq = torch.from_numpy(q.astype(np.int32)).to(self.device)
            tab, cnt = cso.closure_mark(dg, dq, False)
            ds = cso.closure_list(tab, self.N, int(cnt.item()))
            c.query_pos = cso.closure_rank(tab, self.N, dq)
            levels[L] = (ds.cpu().numpy(), ds, tab)
        else:
            top = np.unique(q).astype(np.int32)
            levels[L] = (top, None, None)
            c.query_pos = torch.from_numpy(np.searchsorted(top, q).astype(np.int64))
        c.self_pos = [None] * L
        c.scans, c.blocks, c.rowsegs = [None] * L, [None] * L, [None] * L
        for l in range(L - 1, -1, -1):
            up, dup, _ = levels[l + 1]
            if gcs[l].order == 0:
                levels[l] = levels[l + 1]
                continue
            if self.native:
                tab, cnt = cso.closure_mark(dg, dup, True)
                ds = cso.closure_list(tab, self.N, int(cnt.item()))
                c.self_pos[l] = cso.closure_rank(tab, self.N, dup)
                levels[l] = (ds.cpu().numpy(), ds, tab)
            else:
                cols, _ = _row_entries(g.indptr, g.indices, up.astype(np.int64))
                low = np.unique(np.concatenate([up, cols])).astype(np.int32)
                levels[l] = (low, None, None)
                c.self_pos[l] = torch.from_numpy(np.searchsorted(low, up).astype(np.int64))
            rows = up.astype(np.int64)
            scan = np.concatenate([[0], np.cumsum(g.indptr[rows + 1] - g.indptr[rows])]).astype(np.int64)
            c.scans[l] = scan
            c.blocks[l] = plan_blocks(scan, *self._caps)
            if self.native:
                c.rowsegs[l] = [torch.from_numpy((scan[a:b + 1] - scan[a]).astype(np.int32)).to(self.device)
                                for a, b in c.blocks[l]]
        c.sets = [lv[0] for lv in levels]
        c.dsets = [lv[1] for lv in levels]
        c.tables = [lv[2] for lv in levels]
        return c

    def _scope(self, nodes, scope) -> Optional[Closure]:
        """None for scope "graph", else the Closure to run in (built for "closure")."""
        if isinstance(scope, Closure):
            if scope.num_nodes != self.N or scope.device != self.device or len(scope.sets) != len(
                    self.model.encoder.gcs) + 1:
                raise ValueError("ExactInference: the Closure was built for another graph, device or model")
            return scope
        if scope == "graph":
            return None
        if scope == "closure":
            return self.closure(np.arange(self.N) if nodes is None else nodes)
        raise ValueError(f"ExactInference: scope must be 'graph', 'closure' or a Closure, got {scope!r}")

    # ------------------------------------------------------------------ embed
    def embed(self, feats, closure: Optional[Closure] = None) -> torch.Tensor:
        """The top layer's output [N, encoder.nhid] for all nodes, on the device, without dropout.
        With a ``closure``: the rows of its top set only ([len(closure.sets[-1]), nhid], in
        ascending node order), every layer run over its own level of the closure."""
        table = self._table(feats)
        with torch.no_grad():
            if closure is not None:
                closure = self._scope(None, closure)
                return self._embed_native_closure(table, closure) if self.native \
                    else self._embed_cpu_closure(table, closure)
            out = self._embed_native(table) if self.native else self._embed_cpu(table)
        return out

    def _embed_cpu_closure(self, table: torch.Tensor, c: Closure) -> torch.Tensor:
        g = self.graph
        ip = g.indptr
        H = models._f32(table[torch.from_numpy(c.sets[0].astype(np.int64))]).to(self.device)
        self.orders_taken = []
        for l, gc in enumerate(self.model.encoder.gcs):
            sage, _, _, W, _ = _layer_parts(gc)
            m = c.sets[l + 1].size
            if gc.order == 0:
                self.orders_taken.append("dense")
                outs = [_tail_torch((gc.linearW if sage else gc.linear)(H[a:b]), gc) for a, b in _chunks(m, ROW_CHUNK)]
            else:
                self.orders_taken.append("aggregate")
                outs = []
                rows, low = c.sets[l + 1].astype(np.int64), c.sets[l]
                for a, b in c.blocks[l]:
                    ent, deg = _row_entries(ip, g.indices, rows[a:b])
                    col = np.searchsorted(low, ent)  # every column is a member: the level's definition
                    with np.errstate(divide="ignore"):
                        w = (1.0 / deg.astype(np.float64)).astype(np.float32)
                    r = np.repeat(np.arange(b - a, dtype=np.int64), deg)
                    adj = torch.sparse_coo_tensor(torch.from_numpy(np.stack([r, col.astype(np.int64)])),
                                                  torch.from_numpy(np.repeat(w, deg)), (b - a, low.size),
                                                  is_coalesced=True)
                    agg = gc.spmm_fn(adj, H)
                    if sage:
                        feat = torch.cat([gc.linearB(H[c.self_pos[l][a:b]]), gc.linearW(agg)], 1)
                    else:
                        feat = gc.linear(agg)
                    outs.append(_tail_torch(feat, gc))
            width = W.shape[0] * (2 if sage and gc.order else 1)
            H = torch.cat(outs, 0) if outs else torch.zeros((0, width), dtype=torch.float32, device=self.device)
        return H

    def _closure_bytes(self, table: torch.Tensor, c: Closure) -> int:
        """Peak bytes of the closure embed: X0 (and the staged rows of a host table) first, then
        per layer its input, its output, the projections and the largest block's temporaries —
        all from the closure's sizes; nothing here grows with N."""
        from . import _lib
        from .staging import padded_ld

        L = _lib.lib()
        plan = self._layer_plan(table)
        sizes = c.sizes
        F0 = table.shape[1]
        x0 = sizes[0] * padded_ld(F0, 32) * 4
        peak = x0
        if table.is_cuda:
            peak += sizes[0] * 8  # the gather's int64 row index
        elif table.dtype != torch.float32:  # 16-bit host rows are uploaded as they are, then widened
            esz = table.element_size()
            peak += sizes[0] * padded_ld(F0, 128 // esz) * esz
        h_bytes = x0
        for l, (kind, n_in, n_out, width, sage) in enumerate(plan):
            n_low, m = sizes[l], sizes[l + 1]
            out_bytes = m * width * 4
            tmp = min(ROW_CHUNK, max(n_low, 1)) * 4 * (n_in + (n_in & 1) + 3 * width)
            proj = 0
            if kind == "project":
                proj = (n_low + (m if sage else 0)) * n_out * 4 + (m * (n_in + (n_in & 1)) * 4 if sage else 0)
            if kind != "dense":
                Fa4 = ((n_out if kind == "project" else n_in) + 3) & ~3
                for a, b in c.blocks[l]:
                    rows, nnz = b - a, int(c.scans[l][b] - c.scans[l][a])
                    tmp = max(tmp, L.gnn_spmm_rows_workspace_bytes(rows, nnz, Fa4) + rows * 4 * (2 * Fa4 + 3 * width))
            peak = max(peak, h_bytes + out_bytes + proj + tmp)
            h_bytes = out_bytes
        return int(peak)

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

    def memory_needed(self, feats, closure: Optional[Closure] = None) -> int:
        """Bytes of device memory ``embed`` needs for this table: the resident table (if it is not
        on the device already), two ping-pong activation buffers, the projection buffers and the
        largest block's temporaries. With a ``closure``: what ``embed(feats, closure)`` needs,
        computed from the closure's level sizes alone (no N-row buffer exists in that scope)."""
        table = self._table(feats)
        if closure is not None:
            return self._closure_bytes(table, self._scope(None, closure))
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

    def _gather_f32(self, H: torch.Tensor, idx: Optional[torch.Tensor], n: int, ld: Optional[int] = None) -> torch.Tensor:
        """Rows ``idx`` (int64; None: the first n) of H as fp32 rows of stride ld (default: the width
        made even, the GEMM's operand contract); 16-bit rows are widened, exactly."""
        Fw = H.shape[1]
        ld = Fw + (Fw & 1) if ld is None else ld
        dst = torch.empty((n, ld), dtype=torch.float32, device=H.device)[:, :Fw]
        if n:
            cso.gather_rows(H, idx, dst, None, n=n)
        return dst

    def _embed_native_closure(self, table: torch.Tensor, c: Closure) -> torch.Tensor:
        from . import _lib, fused
        from .staging import padded_ld

        dev = self.device
        need = self._closure_bytes(table, c)
        free = self._free_bytes()
        if need > free:
            raise RuntimeError(f"ExactInference: {need} bytes of device memory needed (a closure of "
                               f"{c.sizes[0]} nodes), {free} free: the closure does not fit")
        plan = self._layer_plan(table)
        self.orders_taken = [p[0] for p in plan]
        dg = self.dgraph
        with _lib.on_device(dev):
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            # X0: the closure's bottom rows as fp32, whole-line rows
            n0, F0 = c.sizes[0], table.shape[1]
            if table.is_cuda:
                if table.device != dev:
                    raise ValueError("ExactInference: feats is on another device")
                src = table if table.stride(1) == 1 else table.contiguous()
                H = self._gather_f32(src, c.dsets[0].long(), n0, padded_ld(F0, 32))
            else:  # indexed on the host, uploaded once in the table's own dtype, widened on the device
                sub = table[torch.from_numpy(c.sets[0].astype(np.int64))]
                if table.dtype == torch.float32:
                    H = torch.empty((n0, padded_ld(F0, 32)), dtype=torch.float32, device=dev)[:, :F0]
                    H.copy_(sub)
                else:
                    ld = padded_ld(F0, 128 // table.element_size())
                    up = torch.empty((n0, ld), dtype=table.dtype, device=dev)[:, :F0]
                    up.copy_(sub)
                    H = self._gather_f32(up, None, n0, padded_ld(F0, 32))
            for li, (gc, (kind, n_in, n_out, width, sage)) in enumerate(zip(self.model.encoder.gcs, plan)):
                _, WB, bB, WW, bW = _layer_parts(gc)
                m = c.sizes[li + 1]
                out = torch.empty((m, width), dtype=torch.float32, device=dev)
                if kind == "dense":
                    for a, b in _chunks(m, ROW_CHUNK):
                        with self._phase(li, "products"):
                            (hW,) = fused.linear_pair([self._rows_f32(H, a, b)], [WW])
                        with self._phase(li, "tail"):
                            out[a:b] = fused.sage_norm(None, hW, gc.scale, gc.offset, 0.0, False, None, bW)
                    H = out
                    continue
                rows, tab, K, spos = c.dsets[li + 1], c.tables[li], c.sizes[li], c.self_pos[li]
                scan = c.scans[li]
                blocks = list(zip(c.blocks[li], c.rowsegs[li]))
                if kind == "project":
                    PW = torch.empty((K, n_out), dtype=torch.float32, device=dev)
                    for a, b in _chunks(K, ROW_CHUNK):
                        with self._phase(li, "products"):
                            PW[a:b] = self._products(self._rows_f32(H, a, b), [WW])[0]
                    PB = None
                    if sage:  # linearB at the self rows only
                        PB = torch.empty((m, n_out), dtype=torch.float32, device=dev)
                        for a, b in _chunks(m, ROW_CHUNK):
                            with self._phase(li, "products"):
                                PB[a:b] = self._products(self._gather_f32(H, spos[a:b], b - a), [WB])[0]
                    for (a, b), seg in blocks:
                        with self._phase(li, "aggregation"):
                            Z = cso.spmm_rows(dg, rows[a:b], seg, int(scan[b] - scan[a]), tab, K, PW, err=err)
                        with self._phase(li, "tail"):
                            out[a:b] = fused.sage_norm(PB[a:b] if sage else None, Z, gc.scale, gc.offset, 0.0, False,
                                                       bB if sage else None, bW)
                else:
                    for (a, b), seg in blocks:
                        with self._phase(li, "aggregation"):
                            agg = cso.spmm_rows(dg, rows[a:b], seg, int(scan[b] - scan[a]), tab, K, H, err=err)
                        with self._phase(li, "products"):
                            if sage:
                                ld = agg.stride(0) if b - a > 1 else None
                                hB, hW = fused.linear_pair([self._gather_f32(H, spos[a:b], b - a, ld), agg], [WB, WW])
                            else:
                                hB = None
                                (hW,) = fused.linear_pair([agg], [WW])
                        with self._phase(li, "tail"):
                            out[a:b] = fused.sage_norm(hB, hW, gc.scale, gc.offset, 0.0, False,
                                                       bB if sage else None, bW)
                H = out
            if int(err.item()):  # one read at the end: a column outside its level's set
                raise RuntimeError("ExactInference: gnn_spmm_rows_f32 met a column outside the closure "
                                   "(the Closure does not belong to this graph)")
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

    def _embed_scoped(self, feats, nodes, scope):
        """(embedded rows, int64 row index of ``nodes`` into them or None for all rows in order)."""
        c = self._scope(nodes, scope)
        if c is None:
            return self.embed(feats), self._node_index(nodes)
        emb = self.embed(feats, c)
        if isinstance(scope, Closure):  # a prebuilt closure: its own nodes, or any of its query set
            return emb, (c.query_pos if nodes is None else c.positions(nodes))
        return emb, c.query_pos

    def logits(self, feats, nodes=None, scope="graph") -> torch.Tensor:
        """The model's logits [len(nodes), C] (all N nodes when ``nodes`` is None), on the device.
        ``scope``: "graph" embeds every node and picks the rows; "closure" embeds only the k-hop
        closure of ``nodes`` (``closure``), the same scores at the closure's cost; a prebuilt
        ``Closure`` is reused (``nodes``: None for the nodes it was built with, or any of them)."""
        emb, idx = self._embed_scoped(feats, nodes, scope)
        n = int(emb.shape[0]) if idx is None else int(idx.numel())
        C = self.model.linear.weight.shape[0]
        out = torch.empty((n, C), dtype=torch.float32, device=self.device)
        with torch.no_grad():
            for a, b in _chunks(n, ROW_CHUNK):
                out[a:b] = self._head(self._take(emb, idx, a, b), None, 0, True)[0]
        return out

    def evaluate(self, feats, nodes, labels, sigmoid_loss: bool = True, mode: Optional[int] = None,
                 scope="graph") -> dict:
        """Loss and F1 of ``nodes`` (None: all) against ``labels`` (one float row of C entries per
        node of ``nodes``, host or device): chunks of nodes through the evaluation head, accumulated
        in train.Evaluator's buffer, one host copy at the end. Returns ``Evaluator.result()``'s keys;
        the pooled (tp, fp, fn) counts stay in ``self.last_counts``. ``scope`` as ``logits``."""
        from .train import Evaluator

        emb, idx = self._embed_scoped(feats, nodes, scope)
        n = int(emb.shape[0]) if idx is None else int(idx.numel())
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
