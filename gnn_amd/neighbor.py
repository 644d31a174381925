"""Node-wise neighbour sampling (GraphSAGE's sampler) with a fanout per layer, drawn on the device
over the resident graph.

The layer-wise samplers (``loader.KINDS``) draw on the host from U's column counts. Here every
output row draws on its own: row r of degree d keeps k = min(d, f) of its entries, a uniform
k-subset without replacement, each with the weight ``float32(1 / k)`` — ``lap``'s 1/d times d/k, an
unbiased estimate of ``lap[r, :]`` and the row itself whenever d <= f. No column counts exist.

A layer has output rows ``rows`` (node ids); its input set is ``rows ∪ kept columns`` in ascending
order, its columns are positions in that set and ``sampled_nodes[l]`` the positions of ``rows`` in
it. Layers are drawn from the top down: the top layer's rows are the batch nodes in the caller's
order (duplicates allowed), every lower layer's rows are the set above it; an order-0 layer takes
``None`` and an empty ``sampled_nodes`` and passes its set down unchanged, as the other samplers do.

The draw is a pure integer function of (seed, layer, node id, d, f) — include/gnn_extract.h states
it, ``neighbor_keep`` restates it in numpy (the tests' oracle) and gnn_nbr_draw runs it a wave per
row — so a row's entries do not depend on its place in the batch or on the device:
``neighbor_sample_host`` builds in numpy the batch ``NeighborSampler.sample`` builds on the GPU,
array for array. ``layer`` is the model's layer index (0 = the bottom layer, as ``adjs``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence

import numpy as np
import scipy.sparse as sp
import torch

from . import custom_sparse_ops as cso
from .sampler import device_graph, native_graph

MAX_FANOUT = 64


def _u32(x) -> np.ndarray:
    return (np.asarray(x).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def mix32(x) -> np.ndarray:
    """sage.hip's "lowbias32" hash over uint32 (arrays or scalars), in 32-bit arithmetic."""
    x = np.array(x, dtype=np.uint32, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def layer_key(seed, layer: int) -> np.ndarray:
    """key = mix32((mix32(lo32(seed) ^ 0x9e3779b9) ^ hi32(seed)) + layer * 0x85EBCA6B), uint32."""
    s = np.asarray(seed).astype(np.uint64)
    lo, hi = _u32(s), _u32(s >> np.uint64(32))
    with np.errstate(over="ignore"):
        return mix32((mix32(lo ^ np.uint32(0x9E3779B9)) ^ hi) + _u32(int(layer) * 0x85EBCA6B))


def batch_seed(seed: int, b: int) -> int:
    """The draw seed of batch b of a pass seeded ``seed``: lo32(seed) in the low word,
    hi32(seed) ^ mix32(b + 1) in the high one — distinct batches get distinct layer keys."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed & 0xFFFFFFFF) | ((((seed >> 32) ^ int(mix32(_u32(b + 1)))) & 0xFFFFFFFF) << 32)


def _floyd(rk: np.ndarray, d: np.ndarray, k: int) -> np.ndarray:
    """Floyd's algorithm for T rows at once: rk uint32[T], d int64[T] (all > k >= 1); the kept
    positions int64[T, k], ascending per row."""
    T = rk.shape[0]
    S = np.empty((T, k), dtype=np.int64)
    for s in range(k):
        j = d - k + s
        u = mix32(rk ^ mix32(np.uint32((s + 0x632BE5AB) & 0xFFFFFFFF)))
        t = ((u.astype(np.uint64) * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        hit = (S[:, :s] == t[:, None]).any(axis=1)
        S[:, s] = np.where(hit, j, t)
    S.sort(axis=1)
    return S


def neighbor_keep(seed, layer: int, node, d: int, f: int) -> np.ndarray:
    """The positions in [0, d) a row of degree ``d`` keeps at fanout ``f``: k = min(d, f) distinct
    positions in ascending order, int64. ``seed`` and ``node`` may be arrays (broadcast against
    each other); the result then has their shape plus a last axis of k."""
    d, f = int(d), int(f)
    if not 1 <= f <= MAX_FANOUT:
        raise ValueError(f"neighbor_keep: fanout {f} outside [1, {MAX_FANOUT}]")
    if d < 0:
        raise ValueError("neighbor_keep: negative degree")
    key = layer_key(seed, layer)
    rk = mix32(_u32(node) ^ key)
    shape = rk.shape
    if d <= f:
        return np.broadcast_to(np.arange(d, dtype=np.int64), shape + (d,)).copy()
    flat = rk.reshape(-1)
    return _floyd(flat, np.full(flat.shape[0], d, dtype=np.int64), f).reshape(shape + (f,))


def _kept_entries(indptr: np.ndarray, rows: np.ndarray, f: int, key: np.ndarray):
    """(rowptr int32[M+1], the kept entries' offsets into the graph's index array int64[nnz]) of
    the draw of ``rows`` at fanout f under the layer key."""
    start = indptr[rows]
    deg = indptr[rows + 1] - start
    k = np.minimum(deg, f)
    rowptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    pos = np.arange(int(rowptr[-1]), dtype=np.int64) - np.repeat(rowptr[:-1], k)  # d <= f: every entry, 0 .. d-1
    big = deg > f
    if big.any():
        S = _floyd(mix32(_u32(rows[big]) ^ key), deg[big].astype(np.int64), f)
        pos[(rowptr[:-1][big][:, None] + np.arange(f)[None, :]).reshape(-1)] = S.reshape(-1)
    return rowptr.astype(np.int32), pos + np.repeat(start, k)


@dataclass
class HostNeighborBatch:
    """``neighbor_sample_host``'s result. ``layers[l]``: (rowptr int32[M+1], col int32[nnz],
    val float32[nnz], (M, K)) or None for an order-0 layer; ``sampled_nodes[l]`` int64;
    ``input_nodes`` = ``sets[0]``; ``sets[l]`` the ascending int64 input set of layer l and
    ``sets[L]`` the batch nodes as given. Unpacks as (layers, sampled_nodes, input_nodes)."""
    layers: list
    sampled_nodes: List[np.ndarray]
    input_nodes: np.ndarray
    sets: List[np.ndarray]

    def __iter__(self):
        return iter((self.layers, self.sampled_nodes, self.input_nodes))


def _fanout_list(fanouts, orders) -> List[Optional[int]]:
    """One fanout per layer (None for an order-0 layer) from one int or one per aggregating layer."""
    orders = [int(o) for o in orders]
    if not orders or any(o not in (0, 1) for o in orders):
        raise ValueError(f"neighbor sampling: orders must be a non-empty list of 0 / 1, got {orders}")
    nagg = sum(orders)
    fl = [int(fanouts)] * nagg if np.ndim(fanouts) == 0 else [int(f) for f in fanouts]
    if len(fl) != nagg:
        raise ValueError(f"neighbor sampling: {len(fl)} fanouts for {nagg} aggregating layers (orders {orders})")
    if any(not 1 <= f <= MAX_FANOUT for f in fl):
        raise ValueError(f"neighbor sampling: fanouts must lie in [1, {MAX_FANOUT}], got {fl}")
    it = iter(fl)
    return [next(it) if o else None for o in orders]


def _graph_of(lap):
    g = native_graph(lap)
    if g.data is not None:
        raise ValueError("neighbor sampling: the graph stores values of its own (explicit zeros among its entries); "
                         "the draw weighs every entry of a row 1/deg")
    return g


def _batch_ids(batch_nodes, N: int) -> np.ndarray:
    q = np.asarray(batch_nodes.cpu() if isinstance(batch_nodes, torch.Tensor) else batch_nodes).reshape(-1)
    if q.size and (q.dtype.kind not in "iu" or q.min() < 0 or q.max() >= N):
        raise ValueError(f"neighbor sampling: batch nodes must be integer ids in [0, {N})")
    return q.astype(np.int64)


def neighbor_sample_host(seed: int, batch_nodes, fanouts, lap, orders: Sequence[int]) -> HostNeighborBatch:
    """The whole batch in numpy: per layer (bottom-up, as ``adjs``) the operand pieces, the self
    positions and the layer-0 input nodes. ``fanouts``: one int, or one per aggregating layer
    bottom-up; ``lap`` a scipy matrix or a sampler.NativeGraph without stored values."""
    g = _graph_of(lap)
    fl = _fanout_list(fanouts, orders)
    L = len(fl)
    rows = _batch_ids(batch_nodes, g.num_nodes)
    layers, sampled, sets = [None] * L, [np.zeros(0, np.int64)] * L, [None] * (L + 1)
    sets[L] = rows
    for l in range(L - 1, -1, -1):
        if fl[l] is None:
            sets[l] = rows
            continue
        rowptr, ent = _kept_entries(g.indptr, rows, fl[l], layer_key(seed, l))
        ids = g.indices[ent].astype(np.int64)
        low = np.unique(np.concatenate([rows, ids]))
        k = np.diff(rowptr)
        with np.errstate(divide="ignore"):
            w = (1.0 / k.astype(np.float64)).astype(np.float32)
        layers[l] = (rowptr, np.searchsorted(low, ids).astype(np.int32), np.repeat(w, k), (int(rows.size), int(low.size)))
        sampled[l] = np.searchsorted(low, rows).astype(np.int64)
        sets[l] = rows = low
    return HostNeighborBatch(layers, sampled, sets[0], sets)


class NeighborBatch:
    """One sampled batch: ``x0`` (fp32 rows of ``input_nodes``), ``adjs`` (bottom-up; None for an
    order-0 layer), ``sampled_nodes`` (int64), ``labels`` (float32 rows of the batch nodes) and
    ``input_nodes`` (int64), on the sampler's device. Unpacks as the (x0, adjs, sampled_nodes,
    labels) of ``Trainer.step`` / ``Trainer.evaluate``."""

    __slots__ = ("x0", "adjs", "sampled_nodes", "labels", "input_nodes", "batch_nodes", "seed")

    def __init__(self, x0, adjs, sampled_nodes, labels, input_nodes, batch_nodes, seed):
        self.x0, self.adjs, self.sampled_nodes, self.labels = x0, adjs, sampled_nodes, labels
        self.input_nodes, self.batch_nodes, self.seed = input_nodes, batch_nodes, seed

    def __iter__(self):
        return iter((self.x0, self.adjs, self.sampled_nodes, self.labels))


class ResidentSampler:
    """What the samplers that draw over the resident graph share (``NeighborSampler`` here,
    ``layerwise.LayerwiseSampler``): the graph and the feature table on the device, the labels and
    X0 of a batch, the top layer's transpose and row map, and the passes. A subclass provides
    ``sample(batch_nodes, seed)``."""

    def _setup(self, orders, feats, labels_full, device) -> None:
        from .placed import PlacedFeatures

        who = type(self).__name__
        self.orders = [int(o) for o in orders]
        self.N = self.graph.num_nodes
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.native = dev.type == "cuda"
        self.placed = isinstance(feats, PlacedFeatures)
        if self.placed:
            if feats.device != dev:
                raise ValueError(f"{who}: feats (a PlacedFeatures) is on {feats.device}, the sampler on {dev}")
        elif not isinstance(feats, torch.Tensor) or feats.dim() != 2 or feats.dtype not in cso.FEAT_KIND:
            raise ValueError(f"{who}: feats must be a 2-D float32 / float16 / bfloat16 tensor or a PlacedFeatures")
        if feats.shape[0] != self.N:
            raise ValueError(f"{who}: feats has {feats.shape[0]} rows, the graph {self.N} nodes")
        if labels_full.shape[0] != self.N:
            raise ValueError(f"{who}: labels_full has {labels_full.shape[0]} rows, the graph {self.N} nodes")
        self.labels_full = labels_full
        self.F = int(feats.shape[1])
        if self.native:
            self.dgraph = device_graph(self.graph, dev)
            self.feats = feats if self.placed else self._resident(feats)
        else:
            if not self.placed and feats.is_cuda:
                raise ValueError(f"{who}: device='cpu' takes a host feature table")
            self.dgraph = None
            self.feats = feats

    # ------------------------------------------------------------------ set-up
    def _free_bytes(self) -> int:
        free, _ = torch.cuda.mem_get_info(self.device)
        return int(free) + int(torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device))

    def _resident(self, feats: torch.Tensor) -> torch.Tensor:
        """The table on the device with unit column stride: itself, or one upload into whole-line rows."""
        from . import _lib
        from .staging import padded_ld

        if feats.is_cuda:
            if feats.device != self.device:
                raise ValueError(f"{type(self).__name__}: feats is on another device")
            return feats if feats.stride(1) == 1 else feats.contiguous()
        esz = feats.element_size()
        ld = padded_ld(self.F, 128 // esz)
        need = self.N * ld * esz
        free = self._free_bytes()
        if need > free:
            raise RuntimeError(f"{type(self).__name__}: the feature table needs {need} bytes of device memory, "
                               f"{free} free: a partially buffered feature store is out of scope here "
                               "(placed.PlacedFeatures serves one)")
        with _lib.on_device(self.device):
            table = torch.zeros((self.N, ld), dtype=feats.dtype, device=self.device)[:, : self.F]
            table.copy_(feats)
        return table

    def _labels(self, q: np.ndarray) -> torch.Tensor:
        lf = self.labels_full
        if sp.issparse(lf):
            lab = np.asarray(lf[q].todense(), dtype=np.float32)
        elif isinstance(lf, torch.Tensor):
            lab = lf[torch.from_numpy(q)].to(torch.float32).cpu().numpy()
        else:
            lab = np.asarray(lf[q], dtype=np.float32)
        t = torch.from_numpy(np.ascontiguousarray(lab.reshape(q.size, -1)))
        return t.to(self.device) if self.native else t

    def _top_maps(self, op, sn: torch.Tensor, M: int, K: int, with_rmap: bool) -> None:
        """The backward's operand and the fused residual's row map of a layer above layer 0."""
        op.transpose()
        if with_rmap:
            rmap = torch.full((K,), -1, dtype=torch.int32, device=self.device)
            rmap[sn] = torch.arange(M, dtype=torch.int32, device=self.device)
            sn._gnn_rmap = rmap

    def _x0(self, idx: torch.Tensor) -> torch.Tensor:
        """feats[idx] as fp32 whole-line rows (16-bit rows widened exactly): gnn_gather_rows_*, or
        over a placed store gnn_gather_placed_f32."""
        from .staging import padded_ld

        if self.placed:
            return self.feats.gather(idx)
        n = int(idx.numel())
        x0 = torch.empty((n, padded_ld(self.F, 32)), dtype=torch.float32, device=self.device)[:, : self.F]
        if n:
            cso.gather_rows(self.feats, idx, x0, None, n=n)
        return x0

    def _x0_host(self, idx: torch.Tensor) -> torch.Tensor:
        """The ``device="cpu"`` form of ``_x0``."""
        return self.feats.gather(idx) if self.placed else self.feats[idx].float()

    # ------------------------------------------------------------------ passes
    def epoch(self, nodes, batch_size: int, seed: int, shuffle: bool = True, rank: int = 0,
              world_size: int = 1) -> Iterator[NeighborBatch]:
        """Batches of ``batch_size`` over ``nodes`` (shuffled by ``seed`` unless ``shuffle`` is
        False), the last one short; batch b draws under ``batch_seed(seed, b)``. With ``world_size``
        ranks the list — the same on every rank, the seed being the same — is cut into the
        reference's contiguous chunks of ceil(n / world_size) (sampler.py:170-175, as
        ``sampler.rank_batches``) and ``rank`` takes its own. A pass over a placed store ends with
        its ``check()``."""
        from .loader import sequential_chunks

        nodes = np.asarray(nodes)
        if not 0 <= rank < world_size:
            raise ValueError(f"{type(self).__name__}.epoch: rank {rank} outside a world of {world_size}")
        if shuffle:
            nodes = nodes[np.random.default_rng(int(seed) & 0xFFFFFFFFFFFFFFFF).permutation(len(nodes))]
        if world_size > 1:
            n = len(nodes)
            chunk_size = n // world_size + (1 if n % world_size else 0)
            nodes = nodes[rank * chunk_size: min((rank + 1) * chunk_size, n)]
        for b, chunk in enumerate(sequential_chunks(nodes, batch_size)):
            yield self.sample(chunk, batch_seed(seed, b))
        if self.placed:
            self.feats.check()

    def sequential(self, nodes, batch_size: int, seed: int = 0) -> Iterator[NeighborBatch]:
        """``nodes`` in order, in chunks of ``batch_size`` (validation / test passes)."""
        return self.epoch(nodes, batch_size, seed, shuffle=False)


class NeighborSampler(ResidentSampler):
    """Neighbour-sampled batches of ``lap`` for a model with layer ``orders`` (0 / 1, bottom-up).

    ``fanouts``: one int, or one per aggregating layer (bottom-up, as ``orders``), each in [1, 64].
    ``feats``: the float32 / float16 / bfloat16 feature table [N, F]; on a GPU it lives on the
    device (a host table is uploaded once; one that does not fit is refused with the byte count),
    or a ``placed.PlacedFeatures`` on the sampler's device: the table served from the placement's
    sources — this rank's buffer, the peers' buffers, the host table — by node id.
    ``labels_full``: dense or scipy-sparse [N, C]; a batch's rows are gathered on the host (the
    batch nodes are host data) and uploaded.

    On a GPU ``sample`` draws on the device over ``sampler.DeviceGraph``: per aggregating layer
    gnn_nbr_rowptr, gnn_nbr_draw, gnn_closure_mark over rows ++ kept ids, one small device-to-host
    read of (nnz, |set|, error flag), then gnn_closure_list, gnn_nbr_relabel, gnn_closure_rank and,
    above layer 0, the transpose; buffers are sized by the bound M * f before that read. The
    operands are ``CsrOperand``s with their transposes and row maps in place, so the native step
    takes the batch. With ``device="cpu"`` the same batches come from ``neighbor_sample_host`` as
    torch COO operands (``HostBatch.cpu_inputs``' construction).

    Batch nodes may repeat (scoring a list with repeats); the fused backward maps every input row
    to at most one output row, so train on unique batch nodes, as ``epoch`` yields them."""

    def __init__(self, lap, fanouts, orders, feats: torch.Tensor, labels_full, device):
        self.graph = _graph_of(lap)
        self.fanouts = _fanout_list(fanouts, orders)
        self._setup(orders, feats, labels_full, device)

    # ------------------------------------------------------------------ one batch
    def sample(self, batch_nodes, seed: int) -> NeighborBatch:
        """The batch of ``batch_nodes`` (integer node ids, any order) under the draw seed ``seed``."""
        q = _batch_ids(batch_nodes, self.N)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if not self.native:
            return self._sample_cpu(q, seed)
        from . import _lib

        dev, N, dg = self.device, self.N, self.dgraph
        Lb = _lib.lib()
        nl = len(self.orders)
        adjs: list = [None] * nl
        sampled: list = [None] * nl
        unique_top = np.unique(q).size == q.size
        with _lib.on_device(dev):
            st = _lib.stream_of(dev)
            E = int(dg.indices.numel())
            rows = torch.from_numpy(q.astype(np.int32)).to(dev)
            empty = torch.zeros(0, dtype=torch.int64, device=dev)
            top = True
            for l in range(nl - 1, -1, -1):
                f = self.fanouts[l]
                if f is None:
                    sampled[l] = empty
                    continue
                M = int(rows.numel())
                cap = M * f
                # (nnz, |set|, error flag): the layer's one device-to-host read
                word = torch.zeros(3, dtype=torch.int64, device=dev)
                err = word[2:].view(torch.int32)
                rowptr = torch.empty(M + 1, dtype=torch.int32, device=dev)
                # rows ++ kept ids, the set's seeds; the slots past nnz stay -1, which mark skips
                seeds = torch.full((M + cap,), -1, dtype=torch.int32, device=dev)
                seeds[:M] = rows
                ids = seeds[M:]
                val = torch.empty(cap, dtype=torch.float32, device=dev)
                wsb = max(Lb.gnn_nbr_workspace_bytes(M), Lb.gnn_closure_workspace_bytes(N))
                ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
                _lib.check(Lb.gnn_nbr_rowptr(dg.indptr.data_ptr(), N, E, rows.data_ptr(), M, f, rowptr.data_ptr(),
                                             word.data_ptr(), ws.data_ptr(), wsb, err.data_ptr(), st), "gnn_nbr_rowptr")
                _lib.check(Lb.gnn_nbr_draw(dg.indptr.data_ptr(), dg.indices.data_ptr(), N, E, rows.data_ptr(), M, f,
                                           seed, l, rowptr.data_ptr(), ids.data_ptr() if cap else None,
                                           val.data_ptr() if cap else None, cap, err.data_ptr(), st), "gnn_nbr_draw")
                table = torch.empty(Lb.gnn_closure_table_bytes(N), dtype=torch.uint8, device=dev)
                _lib.check(Lb.gnn_closure_mark(None, None, N, seeds.data_ptr(), M + cap, 0, table.data_ptr(),
                                               word[1:].data_ptr(), ws.data_ptr(), wsb, st), "gnn_closure_mark")
                nnz, K, flag = (int(v) for v in word.tolist())
                if flag:
                    raise RuntimeError(f"NeighborSampler: the device draw of layer {l} met a row or column outside "
                                       "the graph (the resident graph does not match its row pointer)")
                low = cso.closure_list(table, N, K)
                col = torch.empty(nnz, dtype=torch.int32, device=dev)
                val = val[:nnz]
                _lib.check(Lb.gnn_nbr_relabel(table.data_ptr(), N, ids.data_ptr() if nnz else None, nnz,
                                              col.data_ptr() if nnz else None, val.data_ptr() if nnz else None,
                                              err.data_ptr(), st), "gnn_nbr_relabel")
                sn = cso.closure_rank(table, N, rows)
                op = cso.CsrOperand(rowptr, col, val, (M, K))
                if l >= 1:
                    self._top_maps(op, sn, M, K, unique_top or not top)
                adjs[l], sampled[l] = op, sn
                rows, top = low, False
            input_nodes = rows.long()
            x0 = self._x0(input_nodes)
        return NeighborBatch(x0, adjs, sampled, self._labels(q), input_nodes, q, seed)

    def _sample_cpu(self, q: np.ndarray, seed: int) -> NeighborBatch:
        hb = neighbor_sample_host(seed, q, [f for f in self.fanouts if f is not None], self.graph, self.orders)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        adjs = []
        for lay in hb.layers:
            if lay is None:
                adjs.append(None)
                continue
            rowptr, col, _, (M, K) = lay
            # create_coo_tensor's CPU branch with the kept count as the row's degree and
            # normfact = 1: value = (float)((1.0 / k) * 1.0), the device draw's weight
            adjs.append(cso.create_coo_tensor(t(rowptr), t(rowptr), t(col), torch.ones(K), M, K))
        idx = t(hb.input_nodes.astype(np.int64))
        x0 = self._x0_host(idx)
        return NeighborBatch(x0, adjs, [t(s) for s in hb.sampled_nodes], self._labels(q), idx, q, seed)
