"""The subgraph sampler (the reference's sampler.py:7-88, ``--sampler subgraph``) drawn on the device
over the resident graph: ONE draw over the batch rows, one induced square operand for every layer
below the drawn one.

Let t be the topmost layer with ``orders[t] = 1`` and ``rows`` the batch nodes. The draw is
``layerwise``'s race over U = lap[rows, :] with layer = t — the same key, entry values, replicas,
counts and select, so its law is ``np.random.choice``'s on U's column counts and its stream is
another than the host sampler's MT19937 draw. ``after = unique(selected ∪ rows)`` and ``normfact``
(sampler.py:40) are that layer's; layer t gets adj = lap[rows, :][:, after], for the same
(rows, seed, samp_num) bit for bit the operand ``LayerwiseSampler`` hands its top layer. Every
aggregating layer below t gets S = lap[after, :][:, after] with the values
(float)((1.0 / deg(after[i])) * (double)normfact[col]) — the same normfact array (sampler.py:62) —
and ``sampled_nodes = arange(K)``: S is built once per batch and the same operand object goes to
each of them. The input nodes are ``after``. include/gnn_extract.h states the law and the two
launches S needs beyond the layer-wise draw's (gnn_sg_count, gnn_sg_finish).

``subgraph_race_host`` builds the batch in numpy (the GPU tests' oracle and the source of
``device="cpu"``), ``SubgraphSampler.sample`` builds it on the GPU, array for array.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import custom_sparse_ops as cso
from .layerwise import (_MASK, HostLayerwiseBatch, RaceSampler, _entries, _favoured_ids, _graph_of, _operand_of, _race,
                        _replicas, _samp_list, _scale_of, race_normfact, race_select)
from .neighbor import NeighborBatch, _batch_ids


def _plan(samp_num, orders):
    """(t, samp, lower): the drawn layer, its sample size — one int, or element [0] of the
    reference's list (sampler.py:28) — and the aggregating layers below t."""
    samp = int(samp_num) if np.ndim(samp_num) == 0 else int(np.asarray(samp_num).reshape(-1)[0])
    sl = _samp_list(samp, orders)  # the orders' and the size's refusals
    agg = [l for l, s in enumerate(sl) if s is not None]
    if not agg:
        raise ValueError(f"subgraph sampling: orders {list(orders)} hold no aggregating layer: there is nothing to draw")
    return agg[-1], samp, agg[:-1]


def _one_favoured(skewed_sampling_nodes, N: int) -> Optional[np.ndarray]:
    if skewed_sampling_nodes is None:
        return None
    if isinstance(skewed_sampling_nodes, (list, tuple)) and any(
            s is None or np.ndim(s) > 0 for s in skewed_sampling_nodes):
        raise ValueError("subgraph sampling: a per-layer list of favoured sets; the subgraph sampler draws once, so it "
                         "takes one id array (the reference's flatnonzero(device_id_of_nodes == device), for which "
                         "PlacedFeatures.resident_nodes('own') stands in)")
    return _favoured_ids(skewed_sampling_nodes, N)


def subgraph_operand(lap, rows, after, normfact):
    """(rowptr int32[M+1], col int32[nnz], val float32[nnz], (M, K)) of lap[rows, :][:, after]
    (``after`` ascending and unique) with the values (float)((1.0 / deg(rows[i])) *
    (double)normfact[col]): the top operand with the batch rows, the square one with rows = after."""
    g = _graph_of(lap)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    i, c, deg = _entries(g.indptr, g.indices, rows)
    return _operand_of(i, c, deg, np.asarray(after, dtype=np.int64), np.asarray(normfact, dtype=np.float32))


def subgraph_race_host(seed: int, batch_nodes, samp_num, lap, orders: Sequence[int], skewed_sampling_nodes=None,
                       scale_factor=1) -> HostLayerwiseBatch:
    """The whole batch in numpy, as ``layerwise.ladies_race_host`` returns one: layer t the top
    operand, every aggregating layer below it the SAME tuple of S's pieces, ``sets[l]`` = after for
    l <= t and the batch nodes above, ``s_num`` / ``normfact`` the one draw's at every aggregating
    layer. ``samp_num``: one int or the reference's list (element [0] is used)."""
    g = _graph_of(lap)
    t, samp, lower = _plan(samp_num, orders)
    L, N = len(orders), g.num_nodes
    scale = _scale_of(scale_factor)
    fav = _one_favoured(skewed_sampling_nodes, N)
    rows = _batch_ids(batch_nodes, N)
    i, c, deg = _entries(g.indptr, g.indices, rows)
    s = _replicas(N, fav, scale)
    counts, keys = _race(seed, t, N, i, c, s, rows.size)
    s_num, selected = race_select(counts, keys, samp)
    after = np.unique(np.concatenate([selected, rows]))
    nf = race_normfact(counts, after, s_num, None if s is None else counts * s)
    layers, sampled = [None] * L, [np.zeros(0, np.int64)] * L
    s_nums, nfs = [None] * L, [None] * L
    layers[t] = _operand_of(i, c, deg, after, nf)
    sampled[t] = np.searchsorted(after, rows).astype(np.int64)
    square = subgraph_operand(g, after, after, nf) if lower else None
    for l in lower:
        layers[l], sampled[l] = square, np.arange(after.size, dtype=np.int64)
    for l in lower + [t]:
        s_nums[l], nfs[l] = s_num, nf
    sets = [after] * (t + 1) + [rows] * (L - t)
    return HostLayerwiseBatch(layers, sampled, after, sets, s_nums, nfs)


class SubgraphSampler(RaceSampler):
    """Subgraph-sampler batches of ``lap`` for a model with layer ``orders`` (0 / 1, bottom-up), drawn
    by the race over the resident graph: one draw at the topmost aggregating layer t, the square
    operand lap[after, :][:, after] for every aggregating layer below it.

    ``samp_num``: one int, or the reference's ``samp_num_list``, of which element [0] is used.
    ``feats`` (a table or a ``placed.PlacedFeatures``) / ``labels_full`` / ``device`` and the methods
    ``sample`` / ``epoch`` / ``sequential`` as ``layerwise.LayerwiseSampler``; so is the batch, a
    ``NeighborBatch``. ``scale_factor`` (an integer in [1, 64]) with ``skewed_sampling_nodes`` (ONE id
    array) is the locality-skewed draw.

    On a GPU ``sample`` runs on the current stream the layer-wise draw's launches for layer t
    (mark(expand), list, gnn_lw_race_skew, gnn_lw_select, mark(rows ++ ids), list,
    gnn_lw_finish_skew), then — only when a layer below t aggregates — gnn_sg_count and gnn_sg_finish
    (S's column counts over lap^T, its transposed row pointer and its row segments), then ONE
    device-to-host read per batch, however many layers the model has: (K, the top operand's nnz, the
    colseg total, the sum of deg(after), the flags, S's nnz). Then ``extract_operand`` for the top
    operand (its transpose from ``CsrOperand.transpose()``, its row map only for unique batch nodes),
    ``extract_operand(rows = cols = after)`` for S — which builds S's transpose too when one of its
    layers lies above layer 0 — gnn_closure_rank, X0 and one ``dgraph.check()``. Buffers are sized
    before the read by cap = min(N, M + sum of deg(rows)) and kcap = min(N, M + min(cap, samp)).
    With ``device="cpu"`` the same batches come from ``subgraph_race_host`` as torch COO operands.

    An order-0 layer gets None and an empty int64 index, as the other device samplers hand it. (The
    reference hands every layer below t the square operand whatever its order; its model never
    reads the operand of an order-0 layer.)

    Out of scope, refused: weighted graphs, a non-integer scale_factor or one above 64,
    scale_factor > 1 with nothing to favour, a per-layer list of favoured sets, 2^26 batch rows or
    more under a skew; ``NativeLoader`` / ``Stager`` / ``bench.py`` keep the host draw."""

    def __init__(self, lap, samp_num, orders, feats, labels_full, device, scale_factor: float = 1.0,
                 skewed_sampling_nodes=None):
        self.scale = _scale_of(scale_factor)
        if self.scale > 1 and skewed_sampling_nodes is None:
            raise ValueError(f"SubgraphSampler: scale_factor {scale_factor} without skewed_sampling_nodes: there is "
                             "nothing to favour")
        self.graph = _graph_of(lap)
        self.top, self.samp, self.lower = _plan(samp_num, orders)
        self._setup(orders, feats, labels_full, device)
        f = _one_favoured(skewed_sampling_nodes, self.N)
        self.favoured = f if f is not None and f.size and self.scale > 1 else None  # None: the plain draw
        self._favoured_dev = self._favoured_table(self.favoured) if self.native and self.favoured is not None else None

    def sample(self, batch_nodes, seed: int) -> NeighborBatch:
        """The batch of ``batch_nodes`` (integer node ids, any order) under the draw seed ``seed``."""
        q = _batch_ids(batch_nodes, self.N)
        seed = int(seed) & _MASK
        if not self.native:
            hb = subgraph_race_host(seed, q, self.samp, self.graph, self.orders, self.favoured, self.scale)
            return self._host_batch(hb, q, seed)
        from . import _lib

        dev, N, dg = self.device, self.N, self.dgraph
        Lb = _lib.lib()
        t, lower = self.top, self.lower
        nl = len(self.orders)
        M = int(q.size)
        hp = dg.host_indptr
        with _lib.on_device(dev):
            st = _lib.stream_of(dev)
            rows = torch.from_numpy(q.astype(np.int32)).to(dev)
            rowseg_total = int((hp[q + 1] - hp[q]).sum())  # host data
            # words 9, 10: S's nnz and its rowseg total (the sum of deg(after) again); M + samp >= kcap
            d = self._draw(rows, rowseg_total, seed, t, self.samp, self._favoured_dev, extra_words=2,
                           extra_ws=Lb.gnn_sg_finish_workspace_bytes(min(N, M + self.samp)) if lower else 0)
            kcap = d.kcap
            if lower:
                colcnt = torch.empty(kcap, dtype=torch.int32, device=dev)
                colptr_s = torch.empty(kcap + 1, dtype=torch.int32, device=dev)
                rowseg_s = torch.empty(kcap + 1, dtype=torch.int32, device=dev)
                p = lambda x: x.data_ptr() if x.numel() else None
                _lib.check(Lb.gnn_sg_count(dg.indptr_t.data_ptr(), dg.indices_t.data_ptr(), N, int(dg.indices_t.numel()),
                                           p(d.after), d.word[4:].data_ptr(), kcap, d.table.data_ptr(), p(colcnt),
                                           d.err.data_ptr(), st), "gnn_sg_count")
                self._mark(t, "sg_count")
                _lib.check(Lb.gnn_sg_finish(dg.indptr.data_ptr(), int(dg.indices.numel()), N, p(d.after),
                                            d.word[4:].data_ptr(), kcap, p(colcnt), colptr_s.data_ptr(),
                                            rowseg_s.data_ptr(), d.word[9:].data_ptr(), d.ws.data_ptr(), d.wsb,
                                            d.err.data_ptr(), st), "gnn_sg_finish")
                self._mark(t, "sg_finish")
            K, nnz, colseg_total, deg_total, nnz_s, _ = self._read(d, t)  # the batch's one read
            after = d.after[:K]
            normfact = d.normfact[:K]
            adjs: list = [None] * nl
            sampled: list = [torch.zeros(0, dtype=torch.int64, device=dev)] * nl
            op = cso.extract_operand(dg, rows, after, normfact, nnz, d.rowseg, rowseg_total=rowseg_total)
            sn = cso.closure_rank(d.table, N, rows)
            if t >= 1:
                self._top_maps(op, sn, M, K, np.unique(q).size == M)
            adjs[t], sampled[t] = op, sn
            self._mark(t, "read+extract_top+rank+maps")
            if lower:
                if 2 * K + deg_total >= 2**31:
                    raise RuntimeError(f"SubgraphSampler: the square operand spans {deg_total} graph entries (>= 2^31)")
                tr = lower[-1] >= 1  # one of S's layers needs a backward: the extraction builds S^T as well
                sq = cso.extract_operand(dg, after, after, normfact, nnz_s, rowseg_s[: K + 1],
                                         d.colseg[: K + 1] if tr else None, colptr_s[: K + 1] if tr else None,
                                         rowseg_total=deg_total, colseg_total=colseg_total if tr else None)
                ar = torch.arange(K, dtype=torch.int64, device=dev)
                if tr:
                    self._top_maps(sq, ar, K, K, True)  # the transpose is in place; the row map is the identity
                for l in lower:
                    adjs[l], sampled[l] = sq, ar
                self._mark(t, "extract_square")
            dg.check()  # the extractions' flag
            input_nodes = after.long()
            x0 = self._x0(input_nodes)
        return NeighborBatch(x0, adjs, sampled, self._labels(q), input_nodes, q, seed)
