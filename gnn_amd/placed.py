"""X0 by node id over a placed feature store: the device draws' way to the placement's three sources.

The host samplers split a batch's input nodes by source on the CPU (sampler.py:150-158, the masks
and slot lists ``staging.make_plan`` turns into a ``StagePlan``). A device draw
(``neighbor.NeighborSampler``, ``layerwise.LayerwiseSampler``) cannot: its input nodes exist only
on the device. Here the placement itself lives there, as one int32 per node — this rank's view of
the reference's ``device_id_of_nodes`` and ``idx_of_nodes_on_device`` (preprocess.py:343-386):

    place[v] = PLACE_HOST (-1)             row v of the host table
             = src << PLACE_SHIFT | slot   row ``slot`` of source ``src``

Source 0 is the rank's own buffer, sources 1.. are the peers' buffers in ``devices`` order (mapped
by ``staging.PeerDirect``). ``gnn_gather_placed_f32`` (include/gnn_spmm.h) looks every node up and
reads its row from where the map says, in one launch: no host mask, no compaction, no
device-to-host read. ``placed_gather_host`` restates it in numpy (the tests' oracle, and what
``device="cpu"`` runs). DESIGN.md §3.17.
"""
from __future__ import annotations

import weakref
from typing import Optional, Sequence

import numpy as np
import torch

from . import custom_sparse_ops as cso

PLACE_HOST = -1
PLACE_SHIFT = 27
MAX_SOURCES = 16
_SLOT_MASK = (1 << PLACE_SHIFT) - 1


def pack_placement(device_id_of_nodes, idx_of_nodes_on_device, devices: Sequence[int], rank: int) -> np.ndarray:
    """One rank's placement map, int32[N]: PLACE_HOST where ``device_id_of_nodes`` is -1, else
    ``src << PLACE_SHIFT | idx_of_nodes_on_device`` with src 0 for ``devices[rank]`` and 1.. for
    the other devices in ``devices`` order."""
    devices = [int(d) for d in devices]
    if len(devices) > MAX_SOURCES:
        raise ValueError(f"pack_placement: {len(devices)} devices, the map names at most {MAX_SOURCES} sources")
    if not 0 <= rank < len(devices):
        raise ValueError(f"pack_placement: rank {rank} outside the {len(devices)} devices")
    dev = np.asarray(device_id_of_nodes).astype(np.int64)
    idx = np.asarray(idx_of_nodes_on_device).astype(np.int64)
    if dev.shape != idx.shape or dev.ndim != 1:
        raise ValueError("pack_placement: device ids and slots must be 1-D arrays of one length")
    on = dev != -1
    src_of = {devices[rank]: 0}
    for d in devices[:rank] + devices[rank + 1:]:
        src_of.setdefault(d, len(src_of))
    unknown = np.setdiff1d(np.unique(dev[on]), np.fromiter(src_of, np.int64, len(src_of)))
    if unknown.size:
        raise ValueError(f"pack_placement: device id {int(unknown[0])} is not among the devices {devices}")
    if on.any() and (idx[on].min() < 0 or idx[on].max() > _SLOT_MASK):
        raise ValueError(f"pack_placement: a buffer slot outside [0, 2^{PLACE_SHIFT})")
    lut = np.zeros(max(src_of) + 1 if src_of else 1, dtype=np.int64)
    for d, s in src_of.items():
        lut[d] = s
    place = np.full(dev.shape[0], PLACE_HOST, dtype=np.int32)
    place[on] = ((lut[dev[on]] << PLACE_SHIFT) | idx[on]).astype(np.int32)
    return place


def widen_rows(t: torch.Tensor) -> torch.Tensor:
    """``t.float()`` with every NaN word fixed to the IEEE conversion's: the sign, a quiet NaN, the
    payload moved up (fp16: 13 bits; bf16: the pattern itself, 16 bits up) — what the GPU's convert
    stores. torch's CPU conversion of an fp16 NaN depends on where the element falls (the vector
    body gives this word, the scalar tail 0x7fffffff), so a restatement cannot leave it to that."""
    x = t.float()
    if t.dtype == torch.float32 or not bool(torch.isnan(x).any()):
        return x
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    if t.dtype == torch.bfloat16:
        w = b << 16
    else:
        w = ((b & 0x8000) << 16) | 0x7FC00000 | ((b & 0x3FF) << 13)
    nan = torch.isnan(x)
    xi = x.view(torch.int32)
    xi[nan] = w.to(torch.int32)[nan]
    return x


def placed_gather_host(place, sources, host_table: Optional[torch.Tensor], nodes, F: Optional[int] = None,
                       info: bool = False):
    """gnn_gather_placed_f32 on the host: float32 [n, F] rows of ``nodes`` (any integer array) from
    ``sources`` (2-D CPU tensors, or None for a source without a buffer) and ``host_table`` (or
    None), one kind throughout, 16-bit rows widened exactly (``widen_rows``). A row the map cannot
    serve — a node outside the map, a source the list does not hold, a slot past its source's rows,
    a missing buffer or host table — is zeros and sets the flag. With ``info`` returns (rows, counts
    int64[nsrc + 1] with the host last, flag)."""
    place = np.asarray(place.cpu() if isinstance(place, torch.Tensor) else place).astype(np.int64)
    nodes = np.asarray(nodes.cpu() if isinstance(nodes, torch.Tensor) else nodes).astype(np.int64).reshape(-1)
    nsrc = len(sources)
    if F is None:
        F = next(int(t.shape[1]) for t in list(sources) + [host_table] if t is not None)
    out = torch.zeros((nodes.size, F), dtype=torch.float32)
    counts = np.zeros(nsrc + 1, dtype=np.int64)
    valid = (nodes >= 0) & (nodes < place.size)
    p = np.where(valid, place[np.where(valid, nodes, 0)], 0)
    is_host = valid & (p == PLACE_HOST)
    src = (p & 0xFFFFFFFF) >> PLACE_SHIFT  # the word as unsigned: a negative value names no source
    slot = p & _SLOT_MASK
    served = np.zeros(nodes.size, dtype=bool)
    if host_table is not None and host_table.shape[1] >= F:
        sel = np.flatnonzero(is_host)
        out[torch.from_numpy(sel)] = widen_rows(host_table[torch.from_numpy(nodes[sel]), :F])
        served[sel] = True
        counts[nsrc] = sel.size
    for s, t in enumerate(sources):
        if t is None or t.shape[1] < F:
            continue
        sel = np.flatnonzero(valid & ~is_host & (src == s) & (slot < t.shape[0]))
        out[torch.from_numpy(sel)] = widen_rows(t[torch.from_numpy(slot[sel]), :F])
        served[sel] = True
        counts[s] = sel.size
    flag = int(not served.all())
    return (out, counts, flag) if info else out


def _host_unregister(ptr: int, device) -> None:
    from . import _lib

    try:
        torch.cuda.synchronize(device)  # no gather still in flight reads the table
    except RuntimeError:  # interpreter shutdown / a device already in error: unregister anyway
        pass
    with _lib.on_device(device):
        _lib.lib().gnn_host_unregister(ptr)


class PlacedFeatures:
    """A feature table served from where the placement put its rows: what the device samplers take
    as ``feats`` when the table does not live whole on their GPU.

    ``host_table``: the CPU table [N, F] (float32 / float16 / bfloat16, unit column stride; a table
    without one is made contiguous), or None when no node is host-placed. ``place``: the map of
    ``pack_placement`` (int32[N]). ``sources``: per source a tensor on ``device`` (rows of the
    table's dtype, unit column stride), a ``(pointer, rows, ld)`` triple — ``PeerDirect.peers[j]`` —
    or None for a source that buffers nothing. On a GPU the host table is registered where it is
    (gnn_host_register: pinned and mapped, no copy; ``registered=True``: the caller has done so),
    unless no node is host-placed, and released by ``close()`` or a finalizer, after a device
    sync. ``validate`` checks the map against the sources on the host, once; the kernel's own guards
    (zero row + flag, ``check()``) hold either way.

    ``gather(nodes)`` is X0: fp32 whole-line rows of ``nodes`` (int32 / int64 on the device),
    stream-ordered, nothing read back. ``counts()`` are the rows each source has served since
    ``reset_counts()`` — the buffer hit rate."""

    def __init__(self, host_table: Optional[torch.Tensor], place, sources, device, F: Optional[int] = None,
                 registered: bool = False, validate: bool = True):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.native = dev.type == "cuda"
        place = np.ascontiguousarray(place.cpu().numpy() if isinstance(place, torch.Tensor) else place)
        if place.ndim != 1 or place.dtype != np.int32:
            raise ValueError("PlacedFeatures: place must be a 1-D int32 array (pack_placement's)")
        self.N = int(place.shape[0])
        sources = list(sources)
        if not 1 <= len(sources) <= MAX_SOURCES:
            raise ValueError(f"PlacedFeatures: {len(sources)} sources, the map names 1 to {MAX_SOURCES}")
        tensors = [t for t in sources + [host_table] if isinstance(t, torch.Tensor)]
        if not tensors:
            raise ValueError("PlacedFeatures: neither a host table nor a source tensor to take the dtype from")
        self.dtype = tensors[0].dtype
        if self.dtype not in cso.FEAT_KIND:
            raise ValueError(f"PlacedFeatures: rows must be float32, float16 or bfloat16, got {self.dtype}")
        self.kind = cso.FEAT_KIND[self.dtype]
        if F is None:
            F = int(host_table.shape[1]) if host_table is not None else min(int(t.shape[1]) for t in tensors)
        self.F = int(F)
        self.shape = (self.N, self.F)
        esz = tensors[0].element_size()
        for t in tensors:
            if t.dim() != 2 or t.dtype != self.dtype or t.shape[1] < self.F:
                raise ValueError(f"PlacedFeatures: every source and the host table hold 2-D {self.dtype} rows of at "
                                 f"least {self.F} columns")
        has_host = bool((place == PLACE_HOST).any())
        if host_table is not None:
            if host_table.is_cuda:
                raise ValueError("PlacedFeatures: host_table is a CPU tensor")
            if host_table.shape[0] != self.N:
                raise ValueError(f"PlacedFeatures: host_table has {host_table.shape[0]} rows, the map {self.N} nodes")
            if host_table.stride(1) != 1 and host_table.shape[0] > 1:
                host_table = host_table.contiguous()
        elif has_host and validate:
            raise ValueError("PlacedFeatures: the map places nodes on the host and there is no host table")
        # (base, ld, rows) per source; tensors are kept alive here
        self._keep, trip = [], []
        for s, t in enumerate(sources):
            if t is None:
                trip.append((0, 0, 0))
            elif isinstance(t, torch.Tensor):
                if t.device != dev:
                    raise ValueError(f"PlacedFeatures: source {s} is on {t.device}, not on {dev}")
                if t.stride(1) != 1 and t.shape[0] > 1:
                    t = t.contiguous()
                self._keep.append(t)
                trip.append((t.data_ptr() if t.shape[0] else 0, int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]),
                             int(t.shape[0])))
            else:
                ptr, rows, ld = t
                if validate and int(ld) < self.F:
                    raise ValueError(f"PlacedFeatures: source {s} has rows of {ld} elements, F is {self.F}")
                trip.append((int(ptr), int(ld), int(rows)))
        self.sources = trip
        self.nsrc = len(trip)
        if validate:
            on = place != PLACE_HOST
            src = (place[on].astype(np.int64) & 0xFFFFFFFF) >> PLACE_SHIFT
            slot = place[on].astype(np.int64) & _SLOT_MASK
            rows = np.array([r for _, _, r in trip] + [0] * (32 - self.nsrc), dtype=np.int64)
            if src.size and (src.max() >= self.nsrc or (slot >= rows[src]).any()):
                raise ValueError("PlacedFeatures: the map names a source or a slot the sources do not hold")
        self._place_host = place
        self._host = host_table
        self._unregister = None
        self._host_ptr, self._ld_host = None, 0  # the registered table, on a GPU
        self._total = np.zeros(self.nsrc + 1, dtype=np.int64)  # the cpu form's counts and flag
        self._bad = 0
        if not self.native:
            if any(not isinstance(t, torch.Tensor) and t is not None for t in sources):
                raise ValueError("PlacedFeatures: device='cpu' takes CPU tensors as sources")
            self._cpu_sources = [t if isinstance(t, torch.Tensor) else None for t in sources]
            return
        from . import _lib

        with _lib.on_device(dev):
            self._place = torch.from_numpy(place).to(dev)
            rec = np.zeros(self.nsrc, dtype=[("base", "<u8"), ("ld", "<i8"), ("rows", "<i8")])
            for s, (b, ld, r) in enumerate(trip):
                rec[s] = (b, ld, r)
            self._srcs = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)  # gnn_place_src[nsrc]
            self._words = torch.zeros(self.nsrc + 2, dtype=torch.int64, device=dev)  # counts, then the flag
            self._counts = self._words[: self.nsrc + 1]
            self._flag = self._words[self.nsrc + 1:].view(torch.int32)
            if has_host and host_table is not None:
                self._host_ptr = host_table.data_ptr()
                self._ld_host = int(host_table.stride(0)) if self.N > 1 else self.F
                if not registered:
                    span = ((self.N - 1) * self._ld_host + int(host_table.shape[1])) * esz
                    _lib.check(_lib.lib().gnn_host_register(self._host_ptr, span), "gnn_host_register")
                    self._unregister = weakref.finalize(self, _host_unregister, self._host_ptr, dev)

    # ------------------------------------------------------------------ construction from a store
    @classmethod
    def from_store(cls, store, placement, rank: int, devices: Optional[Sequence[int]] = None, peers=None,
                   validate: bool = True) -> "PlacedFeatures":
        """Over ``store`` (``staging.FeatureStore``: this rank's buffer and the host table) and the
        ``placement`` every rank computes (``placement.create_buffer``). With ``peers`` (a
        ``staging.PeerDirect`` over the same store) the mapped peer buffers are sources 1..; without
        it, nodes buffered only on a peer are read from the host table, which every rank holds in
        full."""
        world = len(placement.device_id_of_nodes_group)
        devices = list(range(world)) if devices is None else list(devices)
        place = pack_placement(placement.device_id_of_nodes_group[rank], placement.idx_of_nodes_on_device_group[rank],
                               devices, rank)
        sources: list = [store.gpu_buffer]
        if peers is not None:
            if peers.world != world or peers.rank != rank:
                raise ValueError(f"PlacedFeatures.from_store: peers is rank {peers.rank} of {peers.world}, the "
                                 f"placement rank {rank} of {world}")
            sources += [peers.peers[j] for j in range(world) if j != rank]
        else:
            place[(place != PLACE_HOST) & ((place >> PLACE_SHIFT) != 0)] = PLACE_HOST
        # a zero-copy store has registered its table, and torch's pinned memory is mapped already
        registered = store.zero_copy or (torch.device(store.device).type == "cuda" and store.host.is_pinned())
        return cls(store.host, place, sources, store.device, F=store.F, registered=registered, validate=validate)

    # ------------------------------------------------------------------ the gather
    def gather(self, nodes: torch.Tensor, out: Optional[torch.Tensor] = None, count: bool = True) -> torch.Tensor:
        """fp32 rows [n, F] of ``nodes`` (whole 128-byte-line rows unless ``out`` is given).
        ``count=False`` leaves ``counts()`` out of this call (the kernel then tallies nothing)."""
        from .staging import padded_ld

        if not isinstance(nodes, torch.Tensor) or nodes.dim() != 1 or nodes.dtype not in (torch.int32, torch.int64):
            raise ValueError("PlacedFeatures.gather: nodes must be a 1-D int32 / int64 tensor")
        n = int(nodes.numel())
        if not self.native:
            x, counts, flag = placed_gather_host(self._place_host, self._cpu_sources, self._host, nodes, self.F,
                                                 info=True)
            if count:
                self._total += counts
            self._bad |= flag
            if out is not None:
                out[:, : self.F] = x
                return out
            return x
        from . import _lib

        dev = self.device
        if nodes.device != dev:
            raise ValueError(f"PlacedFeatures.gather: nodes are on {nodes.device}, the store on {dev}")
        with _lib.on_device(dev):
            if out is None:
                out = torch.empty((n, padded_ld(self.F, 32)), dtype=torch.float32, device=dev)[:, : self.F]
            elif (out.dtype != torch.float32 or out.device != dev or out.dim() != 2 or out.shape[0] != n
                  or out.shape[1] != self.F or (out.stride(1) != 1 and n > 0)):
                raise ValueError(f"PlacedFeatures.gather: out must be float32 [{n}, {self.F}] rows on {dev}")
            if n == 0 or self.F == 0:
                return out
            ids = nodes.to(torch.int32).contiguous()
            _lib.check(_lib.lib().gnn_gather_placed_f32(self._place.data_ptr(), self.N, self._srcs.data_ptr(),
                                                        self.nsrc, self._host_ptr, self._ld_host, self.kind,
                                                        ids.data_ptr(), n, out.data_ptr(),
                                                        out.stride(0) if n > 1 else max(out.stride(0), self.F), self.F,
                                                        self._counts.data_ptr() if count else None,
                                                        self._flag.data_ptr(),
                                                        _lib.stream_of(dev)), "gnn_gather_placed_f32")
        return out

    def resident_nodes(self, which: str = "own") -> np.ndarray:
        """Node ids (int64, ascending) the map serves without the host link: ``"own"`` those of source
        0, this rank's buffer (what the reference's subgraph sampler skews by); ``"device"`` those of any
        source, the union of the buffers. The bottom layer's favoured set of a locality-skewed draw
        (``layerwise.LayerwiseSampler(..., skewed_sampling_nodes=...)``)."""
        if which not in ("own", "device"):
            raise ValueError(f"PlacedFeatures.resident_nodes: which is 'own' or 'device', got {which!r}")
        place = self._place_host
        on = place != PLACE_HOST
        if which == "own":
            on &= ((place.astype(np.int64) & 0xFFFFFFFF) >> PLACE_SHIFT) == 0
        return np.flatnonzero(on).astype(np.int64)

    # ------------------------------------------------------------------ counters and the flag
    def _read(self) -> np.ndarray:
        return self._words.cpu().numpy() if self.native else np.concatenate([self._total, [self._bad]])

    def counts(self) -> dict:
        """Rows served per source since the last reset (one device-to-host read): ``own``, ``peers``
        (sources 1.. in order), ``host`` and their ``total``."""
        w = self._read()
        c = [int(v) for v in w[: self.nsrc + 1]]
        return {"own": c[0], "peers": c[1: self.nsrc], "host": c[self.nsrc], "total": sum(c)}

    def reset_counts(self) -> None:
        if self.native:
            self._counts.zero_()
        else:
            self._total[:] = 0

    def check(self) -> None:
        """Raise if a gather met a row it could not serve (one device-to-host read)."""
        if int(self._read()[self.nsrc + 1]) & 0xFFFFFFFF:
            raise RuntimeError("PlacedFeatures: a gather met a node outside the placement map, or one the map sends "
                               "to a source, slot or host table that is not there (its rows are zeros)")

    def close(self) -> None:
        """Release the host table's registration (after a device sync). The store serves no gather after."""
        if self._unregister is not None:
            self._unregister()
            self._unregister = None
        if self.native:
            self._host_ptr = None
