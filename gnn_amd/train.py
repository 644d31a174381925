"""Data-parallel training step (main.py:122-170), one process per GPU.

Reference: per-rank threads in one process; grads flattened with torch.cat, published in a
shared list, ``threading.Barrier``, summed with P2P ``.to(device)`` copies (main.py:149-168);
per-rank clip_grad_norm_(5) BEFORE the sum and no averaging (main.py:146,159).

Here: one process per GPU with torch.distributed (backend "nccl" = RCCL over xGMI). By default
the per-rank clip writes the clipped gradients straight into one flat fp32 buffer (one kernel,
gnn_amd.optim), summed with ONE in-place ``all_reduce(SUM)``, and Adam reads them as views of
that buffer; at N = 1 the clip factor is applied inside the Adam launch. With the native step
executor and GNN_DP_BUCKETS=1 the exchange is bucketed per backward stage and overlapped with
the backward instead (gnn_amd.dp: all-to-all of unscaled shards as each stage finishes, then
the ranks' clip factors, the weighted shard sums and one gather — the same
per-rank-clip-then-sum, bit-identical at world 2); bench.py times both at N > 1. (On the CPU
— the gloo tests — the same semantics run through torch's clip_grad_norm_ and Adam.)
Gradients are reset to None each step, so autograd hands its freshly computed tensors over
instead of accumulating into old ones. Initial weights are broadcast from rank 0 (the
reference never syncs them: SURVEY.md Appendix B, F).
"""
from __future__ import annotations

import os
from typing import Optional

import torch
from torch._utils import _flatten_dense_tensors, _unflatten_dense_tensors

from .models import loss as loss_fn


class Trainer:
    def __init__(self, model: torch.nn.Module, lr: float, device, group=None, sigmoid_loss: bool = True,
                 clip: float = 5.0, gemm=None):
        self.model = model
        self.device = torch.device(device)
        self.sigmoid_loss = sigmoid_loss
        self.clip = clip
        self.group = group
        self.params = [p for p in model.parameters() if p.requires_grad]
        # The reference's default Adam (main.py:102) and clip_grad_norm_(5) (main.py:146).
        self.native = self.device.type == "cuda"
        if self.native:
            # The layer GEMMs (15k x 602..1024 x 512, fp32): rocBLAS ("cublas" on ROCm builds)
            # measured faster than hipBLASLt on MI355X (317 vs 294 mini-batches/s, same box).
            torch.backends.cuda.preferred_blas_library("cublas")
            # clip + Adam in two HIP launches (gnn_amd.optim, include/gnn_optim.h)
            from .optim import ClipAdam

            self.optimizer = ClipAdam(self.params, lr=lr, max_norm=clip)
        else:
            self.optimizer = torch.optim.Adam(self.params, lr=lr)
        # the whole forward + backward as one native call when the model allows it
        # (gnn_amd.executor, include/gnn_step.h); GNN_NATIVE_STEP=0 keeps the autograd path
        self.executor = None
        if self.native:
            from . import executor as ex

            if ex.enabled():
                try:
                    self.executor = ex.NativeStep(model, sigmoid_loss=sigmoid_loss, gemm=gemm)
                except ValueError as e:
                    self.executor = None
                    if gemm is not None:
                        raise ValueError(f"Trainer: gemm={gemm!r} needs the native step executor ({e})") from e
        # the layers' GEMM precision (NativeStep's ``gemm``: "split3", "split2", "bf16" or one name per
        # layer) lives in the executor's descriptor; the Python path reads only GNN_GEMM_ALGO
        if gemm is not None and self.executor is None:
            raise ValueError("Trainer: gemm= needs the native step executor (a fused model on a GPU, "
                             "GNN_NATIVE_STEP not 0); the Python path takes its GEMM mode from GNN_GEMM_ALGO")
        self.world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world = torch.distributed.get_world_size(group)
        # the data-parallel branch of step() (clip into the flat buffer, all-reduce, Adam on the
        # sum): every N > 1 run; tests/test_rccl_gpu.py also drives it through a 1-rank RCCL group
        self.dp = self.world > 1
        if self.world > 1:
            self.broadcast_parameters()
        # N > 1 with the executor: the gradient exchange bucketed per backward stage and started
        # while the backward runs (gnn_amd.dp), built whenever possible; used when
        # GNN_DP_BUCKETS=1 (default: one flat all-reduce after the backward — bench.py times
        # both at N > 1, since neither is measured over RCCL / xGMI on a one-GPU box)
        self.bucketed = None
        if self.world > 1 and self.executor is not None:
            from .dp import BucketedExchange

            try:
                self.bucketed = BucketedExchange(self.executor, self.optimizer, group)
            except ValueError:
                self.bucketed = None
        self.exchange = self.bucketed if os.environ.get("GNN_DP_BUCKETS", "0") == "1" else None
        # (event, layer): recorded by the executor after that layer's forward aggregation; the
        # staging of later batches waits on it (staging.Stager.gate, set by the caller)
        self.stage_gate = None

    @property
    def num_params(self) -> int:
        return sum(p.numel() for p in self.params)

    def broadcast_parameters(self):
        flat = _flatten_dense_tensors([p.detach() for p in self.params])
        torch.distributed.broadcast(flat, src=0, group=self.group)
        with torch.no_grad():
            for p, v in zip(self.params, _unflatten_dense_tensors(flat, self.params)):
                p.copy_(v)

    def param_digest(self) -> str:
        """sha256 (first 16 hex digits) over every parameter's bytes, in parameter order."""
        import hashlib

        h = hashlib.sha256()
        for p in self.params:
            h.update(p.detach().contiguous().cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    def check_ranks_agree(self) -> dict:
        """Cross-rank consistency of the data-parallel step (main.py:146-170): after the summed
        gradient and the same Adam update on every rank, all ranks must hold bit-identical
        parameters. Collective (every rank of the group). Returns {"identical", "digests"}."""
        d = self.param_digest()
        dist = torch.distributed
        if not (dist.is_available() and dist.is_initialized()):
            return {"identical": True, "digests": [d]}
        digests = [None] * dist.get_world_size(self.group)
        torch.distributed.all_gather_object(digests, d, group=self.group)
        return {"identical": all(x == digests[0] for x in digests), "digests": digests}

    def allreduce_grads(self) -> Optional[torch.Tensor]:
        """Σ over ranks of the (already clipped) gradients, in one flat buffer."""
        if not self.dp:
            return None
        grads = [p.grad for p in self.params]
        flat = _flatten_dense_tensors(grads)
        torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM, group=self.group)
        for p, g in zip(self.params, _unflatten_dense_tensors(flat, grads)):
            p.grad = g
        return flat

    def _next_batch(self, prefetch):
        """The next batch (x0, adjs, sampled_nodes, labels) for the executor's layer-0 prefetch, or
        None: data-parallel runs only (there the all-reduce leaves the compute stream idle), the
        flat exchange, not while the per-aggregation timing runs, GNN_PREFETCH_L0=0 turns it off."""
        if prefetch is None or self.executor is None or os.environ.get("GNN_PREFETCH_L0", "1") == "0":
            return None
        from . import custom_sparse_ops as cso

        if cso.timing_enabled():
            return None
        nxt = prefetch() if callable(prefetch) else prefetch
        if nxt is None or not self.executor.supports(*nxt):
            return None
        return nxt

    def step(self, x0, adjs, sampled_nodes, labels, prefetch=None) -> torch.Tensor:
        """One training step. ``prefetch``: the next batch (x0, adjs, sampled_nodes, labels), or a
        callable returning it, whose layer-0 forward aggregation a data-parallel run issues while
        this step's gradient all-reduce is in flight (gnn_amd.executor.NativeStep.prefetch; the
        next step then skips it). Results are the same with or without it."""
        if not self.model.training:  # module.train() walks every submodule: ~50 µs of host time
            self.model.train()
        if self.executor is not None and self.executor.supports(x0, adjs, sampled_nodes, labels):
            if self.exchange is not None:  # buckets leave while the lower layers' backward runs
                loss = self.executor.step(x0, adjs, sampled_nodes, labels, grad_events=self.exchange.events,
                                          stage_gate=self.stage_gate)
                self.exchange.issue()
                self.exchange.finish()  # this rank's clip, Σ_r c_r g_r into the flat gradient
                self.optimizer.step(clipped=True)
                return loss
            loss = self.executor.step(x0, adjs, sampled_nodes, labels,  # grads into the flat buffer
                                      stage_gate=self.stage_gate)
            if self.dp:
                flat = self.optimizer.clip_to_flat()
                # the all-reduce is issued first, on the collective's stream: fetching the next
                # batch may wait on the host for its staging event (GNN_EXTRACT_CHECK=step), which
                # must not hold the collective back on this rank. The next batch's layer-0
                # aggregation (no parameter in it) then fills the compute stream meanwhile, and the
                # optimizer step waits for the sum (Work.wait: a stream wait, not a host one)
                work = torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM, group=self.group,
                                                    async_op=True)
                nxt = self._next_batch(prefetch)
                if nxt is not None:
                    self.executor.prefetch(*nxt, stage_gate=self.stage_gate)
                work.wait()
                self.optimizer.step(clipped=True)
            else:
                # N = 1 takes no prefetch: issuing it with the clip + Adam kernels moved to a side
                # stream beside it measured 0.5-0.8 % slower (two cross-stream events per step
                # against ~30 us of small launches; profiles/round5/prefetch_l0/)
                self.optimizer.step()
            return loss
        for p in self.params:
            p.grad = None
        if hasattr(self.model, "forward_loss"):
            loss, _ = self.model.forward_loss(x0, adjs, sampled_nodes, labels, self.sigmoid_loss)
        else:
            out = self.model(x0, adjs, sampled_nodes)
            loss = loss_fn(out, labels, self.sigmoid_loss, self.device)
        if self.native:
            # d(loss)/d(loss) = 1 from a cached device scalar (no fill launch per step)
            one = getattr(self, "_one", None)
            if one is None or one.device != loss.device:
                one = self._one = torch.ones((), dtype=loss.dtype, device=loss.device)
            loss.backward(one)
        else:
            loss.backward()
        if self.native:
            if self.dp:
                flat = self.optimizer.clip_to_flat()  # this rank's clip, into the all-reduce buffer
                torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM, group=self.group)
                self.optimizer.step(clipped=True)
            else:
                self.optimizer.step()  # clip applied inside the Adam launch
            return loss.detach()
        torch.nn.utils.clip_grad_norm_(self.params, self.clip)
        self.allreduce_grads()
        self.optimizer.step()
        return loss.detach()


    def evaluate(self, batches, mode: Optional[int] = None) -> dict:
        """A validation / test pass (main.py:178-199, 217-241) over ``batches``, any iterable of
        (x0, adjs, sampled_nodes, labels): the model in eval() (its previous mode is restored),
        forward only through this trainer's executor where the batch allows it, one host
        synchronisation at the end. mode: 0 sigmoid / multi-label, 1 argmax / single-label
        (default: by ``sigmoid_loss``). Returns ``Evaluator.result()``."""
        ev = Evaluator(self.model, self.device, self.sigmoid_loss, executor=self.executor, mode=mode)
        was_training = self.model.training
        self.model.eval()
        try:
            for x0, adjs, sampled_nodes, labels in batches:
                ev.add(x0, adjs, sampled_nodes, labels)
        finally:
            self.model.train(was_training)
        return ev.result()

    def evaluate_exact(self, graph, feats, nodes, labels, mode: Optional[int] = None, scope="graph") -> dict:
        """Scores ``nodes`` against ``labels`` with the full neighbourhood of every node — no
        sampler, no importance weights: the model run layer by layer over the whole graph
        (gnn_amd.inference.ExactInference, made once per graph and cached), in eval semantics;
        the model's training mode is restored. Returns the keys of ``Evaluator.result()``.
        ``scope="closure"`` runs the layers over the k-hop closure of ``nodes`` only (the same
        scores at the closure's cost; ``ExactInference.logits``)."""
        from .inference import ExactInference

        cached = getattr(self, "_exact", None)
        if cached is None or cached[0] is not graph:
            cached = self._exact = (graph, ExactInference(self.model, graph, self.device))
        was_training = self.model.training
        self.model.eval()
        try:
            return cached[1].evaluate(feats, nodes, labels, sigmoid_loss=self.sigmoid_loss, mode=mode,
                                      scope=scope)
        finally:
            self.model.train(was_training)


class Evaluator:
    """Accumulates the loss and the per-class prediction counts of evaluation batches on the
    device and turns them into F1 scores once, at ``result()``.

    Reference: the validation block (main.py:178-199) and the test pass (main.py:217-241) pull
    every batch's predictions and labels to the host for sklearn (utils.calc_f1), one stream
    synchronisation per batch. Here a batch is one forward-only executor call
    (NativeStep.evaluate: gnn_eval_step_f32 with the fused evaluation head) — or, for a model or
    batch the executor does not take, ``model.forward_loss`` under no_grad and
    metrics.prediction_counts — whose int32 counts [3, C] and loss land in one growing device
    buffer; nothing is synchronised until ``result()`` copies that buffer to the host."""

    def __init__(self, model, device, sigmoid_loss: bool = True, executor=None, mode: Optional[int] = None):
        self.model = model
        self.device = torch.device(device)
        self.sigmoid_loss = sigmoid_loss
        self.mode = (0 if sigmoid_loss else 1) if mode is None else int(mode)
        self.executor = executor
        self.rows = []  # per batch, known on the host
        self._buf = None  # int32 [capacity, 3 C + 1]: a batch's counts, then its loss's bits
        self.native_batches = 0
        self.counts = None  # set by result()

    def _native(self, x0, adjs, sampled_nodes, labels) -> bool:
        return (self.executor is not None
                and self.executor.supports(x0, adjs, sampled_nodes, labels, inference=True))

    def _eval_mode(self):
        """The model in eval() for one fallback forward; returns whether to switch it back."""
        was_training = self.model.training
        if was_training:
            self.model.eval()
        return was_training

    def add(self, x0, adjs, sampled_nodes, labels):
        """One batch. Returns its (loss, counts) as device tensors; synchronises nothing."""
        from . import metrics

        if self._native(x0, adjs, sampled_nodes, labels):
            loss, counts, _ = self.executor.evaluate(x0, adjs, sampled_nodes, labels, mode=self.mode,
                                                     sigmoid_loss=self.sigmoid_loss)
            self.native_batches += 1
        else:
            was_training = self._eval_mode()
            try:
                with torch.no_grad():
                    if hasattr(self.model, "forward_loss"):
                        loss, out = self.model.forward_loss(x0, adjs, sampled_nodes, labels, self.sigmoid_loss)
                    else:
                        out = self.model(x0, adjs, sampled_nodes)
                        loss = loss_fn(out, labels, self.sigmoid_loss, out.device)
            finally:
                if was_training:
                    self.model.train()
            loss = loss.detach().to(torch.float32)
            counts = metrics.prediction_counts(out, labels, self.mode)
        self.add_counts(loss, counts, int(labels.shape[0]))
        return loss, counts

    def add_counts(self, loss, counts, rows: int) -> None:
        """One batch already scored elsewhere (inference.ExactInference.evaluate: a chunk of nodes
        through the evaluation head): its mean loss (fp32 device scalar) and int32 counts [3, C]
        over ``rows`` rows go into the buffer as ``add`` puts its own; synchronises nothing."""
        n, width = len(self.rows), counts.numel() + 1
        if self._buf is None or n == self._buf.shape[0]:
            grown = torch.empty((max(16, 2 * n), width), dtype=torch.int32, device=counts.device)
            if n:
                grown[:n] = self._buf
            self._buf = grown
        self._buf[n, :width - 1] = counts.reshape(-1)
        self._buf[n, width - 1:] = loss.reshape(1).view(torch.int32)
        self.rows.append(int(rows))

    def predict(self, x0, adjs, sampled_nodes) -> torch.Tensor:
        """The logits [M, C] of one batch (model.eval(), no dropout), on the device."""
        if self._native(x0, adjs, sampled_nodes, None):
            return self.executor.evaluate(x0, adjs, sampled_nodes, None)[2]
        was_training = self._eval_mode()
        try:
            with torch.no_grad():
                return self.model(x0, adjs, sampled_nodes)
        finally:
            if was_training:
                self.model.train()

    def result(self) -> dict:
        """One device-to-host copy, then: ``micro_f1`` / ``macro_f1`` of the counts summed over the
        batches (the scores of the whole pass), ``loss`` (mean over rows), ``batches``, ``rows``,
        and ``ref_batch_weighted_micro_f1`` = Σ_b micro_b rows_b / Σ_b rows_b, the number the
        reference's test pass prints (main.py:237-241)."""
        from . import metrics

        n = len(self.rows)
        if n == 0:
            return {"micro_f1": 0.0, "macro_f1": 0.0, "loss": 0.0, "batches": 0, "rows": 0,
                    "ref_batch_weighted_micro_f1": 0.0}
        host = self._buf[:n].cpu()
        counts = host[:, :-1].reshape(n, 3, -1).numpy().astype("int64")
        losses = host[:, -1:].contiguous().view(torch.float32).reshape(n).double().numpy()
        rows = [float(r) for r in self.rows]
        total = sum(rows)
        pooled = counts.sum(axis=0)
        self.counts = pooled  # int64 [3, C] on the host: (tp, fp, fn) of the whole pass
        micro, macro = metrics.f1_from_counts(pooled[0], pooled[1], pooled[2], self.mode)
        per_batch = [metrics.f1_from_counts(c[0], c[1], c[2], self.mode)[0] for c in counts]
        return {"micro_f1": micro, "macro_f1": macro,
                "loss": float(sum(l * r for l, r in zip(losses, rows)) / total) if total else 0.0,
                "batches": n, "rows": int(total),
                "ref_batch_weighted_micro_f1": float(sum(m * r for m, r in zip(per_batch, rows)) / total)
                if total else 0.0}


DEFAULT_TIMEOUT_S = 180.0


def collective_timeout():
    """How long any collective of this package may wait for its peers (GNN_DIST_TIMEOUT_S,
    default 180 s) before the rank fails. The reference's threads wait on a
    ``threading.Barrier`` with no timeout (main.py:158,214), and torch's defaults are 10 min
    (RCCL) and 30 min (gloo): a stalled collective must instead end the run, non-zero, well
    inside a driver's time limit, with the rank and the call in the log."""
    import datetime

    s = float(os.environ.get("GNN_DIST_TIMEOUT_S", DEFAULT_TIMEOUT_S))
    if not s > 0:
        raise ValueError(f"GNN_DIST_TIMEOUT_S must be > 0, got {s}")
    return datetime.timedelta(seconds=s)


def init_group(backend: str, rank: Optional[int] = None, world: Optional[int] = None, local: int = 0):
    """init_process_group with this package's collective timeout. RCCL ("nccl"): the watchdog's
    asynchronous error handling stays on (TORCH_NCCL_ASYNC_ERROR_HANDLING, set to 1 = abort the
    communicator and end the process unless the caller chose otherwise), so a collective that
    does not complete within the timeout takes the rank down with the watchdog's report of the
    rank, the operation and its sequence number instead of hanging; its heartbeat monitor is
    held to the timeout + 60 s. gloo: every collective raises RuntimeError after the timeout."""
    timeout = collective_timeout()
    kw = {"timeout": timeout}
    if rank is not None:
        kw.update(rank=rank, world_size=world)
    if backend == "nccl":
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
        os.environ.setdefault("TORCH_NCCL_HEARTBEAT_TIMEOUT_SEC", str(int(timeout.total_seconds()) + 60))
        torch.distributed.init_process_group(backend, device_id=torch.device("cuda", local), **kw)
    else:
        from .staging import stdout_to_stderr

        with stdout_to_stderr():  # gloo's connection lines go to stderr, not into the bench's stdout
            torch.distributed.init_process_group(backend, **kw)


def new_gloo_group():
    """A gloo side group (host metadata, IPC handle exchange) with the same timeout."""
    from .staging import stdout_to_stderr

    with stdout_to_stderr():  # gloo prints its connection lines on stdout (bench: one JSON line)
        return torch.distributed.new_group(backend="gloo", timeout=collective_timeout())


def init_distributed(backend: Optional[str] = None):
    """Initialise torch.distributed from torchrun's environment; returns (rank, world, local_rank)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not torch.distributed.is_initialized():
        be = backend or os.environ.get("GNN_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if torch.cuda.is_available():
            # one GPU per local rank (torchrun); more ranks than GPUs (a rehearsal on a smaller
            # box, gloo backend: RCCL refuses two ranks on one GPU) share them round-robin
            local = local % max(torch.cuda.device_count(), 1)
            torch.cuda.set_device(local)
        init_group(be, local=local)
    return rank, world, local
