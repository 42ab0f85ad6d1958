"""Training-step harness equal to the reference's LitModel step (main.py:49-63,137-151):
forward -> nn.MSELoss -> backward -> gradient average across ranks -> Adam(lr, wd).

Data parallelism: one process per GPU, each rank steps its own molecule batch;
the only exchange is ONE all-reduce of a flat gradient buffer per step (RCCL over xGMI when the
backend is "nccl", gloo on CPU for the tests).  Parameter gradients are views into that flat
buffer, so there is no pack/unpack copy, and parameters whose gradient the model never
produces (the reference's dead branches, which is why main.py:281 needs
``find_unused_parameters``) are simply left out: their ``.grad`` stays ``None`` on every rank.
"""
from __future__ import annotations

import contextlib
import gc
import inspect
import types
from typing import Callable, Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from .precision import (get_float32_matmul_precision, get_float32_matmul_precision_edges,
                        get_float32_matmul_precision_panels, get_float32_matmul_precision_wgrads)
from .prefetch import BucketPrefetch, FormCalibration, batch_token, copy_into_static, static_copy_of


def _world() -> int:
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class FlatGradients:
    """One contiguous fp32 buffer holding every live parameter's gradient."""

    def __init__(self, params):
        self.params = list(params)
        n = sum(p.numel() for p in self.params)
        ref = self.params[0]
        self.flat = torch.zeros(n, dtype=ref.dtype, device=ref.device)
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    def zero_(self):
        self.flat.zero_()

    def all_reduce_mean(self):
        w = _world()
        if w > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
            self.flat.mul_(1.0 / w)


def _checked_decay(who: str, decay) -> Optional[float]:
    """``ema_decay`` as a float in [0, 1), or None (no average)."""
    if decay is None:
        return None
    d = float(decay)
    if not 0.0 <= d < 1.0:      # (a NaN fails both comparisons)
        raise ValueError(f"{who}: ema_decay must lie in [0, 1) (got {decay})")
    return d


def _checked_accum(who: str, k) -> int:
    """``accum_steps`` as an integer >= 1 (a bool, a float or a string is not one)."""
    if not isinstance(k, int) or isinstance(k, bool) or k < 1:
        raise ValueError(f"{who}: accum_steps must be an integer >= 1 (got {k!r})")
    return k


def ema_decay_at(decay: float, t: int, warmup: bool) -> float:
    """d_t of update t = 1, 2, ..: ``decay``, or with ``warmup`` min(decay, (1 + t) / (10 + t)) (torch_ema / timm)."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class _StepBase:
    """What TrainStep and GraphedTrainStep share.  The groups of ``accum_steps`` micro-batches: ``micro``, ``updates``,
    ``flush()``; the step class closes a group (``_close_group``).  The weight average (``ema_decay``): ``averaged()`` and
    ``ema_state_dict()``; the step class says how the live and the averaged values change places (``_ema_exchange``, its own
    inverse), where each averaged parameter lies (``_ema_of``: id(parameter) -> tensor, live parameters only) and what holds
    the average meanwhile (``_holds``).  Only parameters that receive a gradient are averaged (the others never change: they
    are their own average); buffers are not (an evaluation on the average reads the live BatchNorm statistics)."""

    ema_decay: Optional[float] = None
    _averaging = False
    accum_steps = 1     # micro-batches per optimiser step
    micro = 0           # micro-batches in the open group (0: none is open)
    updates = 0         # optimiser steps taken

    def _refuse_averaging(self, what: str):
        if self._averaging:
            raise RuntimeError(f"{type(self).__name__}.{what}: inside averaged() {self._holds} the average, not the live weights")

    def flush(self):
        """Close an open group early (the end of an epoch): the update runs on what the group holds, still scaled
        1 / ``accum_steps``.  Nothing when no group is open (always so for accum_steps = 1)."""
        self._refuse_averaging("flush()")
        if self.micro:
            self._close_group()

    def _ema_ready(self, what: str):
        if self.ema_decay is None:
            raise RuntimeError(f"{type(self).__name__}.{what}: built without ema_decay, there is no average")
        if self.opt is None:
            raise RuntimeError(f"{type(self).__name__}.{what}: no optimiser yet (the first step builds it and the average)")

    @contextlib.contextmanager
    def averaged(self):
        """``with step.averaged(): ...``: the model's parameters hold the averaged weights inside the block and the live ones
        again behind it, bit for bit, also when the block raises.  An exchange in place: every address stays what it was, so
        captured graphs (GraphedEvalStep) replay on the average without a re-capture.  No step() inside the block."""
        self._ema_ready("averaged()")
        if self._averaging:
            raise RuntimeError(f"{type(self).__name__}.averaged(): already inside averaged()")
        self._ema_exchange()
        self._averaging = True
        try:
            yield self
        finally:
            self._averaging = False
            self._ema_exchange()

    @torch.no_grad()
    def ema_state_dict(self) -> dict:
        """``model.state_dict()`` with the averaged value of every averaged parameter, all entries clones; the live weights
        are not touched.  (Inside ``averaged()`` the parameters themselves hold the average: the model's state is returned.)"""
        self._ema_ready("ema_state_dict()")
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        if self._averaging:
            return sd
        ema = self._ema_of()
        for name, p in self.model.named_parameters(remove_duplicate=False):
            if id(p) in ema and name in sd:
                sd[name] = ema[id(p)].detach().clone()
        return sd


def _torch_loss(kind: str, beta: float) -> Callable:
    """The ``torch.nn.functional`` loss of ``TrainStep(loss=kind, loss_beta=beta)`` as f(pred, target)."""
    if kind == "mse":
        return F.mse_loss
    if kind == "l1":
        return F.l1_loss
    if kind == "smooth_l1":
        return lambda pred, target: F.smooth_l1_loss(pred, target, beta=beta)
    return lambda pred, target: F.huber_loss(pred, target, delta=beta)


class TrainStep(_StepBase):
    """``loss = step(data)``; ``data.y`` is the target.  Model-agnostic (the gloo tests drive it
    with the CPU oracle, the GPU path with the HIP models)."""

    _holds = "the parameters hold"

    def __init__(self, model: nn.Module, lr: float = 1e-4, weight_decay: float = 0.0,
                 broadcast_from_rank0: bool = True, on_batch: Optional[Callable] = None,
                 clip_gnorm: Optional[float] = None, loss_readout: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False, loss: str = "mse", loss_beta: float = 1.0,
                 accum_steps: int = 1):
        """``accum_steps`` = k: one optimiser step per k calls of ``step()`` (Lightning's ``accumulate_grad_batches``, DDP under
        ``no_sync``).  Every call is one micro-batch and returns that micro-batch's own loss; its gradient is added into the
        flat buffer, which is cleared only in front of a group's first micro-batch.  The k-th call closes the group: ONE
        in-place multiply of the buffer by 1 / k, then the rank average (one collective per group), clip, update and average
        of the weights, once.  ``flush()`` closes an open group early with the same 1 / k (the end of an epoch); ``micro`` is
        the position inside the group, ``updates`` the number of optimiser steps taken.  The weights do not move inside a
        group, so ``averaged()`` and ``ema_state_dict()`` never see a half-applied state and need no refusal of their own.
        k = 1 (default): the step of before, without the multiply.
        ``loss`` / ``loss_beta``: the training loss -- "mse" (the reference's, main.py:49-63), "l1", "smooth_l1" (``loss_beta``
        its beta >= 0) or "huber" (``loss_beta`` its delta > 0); "mse" and "l1" ignore ``loss_beta``.  Checked by
        ``ops.loss_spec`` and fixed at construction; the step calls the matching ``torch.nn.functional`` loss.
        ``clip_gnorm``: clip the rank-averaged gradient by its global L2 norm before the update
        (``torch.nn.utils.clip_grad_norm_``; the reference's ``--clip_gnorm``, main.py:175, which its Trainer never
        receives -- so the default, and the reference's behaviour, is off).  ``loss_readout``: keep {sum, count} of the
        steps' losses in ``loss_sum``, 2 doubles on the model's device (a GPU), added to by one launch behind every step's
        backward; the reader zeroes it.  Off: nothing is allocated or launched.
        ``ema_decay`` / ``ema_warmup``: keep an exponential moving average of the live parameters in shadow tensors
        (``ema_shadows``, laid out at the first step), updated behind ``opt.step()`` by ONE ``torch._foreach_lerp_`` -- update
        t = 1 copies, from t = 2 on e += (1 - d_t) (p - e), d_t = ``ema_decay`` or, with ``ema_warmup``,
        min(ema_decay, (1 + t) / (10 + t)).  ``averaged()`` exchanges the ``p.data`` of the live parameters with the shadows;
        ``ema_state_dict()`` returns the averaged state.  ``None``: no shadows, the step of before."""
        self.model = model
        self.accum_steps = _checked_accum("TrainStep", accum_steps)
        from .ops.readout import loss_spec
        self.loss, self.loss_beta, self.loss_spec = loss, float(loss_beta), loss_spec(loss, loss_beta)
        self._loss_fn = _torch_loss(loss, self.loss_beta)
        self.ema_decay, self.ema_warmup = _checked_decay("TrainStep", ema_decay), bool(ema_warmup)
        self.ema_shadows: Optional[list] = None         # one tensor per live parameter, in self.flat.params' order
        self.ema_updates = 0                            # t of the last update of the average
        self.loss_readout = bool(loss_readout)
        self.loss_sum: Optional[torch.Tensor] = None    # {sum of the steps' losses, number of steps}, float64, on the device
        self.lr, self.wd = lr, weight_decay
        self.on_batch = on_batch
        self.clip_gnorm = None if clip_gnorm is None else float(clip_gnorm)
        self.grad_norm: Optional[torch.Tensor] = None   # {norm before clipping, coef, running max of norm, clipped steps}
        self.flat: Optional[FlatGradients] = None
        self.opt: Optional[torch.optim.Optimizer] = None
        if broadcast_from_rank0 and _world() > 1:  # DDP broadcasts rank 0's parameters at wrap time
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t.data, src=0)

    def _first_step(self, data):
        """Discover which parameters receive a gradient, then lay out the flat buffer."""
        for p in self.model.parameters():
            p.grad = None
        loss = self._loss_fn(self.model(data), data.y)
        loss.backward()
        live = [p for p in self.model.parameters() if p.grad is not None]
        first = [p.grad.clone() for p in live]
        self.flat = FlatGradients(live)
        for p, g in zip(live, first):
            p.grad.copy_(g)
        fused = live[0].is_cuda
        self.opt = torch.optim.Adam(live, lr=self.lr, weight_decay=self.wd, fused=fused)
        if self.ema_decay is not None:
            self.ema_shadows = [p.detach().clone() for p in live]   # before the first update the average IS the live weights
        return loss

    def step(self, data) -> torch.Tensor:
        self._refuse_averaging("step()")
        if self.on_batch is not None:
            self.on_batch(data)
        if self.flat is None:
            loss = self._first_step(data)
        else:
            if self.micro == 0:
                self.flat.zero_()
            loss = self._loss_fn(self.model(data), data.y)
            loss.backward()         # (into the views of the flat buffer: added to what the group's earlier micro-batches left)
        if self.loss_readout:
            _accumulate_loss(self, loss)
        self.micro += 1
        if self.micro == self.accum_steps:
            self._close_group()
        return loss.detach()

    def _close_group(self):
        if self.accum_steps > 1:
            self.flat.flat.mul_(1.0 / self.accum_steps)
        self.flat.all_reduce_mean()
        if self.clip_gnorm is not None:
            self._clip()
        self.opt.step()
        if self.ema_decay is not None:
            self._ema_update()
        self.micro = 0
        self.updates += 1

    @torch.no_grad()
    def _ema_update(self):
        self.ema_updates += 1
        live = [p.data for p in self.flat.params]
        if self.ema_updates == 1:
            torch._foreach_copy_(self.ema_shadows, live)
        else:
            torch._foreach_lerp_(self.ema_shadows, live, 1.0 - ema_decay_at(self.ema_decay, self.ema_updates, self.ema_warmup))

    def _ema_exchange(self):
        for i, p in enumerate(self.flat.params):
            p.data, self.ema_shadows[i] = self.ema_shadows[i], p.data

    def _ema_of(self):
        return {id(p): e for p, e in zip(self.flat.params, self.ema_shadows)}

    @torch.no_grad()
    def _clip(self):
        """clip_grad_norm_(norm_type=2, error_if_nonfinite=False) of the flat buffer, which the averaged gradient of every
        live parameter tiles exactly: torch's own norm over the per-parameter views, ONE in-place scaling of the buffer, and
        the readout kept on its device (no sync here; whoever reads ``grad_norm`` pays for it)."""
        total = torch.nn.utils.get_total_norm([p.grad for p in self.flat.params], 2.0)
        coef = torch.clamp(self.clip_gnorm / (total + 1e-6), max=1.0)
        self.flat.flat.mul_(coef)
        if self.grad_norm is None:
            self.grad_norm = torch.zeros(4, dtype=torch.float32, device=self.flat.flat.device)
        r = self.grad_norm
        r[0], r[1] = total, coef
        r[2] = torch.where(total > r[2], total.to(r.dtype), r[2])
        r[3] += (coef < 1.0).to(r.dtype)

    def sync_buffers(self):
        """DDP's per-forward buffer broadcast (BatchNorm running stats of ``mhnnm``)."""
        if _world() > 1:
            for b in self.model.buffers():
                dist.broadcast(b.data, src=0)


def _accumulate_loss(step, loss):
    """``loss_readout``: one step's loss into the step object's ``loss_sum`` (allocated at the first step), by an ordinary
    stream-ordered launch behind the step, never a node of a captured graph (the graphs' launch lists stay as they are)."""
    from . import ops
    if step.loss_sum is None:
        if not loss.is_cuda:
            raise ValueError("loss_readout keeps the loss sum in device memory: the model must be on a GPU")
        step.loss_sum = torch.zeros(2, dtype=torch.float64, device=loss.device)
    ops.loss_accumulate(loss, step.loss_sum)


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad=False) over ONE flat fp32 parameter through eqh_adam_step: a grid-stride
    kernel instead of the multi-tensor kernel's one block per 64 Ki elements (12 us against 46 us for the
    2.6 M parameters of egnn_equihnns).  Learning rate and step counter live in device memory, so a
    captured hipGraph follows a scheduler (``sync_lr`` before each replay); ``grad_scale`` folds the
    1 / world_size of the gradient average into the update.

    ``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_(.., max_grad_norm)`` of ``grad * grad_scale`` inside the step, without
    a host round trip: ``step()`` then makes two launches on the optimiser's stream, both capturable -- eqh_grad_sumsq (per
    workgroup partial sums of squares, in double) and eqh_adam_step_clip (sums them, scales the gradient by
    min(1, max / (norm + 1e-6)), updates).  The threshold is FIXED at construction: it is a kernel argument of a captured
    graph, which a replay does not read again.  ``grad_norm``: 4 floats on the device, {norm before clipping, coef, running
    maximum of the norm, number of steps with coef < 1}; the kernel keeps the last two running, the reader zeroes them.
    ``None`` (default): one eqh_adam_step call, as before, and ``grad_norm`` is ``None``.

    ``ema_decay``: keep an exponential moving average of the parameter in ``state[param]["ema"]`` (a clone of the parameter
    at construction, carried by ``state_dict()``), updated by the SAME launch: ``step()`` calls the ``_ema`` twin of the entry
    it would have called (eqh_adam_step_ema / eqh_adam_step_clip_ema), which streams the average beside p, grad and the
    moments.  Update t = 1 copies the parameter; from t = 2 on e += (1 - d_t) (p - e) with d_t = ``ema_decay``, or
    min(``ema_decay``, (1 + t) / (10 + t)) with ``ema_warmup`` (the torch_ema / timm warm-up).  Decay and flag are FIXED at
    construction, as the threshold is.  ``None`` (default): today's calls and no ``"ema"`` key."""

    def __init__(self, param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 ema_decay=None, ema_warmup=False):
        super().__init__([param], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"FlatAdam: max_grad_norm must be positive (got {max_grad_norm})")
        self.ema_decay, self.ema_warmup = _checked_decay("FlatAdam", ema_decay), bool(ema_warmup)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None
        self.grad_scale = 1.0
        self.zero_grad_in_step = False      # clear the flat gradient inside the update kernel (GraphedTrainStep)
        self.zero_also = None               # callable -> a second buffer the update clears (the owner's MergedScratch)
        self._lr_dev = None
        st = self.state[param]
        st["exp_avg"] = torch.zeros_like(param.data)
        st["exp_avg_sq"] = torch.zeros_like(param.data)
        st["step_block"] = torch.zeros(2, dtype=torch.int64, device=param.device)   # {step, ticket}
        st["lr"] = torch.tensor([float(lr)], dtype=torch.float32, device=param.device)
        self._lr_dev = float(lr)
        if self.max_grad_norm is not None:
            from . import hip
            nbytes = hip.lib().eqh_grad_sumsq_workspace_bytes(param.numel())
            st["clip_partials"] = torch.empty(nbytes // 8, dtype=torch.float64, device=param.device)   # never cleared
            self.grad_norm = torch.zeros(4, dtype=torch.float32, device=param.device)
        if self.ema_decay is not None:
            st["ema"] = param.data.detach().clone()     # before the first update the average IS the live parameter

    def sync_lr(self):
        """Mirror param_groups[0]['lr'] (what schedulers write) into the device scalar; outside capture."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_dev:
            p = self.param_groups[0]["params"][0]
            self.state[p]["lr"].fill_(lr)
            self._lr_dev = lr

    @torch.no_grad()
    def step(self, closure=None):
        from . import hip, ops
        g = self.param_groups[0]
        p = g["params"][0]
        st = self.state[p]
        b1, b2 = g["betas"]
        zs = self.zero_also() if (self.zero_grad_in_step and self.zero_also is not None) else None
        stream = ops._stream(p.device)
        args = (ops._ptr(p.data), ops._ptr(p.grad), ops._ptr(st["exp_avg"]), ops._ptr(st["exp_avg_sq"]), p.numel(),
                ops._ptr(st["lr"]), b1, b2, g["eps"], g["weight_decay"], self.grad_scale, ops._ptr(st["step_block"]),
                1 if self.zero_grad_in_step else 0, ops._ptr(zs) if zs is not None else None,
                zs.numel() if zs is not None else 0)
        ema = () if self.ema_decay is None else (ops._ptr(st["ema"]), self.ema_decay, 1 if self.ema_warmup else 0)
        if self.max_grad_norm is None:
            if ema:
                hip.check(hip.lib().eqh_adam_step_ema(*args, *ema, stream), "eqh_adam_step_ema")
            else:
                hip.check(hip.lib().eqh_adam_step(*args, stream), "eqh_adam_step")
            return
        partials = ops._ptr(st["clip_partials"])
        hip.check(hip.lib().eqh_grad_sumsq(ops._ptr(p.grad), p.numel(), partials, stream), "eqh_grad_sumsq")
        clip = (partials, self.max_grad_norm, ops._ptr(self.grad_norm))
        if ema:
            hip.check(hip.lib().eqh_adam_step_clip_ema(*args, *clip, *ema, stream), "eqh_adam_step_clip_ema")
        else:
            hip.check(hip.lib().eqh_adam_step_clip(*args, *clip, stream), "eqh_adam_step_clip")


def with_next(batches):
    """(batch, next batch or None) pairs of an iterable: the one batch of look-ahead ``GraphedTrainStep.step(data, next_data)``
    uses to build the next batch's index beside the current step."""
    it = iter(batches)
    try:
        cur = next(it)
    except StopIteration:
        return
    for nxt in it:
        yield cur, nxt
        cur = nxt
    yield cur, None


class CollectiveCaptureRefused(RuntimeError):
    """The process-group backend could not record a collective into a hipGraph (raised by ``capture_graph``)."""


def capture_graph(body, graph=None, context=None):
    """``body(collective)`` captured into a hipGraph: (the graph, what ``body`` returned).  ``collective(call)`` makes a
    collective call of the process group and says whether the backend recorded it; the body ends at the first False.
    Raises ``CollectiveCaptureRefused`` when -- and only when -- such a call failed with a RuntimeError (RCCL:
    ``DistBackendError``); an error of a kernel launch or of an argument check anywhere else in the body propagates as
    itself (a capture without the collective would hit it too).  ``graph`` / ``context``: stand-ins (tests without a device)."""
    g = torch.cuda.CUDAGraph() if graph is None else graph
    refused = []

    def collective(call) -> bool:
        try:
            call()
        except RuntimeError as exc:
            refused.append(exc)
        return not refused
    out = None
    try:
        # thread_local: the RCCL watchdog thread may query events while this thread captures
        with (context or torch.cuda.graph)(g, capture_error_mode="thread_local"):
            out = body(collective)
    except RuntimeError:
        if not refused:
            raise
        # (the refused collective also invalidated the capture: ending it raised again -- the refusal is the cause)
    if refused:
        raise CollectiveCaptureRefused(f"{type(refused[0]).__name__}: {refused[0]}") from refused[0]
    return g, out


class GraphedTrainStep(_StepBase):
    """TrainStep with the launch-bound part captured in hipGraphs.

    forward + MSE + backward (≈700 kernel launches for egnn_equihnns, including the per-batch index
    build), the gradient all-reduce and the fused Adam update are captured ONCE per static shape bucket
    as ONE hipGraph and replayed: with the "nccl" backend (RCCL) the collective is a node of that graph
    (``collective_mode == "in_graph"``; RCCL kernels are stream-capturable), so a multi-rank step is one
    graph launch exactly like the single-rank one.  Where the collective cannot be captured (gloo, or
    a capture that RCCL refuses) the step falls back to graph A -> eager all-reduce -> graph B
    (``"split"``) -- on EVERY rank: the ranks settle the form with one eager all-reduce (MIN of a success flag) at their
    first capture, and only a failing collective call triggers the fallback (kernel / argument errors re-raise).  Batches must be padded to bucket extents with ``batch.pad_batch`` (exact for models
    without batch statistics); the loss is taken over the real molecules only.

    Parameters live in ONE flat buffer (``pflat``; every ``nn.Parameter`` is a view into it) and so
    do their gradients (``gflat``, same element order): the weight gradients of ``ops.linear`` are
    accumulated straight into its head by the GEMMs, the gradients autograd allocates inside the
    captured backward (``grad=None`` before the capture, so the first contribution is written, not
    added) are packed behind them by one batched copy at the end of the first graph.  The all-reduce
    and the fused Adam therefore each see a single tensor.
    """

    _holds = "pflat holds"
    CAL_WARM, CAL_STEPS = FormCalibration.CAL_WARM, FormCalibration.CAL_STEPS

    def __init__(self, model: nn.Module, lr: float = 1e-4, weight_decay: float = 0.0,
                 broadcast_from_rank0: bool = True, collective: bool = True, keep_grads: bool = False,
                 force_collective: bool = False, graph_collective: bool = True, clip_gnorm: Optional[float] = None,
                 loss_readout: bool = False, ema_decay: Optional[float] = None, ema_warmup: bool = False,
                 loss: str = "mse", loss_beta: float = 1.0, accum_steps: int = 1):
        """``accum_steps`` = k > 1: one optimiser step per k calls of ``step()``, as ``TrainStep(accum_steps=k)``.  Two kinds of
        graph: one ACCUMULATE graph per bucket -- the backward graph of the split form, closed by eqh_add_many instead of
        eqh_copy_many: the gradients autograd allocates are ADDED into their ``gflat`` slots, and the same launch clears the
        merged weights' scratch, which no update clears between two micro-batches -- and ONE UPDATE graph shared by all
        buckets: ``opt.step()`` (with ``clip_gnorm`` / ``ema_decay`` their forms of it) behind the gradient all-reduce, which is
        its first node where the backend can be captured (``collective_mode``, settled among the ranks at that capture) and
        runs eagerly in front of it otherwise.  A group's last micro-step replays both; the gradient scale of the update is
        1 / (k * world).  The first group's update runs eagerly, as the first step's does for k = 1; the update graph is
        captured at the next one.  ``flush()`` closes an open group early with the same scale; ``micro`` is the position
        inside the group, ``updates`` the optimiser steps taken (the device counter of ``FlatAdam`` agrees).  With
        ``keep_grads`` ``gflat`` holds the unscaled sum over the group after its last micro-step, and ``step()`` clears it in
        front of a group's first micro-step.  The weights do not move inside a group: ``averaged()`` and
        ``ema_state_dict()`` need no refusal of their own while one is open.  k = 1 (default): the graphs and launches of before.
        ``loss`` / ``loss_beta``: the training loss, as ``TrainStep``'s -- "mse", "l1", "smooth_l1" (beta) or "huber" (delta).
        Anything but "mse" travels as an ``ops.loss_spec`` in the head tuple, so the fused read-out heads take their ``sl1`` forms
        and the other models end in ``ops.regression_loss``: the launch count of the step is that of "mse".  Fixed at
        construction (beta and scale are kernel arguments of the captured graphs).
        ``ema_decay`` / ``ema_warmup``: keep an exponential moving average of ``pflat`` (``FlatAdam(ema_decay=..)``: a fifth
        stream of the update launch, no launch more in the step; every rank forms the same average from the same averaged
        gradient, without a collective).  Fixed at construction (kernel arguments of the captured graphs).  ``averaged()``
        then exchanges ``pflat`` and the average in place by ONE launch on the current stream (eqh_swap_f32) and exchanges
        them back on leaving: the graphs of a ``GraphedEvalStep`` hold addresses, so they replay on the average as they are.
        ``ema_state_dict()``: the model's state with the averaged parameters.  ``None``: nothing allocated, the calls of before.
        ``loss_readout``: keep {sum, count} of the steps' losses in ``loss_sum`` (2 doubles on the device): behind every
        step -- the eager bootstrap step, a capture step, a calibration step, a replay -- ``step()`` issues one ordinary
        launch that adds the step's loss scalar to it (``ops.loss_accumulate``), stream-ordered behind the replay.  It is no
        node of the captured graphs: their launch lists, and what ``step()`` returns, are those of before.  Whoever reads
        ``loss_sum`` zeroes it (``Fitter`` does, once per epoch).  Off: nothing is allocated or launched.
        ``clip_gnorm``: clip the gradient by its global L2 norm inside the captured step (``FlatAdam(max_grad_norm=..)``:
        one more launch in front of the update, behind the all-reduce -- in the one graph in "in_graph" mode, in ``g_opt`` in
        "split" mode); the norm is that of ``gflat * grad_scale``, the rank-averaged gradient, so every rank scales alike.
        Fixed at construction (a kernel argument of the captured graphs).  ``None``: no clipping, the launch list of before.
        ``collective=False``: a rank-local trainer inside a multi-rank job (no broadcast, no all-reduce) -- what a
        measurement on ONE rank needs while the other ranks wait at a barrier.  ``keep_grads``: leave the gradients of the
        last step readable in ``p.grad`` after ``step()`` (tests); by default the update kernel clears the flat gradient
        buffer as it consumes it -- optimizer.zero_grad() without the fill launch at the head of every replayed step.
        ``force_collective``: take the multi-rank code path (broadcasts, all-reduce, 1 / world scaling) even when the
        process group has ONE rank -- how the path is exercised on a one-GPU box.  ``graph_collective=False``: never
        capture the collective (always graph A -> eager all-reduce -> graph B)."""
        self.model, self.lr, self.wd = model, lr, weight_decay
        self.accum_steps = _checked_accum("GraphedTrainStep", accum_steps)
        self._g_update = None               # accum_steps > 1: the update graph shared by all buckets (_capture_update)
        from .ops.readout import loss_spec
        self.loss, self.loss_beta, self.loss_spec = loss, float(loss_beta), loss_spec(loss, loss_beta)
        self.clip_gnorm = clip_gnorm
        self.ema_decay, self.ema_warmup = _checked_decay("GraphedTrainStep", ema_decay), bool(ema_warmup)
        self.loss_readout = bool(loss_readout)
        self.loss_sum: Optional[torch.Tensor] = None    # {sum of the steps' losses, number of steps}, float64, on the device
        self.collective = collective
        self.keep_grads = keep_grads
        self.force_collective = bool(force_collective) and collective and dist.is_available() and dist.is_initialized()
        self.graph_collective = graph_collective
        self.collective_mode = "none"       # "none" | "in_graph" | "split": what the captured steps do (set by _capture)
        self.capture_error = None           # why an in-graph capture fell back to "split", if it did
        self.in_graph_backends = ("nccl",)  # backends whose collectives are stream-capturable (RCCL)
        # Index prefetch: the per-batch index (three CSR sorts, kNN + its transpose: ~100 us of a 1.1 ms egnn_equihnns step)
        # depends on the batch only, not on the parameters.  step(data, next_data) builds next_data's index on a side
        # stream (its own small hipGraph) WHILE the step graph of `data` runs, and the step graph then starts at the
        # embedding.  EQH_NO_INDEX_PREFETCH=1: the index stays at the head of the step graph (rounds 1-5).
        #
        # Whether that pays depends on the model (round 6, same box, ms per step with / without): egnn_equihnns 1.122 / 1.181 at
        # batch 256 and 5.24 / 5.54 on PCQM batches of 1024, faformer_equihnns 18.9 / 19.0 -- but equiformer_equihnns 5.20 / 4.95,
        # mhnnm 0.872 / 0.810 at batch 32, egnn_equihnn 1.85 / 1.79: the staged -> live copy, the signal and the rendezvous of the
        # two streams cost a step more than a short index build saves, and neither the index graph's own time (93 us for both
        # EGNN models) nor the step's length predicts the sign.  So the trainer MEASURES (``prefetch_policy == "auto"``): the
        # first captured steps run in the built-ahead form, a window of them is timed, the same number in the in-step form, and
        # the faster form stays (``calibrating``, ``calibration``; the two forms are numerically the same step).
        # EQH_NO_INDEX_PREFETCH=1 / EQH_INDEX_PREFETCH=1 (or assigning ``index_prefetch``) pin a form.
        import os
        self.prefetch_policy = ("off" if os.environ.get("EQH_NO_INDEX_PREFETCH") else
                                "on" if os.environ.get("EQH_INDEX_PREFETCH") else "auto")
        self._prefetch_on = self.prefetch_policy != "off"
        self.form_calibration = None        # FormCalibration, from the first graphed step to the decision; holds the other form's graphs
        self.calibration = None             # {"built_ahead_ms": .., "in_step_ms": .., "chosen": ..} once decided
        self.index_build_us = None          # the index graph alone, timed at the latest capture (BucketPrefetch.capture)
        self._prefetch_stream = None        # the side stream the buckets' index graphs replay on
        self.signal_in_model = not os.environ.get("EQH_PREFETCH_AT_HEAD")    # start the next index at the model's ops.signal_point()
        # which of the marked points releases it.  Measured at the BASELINE batch (same box, ms per step): index at the head
        # of the step graph 1.137; built ahead and released at the step's head 1.138 (it then competes with the chip-filling
        # front-end kernels), behind the EGNN edge kernel 1.112, before the read-out head 1.098, before the closing
        # reductions 1.160 (too late: it spills into the next step)
        # (round 6, second scan: before the conv stack's last application 1.075 / 1.076 against 1.079-1.083 before the read-out
        # head and 1.10 before its first or second application.)  A comma list: the first point the model's step reaches.
        self.signal_at = os.environ.get("EQH_PREFETCH_SIGNAL", "conv_last,readout")
        self._signal = None                 # ops.StepSignal: posted by a node of every step graph with index prefetch
        self.prefetch_hits = 0              # steps whose index had been built ahead
        self.prefetch_misses = 0            # steps that had to build it first (no next_data was given for them)
        self._mode_agreed = False           # the ranks have settled on one collective_mode (first capture, _agree_on_mode)
        from . import ops
        self.scratch = ops.MergedScratch()  # accumulators of the merged weights: owned here, part of the captured graphs
        self.bflat = []                     # flat buffers (one per dtype) behind the model's buffers (multi-rank BatchNorm)
        self.live = None
        self.opt = None
        self.slots = {}
        self.wflat = None
        self.gflat = None
        self.pflat = None
        self.gb_params = []
        self.others = []
        self.other_slots = []
        self.n_w = 0
        self.fused_head = "head" in inspect.signature(model.forward).parameters
        self._has_buffers = self._multi() and any(True for _ in model.buffers())
        # (--normalization bn: BatchNorm inside the MLPs takes its training statistics over the REAL rows of the padded static
        # batch -- HyperIndex.pad_masks, layers.MLP._norm -- so those models replay under hipGraph like the others)
        if broadcast_from_rank0 and self._multi():
            for t in list(model.parameters()):
                dist.broadcast(t.data, src=0)
            self._flatten_buffers()
            self.sync_buffers()

    def _w(self) -> int:
        return _world() if self.collective else 1

    def _multi(self) -> bool:
        """Whether this trainer takes the multi-rank path (collectives, 1 / world gradient scale)."""
        return self._w() > 1 or self.force_collective

    def _flatten_buffers(self):
        """Re-seat the model's buffers (BatchNorm running statistics, batch counters) as views into ONE flat tensor per
        dtype, so that DDP's per-forward buffer broadcast is one collective per dtype instead of one per buffer."""
        if self.bflat:
            return
        groups = {}
        for b in self.model.buffers():
            groups.setdefault(b.dtype, []).append(b)
        for dt, bs in groups.items():
            pad = lambda k: (k + 3) // 4 * 4
            flat = torch.zeros(sum(pad(b.numel()) for b in bs), dtype=dt, device=bs[0].device)
            off = 0
            for b in bs:
                k = b.numel()
                flat[off:off + k].copy_(b.data.reshape(-1))
                b.data = flat[off:off + k].view_as(b)
                off += pad(k)
            self.bflat.append(flat)

    def close(self):
        """Detach this trainer from the model: the persistent gradient accumulators the kernels add into
        (``param._eqh_gbuf``) belong to the trainer, and a later backward outside it (TrainStep, a user loop, another
        GraphedTrainStep) must hand its gradients to autograd again."""
        for p in self.model.parameters():
            if hasattr(p, "_eqh_gbuf"):
                del p._eqh_gbuf
        self.gb_params, self.slots, self.live = [], {}, None
        self.form_calibration = None
        self._g_update = None

    def _buffer_snapshot(self):
        return [b.detach().clone() for b in self.model.buffers()]

    def _buffer_restore(self, snap):
        """The probe, warm-up and capture passes run the model in training mode without being optimiser steps: put the
        BatchNorm running statistics / batch counters (mhnnm, egnn_equihnnm) back, so that they move once per step
        as in the reference and in TrainStep."""
        with torch.no_grad():
            for b, s0 in zip(self.model.buffers(), snap):
                b.copy_(s0)

    def sync_buffers(self):
        """DDP's per-forward buffer broadcast from rank 0 (BatchNorm running statistics): one collective per dtype."""
        if self._multi():
            self._flatten_buffers()
            for flat in self.bflat:
                dist.broadcast(flat, src=0)

    @staticmethod
    def _key(b):
        # (the matmul precision mode, and whether it governs the panel kernels, the batched weight gradients and the EGNN edge
        # kernels, are part of the key: a graph replays the arithmetic it was captured under -- the step's weight packs and its batched weight-gradient
        # launch are launches of that graph, so they follow the key too)
        mode, panels = get_float32_matmul_precision(), get_float32_matmul_precision_panels()
        wgrads, edges = get_float32_matmul_precision_wgrads(), get_float32_matmul_precision_edges()
        if not hasattr(b, "edge_index0"):       # a 2-D batch (batch.GBatch): atoms, edges, molecules
            return (b.x.shape[0], b.edge_index.shape[1], b.y.shape[0], edges, wgrads, panels, mode)
        return (b.x.shape[0], b.edge_attr.shape[0], b.edge_index0.shape[0], b.y.shape[0], edges, wgrads, panels, mode)

    def _loss(self, data):
        nb = getattr(data, "num_real_graphs", None) or data.y.shape[0]
        if getattr(data, "_index_is_live", False):
            data._hyper_index.reset_lazy()      # (built ahead by the index graph and refreshed before this pass: see _capture_index)
        elif hasattr(data, "_hyper_index"):
            data._hyper_index = None
        from . import ops
        if self.fused_head and data.y.is_cuda:
            # pool + output MLP + MSE and their backward in one launch; the gradient that loss.backward()
            # feeds in is the implicit 1, so the head's parameter gradients go straight to the accumulators
            if self.loss_spec is not None:
                return self.model(data, head=(data.y, nb, True, self.loss_spec))
            return self.model(data, head=(data.y, nb, True))
        out = self.model(data)[:nb]
        if self.loss_spec is not None:
            return ops.regression_loss(out, data.y[:nb], self.loss_spec)
        return ops.mse_loss(out, data.y[:nb]) if out.is_cuda else F.mse_loss(out, data.y[:nb])

    def _fwd_bwd(self, data):
        for p in self.model.parameters():
            p.grad = None
        if self.wflat is not None:
            self.wflat.zero_()
        if self.scratch.buf is not None:
            self.scratch.buf.zero_()
        return self._loss_backward(data)

    def _loss_backward(self, data):
        """forward + backward with the accumulating gradient reductions of the fused kernels deferred into
        one launch (ops.defer_begin / defer_flush; the fused readout head produces its parameter gradients
        during the forward pass, so the window opens before it), then the packing of the remaining gradients."""
        from . import ops
        dev = data.y.device
        defer = self.gflat is not None and dev.type == "cuda"
        if defer:
            # accumulators of merged weights: this trainer's persistent scratch, which its update kernel clears (no fill
            # launch per step); with keep_grads a fresh zero-filled slab per window
            ops.defer_begin(dev, scratch=None if self.keep_grads else self.scratch)
        try:
            loss = self._loss(data)
            unit = getattr(self, "_unit", None)         # (loss.backward() would fill a fresh ones_like(loss) every step)
            if unit is None or unit.device != loss.device or unit.dtype != loss.dtype:
                unit = self._unit = torch.ones((), dtype=loss.dtype, device=loss.device)
            loss.backward(unit)
        finally:
            if defer:
                ops.defer_flush(dev)
        self._join()
        self._gather_grads()
        return loss

    def _join(self):
        from . import ops
        if self.gb_params:
            ops.join_wgrad_stream(self.gb_params[0].device)

    def _gather_grads(self):
        """After a backward: the weights the GEMMs accumulated in place already sit in the head of
        ``gflat``; the gradients autograd allocated (biases, norms, embeddings, ...) are packed behind
        them by one batched copy (the padding between slots stays zero, which Adam maps to a zero update)."""
        for p in self.gb_params:
            p.grad = p._eqh_gbuf
        if self.gflat is None:
            return
        if self.accum_steps > 1:
            # the adding form: the slots hold what the group's earlier micro-batches left.  The same launch clears the merged
            # weights' scratch, handed on to the parameters by defer_flush just now: the next micro-batch accumulates into zeros
            from . import ops
            scratch = None if self.keep_grads else self.scratch.buf
            grads = [p.grad for p in self.others]
            if scratch is not None:
                lo, hi = scratch.data_ptr(), scratch.data_ptr() + 4 * scratch.numel()
                if any(lo <= g.data_ptr() < hi for g in grads):
                    raise RuntimeError("GraphedTrainStep: a parameter's gradient lies inside the merged weights' scratch, "
                                       "which the adding launch clears")
            ops.add_many(self.other_slots, grads, zero_also=scratch)
        elif self.others:
            from . import ops
            ops.copy_many(self.other_slots, [p.grad for p in self.others])

    def _setup_grad_buffers(self, data, live):
        """Give every weight that is used ONLY through ops.linear, and every bias / LayerNorm vector used
        ONLY through the fused kernels, a persistent gradient accumulator (the head of one flat buffer,
        zeroed by a single fill per step): the kernels add into it, so a layer applied L times costs no
        autograd add kernels.  A probe pass drops any parameter that autograd still produces a gradient
        for (i.e. that is also used some other way)."""
        from . import ops
        cand = [p for p in live if (id(p) in ops.LINEAR_PARAMS and p.dim() == 2) or id(p) in ops.ACC_PARAMS]
        dev, dt = live[0].device, live[0].dtype
        if cand:
            probe = torch.zeros(sum(p.numel() for p in cand), dtype=dt, device=dev)
            off = 0
            for p in cand:
                p._eqh_gbuf = probe[off:off + p.numel()].view_as(p)
                off += p.numel()
            for p in self.model.parameters():
                p.grad = None
            self._loss(data).backward()
            self._join()
            for p in cand:
                if p.grad is not None:
                    del p._eqh_gbuf
        self.gb_params = [p for p in cand if hasattr(p, "_eqh_gbuf")]
        gb = {id(p) for p in self.gb_params}
        self.others = [p for p in live if id(p) not in gb]
        order = self.gb_params + self.others
        pad = lambda k: (k + 63) // 64 * 64   # every view starts 256-byte aligned (the kernels want 16)
        n = sum(pad(p.numel()) for p in order)
        self.n_w = sum(pad(p.numel()) for p in self.gb_params)
        # one flat buffer each for parameters and gradients, same element order: the optimiser, the
        # all-reduce and the zero-fill all see ONE tensor instead of ~100
        self.gflat = torch.zeros(n, dtype=dt, device=dev)
        pflat = torch.zeros(n, dtype=dt, device=dev)
        self.other_slots = []
        off = 0
        for p in order:
            k = p.numel()
            pflat[off:off + k].copy_(p.data.reshape(-1))
            p.data = pflat[off:off + k].view_as(p)
            if id(p) in gb:
                p._eqh_gbuf = self.gflat[off:off + k].view_as(p)
            else:
                self.other_slots.append(self.gflat[off:off + k].view_as(p))
            off += pad(k)
        self.wflat = self.gflat[:self.n_w] if self.n_w else None
        self.pflat = torch.nn.Parameter(pflat)
        self.pflat.grad = self.gflat

    def _bootstrap(self, data):
        """Eager first step: discovers the live parameters, lays out the flat buffers and creates
        the capturable fused Adam (also performs every lazy one-time initialisation of the HIP
        library and of the GEMM libraries before anything is captured)."""
        from . import ops
        for p in self.model.parameters():      # accumulators of an earlier trainer on this model are stale
            if hasattr(p, "_eqh_gbuf"):
                del p._eqh_gbuf
        ops.LINEAR_PARAMS.clear()
        ops.ACC_PARAMS.clear()
        self.gflat = None
        snap = self._buffer_snapshot()
        loss = self._fwd_bwd(data)
        self.live = [p for p in self.model.parameters() if p.grad is not None]
        self._setup_grad_buffers(data, self.live)
        self._buffer_restore(snap)             # discovery + probe passes were not steps
        loss = self._fwd_bwd(data)
        # Adam is elementwise: one update over the flat tensor equals the per-parameter updates
        self.opt = FlatAdam(self.pflat, lr=self.lr, weight_decay=self.wd, max_grad_norm=self.clip_gnorm,
                            ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
        self.opt.zero_grad_in_step = not self.keep_grads
        self.opt.zero_also = lambda: self.scratch.buf
        if self.accum_steps > 1:
            # micro-step 1 of group 1: gflat holds this micro-batch's gradient and nothing is updated.  The group's close
            # (_close_group, eager for the first group) makes the all-reduce that creates the communicator
            self.opt.grad_scale = 1.0 / (self.accum_steps * self._w())
            self.micro = 1
            return loss.detach()
        self.updates += 1
        if self._multi():
            dist.all_reduce(self.gflat, op=dist.ReduceOp.SUM)     # (eager: also creates the communicator before any capture)
            self.opt.grad_scale = 1.0 / self._w()     # the average is folded into the update
        self.opt.step()
        return loss.detach()

    def _captured_all_reduce(self):
        """The gradient all-reduce as a node of the step graph.  A backend that cannot be stream-captured raises here
        (RCCL: ``DistBackendError``, a RuntimeError); that -- and nothing else -- is what makes a capture fall back to the
        split form.  (A method so that the two-rank tests can stand in a backend that refuses on one rank.)"""
        dist.all_reduce(self.gflat, op=dist.ReduceOp.SUM)

    def _capture_pass(self, static, in_graph: bool, update: bool = True):
        """One capture of the step for the static batch.  ``in_graph``: buffer broadcast, all-reduce and update are nodes of
        the one graph; else the graph ends after the backward pass and the update is a second graph (g_opt).
        ``update=False`` (with ``in_graph=False``; accum_steps > 1): the accumulate graph -- the backward pass alone, whatever
        the number of ranks: no update in it, no g_opt beside it, and no clearing of ``wflat`` at its head.  Raises
        ``CollectiveCaptureRefused`` as ``capture_graph`` does."""
        from . import ops
        multi = self._multi()
        for p in self.model.parameters():
            p.grad = None
        tl = ops.TIMELINE            # bench.py's in-graph kernel timing: only the captured pass is recorded
        if tl is not None:
            tl.reset()

        def body(collective):
            if tl is not None:
                for _ in range(4):
                    tl.pair("stamp_pair")
            if in_graph and self._has_buffers and not collective(self.sync_buffers):
                return None
            if self.wflat is not None and self.keep_grads and update:
                self.wflat.zero_()
            sig = self._signal if getattr(static, "_index_is_live", False) else None
            if sig is not None:
                # the post that releases the NEXT batch's index build: where the model marks it (ops.signal_point:
                # behind the EGNN edge kernel, when the chip stops being full), else at the head of the step
                sig.armed, sig.at = True, self._signal_name
                ops.SIGNAL = sig
                if not (self.signal_in_model and self._signal_reached):
                    sig.post()
            try:
                loss = self._loss_backward(static)
            finally:
                if sig is not None:
                    ops.SIGNAL = None
                    if sig.armed:       # (cannot happen after the probe; a step without its post would stall the next index build until the wait's timeout)
                        sig.post()
            if in_graph and not collective(self._captured_all_reduce):
                return loss
            if update and (in_graph or not multi):
                self.opt.step()     # nothing the host must do between backward and update: one graph, one launch
            return loss
        g_bwd, loss = capture_graph(body)
        g_opt = None
        if update and multi and not in_graph:
            g_opt = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_opt, capture_error_mode="thread_local"):
                self.opt.step()
        return g_bwd, g_opt, loss

    def _agree_on_mode(self, mode: str) -> str:
        """All ranks take the SAME form of the step: "in_graph" only if every rank captured the collective.  One eager
        all-reduce (MIN) of a success flag, at the FIRST capture of the run -- every rank reaches it at its second step,
        after the eager bootstrap step, whatever its batches look like -- and the outcome then binds every later capture
        (``_capture`` raises if a later bucket cannot follow it: a rank that changed form alone would leave the others
        waiting in a collective it never enters)."""
        flag = torch.tensor([1 if mode == "in_graph" else 0], dtype=torch.int32, device=self.gflat.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return "in_graph" if int(flag.item()) == 1 else "split"

    def _capture(self, static):
        multi = self._multi()
        # autograd graphs of earlier eager passes that are only kept alive by reference cycles hold AccumulateGrad nodes bound
        # to the stream they ran on; a capture that meets one is invalidated (and capture_end of an invalidated capture
        # segfaults on ROCm 7.2): collect them first (a capture is rare and costs ~0.3 s anyway)
        gc.collect()
        # accum_steps > 1: a bucket first met in the middle of a group -- the warm-up passes below clear wflat and write
        # gradients of their own over what the group has summed so far: set it aside, put it back behind the capture
        held = self.gflat.clone() if self.accum_steps > 1 else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        snap = self._buffer_snapshot()
        from . import ops
        probe = types.SimpleNamespace(armed=False, seen=set())     # which signal points does this model's step reach?
        with torch.cuda.stream(side):  # warm-up on a side stream, as graph capture requires
            for _ in range(2):
                ops.SIGNAL = probe
                try:
                    self._fwd_bwd(static)
                finally:
                    ops.SIGNAL = None
            self._buffer_restore(snap)
        torch.cuda.current_stream().wait_stream(side)
        # the first of the preferred points this model reaches (conv-stack models: before the last application; models without
        # the stack: before the read-out head; else the head of the step)
        self._signal_name = next((n for n in self.signal_at.split(",") if n in probe.seen), None)
        self._signal_reached = self._signal_name is not None
        self.scratch.freeze()          # its address is about to become part of a graph
        prefetch = BucketPrefetch.capture(static, self._prefetch_stream, self._signal) if self._prefetch_on else None
        if prefetch is not None:
            self._prefetch_stream, self._signal, self.index_build_us = prefetch.stream, prefetch.signal, prefetch.index_build_us
        if held is not None:
            # the accumulate graph: the backward pass alone on every rank; the collective belongs to the update graph
            g_bwd, g_opt, loss = self._capture_pass(static, False, update=False)
            mode = "split" if multi else "none"
            self.gflat.copy_(held)      # (the scratch is empty already: the adding launch of every pass clears it)
        else:
            g_bwd, g_opt, loss = self._settle_mode(lambda in_graph: self._capture_pass(static, in_graph),
                                                   abandoned=lambda: self._buffer_restore(snap))
            mode = self.collective_mode
            if self.wflat is not None and not self.keep_grads:
                self.wflat.zero_()       # what the captured update leaves behind after every replay: zeros to accumulate into
                if self.scratch.buf is not None:
                    self.scratch.buf.zero_()
        return {"static": static, "bwd": g_bwd, "opt": g_opt, "loss": loss, "mode": mode, "prefetch": prefetch}

    def _settle_mode(self, capture: Callable, abandoned: Callable = lambda: None):
        """``capture(in_graph=True)``, with the gradient all-reduce inside the graph, where that is possible and every rank
        can, else ``capture(False)``: returns what the capture that stays returned and sets ``collective_mode``.  The ranks
        settle the form at their FIRST capture (``_agree_on_mode``): a refusal there takes every rank to "split", a refusal
        later is an error.  ``abandoned()`` runs behind an in-graph capture that does not stay (it moved the model's buffers)."""
        multi = self._multi()
        mode = "none"
        if multi:
            mode = "in_graph" if (self.graph_collective and dist.get_backend() in self.in_graph_backends
                                  and self.collective_mode != "split") else "split"
        first = multi and not self._mode_agreed
        cap = None
        if mode == "in_graph":
            try:
                cap = capture(True)
            except CollectiveCaptureRefused as exc:    # the split form is always available -- if every rank takes it
                if not first:
                    raise RuntimeError("GraphedTrainStep: the ranks agreed on the in-graph all-reduce at the first capture "
                                       f"and this rank can no longer capture it ({exc})") from exc
                self.capture_error = str(exc)
                torch.cuda.synchronize()
                abandoned()
                mode = "split"
            if mode == "split":
                # the abandoned pass's CUDAGraph sits in the exception's traceback (a reference cycle): destroy it NOW --
                # a hipGraphDestroy issued by the collector in the middle of the next capture aborts the process
                gc.collect()
        if first:
            agreed = self._agree_on_mode(mode)
            self._mode_agreed = True
            if agreed != mode:         # this rank captured the collective, another one could not: drop the graph, follow
                self.capture_error = "another rank could not capture the collective"
                cap, mode = None, agreed
                abandoned()
                gc.collect()
        if cap is None:
            cap = capture(False)
        self.collective_mode = mode
        return cap

    def _capture_update(self):
        """The update graph shared by all buckets (accum_steps > 1), captured at the second close of a group (the first ran
        eagerly: every launch of the update and the communicator exist): ``opt.step()`` in its ``clip_gnorm`` / ``ema_decay``
        form, behind the gradient all-reduce where the ranks settle on "in_graph", else the all-reduce stays in front of it."""
        gc.collect()

        def update(in_graph):
            def body(collective):
                if not in_graph or collective(self._captured_all_reduce):
                    self.opt.step()
            return capture_graph(body)[0]
        self._g_update = self._settle_mode(update)

    def _close_group(self):
        """accum_steps > 1: the one collective and the one update of a group, on the sum ``gflat`` holds (scaled
        1 / (accum_steps * world) inside the update).  Eager for the first group, the replayed update graph from then on."""
        if self._g_update is None and self.updates > 0:
            self._capture_update()
        self.opt.sync_lr()
        if self._g_update is None:
            if self._multi():
                dist.all_reduce(self.gflat, op=dist.ReduceOp.SUM)
            self.opt.step()
        else:
            if self.collective_mode == "split":
                dist.all_reduce(self.gflat, op=dist.ReduceOp.SUM)
            self._g_update.replay()
        self.micro = 0
        self.updates += 1

    @property
    def ema_flat(self) -> Optional[torch.Tensor]:
        """With ``ema_decay``: the average of ``pflat``, same length and element order (the optimiser's ``state["ema"]``);
        ``None`` without it or before the first step."""
        return self.opt.state[self.pflat].get("ema") if self.opt is not None else None

    def _ema_exchange(self):
        from . import hip, ops
        live, ema = self.pflat.data, self.ema_flat
        hip.check(hip.lib().eqh_swap_f32(ops._ptr(live), ops._ptr(ema), live.numel(), ops._stream(live.device)), "eqh_swap_f32")

    def _ema_of(self):
        ema, base, out = self.ema_flat, self.pflat.data_ptr(), {}
        for p in self.live:
            off = (p.data_ptr() - base) // 4
            out[id(p)] = ema[off:off + p.numel()].view_as(p)
        return out

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """With ``clip_gnorm``: the update kernel's readout, 4 floats on the device -- {norm of the averaged gradient before
        clipping, coef, running maximum of the norm, number of clipped steps}; zero the last two to restart them.  Reading
        the property does not synchronise; ``None`` without clipping or before the first step."""
        return self.opt.grad_norm if self.opt is not None else None

    @property
    def index_prefetch(self) -> bool:
        """Whether newly captured steps take the built-ahead form.  Assigning it pins the form (no calibration)."""
        return self._prefetch_on

    @index_prefetch.setter
    def index_prefetch(self, on: bool):
        self._prefetch_on = bool(on)
        self.prefetch_policy = "on" if on else "off"
        dropped, self.form_calibration = getattr(self.form_calibration, "aside", None) is not None, None
        if dropped:
            gc.collect()

    @property
    def calibrating(self) -> bool:
        """True until the auto policy has timed both forms of the step and kept one (callers that time steps themselves --
        bench.py -- run steps until this clears before their own warm-up)."""
        return self.prefetch_policy == "auto" and self.calibration is None

    def _calibrate(self, key):
        """Auto policy, at the head of every graphed step until the decision: carries out FormCalibration's answers on ``slots``."""
        cal = self.form_calibration = self.form_calibration or FormCalibration(self.accum_steps)
        act = cal.step(key)
        if act == cal.SET_ASIDE:            # now the other form: every bucket is captured again
            cal.aside, self.slots = self.slots, {}
            self._prefetch_on = False
        elif act is not None:
            if act == cal.RESTORE:          # back to the graphs of the first window
                self.slots = cal.aside
                self._prefetch_on = True
            cal.aside = None
            self.calibration, self.form_calibration = cal.result, None
            gc.collect()                    # (dropped graphs are destroyed now, not inside a later capture)

    def step(self, data, next_data=None) -> torch.Tensor:
        """One training step on ``data``.  ``next_data``: the batch of the NEXT call, if the caller has it (a loader with one
        batch of look-ahead, ``with_next``): its per-batch index is then built beside this step instead of at the head of
        the next one.  Numerically the two forms are the same step."""
        self._refuse_averaging("step()")
        if self.live is None:
            loss = self._bootstrap(data)
            if self.loss_readout:
                _accumulate_loss(self, loss)
            return loss
        key = self._key(data)
        if self.prefetch_policy == "auto" and self.calibration is None:
            self._calibrate(key)
        slot = self.slots.get(key)
        if slot is None:
            slot = self.slots[key] = self._capture(static_copy_of(data))
        pf = slot.get("prefetch")
        if pf is not None:
            token = batch_token(data)
            if pf.holds != token:
                self.prefetch_misses += 1
                pf.stream.wait_stream(torch.cuda.current_stream())     # (data may have been produced on this stream)
                pf.stage(data, token)
            else:
                self.prefetch_hits += 1
            pf.refresh()
        else:
            copy_into_static(slot["static"], data)
        self.opt.sync_lr()
        if self._has_buffers and slot["mode"] != "in_graph":
            self.sync_buffers()
        if self.accum_steps > 1 and self.keep_grads and self.micro == 0:
            self.gflat.zero_()            # (no update clears it: in front of a group's first micro-step, not inside the graph)
        slot["bwd"].replay()
        if pf is not None:
            self._signal.posted += 1      # (one post per replay of a step graph with a live index)
        if self.accum_steps > 1:
            self.micro += 1
            if self.micro == self.accum_steps:
                self._close_group()
        else:
            self.updates += 1
            if slot["opt"] is not None:
                dist.all_reduce(self.gflat, op=dist.ReduceOp.SUM)
                slot["opt"].replay()
        if self.loss_readout:
            _accumulate_loss(self, slot["loss"])     # (the replay's static loss scalar, read before the next replay writes it)
        if next_data is not None:
            nslot = self.slots.get(self._key(next_data))
            npf = nslot.get("prefetch") if nslot is not None else None
            if npf is not None:
                npf.stage(next_data, batch_token(next_data), after_signal=self._signal.posted if pf is not None else None)
        return slot["loss"].detach()


class GraphedEvalStep:
    """``model(data)`` in eval mode under ``no_grad`` -- the validation / test passes the reference runs every epoch
    (main.py:65-87,89-132) -- captured ONCE per static shape bucket as a forward-only hipGraph and replayed: an eager forward
    pass is bound by Python launch issue (4-6 x the replayed time), exactly like the eager training step.  Batches must be
    padded to bucket extents (``batch.pad_batch`` / ``fit.BucketedLoader``); the returned predictions are a STATIC tensor,
    valid until the next call (rows past ``num_real_graphs`` are padding).  The graphs read the parameters and buffers in
    place, so they follow the optimiser and ``load_state_dict`` without re-capture.  A captured graph holds the ADDRESSES of
    the parameters and buffers: every call compares them with the ones recorded at capture, and when they have moved (a
    GraphedTrainStep's bootstrap re-seats ``p.data`` into its flat buffer; ``model.to`` / a re-seated BatchNorm buffer) the
    stale graphs are dropped and the bucket is captured again instead of replaying reads of freed storage."""

    def __init__(self, model: nn.Module):
        self.model = model
        self.slots = {}
        self.addresses = None
        self.recaptures = 0

    def _addresses(self):
        return tuple(t.data_ptr() for t in self.model.parameters()) + tuple(t.data_ptr() for t in self.model.buffers())

    def close(self):
        self.slots = {}

    def _capture(self, static):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                static._hyper_index = None
                self.model(static)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        static._hyper_index = None
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = self.model(static)
        return {"static": static, "graph": g, "out": out}

    @torch.no_grad()
    def __call__(self, data) -> torch.Tensor:
        if self.model.training:
            raise RuntimeError("GraphedEvalStep: put the model in eval mode first (the captured graphs are eval-mode forwards)")
        key = GraphedTrainStep._key(data)
        addr = self._addresses()
        if addr != self.addresses:
            if self.slots:
                self.recaptures += 1
            self.slots = {}
            self.addresses = addr
        slot = self.slots.get(key)
        if slot is None:
            slot = self.slots[key] = self._capture(static_copy_of(data))
        copy_into_static(slot["static"], data)
        slot["graph"].replay()
        return slot["out"]
