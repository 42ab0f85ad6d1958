"""What GraphedTrainStep keeps per static batch beside the step graph itself: the static copies of a batch, the index
prefetch of one bucket (``BucketPrefetch``) and the measurement that decides whether the prefetch pays (``FormCalibration``)."""
from __future__ import annotations

import dataclasses
import os
import time
from typing import Optional

import torch


def static_copy_of(data):
    """A batch of ``data``'s extents in storage of its own, for a captured graph to read: ``packed()`` (one flat buffer,
    refreshed by ONE copy per step) where the batch has it, else a clone field by field."""
    if hasattr(data, "packed"):
        static = data.packed()
    else:
        static = type(data)(**{f: (getattr(data, f).clone() if torch.is_tensor(getattr(data, f)) else getattr(data, f))
                               for f in data.__dataclass_fields__})
    static.num_real_graphs = getattr(data, "num_real_graphs", None)
    return static


def copy_into_static(static, data):
    """``data`` into its static twin on the current stream: one copy of the flat buffer when the layouts match, else tensor
    field by tensor field."""
    lay = getattr(data, "_layout", None)
    if lay is not None and lay == getattr(static, "_layout", None):
        static._flat.copy_(data._flat, non_blocking=True)
    else:
        for f in data.__dataclass_fields__:
            v = getattr(data, f)
            if torch.is_tensor(v):
                getattr(static, f).copy_(v, non_blocking=True)


def batch_token(data):
    """Identity of a batch's CONTENTS: loaders hand the same device buffers out again with new molecules (and bump
    ``_generation``, fit.BucketedLoader)."""
    return (id(data), getattr(data, "_generation", 0))


class TorchEvent:
    """``torch.cuda.Event`` behind the ``record(stream)`` / ``wait(stream)`` of ``ops.StreamEvent``, which is the other kind of
    event a ``BucketPrefetch`` takes.  A fresh event per record: a recorded torch event is not re-armed."""

    _ev = None

    def record(self, stream):
        self._ev = torch.cuda.Event()
        self._ev.record(stream)

    def wait(self, stream):
        stream.wait_event(self._ev)


@dataclasses.dataclass(eq=False)
class BucketPrefetch:
    """The index prefetch of one bucket: ONE batched copy at the head of every step moves what the index graph built beside
    the last step from staged to live (3 MB, ~4.4 us).  One step graph per bucket (two step graphs over two sets of live
    buffers would save the copy and double the captures and the graphs' memory)."""

    staged: object          # a second packed copy of the static batch, which a step's successor is written into
    g_index: object         # hipGraph that builds the staged batch's HyperIndex (CSR sorts, kNN, transposed kNN CSR) on `stream`
    ix_staged: object       # that index
    live: object            # a clone of it, installed on the static batch: ALL the step graph reads
    dsts: list              # the tensor pairs of the head copy: index tensors + the batch's flat buffer, live ...
    srcs: list              # ... and staged
    stream: object          # the side stream and ...
    signal: object          # ... the ops.StepSignal that the buckets of one trainer share
    free: object            # event behind the head copy of the last step that read the staged buffers
    ready: object           # event behind the index build
    index_build_us: float   # the index graph alone, timed at the capture (a pure function of the staged batch)
    holds: Optional[tuple] = None   # the token of the batch that is staged, None once a step has taken it

    @classmethod
    def capture(cls, static, stream=None, signal=None):
        """Set up the prefetch for the static batch of a bucket, or return None when the model's index cannot be built ahead
        (no index on the batch, or a neighbour search on coordinates other than the batch's own ``pos``).  ``stream`` /
        ``signal``: those of the trainer's earlier buckets (made here for the first)."""
        from . import ops
        from .index import HyperIndex
        ixw = getattr(static, "_hyper_index", None)
        flat = getattr(static, "_flat", None)
        if ixw is None or flat is None or not static.pos.is_cuda:
            return None
        want = (static.pos.data_ptr(), tuple(static.pos.shape), static.pos.dtype)
        keys = list(ixw._knn.keys())
        if any(ixw._knn_pos.get(k) != want for k in keys) or any(static.pos.shape[0] - 1 < k for k, m in keys if m == 1):
            return None
        rkeys = list(getattr(ixw, "_radius_args", {}).items())      # (r, k) -> (coordinates, RBF means, betas): ViSNet
        if any(at != want for _, (at, _m, _b) in rkeys):
            return None
        staged = static_copy_of(static)
        if signal is None:
            signal = ops.StepSignal(static.pos.device)
        if stream is None:
            stream = torch.cuda.Stream()

        def build():
            staged._hyper_index = None
            ix = HyperIndex.from_batch(staged)
            for k, m in keys:
                ix.knn(staged.pos, k, m)
            for (r, k), (_at, means, betas) in rkeys:
                ix.radius(staged.pos, r, k, means, betas)
            return ix
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            build()                                  # (warm-up on the stream the graph will be replayed on)
        torch.cuda.current_stream().wait_stream(stream)
        g_index = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_index, capture_error_mode="thread_local"):
            ix_staged = build()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            g_index.replay()
            e0.record(stream)
            for _ in range(3):
                g_index.replay()
            e1.record(stream)
        e1.synchronize()
        index_build_us = e0.elapsed_time(e1) * 1e3 / 3
        live, dsts, srcs = ix_staged.live_clone(static)
        static._hyper_index, static._index_is_live = live, True
        as_words = lambda t: t.view(torch.float32) if t.dtype != torch.float32 else t
        nf = flat.numel() // 4 * 4
        dsts = [as_words(t).reshape(-1) for t in dsts] + [flat[:nf].view(torch.float32)]
        srcs = [as_words(t).reshape(-1) for t in srcs] + [staged._flat[:nf].view(torch.float32)]
        # (ops.StreamEvent: no system-scope fence -- a torch.cuda.Event recorded at the head of every step writes the L2 back and
        # invalidates it; EQH_TORCH_EVENTS=1 restores those for A/B runs)
        event = TorchEvent if os.environ.get("EQH_TORCH_EVENTS") else ops.StreamEvent
        free, ready = event(), event()
        free.record(torch.cuda.current_stream())
        return cls(staged=staged, g_index=g_index, ix_staged=ix_staged, live=live, dsts=dsts, srcs=srcs, stream=stream,
                   signal=signal, free=free, ready=ready, index_build_us=index_build_us)

    def stage(self, data, token, after_signal=None):
        """Write ``data`` into the staged batch and build its index there, on the prefetch stream: ordered behind the head
        copy of the last step that read the staged buffers (``free``), not behind the step itself -- and, with
        ``after_signal`` (the count the running step's signal node brings the counter to), held back until that step has
        reached its signal point.  ``token``: what ``holds`` then says is staged (``batch_token(data)``)."""
        with torch.cuda.stream(self.stream):
            self.free.wait(self.stream)
            if after_signal is not None:
                self.signal.wait(after_signal)
            copy_into_static(self.staged, data)
            self.g_index.replay()
            self.ready.record(self.stream)
        self.holds = token

    def refresh(self):
        """Head of a step: staged -> live (index tensors and the batch itself) in one launch on the step's stream; the
        staged batch is then taken."""
        from . import ops
        cur = torch.cuda.current_stream()
        self.ready.wait(cur)
        ops.copy_many(self.dsts, self.srcs)
        self.free.record(cur)
        self.holds = None


class FormCalibration:
    """Which form of the step is faster, the one with the index built ahead or the one with it in the step graph: per form,
    one capture step, CAL_WARM replays, then a window of steps between two device synchronisations (wall clock: the two
    streams overlap, so no single stream's events see a step).  ``step(key)`` is told the bucket of every graphed step and
    answers what the trainer must do with its captured steps: SET_ASIDE (the first window is timed: park them in ``aside``
    and capture every bucket again in the other form), RESTORE (decided for the built-ahead form: back to the ones in
    ``aside``), KEEP (decided for the form that is running: drop ``aside``) or None.  ``result``: the ``calibration`` dict."""

    CAL_WARM, CAL_STEPS = 3, 12         # replays before a timed window, steps in it
    MAX_RESTARTS, MARGIN = 16, 0.99     # windows a step of another bucket may break off; built ahead has to win by 1 %
    SET_ASIDE, RESTORE, KEEP = "set_aside", "restore", "keep"

    def __init__(self, accum_steps: int = 1, sync=None, clock=None):
        self.sync = torch.cuda.synchronize if sync is None else sync
        self.clock = time.perf_counter if clock is None else clock
        # steps in a timed window: CAL_STEPS, rounded up to whole groups of ``accum_steps`` -- any run of whole groups holds
        # the same number of update launches, wherever in a group it starts, so both forms are timed over the same work
        self.steps = (self.CAL_STEPS + accum_steps - 1) // accum_steps * accum_steps
        self.form, self.key, self.n, self.restarts = "built_ahead", None, 0, 0
        self.t, self.t0, self.aside, self.result = {}, None, None, None

    def step(self, key):
        if self.key is None:
            self.key = key
        if key != self.key:                 # a step of another bucket restarts the window
            self.key, self.n = key, 0
            self.restarts += 1
            # (buckets that alternate too fast to time a window: keep the form that is running)
            return self._decide(None) if self.restarts > self.MAX_RESTARTS else None
        self.n += 1
        first_timed = 1 + self.CAL_WARM + 1
        if self.n == first_timed:
            self.sync()
            self.t0 = self.clock()
        elif self.n == first_timed + self.steps:
            self.sync()
            self.t[self.form] = (self.clock() - self.t0) / self.steps * 1e3
            if self.form == "in_step":
                return self._decide(self.t)
            self.form, self.n = "in_step", 1
            return self.SET_ASIDE

    def _decide(self, t):
        ahead = self.form == "built_ahead" if t is None else t["built_ahead"] < self.MARGIN * t["in_step"]
        self.result = {"built_ahead_ms": None if t is None else round(t["built_ahead"], 4),
                       "in_step_ms": None if t is None else round(t["in_step"], 4),
                       "steps_per_window": self.steps, "chosen": "built_ahead" if ahead else "in_step"}
        return self.RESTORE if ahead and t is not None else self.KEEP
