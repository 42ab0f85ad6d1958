"""Row kernels: per-incidence hidden layer + reduction, bias/ReLU/LayerNorm rows, gathered LayerNorm reduce, BatchNorm
/ LayerNorm rows, residual mix.

Part of equihgnn_amd.ops (host-side operators over libequihgnn_hip.so; no CPU fallback).
"""
from __future__ import annotations

import torch

from .. import hip
from ._base import (
    LINEAR_PARAMS, _acc_target, _f32c, _hand_out, _note_acc, _ptr, _require_gpu, _rows_ld, _stream, _workspace, timed)
from .aggregate import (CSR, entry_weights, segment_reduce_bytes)
from .products import (mm_nn, mm_nt)
from .grads import (_wgrad_deferred, _wgrad_ok, colsum, wgrad)
from .frames import _dropout_seed

# Training dropout of the hidden layers inside the fused row kernels (the DROP instantiations of csrc/incidence.hip): the
# keep decisions are a hash of (seed, element index), recomputed by the backward.  False: an MLP with an active dropout
# leaves the fused path and runs ReLU, LayerNorm and F.dropout as ATen launches (layers.MLP.hidden).
FUSED_DROPOUT = True


def _drop_route(p, what: str):
    """(p as float, whether the dropout kernels run).  p < 0 is an error; p = 0 is the call without dropout; p >= 1 drops
    everything (handled by the callers: zeros, as nn.Dropout(p=1))."""
    p = float(p)
    if not p >= 0.0:
        raise ValueError(f"{what}: dropout probability has to be between 0 and 1, but got {p}")
    return p, p > 0.0


class _Zeros(torch.autograd.Function):
    """dropout with p >= 1: zeros of ``shape``, and zero gradients to the tensors that fed the dropped layer."""

    @staticmethod
    def forward(ctx, shape, *inputs):
        ctx.like = [(t.shape, t.dtype, t.device) if isinstance(t, torch.Tensor) else None for t in inputs]
        ref = next(t for t in inputs if isinstance(t, torch.Tensor))
        return torch.zeros(shape, dtype=torch.float32, device=ref.device)

    @staticmethod
    def backward(ctx, dout):
        return (None,) + tuple(None if m is None else torch.zeros(m[0], dtype=m[1], device=m[2]) for m in ctx.like)


def inc_fwd_bytes(nnz: int, rows: int, C: int) -> int:
    """Algorithmic bytes of k_inc_fwd (generic form): two gathered rows per incidence + one output row, three index words
    per incidence, the rowptr, gamma and beta."""
    return 4 * C * (2 * nnz + rows) + 12 * nnz + 4 * (rows + 1) + 8 * C


def inc_fwd_col_bytes(nnz: int, rows: int, C: int) -> int:
    """Algorithmic bytes of k_inc_fwd_col: the row operand is fetched ONCE per output row
    (incidence.hip: own row read before the entry loop), one gathered row per incidence, one output row; the col word of
    every incidence, the rowptr, gamma and beta: 4C (nnz + 2R) + 4 nnz + 4 (R + 1) + 8C."""
    return 4 * C * (nnz + 2 * rows) + 4 * nnz + 4 * (rows + 1) + 8 * C


def _launch(fn: str, *args):
    hip.check(getattr(hip.lib(), fn)(*args), fn)


def _param_grads(ctx_acc, n: int, C: int, device):
    """Where a backward kernel writes the ``n`` parameter gradients of ``ctx_acc``: (targets, acc, small, o) -- in place
    into the parameters' accumulators when every one has one (acc), else into the rows of a fresh ``small``."""
    tg = [_acc_target(q) for q in ctx_acc]
    acc = all(t is not None for t in tg)   # all accumulate in place: nothing for autograd to add
    small = None if acc else torch.empty((n, C), dtype=torch.float32, device=device)
    return tg, acc, small, (tg if acc else list(small))


class _IncidenceLnReduce(torch.autograd.Function):
    """S[r] = reduce_{p in row r} LayerNorm(relu(pa[ia[p]] + qb[ib[p]])) — one launch instead of
    gather, gather, add, ReLU, LayerNorm, segmented reduce (csrc/incidence.hip).
    ``p`` > 0: dropout behind the LayerNorm, S[r] = reduce keep[p] * LN(..), the decision of incidence p, channel c being
    element p * C + c (hg_incidence_ln_reduce_drop_*).  That backward kernel yields d beta too (a mask sits between beta
    and the sum)."""

    @staticmethod
    def forward(ctx, pa, qb, gamma, beta, ia32, ib32, csr_a: CSR, csr_b: CSR, out_csr: CSR, okey32, mean, eps,
                acc_params, p=0.0, seed=None):
        _require_gpu(pa, "incidence_ln_reduce")
        pa, qb, gamma, beta = _f32c(pa), _f32c(qb), _f32c(gamma), _f32c(beta)
        C = pa.shape[1]
        drop = p > 0.0
        if drop and seed is None:
            seed = _dropout_seed(pa.device, p)
        dargs = (p, _ptr(seed)) if drop else ()
        out = torch.empty((out_csr.n_rows, C), dtype=torch.float32, device=pa.device)
        tail = (_ptr(gamma), _ptr(beta), out_csr.n_rows, C, 1 if mean else 0, float(eps), *dargs, _ptr(out),
                _stream(pa.device))
        if okey32 is ia32 or okey32 is ib32:
            # the output row is one operand's own index: (rowptr, col) of the output CSR says it all (the dropout
            # decisions belong to the incidences' positions: perm too)
            fn = "hg_incidence_ln_reduce_drop_fwd_col" if drop else "hg_incidence_ln_reduce_fwd_col"
            timed("k_inc_drop_fwd_col" if drop else "k_inc_fwd_col",
                  inc_fwd_col_bytes(out_csr.nnz, out_csr.n_rows, C) + (4 * out_csr.nnz if drop else 0),
                  lambda: _launch(fn, _ptr(pa), _ptr(qb), _ptr(out_csr.rowptr),
                                  _ptr(out_csr.col), *((_ptr(out_csr.perm),) if drop else ()), 1 if okey32 is ia32 else 0,
                                  *tail))
        else:
            fn = "hg_incidence_ln_reduce_drop_fwd" if drop else "hg_incidence_ln_reduce_fwd"
            timed("k_inc_drop_fwd" if drop else "k_inc_fwd", inc_fwd_bytes(out_csr.nnz, out_csr.n_rows, C),
                  lambda: _launch(fn, _ptr(pa), _ptr(qb), _ptr(ia32), _ptr(ib32),
                                  _ptr(out_csr.rowptr), _ptr(out_csr.perm), *tail))
        ctx.save_for_backward(pa, qb, gamma)
        ctx.meta = (ia32, ib32, csr_a, csr_b, out_csr, okey32, mean, eps, p, seed)
        ctx.acc = acc_params
        return out

    @staticmethod
    def backward(ctx, ds):
        pa, qb, gamma = ctx.saved_tensors
        ia32, ib32, csr_a, csr_b, out_csr, okey32, mean, eps, p, seed = ctx.meta
        ds = _f32c(ds)
        C = pa.shape[1]
        dev = pa.device
        dpa, dqb = torch.empty_like(pa), torch.empty_like(qb)
        head = (_ptr(pa), _ptr(qb), _ptr(ia32), _ptr(ib32), _ptr(csr_a.rowptr), _ptr(csr_a.perm), csr_a.n_rows,
                _ptr(csr_b.rowptr), _ptr(csr_b.perm), csr_b.n_rows, _ptr(okey32), _ptr(out_csr.rowptr), _ptr(ds),
                _ptr(gamma), C, 1 if mean else 0, float(eps))
        # algorithmic bytes: each operand side walks every incidence once and gathers, per incidence, the OTHER
        # operand's row and the output-gradient row, reads its own row once and writes its own gradient row:
        # 4C (4 nnz + 2 (Ra + Rb)) + five index words per incidence and side + both rowptrs
        nnz_ = csr_a.nnz
        nbytes = 4 * C * (4 * nnz_ + 2 * (csr_a.n_rows + csr_b.n_rows)) + 2 * 20 * nnz_ + 4 * (csr_a.n_rows + csr_b.n_rows + 2)
        L = hip.lib()
        if p > 0.0:
            tg, acc, small, o = _param_grads(ctx.acc, 2, C, dev)
            ws_bytes = L.hg_incidence_ln_reduce_drop_bwd_workspace_bytes(csr_a.n_rows, C)
            ws = _workspace(ws_bytes, dev)
            timed("k_inc_drop_bwd_both", nbytes, lambda: _launch(
                "hg_incidence_ln_reduce_drop_bwd", *head, p, _ptr(seed), _ptr(dpa), _ptr(dqb), _ptr(o[0]), _ptr(o[1]),
                1 if acc else 0, _ptr(ws), ws_bytes, _stream(dev)))
            dgamma, dbeta = (None, None) if acc else _hand_out(list(small), tg)
        else:
            g_acc, b_acc = (_acc_target(q) for q in ctx.acc)
            dgamma = g_acc if g_acc is not None else torch.empty_like(gamma)
            ws_bytes = L.hg_incidence_ln_reduce_bwd_workspace_bytes(csr_a.n_rows, C)
            ws = _workspace(ws_bytes, dev)
            timed("k_inc_bwd_both", nbytes, lambda: _launch(
                "hg_incidence_ln_reduce_bwd", *head, _ptr(dpa), _ptr(dqb), _ptr(dgamma), 1 if g_acc is not None else 0,
                _ptr(ws), ws_bytes, _stream(dev)))
            if g_acc is not None:
                dgamma = None
            # d beta = sum_r w_r ds[r], w_r = [row non-empty] (mean) or the row length (sum)
            dbeta = colsum(ds, out_csr.rowptr, 1 if mean else 2, into=b_acc)
        return (dpa, dqb, dgamma, dbeta) + (None,) * 11


def _rowln_bwd(ctx_acc, h, a, c, bias, gamma, dy, eps, fan, p, seed, ex):
    """The backward launch of _BiasReluLn and _LinearAddReluLn: (gradient of the pre-activation, the (dbias, dgamma, dbeta)
    for autograd -- None where accumulated in place).  ``ex``: the entry that takes the scale ``a``, the addend ``c`` and
    the GradFan (with ``p`` > 0 there is only that form)."""
    R, C = h.shape
    dpre = torch.empty_like(h)
    L = hip.lib()
    ws_bytes = (L.hg_bias_relu_ln_drop_bwd_workspace_bytes if p > 0.0 else L.hg_bias_relu_ln_bwd_workspace_bytes)(R, C)
    ws = _workspace(ws_bytes, h.device)
    tg, acc, small, o = _param_grads(ctx_acc, 3, C, h.device)
    outs = (_ptr(dpre), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), 1 if acc else 0, _ptr(ws), ws_bytes)
    if fan is not None and fan.buf is None:     # dpre is also the gradient of the layer's fanned-out addend: summed in the kernel
        fan.buf = torch.empty_like(h)
    fanned = (_ptr(fan.buf) if fan is not None else None, 1 if (fan is not None and fan.n == 0) else 0)
    if p > 0.0:
        _launch("hg_bias_relu_ln_drop_bwd", _ptr(h), a, _ptr(c), _ptr(bias), _ptr(gamma), _ptr(dy), R, C, eps, p, _ptr(seed),
                *outs, *fanned, _stream(h.device))
    elif ex:
        _launch("hg_bias_relu_ln_bwd_ex", _ptr(h), a, _ptr(c), _ptr(bias), _ptr(gamma), _ptr(dy), R, C, eps, *outs, *fanned,
                _stream(h.device))
    else:
        _launch("hg_bias_relu_ln_bwd", _ptr(h), _ptr(bias), _ptr(gamma), _ptr(dy), R, C, eps, *outs, _stream(h.device))
    if fan is not None:
        fan.n += 1
    return dpre, ((None,) * 3 if acc else tuple(_hand_out(list(small), tg)))


class _BiasReluLn(torch.autograd.Function):
    """LayerNorm(relu(h + bias)) over dense rows in one launch; the backward returns dh and, from the
    same pass, the bias / gamma / beta gradients (csrc/incidence.hip).  ``p`` > 0: dropout_p of the result in the same
    launch each way (hg_bias_relu_ln_drop_*); the decision of element [r, c] is that of flat index r * C + c."""

    @staticmethod
    def forward(ctx, h, bias, gamma, beta, eps, acc_params, fan=None, p=0.0, seed=None):
        _require_gpu(h, "bias_relu_ln")
        h, bias, gamma, beta = _f32c(h), _f32c(bias), _f32c(gamma), _f32c(beta)
        R, C = h.shape
        if p > 0.0 and seed is None:
            seed = _dropout_seed(h.device, p)
        out = torch.empty_like(h)
        if p > 0.0:
            _launch("hg_bias_relu_ln_drop_fwd", _ptr(h), 1.0, None, _ptr(bias), _ptr(gamma), _ptr(beta), R, C, float(eps), p,
                    _ptr(seed), _ptr(out), _stream(h.device))
        else:
            _launch("hg_bias_relu_ln_fwd", _ptr(h), _ptr(bias), _ptr(gamma), _ptr(beta), R, C, float(eps), _ptr(out),
                    _stream(h.device))
        ctx.save_for_backward(h, bias, gamma)
        ctx.meta = (float(eps), fan, p, seed)
        ctx.acc = acc_params  # the Parameter objects (their accumulators are looked up at backward time)
        return out

    @staticmethod
    def backward(ctx, dy):
        h, bias, gamma = ctx.saved_tensors
        eps, fan, p, seed = ctx.meta
        dh, grads = _rowln_bwd(ctx.acc, h, 1.0, None, bias, gamma, _f32c(dy), eps, fan, p, seed, ex=fan is not None)
        return (dh, *grads) + (None,) * 5


class _LinearAddReluLn(torch.autograd.Function):
    """LayerNorm(relu(scale * (x @ W.T) + c + bias)): the GEMM writes x @ W.T, the addend c (beta = 1 in _LinearAddC, which
    costs a copy of c into the GEMM's output per call) and the scale enter in the LayerNorm kernel
    (hg_bias_relu_ln_fwd_ex / _bwd_ex; with ``p`` > 0 the dropout kernels, see _BiasReluLn).  Backward: the kernel returns
    the gradient of the pre-activation; the two GEMMs take ``scale`` as their alpha; c's gradient goes to its GradFan
    (summed over the applications) or to autograd."""

    @staticmethod
    def forward(ctx, x, weight, c, scale, bias, gamma, beta, eps, fan, acc_params, p=0.0, seed=None):
        _require_gpu(x, "linear_add_relu_ln")
        x, c, bias, gamma, beta = _f32c(x), _f32c(c), _f32c(bias), _f32c(gamma), _f32c(beta)
        h = mm_nt(x, weight)
        R, C = h.shape
        if p > 0.0 and seed is None:
            seed = _dropout_seed(x.device, p)
        fn, dargs = ("hg_bias_relu_ln_drop_fwd", (p, _ptr(seed))) if p > 0.0 else ("hg_bias_relu_ln_fwd_ex", ())
        out = torch.empty_like(h)
        _launch(fn, _ptr(h), float(scale), _ptr(c), _ptr(bias), _ptr(gamma), _ptr(beta), R, C, float(eps),
                *dargs, _ptr(out), _stream(x.device))
        ctx.save_for_backward(x, weight, h, c, bias, gamma)
        ctx.meta = (float(scale), float(eps), fan, p, seed)
        ctx.acc = acc_params
        return out

    @staticmethod
    def backward(ctx, dy):
        x, weight, h, c, bias, gamma = ctx.saved_tensors
        a, eps, fan, p, seed = ctx.meta
        dpre, grads = _rowln_bwd(ctx.acc, h, a, c, bias, gamma, _f32c(dy), eps, fan, p, seed, ex=True)
        dx = mm_nn(dpre, weight, alpha=a) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            gbuf = getattr(weight, "_eqh_gbuf", None)
            if gbuf is not None and _wgrad_deferred(dpre, x, a, gbuf):
                pass
            elif gbuf is not None and _wgrad_ok(dpre, x):
                wgrad(dpre, x, a, into=gbuf)
            elif gbuf is not None:
                gbuf.addmm_(dpre.t(), x, alpha=a)
            elif _wgrad_ok(dpre, x):
                dw = wgrad(dpre, x, a)
            else:
                dw = torch.addmm(weight, dpre.t(), x, beta=0.0, alpha=a)
        dc = dpre if (fan is None and ctx.needs_input_grad[2]) else None
        return (dx, dw, dc, None, *grads) + (None,) * 5


def linear_add_relu_ln(x, weight, c, scale, bias, gamma, beta, eps: float = 1e-5, fan=None, p: float = 0.0, seed=None):
    """bias_relu_ln(linear_add(x, weight, c, scale), bias, gamma, beta) with the addend and the scale applied inside the
    LayerNorm kernel (2-D fp32 x, c on the GPU); see _LinearAddReluLn.  ``p``, ``seed``: dropout behind the LayerNorm, see
    bias_relu_ln."""
    p, _ = _drop_route(p, "linear_add_relu_ln")
    if p >= 1.0:
        return _Zeros.apply((x.shape[0], weight.shape[0]), x, weight, c, bias, gamma, beta)
    if torch.is_grad_enabled() and weight.requires_grad and weight.is_leaf and not hasattr(weight, "_eqh_transient"):
        LINEAR_PARAMS[id(weight)] = weight
    _note_acc(bias, gamma, beta)
    return _LinearAddReluLn.apply(x, weight, c, scale, bias, gamma, beta, eps, fan, (bias, gamma, beta), p, seed)


class _GatherLnReduce(torch.autograd.Function):
    """out[r] = gamma * reduce_{q in row r of csr} xhat(relu(h[csr.col[q]] + bias)) + beta * [..]: the hidden layer of an
    MLP on dense rows followed by the gathered reduction that is its only consumer, one launch each way
    (hg_gather_ln_reduce_*; csrc/incidence.hip).  ``p`` > 0: dropout behind the LayerNorm, decided per SOURCE row (element
    src * C + c): dropout of the [N, C] hidden tensor followed by the gathered reduction, without that tensor
    (hg_gather_ln_reduce_drop_*)."""

    @staticmethod
    def forward(ctx, h, bias, gamma, beta, csr, csr_t, mean, eps, acc_params, p=0.0, seed=None):
        _require_gpu(h, "gather_ln_reduce")
        h, bias, gamma, beta = _f32c(h), _f32c(bias), _f32c(gamma), _f32c(beta)
        R, C = h.shape
        if csr_t.n_rows != R:
            raise ValueError("gather_ln_reduce: the transposed CSR must have one row per row of h")
        if p > 0.0 and seed is None:
            seed = _dropout_seed(h.device, p)
        fn, dargs = ("hg_gather_ln_reduce_drop_fwd", (p, _ptr(seed))) if p > 0.0 else ("hg_gather_ln_reduce_fwd", ())
        out = torch.empty((csr.n_rows, C), dtype=torch.float32, device=h.device)
        timed("k_gather_ln_drop_fwd" if p > 0.0 else "k_gather_ln_fwd",
              segment_reduce_bytes(csr.nnz, csr.n_rows, C, True, True, False),
              lambda: _launch(fn, _ptr(h), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(csr.rowptr),
                              _ptr(csr.col), csr.n_rows, C, int(mean), float(eps), *dargs, _ptr(out), _stream(h.device)))
        ctx.save_for_backward(h, bias, gamma)
        ctx.meta = (eps, csr_t, p, seed)
        ctx.acc = acc_params
        ctx.ew = entry_weights(csr_t, csr) if mean else None    # once per batch (cached on the CSR)
        return out

    @staticmethod
    def backward(ctx, dout):
        h, bias, gamma = ctx.saved_tensors
        eps, t, p, seed = ctx.meta
        dout = _f32c(dout)
        R, C = h.shape
        dh = torch.empty_like(h)
        L = hip.lib()
        fn, dargs = ("hg_gather_ln_reduce_drop_bwd", (p, _ptr(seed))) if p > 0.0 else ("hg_gather_ln_reduce_bwd", ())
        ws_bytes = (L.hg_gather_ln_reduce_drop_bwd_workspace_bytes if p > 0.0 else L.hg_gather_ln_reduce_bwd_workspace_bytes)(R, C)
        ws = _workspace(ws_bytes, h.device)
        tg, acc, small, o = _param_grads(ctx.acc, 3, C, h.device)
        timed("k_gather_ln_drop_bwd" if p > 0.0 else "k_gather_ln_bwd",
              segment_reduce_bytes(t.nnz, R, C, True, True, False) + 4 * t.nnz + 4 * C * R,
              lambda: _launch(fn, _ptr(h), _ptr(bias), _ptr(gamma), _ptr(dout), _ptr(t.rowptr),
                              _ptr(t.col), _ptr(ctx.ew), R, C, float(eps), *dargs, _ptr(dh), _ptr(o[0]), _ptr(o[1]),
                              _ptr(o[2]), 1 if acc else 0, _ptr(ws), ws_bytes, _stream(h.device)))
        return (dh, *((None,) * 3 if acc else _hand_out(list(small), tg))) + (None,) * 7


def gather_ln_reduce(h, bias, gamma, beta, csr: CSR, csr_t: CSR, reduce: str = "mean", eps: float = 1e-5, p: float = 0.0,
                     seed=None):
    """reduce_gathered(bias_relu_ln(h, bias, gamma, beta), csr, csr_t, reduce) in one launch each way (2-D h).  ``p``,
    ``seed``: dropout of the hidden rows (decided per source row, before the gather), see bias_relu_ln."""
    p, _ = _drop_route(p, "gather_ln_reduce")
    if p >= 1.0:
        return _Zeros.apply((csr.n_rows, h.shape[1]), h, bias, gamma, beta)
    _note_acc(bias, gamma, beta)
    return _GatherLnReduce.apply(h, bias, gamma, beta, csr, csr_t, reduce == "mean", eps, (bias, gamma, beta), p, seed)


class _BatchNormRows(torch.autograd.Function):
    """Training-mode BatchNorm1d over rows with the batch statistics taken over the masked (real) rows only and the running
    buffers updated in the same launch (hg_batch_norm_rows_*; csrc/bn_rows.hip)."""

    @staticmethod
    def forward(ctx, x, mask, gamma, beta, running_mean, running_var, n_tracked, momentum, eps, acc_params, relu=False):
        _require_gpu(x, "batch_norm_rows")
        x, gamma, beta = _f32c(x), _f32c(gamma), _f32c(beta)
        R, C = x.shape
        m = _f32c(mask).reshape(-1) if mask is not None else None
        y = torch.empty_like(x)
        stats = torch.empty((2, C), dtype=torch.float32, device=x.device)
        L = hip.lib()
        ws_bytes = L.hg_batch_norm_rows_workspace_bytes(R, C)
        ws = _workspace(max(ws_bytes, 16), x.device)
        hip.check(L.hg_batch_norm_rows_fwd(_ptr(x), _ptr(m), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                           _ptr(n_tracked), float(momentum), float(eps), R, C, _ptr(y), _ptr(stats[0]),
                                           _ptr(stats[1]), 1 if relu else 0, _ptr(ws), ws_bytes, _stream(x.device)),
                  "hg_batch_norm_rows_fwd")
        ctx.save_for_backward(x, m, gamma, stats, beta)
        ctx.acc, ctx.relu = acc_params, bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, m, gamma, stats, beta = ctx.saved_tensors
        R, C = x.shape
        dy = _f32c(dy)
        dx = torch.empty_like(x)
        small = torch.empty((2, C), dtype=torch.float32, device=x.device)
        L = hip.lib()
        ws_bytes = L.hg_batch_norm_rows_workspace_bytes(R, C)
        ws = _workspace(max(ws_bytes, 16), x.device)
        hip.check(L.hg_batch_norm_rows_bwd(_ptr(x), _ptr(dy), _ptr(m), _ptr(gamma), _ptr(stats[0]), _ptr(stats[1]), R, C,
                                           _ptr(dx), _ptr(small[0]), _ptr(small[1]), _ptr(beta), 1 if ctx.relu else 0, _ptr(ws),
                                           ws_bytes, _stream(x.device)), "hg_batch_norm_rows_bwd")
        dgam, dbet = _hand_out(list(small), [_acc_target(p) for p in ctx.acc])
        return dx, None, dgam, dbet, None, None, None, None, None, None, None


def batch_norm_rows(x, mask, bn, relu: bool = False):
    """Training-mode ``bn`` (nn.BatchNorm1d with running statistics) on 2-D fp32 rows ``x`` with the statistics over the rows
    where ``mask`` [R, 1] is > 0 (None: all rows); running_mean / running_var / num_batches_tracked are updated in place.
    ``relu``: relu(bn(x)) in the same launches."""
    _note_acc(bn.weight, bn.bias)
    return _BatchNormRows.apply(x, mask, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                bn.momentum, bn.eps, (bn.weight, bn.bias), bool(relu))


def batch_norm_rows_supported(x, bn) -> bool:
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[-1] % 4 == 0 and bn.training and bn.affine
            and bn.track_running_stats and bn.momentum is not None and x.shape[0] > 1)


class _LayerNormRows(torch.autograd.Function):
    """Plain LayerNorm over dense rows; one launch each way, dgamma/dbeta from the backward pass.  With ``passthrough`` the
    node also returns x itself for x's OTHER consumer (a residual), whose gradient the backward kernel adds to dx in the
    same pass instead of an autograd add over the [rows, C] tensor."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, acc_params, passthrough=False):
        _require_gpu(x, "layer_norm_rows")
        xin = x
        x, gamma, beta = _f32c(x), _f32c(gamma), _f32c(beta)
        R, C = x.shape
        out = torch.empty_like(x)
        hip.check(hip.lib().hg_layer_norm_fwd(_ptr(x), _ptr(gamma), _ptr(beta), R, C, float(eps), _ptr(out),
                                              _stream(x.device)), "hg_layer_norm_fwd")
        ctx.save_for_backward(x, gamma)
        ctx.eps = eps
        ctx.acc = acc_params
        if passthrough:
            ctx.set_materialize_grads(False)
            return out, xin.view_as(xin)
        return out

    @staticmethod
    def backward(ctx, dy, dpass=None):
        x, gamma = ctx.saved_tensors
        if dy is None:
            return dpass, None, None, None, None, None
        R, C = x.shape
        dy, ld = _rows_ld(dy.reshape(R, C))          # (a column block of a wider gradient -- the backward of a cat -- is read in place)
        add = _f32c(dpass).reshape(R, C) if dpass is not None else None
        dx = torch.empty_like(x)
        L = hip.lib()
        ws_bytes = L.hg_layer_norm_bwd_workspace_bytes(R, C)
        ws = _workspace(ws_bytes, x.device)
        tg = [_acc_target(p) for p in ctx.acc]
        if all(t is not None for t in tg):
            hip.check(L.hg_layer_norm_bwd(_ptr(x), _ptr(gamma), _ptr(dy), ld, _ptr(add), R, C, float(ctx.eps), _ptr(dx), _ptr(tg[0]),
                                          _ptr(tg[1]), 1, _ptr(ws), ws_bytes, _stream(x.device)), "hg_layer_norm_bwd")
            return dx, None, None, None, None, None
        small = torch.empty((2, C), dtype=torch.float32, device=x.device)
        hip.check(L.hg_layer_norm_bwd(_ptr(x), _ptr(gamma), _ptr(dy), ld, _ptr(add), R, C, float(ctx.eps), _ptr(dx), _ptr(small[0]),
                                      _ptr(small[1]), 0, _ptr(ws), ws_bytes, _stream(x.device)), "hg_layer_norm_bwd")
        return (dx, *_hand_out(list(small), tg), None, None, None)


# --------------------------------------------------------------------------------------------
# public functional API
# --------------------------------------------------------------------------------------------
def incidence_ln_reduce(pa, qb, gamma, beta, ia32, ib32, csr_a: CSR, csr_b: CSR, out_csr: CSR, okey32,
                        reduce: str = "mean", eps: float = 1e-5, p: float = 0.0, seed=None):
    """reduce_{p in out row} LayerNorm(relu(pa[ia[p]] + qb[ib[p]])); csr_a / csr_b are the incidence
    CSRs keyed by ia / ib (needed by the backward), out_csr the one keyed by okey32.  ``p``, ``seed``: dropout of the
    per-incidence hidden rows, decided per incidence (its position in ia32 / ib32), see bias_relu_ln."""
    p, _ = _drop_route(p, "incidence_ln_reduce")
    if p >= 1.0:
        return _Zeros.apply((out_csr.n_rows, pa.shape[1]), pa, qb, gamma, beta)
    _note_acc(gamma, beta)
    return _IncidenceLnReduce.apply(pa, qb, gamma, beta, ia32, ib32, csr_a, csr_b, out_csr, okey32,
                                    reduce == "mean", eps, (gamma, beta), p, seed)


def bias_relu_ln(h, bias, gamma, beta, eps: float = 1e-5, fan=None, p: float = 0.0, seed=None):
    """LayerNorm(relu(h + bias)) for 2-D ``h`` [rows, C].  ``fan``: see linear_add / GradFan (h = linear_add(..., c, fan=fan)).
    ``p`` > 0: dropout_p of the result in the same launch (mlp.py:97), keep = 0 or 1 / (1 - p) from the hash of (seed,
    element index) -- ``seed``: an int64 tensor of one element on the device, or None for a draw from the pool of
    ops.dropout_seeds.  p = 0 is the call without the argument; p >= 1 gives zeros."""
    p, _ = _drop_route(p, "bias_relu_ln")
    if p >= 1.0:
        return _Zeros.apply(tuple(h.shape), h, bias, gamma, beta)
    _note_acc(bias, gamma, beta)
    return _BiasReluLn.apply(h, bias, gamma, beta, eps, (bias, gamma, beta), fan, p, seed)


class _ResidualMix(torch.autograd.Function):
    """c = a * X0 + (1 - a) * w_r * bias (hg_residual_mix_f32); backward: dX0 = a * dc and the bias gradient
    as a scaled, row-weighted column sum (batched with the other bias gradients of the step)."""

    @staticmethod
    def forward(ctx, x0, bias, rowptr, weight_mode, alpha, bias_param, passthrough=False):
        _require_gpu(x0, "residual_mix")
        x0, bias = _f32c(x0), _f32c(bias)
        R, C = x0.shape
        out = torch.empty_like(x0)
        hip.check(hip.lib().hg_residual_mix_f32(_ptr(x0), _ptr(bias), _ptr(rowptr), weight_mode, float(alpha), R, C,
                                                _ptr(out), _stream(x0.device)), "hg_residual_mix_f32")
        ctx.rowptr, ctx.mode, ctx.alpha, ctx.bias_param = rowptr, weight_mode, float(alpha), bias_param
        ctx.set_materialize_grads(False)
        if passthrough:     # x0 again, for its OTHER consumer: both gradients then meet here, in one kernel
            return out, x0.view_as(x0)
        return out

    @staticmethod
    def backward(ctx, dc, dpass=None):
        dx0 = db = None
        if dc is not None:
            dc = _f32c(dc)
            if ctx.needs_input_grad[0]:
                dx0 = dc * ctx.alpha if dpass is None else torch.add(dpass, dc, alpha=ctx.alpha)
            if ctx.needs_input_grad[1]:
                db = colsum(dc, ctx.rowptr, ctx.mode, into=_acc_target(ctx.bias_param), scale=1.0 - ctx.alpha)
        elif dpass is not None and ctx.needs_input_grad[0]:
            dx0 = dpass
        return dx0, db, None, None, None, None, None


def residual_mix(x0, bias, rowptr, weight_mode: int, alpha: float, passthrough: bool = False):
    """alpha * x0 + (1 - alpha) * w_r * bias for 2-D x0 [rows, C] (C % 4 == 0); w_r from the int32 CSR ``rowptr``
    (weight_mode 1: [row non-empty], 2: row length).  ``passthrough``: also return x0 itself as a second output of the
    same autograd node -- hand THAT to x0's other consumer and the two gradients of x0 are combined by one kernel here
    instead of a multiply plus autograd's add."""
    _note_acc(bias)
    return _ResidualMix.apply(x0, bias, rowptr, weight_mode, alpha, bias, passthrough)


def layer_norm_rows(x, gamma, beta, eps: float = 1e-5, passthrough: bool = False):
    """nn.LayerNorm over the last dim of 2-D ``x`` [rows, C] (C % 4 == 0, C <= 1024).  ``passthrough``: returns
    (LayerNorm(x), x) -- see _LayerNormRows."""
    _note_acc(gamma, beta)
    return _LayerNormRows.apply(x, gamma, beta, eps, (gamma, beta), passthrough)
