"""SE(3)-Transformer operators: edge basis, the re-associated radial contraction of a PairwiseConv, the 17-slot attention and
NormSE3 (se3_transformer_layer.py; csrc/se3t.hip).  Features are component-major: [*, m, C].

Part of equihgnn_amd.ops (host-side operators over libequihgnn_hip.so; no CPU fallback).
"""
from __future__ import annotations

import torch

from .. import hip
from ._base import _c_void_p, _f32c, _ptr, _require_gpu, _stream, _workspace, timed

SE3T_MID = 128                                       # width of the radial trunk
SE3T_NB = 34                                         # basis floats per edge
# (di, do) -> (offset of the pair's [MO, Q] block in an edge's basis row, MO, Q = mi * F)
SE3T_PAIRS = {(0, 0): (0, 1, 1), (0, 1): (1, 3, 1), (1, 0): (4, 1, 3), (1, 1): (7, 3, 9)}


def se3t_edge_basis(pos, nbr, radius: float, qtab):
    """(dist [E], maskf [N,K], meanw [N,K], basis [E,34]) of the self-excluded neighbour table ``nbr`` [N,K] int32
    (se3t_edge_basis); ``qtab`` [100]: the Q_J matrices, equihgnn_amd.se3_transformer.q_table().  No gradient."""
    _require_gpu(pos, "se3t_edge_basis")
    pos, qtab = _f32c(pos.detach()), _f32c(qtab)
    N, K = nbr.shape
    if nbr.dtype != torch.int32 or pos.shape != (N, 3) or not 1 <= K <= 16 or qtab.numel() != 100:
        raise ValueError("se3t_edge_basis: pos[N,3] fp32, nbr[N,K] int32 (1 <= K <= 16), qtab[100] expected")
    dev = pos.device
    dist = torch.empty(N * K, dtype=torch.float32, device=dev)
    maskf = torch.empty((N, K), dtype=torch.float32, device=dev)
    meanw = torch.empty((N, K), dtype=torch.float32, device=dev)
    basis = torch.empty((N * K, SE3T_NB), dtype=torch.float32, device=dev)
    hip.check(hip.lib().se3t_edge_basis(_ptr(pos), _ptr(nbr.contiguous()), N, K, float(radius), _ptr(qtab), _ptr(dist),
                                        _ptr(maskf), _ptr(meanw), _ptr(basis), _stream(dev)), "se3t_edge_basis")
    return dist, maskf, meanw, basis


class _Se3tPair(torch.autograd.Function):
    """out_e[mo, o] = sum_q B_e[mo, q] (h_e . G_j[q, :, o] + GB_j[q, o]), j the sender of edge e; with ``meanw`` the masked
    mean over each receiver's K slots (se3t_pair_fwd / _bwd).  The basis carries no gradient."""

    @staticmethod
    def forward(ctx, h, G, GB, basis, pair, O, rowptr, perm, meanw):
        _require_gpu(h, "se3t_pair")
        h, G, GB, basis = _f32c(h), _f32c(G), _f32c(GB), _f32c(basis)
        off, MO, Q = SE3T_PAIRS[pair]
        E = h.shape[0]
        N = rowptr.numel() - 1
        if (h.shape != (E, SE3T_MID) or G.numel() != N * Q * SE3T_MID * O or GB.numel() != N * Q * O
                or basis.shape != (E, SE3T_NB) or perm.numel() != E or O % 16):
            raise ValueError("se3t_pair: h[E,128], G[N,Q,128,O], GB[N,Q,O], basis[E,34], perm[E], O % 16 == 0 expected")
        pooled = meanw is not None
        K = E // N
        if pooled:
            meanw = _f32c(meanw)
            if meanw.numel() != E or K * N != E:
                raise ValueError("se3t_pair: meanw[N,K] with E = N K expected")
        dev = h.device
        out = torch.empty((N if pooled else E, MO, O), dtype=torch.float32, device=dev)
        L = hip.lib()
        ws_bytes = L.se3t_pair_fwd_workspace_bytes(E, MO, O, 1 if pooled else 0)
        ws = _workspace(max(ws_bytes, 16), dev)
        coef = _c_void_p(basis.data_ptr() + 4 * off)
        timed("k_se3t_pair_fwd", 2 * E * MO * Q * SE3T_MID * O,
              lambda: hip.check(L.se3t_pair_fwd(_ptr(h), _ptr(G), _ptr(GB), coef, SE3T_NB, _ptr(rowptr), _ptr(perm), N, E, MO, Q,
                                                O, _ptr(meanw), max(K, 1), _ptr(out), 0, _ptr(ws), ws_bytes, _stream(dev)),
                                "se3t_pair_fwd"))
        ctx.save_for_backward(h, G, basis, meanw)
        ctx.meta = (off, MO, Q, O, N, E, K, rowptr, perm, GB.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        h, G, basis, meanw = ctx.saved_tensors
        off, MO, Q, O, N, E, K, rowptr, perm, gb_shape = ctx.meta
        dout = _f32c(dout)
        dev = h.device
        dh = torch.empty_like(h)
        dG = torch.empty_like(G)
        dGB = torch.empty(gb_shape, dtype=torch.float32, device=dev)
        coef = _c_void_p(basis.data_ptr() + 4 * off)
        timed("k_se3t_pair_bwd", 4 * E * MO * Q * SE3T_MID * O,
              lambda: hip.check(hip.lib().se3t_pair_bwd(_ptr(h), _ptr(G), coef, SE3T_NB, _ptr(rowptr), _ptr(perm), N, E, MO, Q, O,
                                                        _ptr(dout), _ptr(meanw), max(K, 1), _ptr(dh), _ptr(dG), _ptr(dGB),
                                                        _stream(dev)), "se3t_pair_bwd"))
        return dh, dG, dGB, None, None, None, None, None, None


def se3t_pair(h, G, GB, basis, pair, O: int, rowptr, perm, meanw=None):
    """One PairwiseConv (se3_transformer_layer.py:339-374 with :283-288) without the per-edge radial weights.
    h [E,128]: the radial trunk; G [N, Q*128*O] / GB [N, Q*O]: the sender's node-level products with the last Linear's weight
    and bias (columns (q, c, o), q = mi * F + f); basis [E,34] of se3t_edge_basis; pair = (di, do); rowptr / perm: the
    transposed neighbour CSR.  -> [E, MO, O], or [N, MO, O] (masked mean over the slots) with ``meanw`` [N,K]."""
    return _Se3tPair.apply(h, G, GB, basis, pair, O, rowptr, perm, meanw)


class _Se3tAttn(torch.autograd.Function):
    """One degree of AttentionSE3 (2 heads x 32, self slot + K neighbour slots): se3t_attn_fwd / _bwd."""

    @staticmethod
    def forward(ctx, q, kself, kedge, vself, vedge, maskf, scale):
        _require_gpu(q, "se3t_attn")
        q, kself, kedge, vself, vedge, maskf = (_f32c(t) for t in (q, kself, kedge, vself, vedge, maskf))
        N, M, D = q.shape
        K = maskf.shape[1]
        if (D != 64 or M not in (1, 3) or maskf.shape[0] != N or not 1 <= K <= 16 or kself.shape != q.shape
                or vself.shape != q.shape or kedge.shape != (N * K, M, 64) or vedge.shape != (N * K, M, 64)):
            raise ValueError("se3t_attn: q/kself/vself [N,M,64], kedge/vedge [N*K,M,64], maskf [N,K] expected")
        out = torch.empty_like(q)
        logits = torch.empty((N, 2, K + 1), dtype=torch.float32, device=q.device)
        hip.check(hip.lib().se3t_attn_fwd(_ptr(q), _ptr(kself), _ptr(kedge), _ptr(vself), _ptr(vedge), _ptr(maskf), N, K, M,
                                          float(scale), _ptr(out), _ptr(logits), _stream(q.device)), "se3t_attn_fwd")
        ctx.save_for_backward(q, kself, kedge, vself, vedge, logits)
        ctx.meta = (N, K, M, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kself, kedge, vself, vedge, logits = ctx.saved_tensors
        N, K, M, scale = ctx.meta
        dout = _f32c(dout)
        dq, dks, dke, dvs, dve = (torch.empty_like(t) for t in (q, kself, kedge, vself, vedge))
        hip.check(hip.lib().se3t_attn_bwd(_ptr(q), _ptr(kself), _ptr(kedge), _ptr(vself), _ptr(vedge), _ptr(logits), _ptr(dout),
                                          N, K, M, scale, _ptr(dq), _ptr(dks), _ptr(dke), _ptr(dvs), _ptr(dve),
                                          _stream(q.device)), "se3t_attn_bwd")
        return dq, dks, dke, dvs, dve, None, None


def se3t_attn(q, kself, kedge, vself, vedge, maskf, scale: float):
    """softmax over (self + K) slots of scale * <q, k_s> per head (2 x 32 channels, all m), masked slots filled with
    -finfo.max, times the values (se3_transformer_layer.py:594-603) for one degree: [N, M, 64]."""
    return _Se3tAttn.apply(q, kself, kedge, vself, vedge, maskf, scale)


class _Se3tNorm(torch.autograd.Function):
    """NormSE3 on [R, M, C] rows (se3t_norm_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, scale, eps):
        _require_gpu(x, "se3t_norm")
        x = _f32c(x)
        sv = _f32c(scale.detach()).reshape(-1)
        R, M, C = x.shape
        if M not in (1, 3) or sv.numel() != C:
            raise ValueError("se3t_norm: x[R,M,C] with M in (1, 3) and scale of C entries expected")
        out = torch.empty_like(x)
        hip.check(hip.lib().se3t_norm_fwd(_ptr(x), _ptr(sv), R, M, C, float(eps), _ptr(out), _stream(x.device)), "se3t_norm_fwd")
        ctx.save_for_backward(x, sv)
        ctx.meta = (float(eps), scale.shape)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, sv = ctx.saved_tensors
        eps, sshape = ctx.meta
        dy = _f32c(dy)
        R, M, C = x.shape
        dx = torch.empty_like(x)
        ds = torch.empty(C, dtype=torch.float32, device=x.device)
        L = hip.lib()
        ws_bytes = L.se3t_norm_bwd_workspace_bytes(R, C)
        ws = _workspace(max(ws_bytes, 16), x.device)
        hip.check(L.se3t_norm_bwd(_ptr(x), _ptr(sv), _ptr(dy), R, M, C, eps, _ptr(dx), _ptr(ds), _ptr(ws), ws_bytes,
                                  _stream(x.device)), "se3t_norm_bwd")
        return dx, ds.view(sshape), None


def se3t_norm(x, scale, eps: float = 1e-12):
    """NormSE3 (se3_transformer_layer.py:162-184): GELU(|x| scale) x / |x| with |x| over m clamped at eps; x [R, M, C],
    ``scale`` the ``transform.<degree>.scale`` parameter [1, 1, C]."""
    return _Se3tNorm.apply(x, scale, eps)
