"""ViSNet front-end (visnet_layer.py) over the vis_* kernels: the per-molecule radius graph with its per-slot geometry, and
the four edge operators of NeighborEmbedding, EdgeEmbedding and ViS_MP, each an autograd node whose forward and backward
are kernel launches on a static [N, 16] slot table (see include/equihgnn_hip.h).

Part of equihgnn_amd.ops (host-side operators over libequihgnn_hip.so; no CPU fallback).
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import hip
from ._base import _f32c, _ptr, _require_gpu, _stream, timed

K = 16        # max_num_neighbors
NRBF = 32
NSH = 8       # lmax 2
HEADS = 8


class RadiusGraph:
    """Slot table and per-slot geometry of one batch (vis_radius_graph).  Edge e = 16 i + s; ``slot`` [N, 16] int32 (-1:
    empty), ``cnt`` [N]; per slot ``r``, ``cut`` [16 N], ``rbf`` [16 N, 32], ``sh`` [16 N, 8]; by source ``src_start``,
    ``src_cnt`` [N], ``src_eid`` [16 N].  Every tensor is int32 or fp32 (HyperIndex.live_clone copies them as words)."""

    def __init__(self, **t):
        self.__dict__.update(t)

    @property
    def N(self) -> int:
        return int(self.cnt.shape[0])

    def edge_index(self):
        """(edge_index [2, E] int64 with edge_index[0] = source, [1] = target, edge ids): the kept slots in the order of
        torch_cluster's radius_graph (by target, then source).  Synchronises: for tests and tools only."""
        slot = self.slot.reshape(-1).long()
        keep = torch.nonzero(slot >= 0).reshape(-1)
        return torch.stack((slot[keep], keep // K)), keep


def radius_graph(pos, batch32, pool_rowptr, n_real: Optional[torch.Tensor], means, betas, cutoff: float) -> RadiusGraph:
    """The radius graph of visnet_layer.py's Distance (r = cutoff, loop = True, max_num_neighbors = 16) over the molecules
    of ``pool_rowptr`` (int32 [B + 1]; ``batch32`` int32 [N] sorted), with the geometry of ExpNormalSmearing(means, betas)
    and Sphere(lmax = 2).  ``n_real``: int32 device [1], the number of real atoms of a padded batch (the rest keep only
    their self-loop), or None."""
    _require_gpu(pos, "vis_radius_graph")
    pos = _f32c(pos.detach())
    N = int(pos.shape[0])
    dev = pos.device
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    E = K * N
    g = RadiusGraph(slot=torch.empty((N, K), **i32), cnt=torch.empty(N, **i32), r=torch.empty(E, **f32),
                    cut=torch.empty(E, **f32), rbf=torch.empty((E, NRBF), **f32), sh=torch.empty((E, NSH), **f32),
                    src_start=torch.empty(N, **i32), src_cnt=torch.empty(N, **i32), src_eid=torch.empty(E, **i32))
    means, betas = _f32c(means.detach()), _f32c(betas.detach())
    if means.numel() != NRBF or betas.numel() != NRBF:
        raise ValueError(f"vis_radius_graph: {NRBF} RBFs expected, got {means.numel()} / {betas.numel()}")
    timed("k_vis_radius", 16 * N + 4 * N * K * (1 + 2 + NRBF + NSH + 1) + 12 * N,
          lambda: hip.check(hip.lib().vis_radius_graph(
              _ptr(pos), _ptr(batch32), _ptr(pool_rowptr), _ptr(n_real), _ptr(means), _ptr(betas), N, float(cutoff),
              _ptr(g.slot), _ptr(g.cnt), _ptr(g.r), _ptr(g.cut), _ptr(g.rbf), _ptr(g.sh), _ptr(g.src_start),
              _ptr(g.src_cnt), _ptr(g.src_eid), _stream(dev)), "vis_radius_graph"))
    return g


def _graph(g: RadiusGraph):
    return _ptr(g.slot), _ptr(g.cnt)


def _src(g: RadiusGraph):
    return _ptr(g.src_start), _ptr(g.src_cnt), _ptr(g.src_eid)


def check_channels(C: int):
    if C % HEADS:
        raise ValueError(f"The number of hidden channels (got {C}) must be evenly divisible by the number of attention "
                         f"heads (got {HEADS})")
    if C > 512:
        raise ValueError(f"ViSNet kernels support at most 512 hidden channels (got {C})")


def edge_bytes(N: int, C: int, node_rows: int, edge_rows: int) -> int:
    """Algorithmic bytes of one launch pair: ``node_rows`` [N, C] streams (gathered rows counted once per edge slot as the
    gathers they are: 16 per target row) and ``edge_rows`` [16 N, C] streams, plus the slot table."""
    return 4 * C * (N * node_rows + K * N * edge_rows) + 8 * K * N


class _NbrEmbed(torch.autograd.Function):
    """NeighborEmbedding.propagate: y_i = sum_{j != i} x_j (W_e cut_e), W = distance_proj(rbf) [16 N, C]."""

    @staticmethod
    def forward(ctx, x, W, g: RadiusGraph):
        x, W = _f32c(x), _f32c(W)
        N, C = x.shape
        y = torch.empty_like(x)
        timed("k_vis_nbr_fwd", edge_bytes(N, C, 1 + K, 1),
              lambda: hip.check(hip.lib().vis_nbr_fwd(_ptr(x), _ptr(W), _ptr(g.cut), *_graph(g), N, C, _ptr(y),
                                                      _stream(x.device)), "vis_nbr_fwd"))
        ctx.save_for_backward(x, W)
        ctx.g = g
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        g = ctx.g
        dy = _f32c(dy)
        N, C = x.shape
        dx, dW = torch.empty_like(x), torch.empty_like(W)
        timed("k_vis_nbr_bwd", edge_bytes(N, C, 2 + 2 * K, 2),
              lambda: hip.check(hip.lib().vis_nbr_bwd(_ptr(x), _ptr(W), _ptr(g.cut), *_graph(g), *_src(g), _ptr(dy), N, C,
                                                      _ptr(dx), _ptr(dW), _stream(x.device)), "vis_nbr_bwd"))
        return dx, dW, None


class _EdgeEmbed(torch.autograd.Function):
    """EdgeEmbedding: f_e = (x_i + x_j) W_e, W = edge_proj(rbf) [16 N, C]; empty slots 0."""

    @staticmethod
    def forward(ctx, x, W, g: RadiusGraph):
        x, W = _f32c(x), _f32c(W)
        N, C = x.shape
        f = torch.empty_like(W)
        timed("k_vis_edge_embed_fwd", edge_bytes(N, C, 2 * K, 2),
              lambda: hip.check(hip.lib().vis_edge_embed_fwd(_ptr(x), _ptr(W), *_graph(g), N, C, _ptr(f),
                                                             _stream(x.device)), "vis_edge_embed_fwd"))
        ctx.save_for_backward(x, W)
        ctx.g = g
        return f

    @staticmethod
    def backward(ctx, df):
        x, W = ctx.saved_tensors
        g = ctx.g
        df = _f32c(df)
        N, C = x.shape
        dx, dW = torch.empty_like(x), torch.empty_like(W)
        timed("k_vis_edge_embed_bwd", edge_bytes(N, C, 2 * K + 1, 5),
              lambda: hip.check(hip.lib().vis_edge_embed_bwd(_ptr(x), _ptr(W), *_graph(g), *_src(g), _ptr(df), N, C,
                                                             _ptr(dx), _ptr(dW), _stream(x.device)), "vis_edge_embed_bwd"))
        return dx, dW, None


class _Attn(torch.autograd.Function):
    """ViS_MP.message's scalar half and the sum of aggregate: (u [16 N, C], xagg [N, C]) from q, k, v [N, C] and the raw
    dk_proj / dv_proj outputs dkr, dvr [16 N, C] (silu applied in the kernel)."""

    @staticmethod
    def forward(ctx, q, k, v, dkr, dvr, g: RadiusGraph):
        q, k, v, dkr, dvr = (_f32c(t) for t in (q, k, v, dkr, dvr))
        N, C = q.shape
        u = torch.empty_like(dkr)
        xagg = torch.empty_like(q)
        pre = torch.empty((K * N, HEADS), dtype=torch.float32, device=q.device)
        timed("k_vis_attn_fwd", edge_bytes(N, C, 1 + 2 * K, 3),
              lambda: hip.check(hip.lib().vis_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(dkr), _ptr(dvr), _ptr(g.cut),
                                                       *_graph(g), N, C, _ptr(u), _ptr(xagg), _ptr(pre),
                                                       _stream(q.device)), "vis_attn_fwd"))
        ctx.save_for_backward(q, k, v, dkr, dvr, pre)
        ctx.g = g
        return u, xagg

    @staticmethod
    def backward(ctx, du, dxagg):
        q, k, v, dkr, dvr, pre = ctx.saved_tensors
        g = ctx.g
        N, C = q.shape
        du = torch.zeros_like(dkr) if du is None else _f32c(du)
        dxagg = torch.zeros_like(q) if dxagg is None else _f32c(dxagg)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        ddkr, ddvr, dpre = torch.empty_like(dkr), torch.empty_like(dkr), torch.empty_like(pre)
        timed("k_vis_attn_bwd", edge_bytes(N, C, 3 + 6 * K, 9),
              lambda: hip.check(hip.lib().vis_attn_bwd(
                  _ptr(q), _ptr(k), _ptr(v), _ptr(dkr), _ptr(dvr), _ptr(g.cut), _ptr(pre), *_graph(g), *_src(g), _ptr(du),
                  _ptr(dxagg), N, C, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ddkr), _ptr(ddvr), _ptr(dpre),
                  _stream(q.device)), "vis_attn_bwd"))
        return dq, dk, dv, ddkr, ddvr, None


class _VecMsg(torch.autograd.Function):
    """ViS_MP.message's vector half and its sum: vo_i = sum_e vec_j silu(sr_e[:C]) + silu(sr_e[C:]) (x) sh_e, vec / vo
    [N, 8, C], sr = s_proj(u) raw [16 N, 2 C].  The [16 N, 8, C] message is never formed."""

    @staticmethod
    def forward(ctx, vec, sr, g: RadiusGraph):
        vec, sr = _f32c(vec), _f32c(sr)
        N, _, C = vec.shape
        vo = torch.empty_like(vec)
        timed("k_vis_vec_fwd", edge_bytes(N, C, NSH + NSH * K, 2),
              lambda: hip.check(hip.lib().vis_vec_fwd(_ptr(vec), _ptr(sr), _ptr(g.sh), *_graph(g), N, C, _ptr(vo),
                                                      _stream(vec.device)), "vis_vec_fwd"))
        ctx.save_for_backward(vec, sr)
        ctx.g = g
        return vo

    @staticmethod
    def backward(ctx, dvo):
        vec, sr = ctx.saved_tensors
        g = ctx.g
        dvo = _f32c(dvo)
        N, _, C = vec.shape
        dvec, dsr = torch.empty_like(vec), torch.empty_like(sr)
        timed("k_vis_vec_bwd", edge_bytes(N, C, 2 * NSH + 2 * NSH * K, 5),
              lambda: hip.check(hip.lib().vis_vec_bwd(_ptr(vec), _ptr(sr), _ptr(g.sh), *_graph(g), *_src(g), _ptr(dvo),
                                                      N, C, _ptr(dvec), _ptr(dsr), _stream(vec.device)), "vis_vec_bwd"))
        return dvec, dsr, None


class _EdgeUpdate(torch.autograd.Function):
    """ViS_MP.edge_update: df_e = silu(fr_e) sum_m rej(wt_i, d_e)_m rej(ws_j, -d_e)_m, wt = w_trg_proj(vec), ws =
    w_src_proj(vec) [N, 8, C], fr = f_proj(f) raw [16 N, C]; neither gathered [16 N, 8, C] operand is formed."""

    @staticmethod
    def forward(ctx, wt, ws, fr, g: RadiusGraph):
        wt, ws, fr = _f32c(wt), _f32c(ws), _f32c(fr)
        N, _, C = wt.shape
        df = torch.empty_like(fr)
        timed("k_vis_edge_update_fwd", edge_bytes(N, C, 2 * NSH * K, 2),
              lambda: hip.check(hip.lib().vis_edge_update_fwd(_ptr(wt), _ptr(ws), _ptr(fr), _ptr(g.sh), *_graph(g), N, C,
                                                              _ptr(df), _stream(wt.device)), "vis_edge_update_fwd"))
        ctx.save_for_backward(wt, ws, fr)
        ctx.g = g
        return df

    @staticmethod
    def backward(ctx, ddf):
        wt, ws, fr = ctx.saved_tensors
        g = ctx.g
        ddf = _f32c(ddf)
        N, _, C = wt.shape
        dwt, dws, dfr = torch.empty_like(wt), torch.empty_like(ws), torch.empty_like(fr)
        timed("k_vis_edge_update_bwd", edge_bytes(N, C, 4 * NSH * K + 2 * NSH, 5),
              lambda: hip.check(hip.lib().vis_edge_update_bwd(
                  _ptr(wt), _ptr(ws), _ptr(fr), _ptr(g.sh), *_graph(g), *_src(g), _ptr(ddf), N, C, _ptr(dwt), _ptr(dws),
                  _ptr(dfr), _stream(wt.device)), "vis_edge_update_bwd"))
        return dwt, dws, dfr, None


def vis_neighbor_sum(x, W, g: RadiusGraph):
    return _NbrEmbed.apply(x, W, g)


def vis_edge_embed(x, W, g: RadiusGraph):
    return _EdgeEmbed.apply(x, W, g)


def vis_attn(q, k, v, dkr, dvr, g: RadiusGraph):
    return _Attn.apply(q, k, v, dkr, dvr, g)


def vis_vec_msg(vec, sr, g: RadiusGraph):
    return _VecMsg.apply(vec, sr, g)


def vis_edge_update(wt, ws, fr, g: RadiusGraph):
    return _EdgeUpdate.apply(wt, ws, fr, g)
