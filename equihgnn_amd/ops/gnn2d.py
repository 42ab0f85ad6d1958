"""Edge messages of the 2-D baselines (GINConv / GCNConv of baseline_2d.py:19-73) over hg_edge_msg_fwd/bwd, and the
per-batch graph index they read.

Part of equihgnn_amd.ops (host-side operators over libequihgnn_hip.so; no CPU fallback).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import hip
from ._base import ACC_PARAMS, _acc_target, _contiguous_run, _f32c, _ptr, _require_gpu, _stacked_view, _stream, _workspace, timed
from .aggregate import CSR, csr_build_batch, reduce_entries

# ogb BondEncoder (ogb 1.3.6 get_bond_feature_dims): bond type, stereo, is-conjugated
BOND_FEATURE_DIMS = (5, 6, 2)
GIN, GCN = 0, 1


def bond_offsets(F: int):
    """Row offsets of the first F bond tables stacked, and their total row count."""
    offs, run = [], 0
    for d in BOND_FEATURE_DIMS[:F]:
        offs.append(run)
        run += d
    return tuple(offs), run


class GraphIndex:
    """The 2-D counterpart of HyperIndex, built once per batch and shared by every layer and by the backward pass:
    ``by_dst`` (incoming edges of each atom: col = source atom), ``by_src`` (outgoing edges: col = target atom; its
    rowptr gives GCN's degrees), ``pool`` (atoms of each molecule) and the int32 per-entry bond codes of both edge CSRs
    (hg_edge_codes).  PyG flow source_to_target: edge_index[0] is the source, edge_index[1] the target."""

    def __init__(self, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor], batch: torch.Tensor, N: int, B: int):
        _require_gpu(edge_index, "GraphIndex")
        self.N, self.B = int(N), int(B)
        src, dst = edge_index[0].contiguous(), edge_index[1].contiguous()
        self.E = int(src.numel())
        self.by_dst, self.by_src, self.pool = csr_build_batch([(dst, src, self.N), (src, dst, self.N),
                                                               (batch.contiguous(), None, self.B)])
        self.batch32 = batch.to(torch.int32)
        self.F = 0 if edge_attr is None else (int(edge_attr.shape[1]) if edge_attr.dim() == 2 else 1)
        if self.F > len(BOND_FEATURE_DIMS):
            raise ValueError(f"edge_attr has {self.F} columns; the ogb BondEncoder has {len(BOND_FEATURE_DIMS)}")
        self.offsets, self.T = bond_offsets(self.F)
        # (an empty tensor's data_ptr() is NULL, which the ABI rejects: a batch without edges passes a one-element stand-in)
        one = torch.zeros(1, dtype=torch.int32, device=src.device)
        self.src_of_dst = self.by_dst.col if self.E else one
        self.dst_of_src = self.by_src.col if self.E else one
        self.code_dst = self._codes(edge_attr, self.by_dst)
        self.code_src = self._codes(edge_attr, self.by_src)

    def _codes(self, edge_attr, csr: CSR):
        code = torch.empty(max(csr.nnz, 1), dtype=torch.int32, device=csr.rowptr.device)
        if self.F == 0 or csr.nnz == 0:
            return code
        attr = edge_attr.reshape(self.E, self.F).to(torch.int64).contiguous()
        off = (ctypes.c_int32 * self.F)(*self.offsets)
        hip.check(hip.lib().hg_edge_codes(_ptr(attr), self.F, off, self.T, _ptr(csr.perm), csr.nnz, _ptr(code),
                                          _stream(code.device)), "hg_edge_codes")
        return code

    @classmethod
    def from_batch(cls, data) -> "GraphIndex":
        idx = getattr(data, "_graph_index", None)
        if idx is not None:
            return idx
        N = int(data.x.shape[0])
        B = int(data.num_graphs)
        return cls(data.edge_index, getattr(data, "edge_attr", None), data.batch, N, B)


def edge_msg_bytes(E: int, N: int, C: int, bwd: bool) -> int:
    """Algorithmic bytes of one launch, in the form of a segment reduce with the bond-table reads counted
    as zero bytes (LDS in the forward, 15.6 KB of cache-resident rows in the backward): forward 4C*E gathered rows + 8*E (source index, bond code) + 4*(N+1) rowptr + 4C*N self rows
    + 4C*N output (+ 4*(N+1) the other rowptr, GCN); backward the same walk over the by-source CSR plus 4C*N dx."""
    b = 4 * C * E + 8 * E + 4 * (N + 1) + 8 * C * N
    return b + (4 * C * N if bwd else 0)


class _EdgeMsg(torch.autograd.Function):
    """out = hg_edge_msg_fwd(mode, x, tables, param) over a GraphIndex; ``param`` is GIN's eps [1] or GCN's root_emb
    weight [1, C]; ``tables``: the bond-table weights the batch's columns select (none without bond columns), used stacked
    as [T, C] -- a view when they lie back to back (the graphed trainer's flat parameter buffer), else a copy.  When their
    gradient accumulators lie back to back too, the backward adds the tables' gradient straight into them
    (accumulate = 1: inside the step's deferral window that is one more record of the batched reduction launch), which is
    how the five layers that share the encoder sum into it without autograd's split and adds."""

    @staticmethod
    def forward(ctx, x, param, gi: GraphIndex, mode: int, *tables):
        _require_gpu(x, "edge_msg")
        x, param = _f32c(x), _f32c(param)
        table = None
        if tables:
            table = _stacked_view(tables) if _contiguous_run(tables) else torch.cat([_f32c(t) for t in tables], 0)
        N, C = x.shape
        out = torch.empty_like(x)
        eps = param if mode == GIN else None
        root = param if mode == GCN else None
        timed("k_edge_msg_fwd", edge_msg_bytes(gi.E, N, C, False),
              lambda: hip.check(hip.lib().hg_edge_msg_fwd(
                  mode, _ptr(x), _ptr(table), gi.T, gi.F, _ptr(gi.by_dst.rowptr), _ptr(gi.src_of_dst), _ptr(gi.code_dst),
                  _ptr(gi.by_src.rowptr), _ptr(eps), _ptr(root), N, C, _ptr(out), _stream(x.device)), "hg_edge_msg_fwd"))
        ctx.save_for_backward(x, table, param)
        ctx.gi, ctx.mode, ctx.tables = gi, mode, tables
        return out

    @staticmethod
    def backward(ctx, dout):
        x, table, param = ctx.saved_tensors
        gi, mode, tables = ctx.gi, ctx.mode, ctx.tables
        dout = _f32c(dout)
        N, C = x.shape
        dx = torch.empty_like(x)
        accs = [_acc_target(t) for t in tables]
        have = bool(tables) and all(a is not None for a in accs)
        direct = have and _contiguous_run(accs)
        if direct:
            dtab = _stacked_view(accs)
        else:
            dtab = torch.empty((max(gi.T, 1), C), dtype=torch.float32, device=x.device)
        dextra = torch.empty(C, dtype=torch.float32, device=x.device)
        L = hip.lib()
        ws_bytes = L.hg_edge_msg_bwd_workspace_bytes(N, C, gi.T)
        ws = _workspace(max(ws_bytes, 16), x.device)
        eps = param if mode == GIN else None
        root = param if mode == GCN else None
        timed("k_edge_msg_bwd", edge_msg_bytes(gi.E, N, C, True),
              lambda: hip.check(L.hg_edge_msg_bwd(
                  mode, _ptr(x), _ptr(table), gi.T, gi.F, _ptr(gi.by_src.rowptr), _ptr(gi.dst_of_src), _ptr(gi.code_src),
                  _ptr(eps), _ptr(root), _ptr(dout), N, C, _ptr(dx), _ptr(dtab), _ptr(dextra), 1 if direct else 0,
                  _ptr(ws), ws_bytes, _stream(x.device)), "hg_edge_msg_bwd"))
        dparam = (dextra[:1] if mode == GIN else dextra.view(1, C)).view_as(param)
        if direct or not tables:
            return (dx, dparam, None, None) + (None,) * len(tables)
        parts = torch.split(dtab[:gi.T], [t.shape[0] for t in tables], 0)
        if have:   # accumulators present but scattered (the trainer's probe pass): add piece by piece
            for a, g in zip(accs, parts):
                a.add_(g.view_as(a))
            return (dx, dparam, None, None) + (None,) * len(tables)
        return (dx, dparam, None, None) + tuple(parts)


def edge_msg(x, tables, param, gi: GraphIndex, mode: int):
    """GIN (mode 0): (1 + eps) x_i + sum_{e -> i} relu(x_src + bond_e); GCN (mode 1): the normalised sum plus
    relu(x_i + root) / deg_i (see include/equihgnn_hip.h).  ``tables``: a sequence of the bond-table weights the batch's
    columns select (or a single stacked [T, C] tensor)."""
    if torch.is_tensor(tables):
        tables = (tables,)
    tables = tuple(tables or ())
    if torch.is_grad_enabled():     # (as embed_sum: the trainer gives these weights a persistent accumulator)
        for t in tables:
            if t.requires_grad and t.is_leaf:
                ACC_PARAMS[id(t)] = t
    return _EdgeMsg.apply(x, param, gi, int(mode), *tables)


def mean_pool(x, gi: GraphIndex):
    """global_mean_pool over the (sorted) batch vector: hg_segment_reduce_f32 with mean on the pool CSR."""
    return reduce_entries(x, gi.pool, gi.batch32, "mean")
