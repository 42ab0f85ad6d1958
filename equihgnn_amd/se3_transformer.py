"""SE(3)-Transformer front-end of ``se3_transformer_equihnns`` (equihnn_se3_transformer.py:37-45: dim=C, heads=2, depth=2,
dim_head=32, num_degrees=2, 16 neighbours, radius 5; every other argument at its default: attend_self, one output degree, no
edge features / rotary embedding / null kv / global features / pre-convolutions, not reversible), MI355X-native, with the
reference's parameter names (se3_transformer_layer.py).

How a PairwiseConv is evaluated (the reference's dominant cost: it forms R_e = Linear(128 -> F I O)(h_e) per edge, 65 536
outputs per edge at C = 256, se3_transformer_layer.py:329-374): the sum over the input channel is moved to the NODE level,
    G_j[(mi, f), c, o] = sum_i W3[(o, i, f), c] x_j[i, mi]                  (ops.matmul_fan: the x6 / library GEMM)
    out_e[mo, o] = sum_(mi, f) B_e[mo, mi, f] (h_e . G_j[(mi, f), :, o] + GB_j[(mi, f), o])      (ops.se3t_pair)
with h_e [128] the radial trunk, B_e the basis and GB the same product with the last Linear's bias; csrc/se3t.hip has the
kernel.  Degree-d features are component-major, [N, 2d + 1, C], so every channel mix is a [m N, C] row product in place.

The Q_J matrices.  The reference takes them from an SVD null space (se3_transformer/basis.py:153-173), so the sign of each
depends on the LAPACK build; here they are closed forms with the signs the reference produced where the fixtures were written
(tests/golden/se3t/se3t_Q.npz).  A checkpoint trained where LAPACK chose another sign for some Q_J computes the same function once
that Q_J is flipped here: ``flip_q_sign``.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops
from .equiformer import _fan
from .index import HyperIndex

MID = 128
# sign of each Q_J, keyed (d_in, d_out, J); flip_q_sign() edits it
Q_SIGNS = {(0, 0, 0): 1.0, (0, 1, 1): -1.0, (1, 0, 1): -1.0, (1, 1, 0): 1.0, (1, 1, 1): 1.0, (1, 1, 2): 1.0}


def flip_q_sign(d_in: int, d_out: int, J: int) -> None:
    """Flip the sign of Q_J for the pair (d_in -> d_out): for a checkpoint trained where the reference's SVD
    (se3_transformer/basis.py:153-173) returned the other sign.  Call before the model is built (SE3Transformer reads the
    table in its constructor)."""
    Q_SIGNS[(d_in, d_out, J)] = -Q_SIGNS[(d_in, d_out, J)]


def q_matrices(dtype=torch.float64):
    """{(d_in, d_out, J): Q_J [m_out * m_in, 2J + 1]} in closed form, components in the reference's (y, z, x) order:
    (0,0): 1;  (0,1), (1,0): I / sqrt 3;  (1,1): J = 0 the identity / sqrt 3, J = 1 the antisymmetric tensor / sqrt 6,
    J = 2 the five symmetric traceless matrices (unit Frobenius norm each); times Q_SIGNS.  Rounded to float32 before the
    cast to ``dtype``, as the reference's are (basis.py:173 returns ``Q_J.float()``)."""
    eye = torch.eye(3, dtype=torch.float64)
    q = {(0, 0, 0): torch.ones(1, 1, dtype=torch.float64), (0, 1, 1): eye / math.sqrt(3), (1, 0, 1): eye / math.sqrt(3),
         (1, 1, 0): eye.reshape(9, 1) / math.sqrt(3)}
    eps = torch.zeros(3, 3, 3, dtype=torch.float64)
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        eps[a, b, c], eps[a, c, b] = 1.0, -1.0
    q[(1, 1, 1)] = eps.reshape(9, 3) / math.sqrt(6)
    s = torch.zeros(5, 3, 3, dtype=torch.float64)
    r10, r30 = 1 / math.sqrt(10), 1 / math.sqrt(30)
    s[0, 0, 2] = s[0, 2, 0] = r10
    s[1, 0, 1] = s[1, 1, 0] = r10
    s[2, 0, 0], s[2, 1, 1], s[2, 2, 2] = -r30, 2 * r30, -r30
    s[3, 1, 2] = s[3, 2, 1] = r10
    s[4, 0, 0], s[4, 2, 2] = -r10, r10
    q[(1, 1, 2)] = s.reshape(5, 9).t().contiguous()
    return {k: (Q_SIGNS[k] * v).float().to(dtype) for k, v in q.items()}


def q_table() -> torch.Tensor:
    """The Q_J matrices as the 100 floats se3t_edge_basis reads."""
    q = q_matrices(torch.float32)
    return torch.cat([q[k].reshape(-1) for k in ((0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 1, 2))])


def _to_order(d: int) -> int:
    return 2 * d + 1


class LinearSE3(nn.Module):
    """se3_transformer_layer.py:104-119 -- ``weights.<degree>`` [d_in, d_out] for the degrees both fibers have."""

    def __init__(self, fiber_in: dict, fiber_out: dict):
        super().__init__()
        self.weights = nn.ParameterDict()
        for d, din in fiber_in.items():
            if d in fiber_out:
                self.weights[str(d)] = nn.Parameter(torch.randn(din, fiber_out[d]) / math.sqrt(din))

    def w(self, d: int):
        return self.weights[str(d)]


def _mix(x, *ws):
    """(einsum("nmd,de->nme", x, w) for w in ws) on component-major x [N, m, d]: one fan of [m N, d] row products."""
    n, m, d = x.shape
    return tuple(o.view(n, m, -1) for o in _fan(x.reshape(n * m, d), *ws))


class NormSE3(nn.Module):
    """se3_transformer_layer.py:122-184 (gated_scale=False, GELU) -- ``transform.<degree>.scale`` [1, 1, C]."""

    def __init__(self, fiber: dict, eps: float = 1e-12):
        super().__init__()
        self.eps = eps
        self.transform = nn.ModuleDict({str(d): nn.ParameterDict({"scale": nn.Parameter(torch.ones(1, 1, c))})
                                        for d, c in fiber.items()})

    def forward(self, feats: dict):
        return {d: ops.se3t_norm(t, self.transform[str(d)]["scale"], self.eps) for d, t in feats.items()}


class RadialFunc(nn.Module):
    """se3_transformer_layer.py:311-336 -- ``net.{0,1,3,4,6}``.  The trunk net[0..5] runs on torch operators over the
    [E, 128] rows (two small Linears with LayerNorm and GELU; not the hot path); the last Linear is never applied per edge."""

    def __init__(self, num_freq: int, in_dim: int, out_dim: int, mid_dim: int = MID):
        super().__init__()
        self.num_freq, self.in_dim, self.out_dim, self.mid_dim = num_freq, in_dim, out_dim, mid_dim
        self.net = nn.Sequential(nn.Linear(1, mid_dim), nn.LayerNorm(mid_dim), nn.GELU(), nn.Linear(mid_dim, mid_dim),
                                 nn.LayerNorm(mid_dim), nn.GELU(), nn.Linear(mid_dim, num_freq * in_dim * out_dim))

    def trunk(self, dist):   # [E, 1] -> [E, 128]
        h = dist
        for i in range(6):
            h = self.net[i](h)
        return h

    def node_weights(self):
        """W3 [(o, i, f), c] as [I, (f, c, o)] and b3 [(o, i, f)] as [I, (f, o)]: the right-hand sides of the node-level
        products."""
        o, i, f, c = self.out_dim, self.in_dim, self.num_freq, self.mid_dim
        w = self.net[6].weight.view(o, i, f, c).permute(1, 2, 3, 0).reshape(i, f * c * o)
        b = self.net[6].bias.view(o, i, f).permute(1, 2, 0).reshape(i, f * o)
        return w, b


class PairwiseConv(nn.Module):
    """se3_transformer_layer.py:339-374 -- ``rp``."""

    def __init__(self, degree_in: int, nc_in: int, degree_out: int, nc_out: int):
        super().__init__()
        self.pair = (degree_in, degree_out)
        self.nc_out = nc_out
        self.rp = RadialFunc(_to_order(min(degree_in, degree_out)), nc_in, nc_out)

    def forward(self, x, geo: "EdgeBasis", pool: bool):
        """x [N, mi, I] (the senders' features) -> [E, mo, O], or [N, mo, O] pooled."""
        n, mi, i = x.shape
        w, b = self.rp.node_weights()
        g, gb = _fan(x.reshape(n * mi, i), w, b)
        h = self.rp.trunk(geo.dist)
        return ops.se3t_pair(h, g, gb, geo.basis, self.pair, self.nc_out, geo.csr_t.rowptr, geo.csr_t.perm,
                             geo.meanw if pool else None)


class ConvSE3(nn.Module):
    """se3_transformer_layer.py:187-308 (no edge features) -- ``kernel_unary.(di,do)`` and, pooled, ``self_interact``."""

    def __init__(self, fiber_in: dict, fiber_out: dict, self_interaction: bool = True, pool: bool = True):
        super().__init__()
        self.fiber_in, self.fiber_out, self.pool = dict(fiber_in), dict(fiber_out), pool
        self.kernel_unary = nn.ModuleDict()
        for di, ci in fiber_in.items():
            for do, co in fiber_out.items():
                self.kernel_unary[f"({di},{do})"] = PairwiseConv(di, ci, do, co)
        self.self_interaction = self_interaction
        if self_interaction:
            self.self_interact = LinearSE3(fiber_in, fiber_out)

    def forward(self, feats: dict, geo: "EdgeBasis"):
        out = {}
        for do in self.fiber_out:
            acc = None
            for di in self.fiber_in:
                o = self.kernel_unary[f"({di},{do})"](feats[di], geo, self.pool)
                acc = o if acc is None else acc + o
            out[do] = acc
        if self.self_interaction:
            for d in out:
                if str(d) in self.self_interact.weights:
                    out[d] = out[d] + _mix(feats[d], self.self_interact.w(d))[0]
        return out


class AttentionSE3(nn.Module):
    """se3_transformer_layer.py:415-605 (attend_self, keys by their own ConvSE3, 2 heads x 32)."""

    def __init__(self, fiber: dict, dim_head: int = 32, heads: int = 2):
        super().__init__()
        if heads != 2 or dim_head != 32:
            raise NotImplementedError("AttentionSE3: the kernels are built for heads=2, dim_head=32")
        hidden = {d: dim_head * heads for d in fiber}
        self.scale = dim_head ** -0.5
        self.to_q = LinearSE3(fiber, hidden)
        self.to_v = ConvSE3(fiber, hidden, self_interaction=False, pool=False)
        self.to_k = ConvSE3(fiber, hidden, self_interaction=False, pool=False)
        self.to_out = LinearSE3(hidden, fiber)
        self.to_self_k = LinearSE3(fiber, hidden)
        self.to_self_v = LinearSE3(fiber, hidden)

    def forward(self, feats: dict, geo: "EdgeBasis"):
        v = self.to_v(feats, geo)
        k = self.to_k(feats, geo)
        out = {}
        for d, f in feats.items():
            q, ks, vs = _mix(f, self.to_q.w(d), self.to_self_k.w(d), self.to_self_v.w(d))
            o = ops.se3t_attn(q, ks, k[d], vs, v[d], geo.maskf, self.scale)
            out[d] = _mix(o, self.to_out.w(d))[0]
        return out


class AttentionBlockSE3(nn.Module):
    """se3_transformer_layer.py:791-842."""

    def __init__(self, fiber: dict, dim_head: int = 32, heads: int = 2):
        super().__init__()
        self.attn = AttentionSE3(fiber, dim_head, heads)
        self.prenorm = NormSE3(fiber)

    def forward(self, feats: dict, geo: "EdgeBasis"):
        out = self.attn(self.prenorm(feats), geo)
        return {d: out[d] + feats[d] for d in feats}


class FeedForwardSE3(nn.Module):
    """se3_transformer_layer.py:380-394."""

    def __init__(self, fiber: dict, mult: int = 4):
        super().__init__()
        hidden = {d: c * mult for d, c in fiber.items()}
        self.project_in = LinearSE3(fiber, hidden)
        self.nonlin = NormSE3(hidden)
        self.project_out = LinearSE3(hidden, fiber)

    def forward(self, feats: dict):
        h = self.nonlin({d: _mix(t, self.project_in.w(d))[0] for d, t in feats.items()})
        return {d: _mix(t, self.project_out.w(d))[0] for d, t in h.items()}


class FeedForwardBlockSE3(nn.Module):
    """se3_transformer_layer.py:397-409."""

    def __init__(self, fiber: dict):
        super().__init__()
        self.prenorm = NormSE3(fiber)
        self.feedforward = FeedForwardSE3(fiber)

    def forward(self, feats: dict):
        out = self.feedforward(self.prenorm(feats))
        return {d: out[d] + feats[d] for d in feats}


class _Sequence(nn.Module):
    """se3_transformer/reversible.py SequentialSequence -- ``blocks.<i>.{0,1}``."""

    def __init__(self, blocks):
        super().__init__()
        self.blocks = nn.ModuleList([nn.ModuleList([a, f]) for a, f in blocks])


class EdgeBasis:
    """Neighbour lists and per-edge geometry of the whole batch cloud, built once per batch (no gradient): self-excluded
    K = min(k, N - 1) nearest by true distance (the Equiformer's search), then distance, radius mask, masked-mean weights and
    the 34 basis coefficients in one launch (ops.se3t_edge_basis)."""

    def __init__(self, pos, index: HyperIndex, k: int, radius: float, qtab):
        n = pos.shape[0]
        if n < 2:
            raise ValueError("SE3Transformer: at least two atoms are needed (the reference asserts one neighbour)")
        self.N, self.K = n, int(min(k, n - 1))
        nbr, _, csr_t = index.knn(pos, self.K, 1)
        self.nbr, self.csr_t = nbr, csr_t
        dist, self.maskf, self.meanw, self.basis = ops.se3t_edge_basis(pos, nbr, radius, qtab)
        self.dist = dist.view(-1, 1)


_DEFAULTS = dict(input_degrees=1, output_degrees=1, reduce_dim_out=False, num_tokens=None, num_positions=None,
                 num_edge_tokens=None, edge_dim=None, reversible=False, attend_self=True, use_null_kv=False,
                 differentiable_coors=False, fourier_encode_dist=False, rel_dist_num_fourier_features=4,
                 attend_sparse_neighbors=False, num_adj_degrees=None, adj_dim=0, max_sparse_neighbors=float("inf"), dim_in=None,
                 dim_out=None, norm_out=False, num_conv_layers=0, causal=False, splits=4, global_feats_dim=None,
                 linear_proj_keys=False, one_headed_key_values=False, tie_key_values=False, rotary_position=False,
                 rotary_rel_dist=False, norm_gated_scale=False, use_egnn=False, egnn_hidden_dim=32,
                 egnn_weights_clamp_value=None, egnn_feedforward=False, hidden_fiber_dict=None, out_fiber_dict=None)


class SE3Transformer(nn.Module):
    """se3_transformer_layer.py:1117-1693 as equihnn_se3_transformer.py:37-45 configures it; any other value of a constructor
    argument raises NotImplementedError (``splits`` only chunks memory in the reference and is accepted)."""

    def __init__(self, *, dim, heads=2, dim_head=32, depth=2, num_degrees=2, valid_radius=5, num_neighbors=16, **kw):
        super().__init__()
        for name, value in kw.items():
            if name not in _DEFAULTS:
                raise TypeError(f"SE3Transformer: unexpected argument {name!r}")
            if name != "splits" and value != _DEFAULTS[name]:
                raise NotImplementedError(f"SE3Transformer: {name}={value!r} is not built (only the configuration of "
                                          f"se3_transformer_equihnns is)")
        if (heads, dim_head, depth, num_degrees, num_neighbors) != (2, 32, 2, 2, 16) or float(valid_radius) != 5.0:
            raise NotImplementedError("SE3Transformer: built for heads=2, dim_head=32, depth=2, num_degrees=2, valid_radius=5, "
                                      "num_neighbors=16 (equihnn_se3_transformer.py:37-45)")
        if dim % 16:
            raise NotImplementedError("SE3Transformer: dim must be a multiple of 16 (the row-product tiles)")
        self.dim, self.k, self.radius = dim, num_neighbors, float(valid_radius)
        hidden = {0: dim, 1: dim}
        self.conv_in = ConvSE3({0: dim}, hidden)
        self.convs = nn.ModuleList([])
        self.net = _Sequence([(AttentionBlockSE3(hidden, dim_head, heads), FeedForwardBlockSE3(hidden)) for _ in range(depth)])
        self.conv_out = ConvSE3(hidden, {0: dim})
        self.register_buffer("_qtab", q_table(), persistent=False)

    def forward(self, feats, coors, index: HyperIndex = None, taps: dict = None):
        """feats [N, C], coors [N, 3] (the whole batch as one cloud, mask all true) -> [N, C], the degree-0 output."""
        if index is None:           # the layer on its own (tests): a one-molecule index over the cloud
            one = torch.zeros(1, dtype=torch.int64, device=feats.device)
            index = HyperIndex(one, one, feats.shape[0], 1)
        geo = EdgeBasis(coors, index, self.k, self.radius, self._qtab)
        x = self.conv_in({0: feats.unsqueeze(1)}, geo)
        if taps is not None:
            taps["conv_in0"], taps["conv_in1"] = x[0], x[1]
        for i, (attn, ff) in enumerate(self.net.blocks):
            x = ff(attn(x, geo))
            if taps is not None:
                taps[f"block{i}_0"], taps[f"block{i}_1"] = x[0], x[1]
        return self.conv_out(x, geo)[0].squeeze(1)
