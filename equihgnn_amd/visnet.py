"""ViSNet front-end of the ``visnet_*`` wrappers (visnet_layer.py:15-1050, as configured by equihnn_visnet.py: lmax 2,
8 heads, 6 layers, 32 RBFs, cutoff 5, max_num_neighbors 16, plain ViS_MP, no vector norm, fixed RBFs, no derivative).

Module tree, parameter and buffer names are the reference's, so its checkpoints load with ``strict=True``.  The radius
graph and every operation that walks it are the vis_* kernels (ops.visnet); the dense products go through ops.linear;
the node-row glue (splits, products of the o_proj / vec_proj pieces, the output blocks' norms and SiLUs) is torch.

Geometry needs no gradient (``pos`` does not require one): HyperIndex.radius builds the graph, r, C(r), the RBFs and the
spherical harmonics once per batch.  VecLayerNorm with ``norm_type=None`` multiplies by a buffer of ones: the identity,
not applied.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .layers import AtomEncoder


def _xavier(lin: nn.Linear):
    nn.init.xavier_uniform_(lin.weight)
    if lin.bias is not None:
        lin.bias.data.zero_()


def _lin(x, lin: nn.Linear):
    """ops.linear over the last dim of ``x`` (any leading shape)."""
    lead = x.shape[:-1]
    y = ops.linear(x.reshape(-1, x.shape[-1]), lin.weight, lin.bias)
    return y.reshape(*lead, y.shape[-1])


class CosineCutoff(nn.Module):
    def __init__(self, cutoff: float):
        super().__init__()
        self.cutoff = cutoff


class ExpNormalSmearing(nn.Module):
    """visnet_layer.py:51-115 with trainable=False: ``means`` / ``betas`` are buffers."""

    def __init__(self, cutoff: float = 5.0, num_rbf: int = 32, trainable: bool = False):
        super().__init__()
        if trainable:
            raise NotImplementedError("ViSNet: trainable RBFs are not supported (no visnet_* wrapper selects them)")
        self.cutoff, self.num_rbf, self.trainable = cutoff, num_rbf, trainable
        self.cutoff_fn = CosineCutoff(cutoff)
        self.alpha = 5.0 / cutoff
        means, betas = self._initial_params()
        self.register_buffer("means", means)
        self.register_buffer("betas", betas)

    def _initial_params(self):
        start_value = torch.exp(torch.tensor(-self.cutoff))
        means = torch.linspace(start_value, 1, self.num_rbf)
        betas = torch.tensor([(2 / self.num_rbf * (1 - start_value)) ** -2] * self.num_rbf)
        return means, betas

    def reset_parameters(self):
        means, betas = self._initial_params()
        self.means.data.copy_(means)
        self.betas.data.copy_(betas)


class VecLayerNorm(nn.Module):
    """visnet_layer.py:196-287 with norm_type=None, trainable=False: a ``weight`` buffer of ones."""

    def __init__(self, hidden_channels: int, trainable: bool = False, norm_type=None):
        super().__init__()
        if norm_type is not None or trainable:
            raise NotImplementedError("ViSNet: only vecnorm_type=None with a fixed weight is supported")
        self.hidden_channels, self.norm_type, self.eps = hidden_channels, norm_type, 1e-12
        self.register_buffer("weight", torch.ones(hidden_channels))

    def reset_parameters(self):
        nn.init.ones_(self.weight)


class Distance(nn.Module):
    def __init__(self, cutoff: float, max_num_neighbors: int = 16, add_self_loops: bool = True):
        super().__init__()
        self.cutoff, self.max_num_neighbors, self.add_self_loops = cutoff, max_num_neighbors, add_self_loops


class Sphere(nn.Module):
    def __init__(self, lmax: int = 2):
        super().__init__()
        self.lmax = lmax


class NeighborEmbedding(nn.Module):
    """visnet_layer.py:355-427: x_nb_i = sum_{j != i} emb_j (distance_proj(rbf_ij) C(r_ij)); combine([x, x_nb])."""

    def __init__(self, hidden_channels: int, num_rbf: int, cutoff: float, max_z: int = 100):
        super().__init__()
        self.embedding = AtomEncoder(emb_dim=hidden_channels)
        self.distance_proj = nn.Linear(num_rbf, hidden_channels)
        self.combine = nn.Linear(hidden_channels * 2, hidden_channels)
        self.cutoff = CosineCutoff(cutoff)
        self.reset_parameters()

    def reset_parameters(self):
        _xavier(self.distance_proj)
        _xavier(self.combine)

    def forward(self, z, x, g):
        W = ops.linear(g.rbf, self.distance_proj.weight, self.distance_proj.bias)
        xn = ops.vis_neighbor_sum(self.embedding(z), W, g)
        return ops.linear(torch.cat([x, xn], dim=1), self.combine.weight, self.combine.bias)


class EdgeEmbedding(nn.Module):
    """visnet_layer.py:430-469: f_ij = (x_i + x_j) edge_proj(rbf_ij)."""

    def __init__(self, num_rbf: int, hidden_channels: int):
        super().__init__()
        self.edge_proj = nn.Linear(num_rbf, hidden_channels)
        self.reset_parameters()

    def reset_parameters(self):
        _xavier(self.edge_proj)

    def forward(self, x, g):
        return ops.vis_edge_embed(x, ops.linear(g.rbf, self.edge_proj.weight, self.edge_proj.bias), g)


class ViS_MP(nn.Module):
    """visnet_layer.py:472-680 (vertex=False)."""

    def __init__(self, num_heads: int, hidden_channels: int, cutoff: float, vecnorm_type=None,
                 trainable_vecnorm: bool = False, last_layer: bool = False):
        super().__init__()
        if hidden_channels % num_heads != 0:
            raise ValueError(f"The number of hidden channels (got {hidden_channels}) must be evenly divisible by the "
                             f"number of attention heads (got {num_heads})")
        ops.visnet.check_channels(hidden_channels)
        if num_heads != ops.visnet.HEADS:
            raise NotImplementedError(f"ViSNet kernels run {ops.visnet.HEADS} heads (got {num_heads})")
        self.num_heads = num_heads
        self.hidden_channels = hidden_channels
        self.head_dim = hidden_channels // num_heads
        self.last_layer = last_layer
        self.layernorm = nn.LayerNorm(hidden_channels)
        self.vec_layernorm = VecLayerNorm(hidden_channels, trainable=trainable_vecnorm, norm_type=vecnorm_type)
        self.act = nn.SiLU()
        self.attn_activation = nn.SiLU()
        self.cutoff = CosineCutoff(cutoff)
        C = hidden_channels
        self.vec_proj = nn.Linear(C, C * 3, False)
        self.q_proj = nn.Linear(C, C)
        self.k_proj = nn.Linear(C, C)
        self.v_proj = nn.Linear(C, C)
        self.dk_proj = nn.Linear(C, C)
        self.dv_proj = nn.Linear(C, C)
        self.s_proj = nn.Linear(C, C * 2)
        if not self.last_layer:
            self.f_proj = nn.Linear(C, C)
            self.w_src_proj = nn.Linear(C, C, False)
            self.w_trg_proj = nn.Linear(C, C, False)
        self.o_proj = nn.Linear(C, C * 3)
        self.reset_parameters()

    def reset_parameters(self):
        self.layernorm.reset_parameters()
        self.vec_layernorm.reset_parameters()
        for lin in (self.q_proj, self.k_proj, self.v_proj, self.o_proj, self.s_proj, self.vec_proj, self.dk_proj,
                    self.dv_proj):
            _xavier(lin)
        if not self.last_layer:
            for lin in (self.f_proj, self.w_src_proj, self.w_trg_proj):
                _xavier(lin)

    def forward(self, x, vec, f, g):
        C = self.hidden_channels
        x = ops.layer_norm_rows(x, self.layernorm.weight, self.layernorm.bias, self.layernorm.eps)
        q, k, v = _lin(x, self.q_proj), _lin(x, self.k_proj), _lin(x, self.v_proj)
        dkr, dvr = _lin(f, self.dk_proj), _lin(f, self.dv_proj)
        vec1, vec2, vec3 = torch.split(_lin(vec, self.vec_proj), C, dim=-1)
        vec_dot = (vec1 * vec2).sum(dim=1)
        u, xagg = ops.vis_attn(q, k, v, dkr, dvr, g)
        vec_out = ops.vis_vec_msg(vec, _lin(u, self.s_proj), g)
        o1, o2, o3 = torch.split(_lin(xagg, self.o_proj), C, dim=1)
        dx = vec_dot * o2 + o3
        dvec = vec3 * o1.unsqueeze(1) + vec_out
        if self.last_layer:
            return dx, dvec, None
        df = ops.vis_edge_update(_lin(vec, self.w_trg_proj), _lin(vec, self.w_src_proj), _lin(f, self.f_proj), g)
        return dx, dvec, df


class ViSNetBlock(nn.Module):
    """visnet_layer.py:754-908."""

    def __init__(self, lmax=2, vecnorm_type=None, trainable_vecnorm=False, num_heads=8, num_layers=6,
                 hidden_channels=128, num_rbf=32, trainable_rbf=False, max_z=100, cutoff=5.0, max_num_neighbors=16,
                 vertex=False):
        super().__init__()
        if vertex:
            raise NotImplementedError("ViSNet: ViS_MP_Vertex (vertex=True) is not supported")
        if lmax != 2:
            raise NotImplementedError(f"ViSNet: lmax={lmax}; the kernels carry the 8 components of lmax 2")
        if num_rbf != ops.visnet.NRBF:
            raise NotImplementedError(f"ViSNet: {ops.visnet.NRBF} RBFs (got num_rbf={num_rbf})")
        if max_num_neighbors != ops.visnet.K:
            raise NotImplementedError(f"ViSNet: the slot table holds {ops.visnet.K} neighbours (got {max_num_neighbors})")
        self.lmax, self.vecnorm_type, self.trainable_vecnorm = lmax, vecnorm_type, trainable_vecnorm
        self.num_heads, self.num_layers, self.hidden_channels = num_heads, num_layers, hidden_channels
        self.num_rbf, self.trainable_rbf, self.max_z = num_rbf, trainable_rbf, max_z
        self.cutoff, self.max_num_neighbors = cutoff, max_num_neighbors
        self.embedding = AtomEncoder(emb_dim=hidden_channels)
        self.distance = Distance(cutoff, max_num_neighbors=max_num_neighbors)
        self.sphere = Sphere(lmax=lmax)
        self.distance_expansion = ExpNormalSmearing(cutoff, num_rbf, trainable_rbf)
        self.neighbor_embedding = NeighborEmbedding(hidden_channels, num_rbf, cutoff, max_z)
        self.edge_embedding = EdgeEmbedding(num_rbf, hidden_channels)
        kw = dict(num_heads=num_heads, hidden_channels=hidden_channels, cutoff=cutoff, vecnorm_type=vecnorm_type,
                  trainable_vecnorm=trainable_vecnorm)
        self.vis_mp_layers = nn.ModuleList([ViS_MP(last_layer=False, **kw) for _ in range(num_layers - 1)])
        self.vis_mp_layers.append(ViS_MP(last_layer=True, **kw))
        self.out_norm = nn.LayerNorm(hidden_channels)
        self.vec_out_norm = VecLayerNorm(hidden_channels, trainable=trainable_vecnorm, norm_type=vecnorm_type)

    def forward(self, z, pos, index):
        de = self.distance_expansion
        g = index.radius(pos, self.cutoff, self.max_num_neighbors, de.means, de.betas)
        x = self.embedding(z)
        x = self.neighbor_embedding(z, x, g)
        vec = torch.zeros(x.shape[0], (self.lmax + 1) ** 2 - 1, x.shape[1], dtype=x.dtype, device=x.device)
        f = self.edge_embedding(x, g)
        for layer in self.vis_mp_layers:
            dx, dvec, df = layer(x, vec, f, g)
            x = x + dx
            vec = vec + dvec
            if df is not None:
                f = f + df
        x = ops.layer_norm_rows(x, self.out_norm.weight, self.out_norm.bias, self.out_norm.eps)
        return x, vec


class GatedEquivariantBlock(nn.Module):
    """torch_geometric.nn.models.visnet.GatedEquivariantBlock (PyG 2.5.3), scalar_activation=True."""

    def __init__(self, hidden_channels: int, out_channels: int, intermediate_channels=None, scalar_activation=False):
        super().__init__()
        self.out_channels = out_channels
        if intermediate_channels is None:
            intermediate_channels = hidden_channels
        self.vec1_proj = nn.Linear(hidden_channels, hidden_channels, bias=False)
        self.vec2_proj = nn.Linear(hidden_channels, out_channels, bias=False)
        self.update_net = nn.Sequential(nn.Linear(hidden_channels * 2, intermediate_channels), nn.SiLU(),
                                        nn.Linear(intermediate_channels, out_channels * 2))
        self.act = nn.SiLU() if scalar_activation else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.vec1_proj.weight)
        nn.init.xavier_uniform_(self.vec2_proj.weight)
        _xavier(self.update_net[0])
        _xavier(self.update_net[2])

    def forward(self, x, v):
        vec1 = torch.linalg.vector_norm(_lin(v, self.vec1_proj), dim=-2)
        vec2 = _lin(v, self.vec2_proj)
        h = _lin(F.silu(_lin(torch.cat([x, vec1], dim=-1), self.update_net[0])), self.update_net[2])
        x, v = torch.split(h, self.out_channels, dim=-1)
        v = v.unsqueeze(1) * vec2
        if self.act is not None:
            x = self.act(x)
        return x, v


class EquivariantScalar(nn.Module):
    def __init__(self, hidden_channels: int):
        super().__init__()
        self.output_network = nn.ModuleList([
            GatedEquivariantBlock(hidden_channels, hidden_channels, scalar_activation=True),
            GatedEquivariantBlock(hidden_channels, hidden_channels, scalar_activation=True),
        ])

    def pre_reduce(self, x, v):
        for layer in self.output_network:
            x, v = layer(x, v)
        return x + v.sum() * 0      # (the reference's: the last vector output reaches the loss as zero gradients)


class ViSNet(nn.Module):
    """visnet_layer.py:952-1050: representation_model -> output_model.pre_reduce -> x * std (per atom, no reduction)."""

    def __init__(self, lmax=1, vecnorm_type=None, trainable_vecnorm=False, num_heads=8, num_layers=6,
                 hidden_channels=128, num_rbf=32, trainable_rbf=False, max_z=100, cutoff=5.0, max_num_neighbors=32,
                 vertex=False, reduce_op="sum", mean=0.0, std=1.0, derivative=False):
        super().__init__()
        if derivative:
            raise NotImplementedError("ViSNet: derivative=True (forces) is not supported")
        self.representation_model = ViSNetBlock(
            lmax=lmax, vecnorm_type=vecnorm_type, trainable_vecnorm=trainable_vecnorm, num_heads=num_heads,
            num_layers=num_layers, hidden_channels=hidden_channels, num_rbf=num_rbf, trainable_rbf=trainable_rbf,
            max_z=max_z, cutoff=cutoff, max_num_neighbors=max_num_neighbors, vertex=vertex)
        self.output_model = EquivariantScalar(hidden_channels=hidden_channels)
        self.reduce_op = reduce_op
        self.derivative = derivative
        self.register_buffer("mean", torch.tensor(mean))
        self.register_buffer("std", torch.tensor(std))

    def forward(self, z, pos, index):
        """``index``: the batch's HyperIndex (its pool CSR gives the molecules; the radius graph is cached on it)."""
        x, v = self.representation_model(z, pos, index)
        x = self.output_model.pre_reduce(x, v)
        return x * self.std

