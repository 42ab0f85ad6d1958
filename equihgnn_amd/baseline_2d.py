"""The 2-D baselines ``gin`` and ``gcn`` (baseline_2d.py:76-206: class GNN_2D) on the edge-message kernels.

main.py:28-31 builds them as ``model_cls(1, gnn_type=method, drop_ratio=dropout)``: 5 layers of width 300.  Parameter
and buffer names and shapes are the reference's (tests/golden/reference_state_dicts_2d.json), so its checkpoints load
with ``strict=True``.

Per layer: GIN = edge message (csrc/gnn2d.hip) -> Linear -> BatchNorm1d + ReLU -> Linear; GCN = Linear -> edge message.
The bond embedding is never materialised: the kernels sum the (shared) BondEncoder tables' rows per edge.  The
BatchNorm statistics count the real atoms only (layers.real_row_mask), so a padded batch (batch.pad_graph_batch) gives
the real molecules the results of the unpadded one.  ``gat`` / ``gatv2`` and the pooling modes ``max`` / ``attention``
/ ``set2set`` are not built (their arithmetic is torch_geometric's, which nothing here pins).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .layers import AtomEncoder, batch_norm_rows, head_loss, real_row_mask
from .ops.gnn2d import BOND_FEATURE_DIMS, GCN, GIN, GraphIndex, edge_msg, mean_pool
from .registry import registry


class BondEncoder(nn.Module):
    """ogb 1.3.6 BondEncoder: ``bond_embedding_list.{0,1,2}`` of sizes (5, 6, 2), summed over the columns present."""

    def __init__(self, emb_dim: int):
        super().__init__()
        self.bond_embedding_list = nn.ModuleList()
        for d in BOND_FEATURE_DIMS:
            emb = nn.Embedding(d, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            self.bond_embedding_list.append(emb)

    def tables(self, n_cols: int):
        """The weights of the first ``n_cols`` tables (the edge-message kernels sum their rows per edge).  Tables of absent
        columns take no part, so their weights end a step with grad None, as in the reference."""
        return tuple(e.weight for e in self.bond_embedding_list[:n_cols])


class GINConv(nn.Module):
    """baseline_2d.py:19-44: mlp((1 + eps) x + sum_{e -> i} relu(x_src + bond_e))."""

    def __init__(self, emb_dim: int):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(emb_dim, emb_dim), nn.BatchNorm1d(emb_dim), nn.ReLU(),
                                 nn.Linear(emb_dim, emb_dim))
        self.eps = nn.Parameter(torch.Tensor([0]))

    def forward(self, x, gi: GraphIndex, tables, mask):
        h = edge_msg(x, tables, self.eps, gi, GIN)
        lin0, bn, lin1 = self.mlp[0], self.mlp[1], self.mlp[3]
        h = ops.linear(h, lin0.weight, lin0.bias)
        h = batch_norm_rows(bn, h, mask, relu=True)
        return ops.linear(h, lin1.weight, lin1.bias)


class GCNConv(nn.Module):
    """baseline_2d.py:47-73: sum_{e -> i} norm_e relu(xl_src + bond_e) + relu(xl_i + root) / deg_i, xl = linear(x)."""

    def __init__(self, emb_dim: int):
        super().__init__()
        self.linear = nn.Linear(emb_dim, emb_dim)
        self.root_emb = nn.Embedding(1, emb_dim)

    def forward(self, x, gi: GraphIndex, tables, mask):
        xl = ops.linear(x, self.linear.weight, self.linear.bias)
        return edge_msg(xl, tables, self.root_emb.weight, gi, GCN)


@registry.register_model("gin")
@registry.register_model("gcn")
class GNN_2D(nn.Module):
    """baseline_2d.py:76-206, same constructor signature (main.py:28-31 calls it with gnn_type and drop_ratio)."""

    def __init__(self, num_tasks, num_layer=5, emb_dim=300, gnn_type="gin", residual=False, drop_ratio=0.0,
                 JK="last", graph_pooling="mean"):
        super().__init__()
        self.num_layer = num_layer
        self.drop_ratio = drop_ratio
        self.JK = JK
        self.emb_dim = emb_dim
        self.num_tasks = num_tasks
        self.residual = residual
        self.graph_pooling = graph_pooling
        self.gnn_type = gnn_type
        if self.num_layer < 2:
            raise ValueError("Number of GNN layers must be greater than 1.")
        if gnn_type in ("gat", "gatv2"):
            raise NotImplementedError(
                f"gnn_type {gnn_type!r}: its arithmetic is torch_geometric's GATConv / GATv2Conv, which this package does "
                "not reproduce (no reference code pins it); use the reference's own class for it")
        if gnn_type not in ("gin", "gcn"):
            raise ValueError("Undefined GNN type called {}".format(gnn_type))
        if graph_pooling in ("max", "attention", "set2set"):
            raise NotImplementedError(
                f"graph_pooling {graph_pooling!r} is not built: main.py only ever selects 'mean' (the default)")
        if graph_pooling not in ("mean", "sum"):
            raise ValueError("Invalid graph pooling type.")
        if JK not in ("last", "sum"):
            raise ValueError(f"JK must be 'last' or 'sum', got {JK!r}")
        self.atom_encoder = AtomEncoder(emb_dim=emb_dim)
        self.bond_encoder = BondEncoder(emb_dim=emb_dim)
        self.convs = nn.ModuleList()
        self.batch_norms = nn.ModuleList()
        for _ in range(num_layer):
            self.convs.append(GINConv(emb_dim) if gnn_type == "gin" else GCNConv(emb_dim))
            self.batch_norms.append(nn.BatchNorm1d(emb_dim))
        self.graph_pred_linear = nn.Linear(emb_dim, num_tasks)

    def forward(self, data, head=None):
        gi = GraphIndex.from_batch(data)
        h = self.atom_encoder(data.x)
        tables = self.bond_encoder.tables(gi.F)      # shared by all layers
        mask = real_row_mask(data, h)
        drop = self.training and self.drop_ratio > 0
        h_list = [h]
        for layer in range(self.num_layer):
            last = layer == self.num_layer - 1
            h = self.convs[layer](h_list[layer], gi, tables, mask)
            h = batch_norm_rows(self.batch_norms[layer], h, mask, relu=not last)
            if drop:
                h = F.dropout(h, self.drop_ratio, training=True)
            if self.residual:
                h = h + h_list[layer]
            h_list.append(h)
        if self.JK == "last":
            h_node = h_list[-1]
        else:
            h_node = h_list[0]
            for t in h_list[1:]:
                h_node = h_node + t
        if self.graph_pooling == "mean":
            h_graph = mean_pool(h_node, gi)
        else:
            h_graph = ops.reduce_entries(h_node, gi.pool, gi.batch32, "sum")
        out = ops.linear(h_graph, self.graph_pred_linear.weight, self.graph_pred_linear.bias)
        return head_loss(out.view(-1), head)
