"""Model classes registered under the reference's ``--method`` names.

Constructor and call contract of main.py:28-34,46-47: ``cls(num_target, args)``;
``model(data) -> float32 Tensor[B]`` on ``data.x.device``.  Parameter / buffer names and shapes are
identical to the reference's, so its checkpoints load with ``strict=True``.

The fourteen hypergraph methods are six front-ends (none, EGNN, Equiformer, FAFormer, SE(3)-Transformer, ViSNet: the
``_Front`` rows below)
times three tails (``_STail``, ``_PairedBase``, ``_MTail``).  A registered class is a subclass of one tail that names its
front-end; a new method is a new row or a new three-line class, never a new ``forward``.
"""
from __future__ import annotations

import contextlib
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn as nn

from . import ops
from .equiformer import Equiformer
from .faformer import FAFormer
from .index import HyperIndex
from .layers import (EGNN, MLP, AtomEncoder, BondEncoder, MHNNConv, MHNNSConv, batch_norm_rows, head_loss, head_spec, pool_sum, readout,
                     real_row_mask)
from .registry import registry
from .se3_transformer import SE3Transformer
from .visnet import ViSNet

_ACT = {"Id": nn.Identity, "relu": nn.ReLU, "prelu": nn.PReLU}


class _Front(NamedTuple):
    """A geometric front-end as the reference's wrappers attach it: applied once, in front of the hypergraph layers."""
    attr: str                 # the reference's attribute name (a state-dict prefix)
    build: Callable           # args -> module
    embeds: bool = True       # fed the wrapper's AtomEncoder rows (ViSNet takes data.x and embeds with its own two)
    masked: bool = False      # also takes real_row_mask (FAFormer: centroid and frames over the real rows of a padded batch)


_EGNN = _Front("egnn_layer", lambda a: EGNN(dim=a.MLP_hidden, num_nearest_neighbors=16))
_EQUIFORMER = _Front("equiformer_layer",
                     lambda a: Equiformer(dim=a.MLP_hidden, dim_head=48, num_neighbors=16, valid_radius=5.0))
_FAFORMER = _Front("fa_former",    # equihnn_fa_former.py:36-49,130-143,210-223
                   lambda a: FAFormer(a.MLP_hidden, n_layers=2, n_heads=2, n_neighbors=16, valid_radius=5.0), masked=True)
_SE3_TRANSFORMER = _Front("se3_transformer_layer",   # equihnn_se3_transformer.py:37-45
                         lambda a: SE3Transformer(dim=a.MLP_hidden, heads=2, depth=2, dim_head=32, num_degrees=2, valid_radius=5,
                                                  num_neighbors=16))
_VISNET = _Front("visnet_layer",   # equihnn_visnet.py:35-37,114-118,183-185
                 lambda a: ViSNet(hidden_channels=a.MLP_hidden, lmax=2, max_num_neighbors=16), embeds=False)


def _mhnn_conv(args):
    return MHNNConv(args.MLP_hidden, mlp1_layers=args.MLP1_num_layers, mlp2_layers=args.MLP2_num_layers,
                    mlp3_layers=args.MLP3_num_layers, mlp4_layers=args.MLP4_num_layers,
                    aggr=args.aggregate, dropout=args.dropout, normalization=args.normalization)


def _head(num_target, args, width=1):
    return MLP(in_channels=args.MLP_hidden * width, hidden_channels=args.output_hidden * width,
               out_channels=num_target, num_layers=args.output_num_layers,
               dropout=args.dropout, Normalization=args.normalization, InputNorm=False)


def _merged_scope(convs, x, e):
    """ops.merged_scope on the GPU (the panel path of MHNNConv); a no-op context elsewhere."""
    return ops.merged_scope(convs, x, e) if x.is_cuda else contextlib.nullcontext()


class _Wrapper(nn.Module):
    """What the three tails share: the scalar hyper-parameters and the one path to the front-end.  Each tail's ``__init__``
    creates its sub-modules in the reference's order for that tail (it is the order of ``state_dict()`` and of the seeded
    random draws), so each decides where ``_build_front`` goes."""

    front: Optional[_Front] = None

    def __init__(self, args):
        super().__init__()
        self.act = _ACT[args.activation]()
        self.dropout = nn.Dropout(args.dropout)
        self.mlp1_layers = args.MLP1_num_layers
        self.mlp2_layers = args.MLP2_num_layers
        self.mlp3_layers = args.MLP3_num_layers
        self.nlayer = args.All_num_layers

    @property
    def _embeds(self):
        return self.front is None or self.front.embeds

    # -- training dropout (--dropout, main.py:202) -------------------------------------------------------------------
    # With ops.FUSED_DROPOUT the tail's dropout sites take their keep decisions from the hash of (seed, element index)
    # (csrc/drop_hash.h) and their seeds, one per site, from one pool of 64 draws per forward pass, in this FIXED order:
    #   per application of a conv layer: the wrapper's input dropout(s) (x, then e), then the layer's MLPs W1, W2, W3 (W4),
    #   one seed per hidden layer of each; after the applications the dropout in front of the pool (the paired / M tails
    #   draw theirs, x then e, after each application instead: mhnn.py:208-214), then the head's hidden layers.  On the
    #   fused read-out (ops.READOUT_DROPOUT) the last three are sites of the one launch, drawn by ops.readout_mse in that
    #   order: pre-pool (S tail), hidden 1, hidden 2.  On the paired tail's one-launch head (ops.PAIRED_READOUT) the LAST
    #   application's x and e dropouts and the head's two are the four sites of that launch, drawn by ops.readout_pair_mse
    #   in the same order: x, e, hidden 1, hidden 2.
    @property
    def _drop_p(self) -> float:
        return float(self.dropout.p) if (self.training and self.dropout.p > 0) else 0.0

    def _dropout_scope(self, x):
        """The seed pool around the tail (it nests with FAFormer's own: the outermost block draws)."""
        return ops.dropout_seeds(x.device, 64, enabled=x.is_cuda and self._drop_p > 0 and ops.FUSED_DROPOUT)

    def _drop(self, x):
        """self.dropout(x) (equihnn_egnn.py:162-166, mhnn.py:208-214) on rows: one pass, no mask tensor."""
        p = self._drop_p
        if p > 0 and ops.FUSED_DROPOUT and x.is_cuda and ops.dropout_add_supported(x, None):
            return ops.dropout_add(x, None, p)
        return self.dropout(x)

    def _build_front(self, args):
        if self.front is not None:
            setattr(self, self.front.attr, self.front.build(args))

    def _apply_front(self, data, index, taps):
        """Node features in front of the hypergraph layers, with the ``atom_encoder`` / ``front_end`` taps."""
        x = data.x
        if self._embeds:
            x = self.atom_encoder(x)
            if taps is not None:
                taps["atom_encoder"] = x
        if self.front is not None:
            extra = (real_row_mask(data, x),) if self.front.masked else ()
            x = getattr(self, self.front.attr)(x, data.pos, index, *extra)
            if taps is not None:
                taps["front_end"] = x
        return x


def _conv_layers(model, x, index, x0, res, fuse_act, taps):
    """The wrappers' loop over the shared conv layer (equihnn_egnn.py:160-165, mhnn.py:208-212): conv -> activation ->
    dropout, ``All_num_layers`` times.  With the merged residual and the ReLU fused, all applications run as ONE autograd
    node on the row-panel kernels (MHNNSConv.forward_stack) -- under an active dropout too (ops.STACK_DROPOUT): the first
    application's input dropout is the pass below, the others are sites of the node, in the seed order of the loop."""
    p_x = float(model.dropout.p) if (model.dropout.training and model.dropout.p > 0) else 0.0
    if model.nlayer >= 1 and fuse_act and taps is None and model.conv.stack_supported(x, res, p_x):
        if p_x > 0:
            if x is res["x0"]:
                x = res["x0_pass"]  # x0 reaches the first application through the residual's autograd node (one route for its gradient)
            x = model._drop(x)
        return model.conv.forward_stack(x, index, res, model.nlayer, relu_out=True, p_x=p_x)
    for i in range(model.nlayer):
        if i == 0 and isinstance(res, dict) and x is res["x0"] and model._drop_p > 0:
            x = res["x0_pass"]      # x0 reaches the first application through the residual's autograd node (one route for its gradient)
        x = model.conv(model._drop(x), index, x0, res, relu_out=fuse_act)
        if taps is not None:
            taps[f"conv{i}"] = x
        if not fuse_act:
            x = model.act(x)
    return x


class _STail(_Wrapper):
    """The S tail: [AtomEncoder ->] front-end (once) -> shared MHNNSConv x L -> pool -> head."""

    def __init__(self, num_target, args):
        super().__init__(args)
        if self._embeds:
            self.atom_encoder = AtomEncoder(emb_dim=args.MLP_hidden)
        self._build_front(args)
        self.conv = MHNNSConv(args.MLP_hidden, mlp1_layers=self.mlp1_layers,
                              mlp2_layers=self.mlp2_layers, mlp3_layers=self.mlp3_layers,
                              aggr=args.aggregate, dropout=args.dropout,
                              normalization=args.normalization)
        self.mlp_out = _head(num_target, args)

    def reset_parameters(self):  # equihnn_egnn.py:151-153
        self.conv.reset_parameters()
        self.mlp_out.reset_parameters()

    def forward(self, data, taps=None, head=None):
        index = HyperIndex.from_batch(data)
        x = self._apply_front(data, index, taps)
        x0 = x
        with self._dropout_scope(x):
            res = self.conv.prepare(x0, index)   # layer-independent residual term, built once
            fuse_act = taps is None and isinstance(res, dict) and isinstance(self.act, nn.ReLU)   # ReLU in the GEMM epilogue
            x = _conv_layers(self, x, index, x0, res, fuse_act, taps)
            return readout(self.mlp_out, x, index, taps, head, p_x=self._drop_p, drop=self._drop)


class _PairedBase(_Wrapper):
    """The paired tail: ONE shared MHNNConv applied L times on (x, e); nodes and hyperedges of order > 2 are pooled per
    molecule and concatenated.  The reference sizes the hyperedge pool by ``he_batch.max()+1`` and fails in ``torch.cat``
    when the last molecules of a batch have no such hyperedge; here they get a zero row."""

    front_leads = False   # the front-end is the FIRST sub-module (equihnn_egnn.py:12-95 only); the others append theirs

    def __init__(self, num_target, args):
        super().__init__(args)
        self.mlp4_layers = args.MLP4_num_layers
        if self.front_leads:
            self._build_front(args)
        self.atom_encoder = AtomEncoder(emb_dim=args.MLP_hidden)
        self.bond_encoder = BondEncoder(6, args.MLP_hidden)
        self.conv = _mhnn_conv(args)
        self.mlp_out = _head(num_target, args, width=2)
        if not self._embeds:
            del self.atom_encoder   # never used, but its random draws come before those of every module after it
        if not self.front_leads:
            self._build_front(args)

    def forward(self, data, taps=None, head=None):
        index = HyperIndex.from_batch(data)
        x = self._apply_front(data, index, taps)
        e = self.bond_encoder(data.edge_attr)
        with self._dropout_scope(x):
            with _merged_scope([self.conv], x, e):      # the shared layer's weight-level products once per step
                for i in range(self.nlayer):
                    x, e = self.conv(x, e, index)
                    if i != self.nlayer - 1:
                        x, e = self.act(x), self.act(e)
                    elif self._one_launch_head(x, e, taps, head):
                        # the last application's two dropouts, the pools, the head, the loss and their backward: one launch
                        loss, _ = ops.readout_pair_mse(x, e, index, data.n_e, data.e_order, self.mlp_out, head[0], head[1],
                                                       unit_grad=bool(head[2]) if len(head) > 2 else False, p_x=self._drop_p,
                                                       loss=head_spec(head))
                        return loss
                    x, e = self._drop(x), self._drop(e)
            both = self._pool(x, e, index, data)
            if taps is not None:
                taps["pool"] = both
            return head_loss(self.mlp_out(both, mask=index.pad_masks()[3]).view(-1), head)

    def _one_launch_head(self, x, e, taps, head) -> bool:
        """Whether the tail ends in ops.readout_pair_mse: training mode, a loss is asked for, nothing is tapped, ops.PAIRED_READOUT
        is on and the head has a shape the launch is built for (under an active dropout: its dropout form)."""
        if head is None or taps is not None or not (self.training and ops.PAIRED_READOUT and x.is_cuda and head[0].is_cuda):
            return False
        p_x = self._drop_p
        if p_x == 0.0 and ops.readout_pair_mse_supported(x, e, self.mlp_out):
            return True
        return ops.readout_pair_mse_drop_supported(x, e, self.mlp_out, p_x)

    fused_pool = False   # the read-out as ONE launch each way (ops.pool_pair) instead of mask, product, two reduces and a cat

    def _pool(self, x, e, index, data):
        """[B, 2C]: node rows and hyperedge rows of order > 2 summed per molecule, side by side (mhnn.py:58,72)."""
        if self.fused_pool:
            return ops.pool_pair(x, e, index, data.n_e, data.e_order)
        xp = pool_sum(x, index)
        he_csr, he_key = index.hyperedge_pool(data.n_e)
        keep = (data.e_order > 2).to(e.dtype).unsqueeze(-1)
        ep = ops.reduce_entries(e * keep, he_csr, he_key, "sum")
        return torch.cat((xp, ep), -1)


class _MTail(_Wrapper):
    """The M tail: L unshared MHNNConv layers + BatchNorm1d on node rows -> pool -> head.  The host-side per-molecule
    ``.item()`` loop of mhnn.py:196-199 builds a tensor the model never uses; it is not reproduced (it costs B device syncs
    per step)."""

    # Whether the layer loop runs inside ops.merged_scope (all layers' weight-level products in one launch each way).
    # True on ``mhnnm`` alone: the three methods with a front-end have never opened it, and that was inherited from the
    # order the code was written in, not measured.  Turning it on for them changes their launch sequence and needs a
    # number behind it.
    merged_layers = False

    def __init__(self, num_target, args):
        super().__init__(args)
        self.mlp4_layers = args.MLP4_num_layers
        self.atom_encoder = AtomEncoder(emb_dim=args.MLP_hidden)
        self.bond_encoder = BondEncoder(6, args.MLP_hidden)
        self.layers = nn.ModuleList()
        self.batch_norms = nn.ModuleList()
        for _ in range(self.nlayer):
            self.layers.append(_mhnn_conv(args))
            self.batch_norms.append(nn.BatchNorm1d(args.MLP_hidden))
        self.mlp_out = _head(num_target, args)
        if not self._embeds:
            del self.atom_encoder   # never used, but its random draws come before those of every module after it
        self._build_front(args)

    def forward(self, data, taps=None, head=None):
        index = HyperIndex.from_batch(data)
        x = self._apply_front(data, index, taps)
        e = self.bond_encoder(data.edge_attr)
        mask = real_row_mask(data, x)   # padded batch: BatchNorm statistics over the real atoms only
        with self._dropout_scope(x):
            with _merged_scope(self.layers, x, e) if self.merged_layers else contextlib.nullcontext():
                for i, layer in enumerate(self.layers):
                    x, e = layer(x, e, index)
                    # (the ReLU behind the normalisation rides its launches, unless the pre-activation value is tapped)
                    fuse = taps is None and i != self.nlayer - 1 and isinstance(self.act, nn.ReLU)
                    x = batch_norm_rows(self.batch_norms[i], x, mask, relu=fuse)
                    if taps is not None:
                        taps[f"bn{i}"] = x
                    if i != self.nlayer - 1:  # no activation after the last layer, mhnn.py:208-214
                        x, e = (x if fuse else self.act(x)), self.act(e)
                    x, e = self._drop(x), self._drop(e)
            return readout(self.mlp_out, x, index, taps, head)


@registry.register_model("mhnns")
class MHNNS(_STail):
    """mhnn.py:84-141: shared MHNNSConv x L on atom embeddings (no geometric front-end)."""


@registry.register_model("egnn_equihnns")
class EGNNEquiHNNS(_STail):
    """equihnn_egnn.py:98-169: AtomEncoder -> EGNN (once) -> shared MHNNSConv x L -> pool -> head."""
    front = _EGNN


@registry.register_model("equiformer_equihnns")
class EquiformerEquiHNNS(_STail):
    """equihnn_equiformer.py:12-93: AtomEncoder -> Equiformer (once, type-0 output) -> shared
    MHNNSConv x L -> pool -> head.  The reference keeps a leading batch dim of 1 through the conv /
    pool / head (equihnn_equiformer.py:82-85) and flattens at the end; values are identical."""
    front = _EQUIFORMER


@registry.register_model("faformer_equihnns")
class FAFormerEquiHNNS(_STail):
    """equihnn_fa_former.py:105-184: AtomEncoder -> FAFormer (once) -> shared MHNNSConv x L -> pool
    -> head.  Note the reference keeps proj_drop = attn_drop = 0.1 inside FAFormer in training mode
    (fa_former_layer.py:20-21), whatever ``--dropout`` says."""
    front = _FAFORMER


@registry.register_model("se3_transformer_equihnns")
class SE3TransformerEquiHNNS(_STail):
    """equihnn_se3_transformer.py:12-91: AtomEncoder -> SE3Transformer (once, degree-0 output) -> shared MHNNSConv x L -> pool
    -> head."""
    front = _SE3_TRANSFORMER


@registry.register_model("visnet_equihnns")
class VisNetEquiHNNS(_STail):
    """equihnn_visnet.py:92-158: ViSNet (once) -> shared MHNNSConv x L -> pool -> head."""
    front = _VISNET


@registry.register_model("mhnn")
class MHNN(_PairedBase):
    """mhnn.py:11-81: AtomEncoder -> shared MHNNConv x L on (x, e) -> node and order > 2 hyperedge pools -> head."""


@registry.register_model("egnn_equihnn")
class EGNNEquiHNN(_PairedBase):
    """equihnn_egnn.py:12-95: mhnn with the EGNN front-end applied once to the atom embeddings."""
    front = _EGNN
    front_leads = True


@registry.register_model("faformer_equihnn")
class FAFormerEquiHNN(_PairedBase):
    """equihnn_fa_former.py:12-102: AtomEncoder -> FAFormer (once) -> ONE shared MHNNConv x L on (x, e) -> node and
    order > 2 hyperedge pools side by side (one launch, ops.pool_pair) -> head on [B, 2C].  A molecule without a hyperedge
    of order > 2 gets a zero row in the hyperedge pool; the reference sizes that pool by ``he_batch.max() + 1`` and fails in
    ``torch.cat`` (:101) when the LAST molecules of a batch have none.  The reference keeps proj_drop = attn_drop = 0.1
    inside FAFormer in training mode (fa_former_layer.py:20-21), whatever ``--dropout`` says."""
    front = _FAFORMER
    fused_pool = True


@registry.register_model("visnet_equihnn")
class VisNetEquiHNN(_PairedBase):
    """equihnn_visnet.py:11-89: ViSNet (its own two AtomEncoders) -> shared MHNNConv x L -> node and order > 2 hyperedge
    pools -> head.  No AtomEncoder of its own."""
    front = _VISNET


@registry.register_model("mhnnm")
class MHNNM(_MTail):
    """mhnn.py:144-218: L unshared MHNNConv layers + BatchNorm1d on atom embeddings (no geometric front-end)."""
    merged_layers = True    # 1.30 -> 1.28 ms when the scope came in


@registry.register_model("egnn_equihnnm")
class EGNNEquiHNNM(_MTail):
    """equihnn_egnn.py:172-261: mhnnm with the EGNN front-end applied once to the atom embeddings."""
    front = _EGNN


@registry.register_model("faformer_equihnnm")
class FAFormerEquiHNNM(_MTail):
    """equihnn_fa_former.py:187-283: mhnnm with the FAFormer front-end applied once to the atom embeddings.  FAFormer keeps
    its own proj_drop = attn_drop = 0.1 in training mode (fa_former_layer.py:20-21), whatever ``--dropout`` says."""
    front = _FAFORMER


@registry.register_model("visnet_equihnnm")
class VisNetEquiHNNM(_MTail):
    """equihnn_visnet.py:161-243: mhnnm with ViSNet in place of the AtomEncoder."""
    front = _VISNET


from .baseline_2d import GNN_2D  # noqa: E402, F401  (registers gin / gcn; constructed as GNN_2D(1, gnn_type=...))

MODELS = dict(registry.mapping["model_name_mapping"])   # the fourteen above plus gin / gcn
