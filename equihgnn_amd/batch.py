"""Molecular-hypergraph batch container, collate rule and synthetic generator.

The hot path consumes a PyG ``Batch`` of ``HData`` objects
(reference: equihgnn/data/utils.py:150-178).  PyG is not part of this image, so
this module carries the few fields the path reads, with the reference's batching
rule (``HData.__inc__``: ``edge_index0`` is offset by the number of nodes and
``edge_index1`` by ``n_e``, data/utils.py:172-178).  A real PyG ``Batch`` exposes
the same attribute names, so the model classes accept either.

Field layout (all row-major, on one device):
    x           [N, 9]  int64   ogb atom features
    pos         [N, 3]  float32 coordinates
    edge_index0 [nnz]   int64   node id of every incidence
    edge_index1 [nnz]   int64   hyperedge id of every incidence
    edge_attr   [M, 1]  int64   bond type 0-4, 5 = conjugated group
    n_e         [B]     int64   hyperedges per molecule
    e_order     [M]     int64   nodes per hyperedge
    batch       [N]     int64   molecule id per node (sorted)
    y           [B]     float32 regression target

The synthetic generator follows SURVEY.md §8(d): random spanning-tree molecules
with a few ring-closing bonds, at most one conjugated hyperedge, incidences in
the reference's order (data/utils.py:123-145: two incidences per bond, bond
hyperedges first, conjugated-group incidences after, in atom order).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, fields
from typing import List, Optional, Sequence

import numpy as np
import torch

# ogb 1.3.6 full_atom_feature_dims (ogb/utils/features.py), used by AtomEncoder.
ATOM_FEATURE_DIMS = (119, 5, 12, 12, 10, 6, 6, 2, 2)
NUM_BOND_TYPES = 6  # 0-4 bond types + 5 = conjugated hyperedge (data/utils.py:129-145)

# (mean atoms, std, max atoms, P(conjugated hyperedge)) per dataset flavour, SURVEY §8(d)
FLAVOURS = {
    "qm9": (18.0, 3.0, 29, 0.3),
    "pcqm": (30.0, 7.0, 60, 0.8),
}


@dataclass
class HBatch:
    x: torch.Tensor
    pos: torch.Tensor
    edge_index0: torch.Tensor
    edge_index1: torch.Tensor
    edge_attr: torch.Tensor
    n_e: torch.Tensor
    e_order: torch.Tensor
    batch: torch.Tensor
    y: torch.Tensor
    # host-side sizes, kept so the GPU path never needs a device sync to learn them
    num_nodes: int = 0
    num_hyperedges: int = 0
    num_graphs: int = 0

    def to(self, device, non_blocking: bool = False) -> "HBatch":
        flat = getattr(self, "_flat", None)
        if flat is not None:   # packed: ONE transfer, then the same views over the new buffer
            return self._from_flat(flat.to(device, non_blocking=non_blocking), self._layout)
        kw = {}
        for f in fields(self):
            v = getattr(self, f.name)
            kw[f.name] = v.to(device, non_blocking=non_blocking) if torch.is_tensor(v) else v
        out = HBatch(**kw)
        if hasattr(self, "num_real_graphs"):
            out.num_real_graphs = self.num_real_graphs
        return out

    def packed(self) -> "HBatch":
        """The same batch with every tensor field a view into ONE flat byte buffer (256-byte aligned
        slots): host-to-device staging and the refresh of a captured graph's static inputs become a
        single copy instead of one per field."""
        names = [f.name for f in fields(self) if torch.is_tensor(getattr(self, f.name))]
        layout, total = [], 0
        for n in names:
            t = getattr(self, n)
            layout.append((n, total, tuple(t.shape), t.dtype))
            total += (t.numel() * t.element_size() + 255) // 256 * 256
        flat = torch.empty(max(total, 256), dtype=torch.uint8, device=self.x.device)
        out = self._from_flat(flat, tuple(layout))
        for n in names:
            getattr(out, n).copy_(getattr(self, n))
        return out

    @classmethod
    def empty_packed(cls, n_nodes: int, n_hyperedges: int, n_inc: int, n_graphs: int, pin: bool = False,
                     device=None) -> "HBatch":
        """An uninitialised packed host batch of the given extents (one flat buffer, optionally pinned): the staging
        buffer a loader thread collates into and the trainer's static inputs are refreshed from with ONE copy.
        ``device``: the same layout in that device's memory (what a ``DeviceMolStore`` collates into)."""
        spec = (("x", (n_nodes, 9), torch.int64), ("pos", (n_nodes, 3), torch.float32),
                ("edge_index0", (n_inc,), torch.int64), ("edge_index1", (n_inc,), torch.int64),
                ("edge_attr", (n_hyperedges, 1), torch.int64), ("n_e", (n_graphs,), torch.int64),
                ("e_order", (n_hyperedges,), torch.int64), ("batch", (n_nodes,), torch.int64),
                ("y", (n_graphs,), torch.float32))
        layout, total = [], 0
        for name, shape, dtype in spec:
            layout.append((name, total, tuple(shape), dtype))
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
            total += (nbytes + 255) // 256 * 256
        flat = torch.empty(max(total, 256), dtype=torch.uint8, device=device)
        if pin and device is None:
            flat = flat.pin_memory()
        proto = cls(**{name: torch.empty(0) for name, _, _ in spec}, num_nodes=n_nodes, num_hyperedges=n_hyperedges,
                    num_graphs=n_graphs)
        return proto._from_flat(flat, tuple(layout))

    def _from_flat(self, flat, layout) -> "HBatch":
        kw = {f.name: getattr(self, f.name) for f in fields(self) if not torch.is_tensor(getattr(self, f.name))}
        for n, off, shape, dtype in layout:
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
            kw[n] = flat[off:off + nbytes].view(dtype).view(shape)
        out = HBatch(**kw)
        out._flat, out._layout = flat, layout
        if hasattr(self, "num_real_graphs"):
            out.num_real_graphs = self.num_real_graphs
        return out

    def pin_memory(self) -> "HBatch":
        kw = {}
        for f in fields(self):
            v = getattr(self, f.name)
            kw[f.name] = v.pin_memory() if torch.is_tensor(v) else v
        return HBatch(**kw)

    @property
    def nnz(self) -> int:
        return int(self.edge_index0.shape[0])


@dataclass
class HMol:
    """One molecule before batching (the HData fields the path reads)."""

    x: np.ndarray            # [n, 9] int64
    pos: np.ndarray          # [n, 3] float32
    edge_index0: np.ndarray  # [nnz] int64, local node ids
    edge_index1: np.ndarray  # [nnz] int64, local hyperedge ids
    edge_attr: np.ndarray    # [m, 1] int64
    e_order: np.ndarray      # [m] int64
    y: float


def collate(mols: Sequence[HMol]) -> HBatch:
    """PyG ``Batch.from_data_list`` restricted to HData's fields.

    Offsets follow ``HData.__inc__`` (data/utils.py:172-178): node ids shift by the
    running node count, hyperedge ids by the running ``n_e``.
    """
    xs, ps, v, e, ea, eo, bt, ys, ne = [], [], [], [], [], [], [], [], []
    n_off = 0
    m_off = 0
    for b, mol in enumerate(mols):
        n = mol.x.shape[0]
        m = mol.edge_attr.shape[0]
        xs.append(mol.x)
        ps.append(mol.pos)
        v.append(mol.edge_index0 + n_off)
        e.append(mol.edge_index1 + m_off)
        ea.append(mol.edge_attr)
        eo.append(mol.e_order)
        bt.append(np.full((n,), b, dtype=np.int64))
        ys.append(mol.y)
        ne.append(m)
        n_off += n
        m_off += m
    return HBatch(
        x=torch.from_numpy(np.concatenate(xs, 0).astype(np.int64)),
        pos=torch.from_numpy(np.concatenate(ps, 0).astype(np.float32)),
        edge_index0=torch.from_numpy(np.concatenate(v, 0).astype(np.int64)),
        edge_index1=torch.from_numpy(np.concatenate(e, 0).astype(np.int64)),
        edge_attr=torch.from_numpy(np.concatenate(ea, 0).astype(np.int64)),
        n_e=torch.tensor(ne, dtype=torch.int64),
        e_order=torch.from_numpy(np.concatenate(eo, 0).astype(np.int64)),
        batch=torch.from_numpy(np.concatenate(bt, 0)),
        y=torch.tensor(ys, dtype=torch.float32),
        num_nodes=n_off,
        num_hyperedges=m_off,
        num_graphs=len(mols),
    )


class MolStore:
    """A dataset of molecules as a structure of arrays -- the concatenated fields plus per-molecule offsets -- so
    that a batch is assembled by array operations only (numpy gathers driven by ``cumsum`` offsets): no Python loop
    over molecules, which at 256-1024 molecules per batch and > 100 k molecules/s per GPU would be the bottleneck of
    the whole training step (the reference leaves this to PyG's ``Batch.from_data_list``, a per-molecule loop).
    Field semantics as HBatch / HData (data/utils.py:150-178)."""

    def __init__(self, mols: Sequence[HMol]):
        n = np.array([m.x.shape[0] for m in mols], dtype=np.int64)
        h = np.array([m.edge_attr.shape[0] for m in mols], dtype=np.int64)
        z = np.array([m.edge_index0.shape[0] for m in mols], dtype=np.int64)
        off = lambda c: np.concatenate(([0], np.cumsum(c)))
        self.n_nodes, self.n_he, self.n_inc = n, h, z
        self.node_off, self.he_off, self.inc_off = off(n), off(h), off(z)
        cat = lambda xs, dt, shape: (np.concatenate(xs, 0).astype(dt) if len(xs) else np.zeros(shape, dt))
        self.x = cat([m.x for m in mols], np.int64, (0, 9))
        self.pos = cat([m.pos for m in mols], np.float32, (0, 3))
        self.v = cat([m.edge_index0 for m in mols], np.int64, (0,))          # local node ids
        self.e = cat([m.edge_index1 for m in mols], np.int64, (0,))          # local hyperedge ids
        self.edge_attr = cat([m.edge_attr for m in mols], np.int64, (0, 1))
        self.e_order = cat([m.e_order for m in mols], np.int64, (0,))
        self.y = np.array([m.y for m in mols], dtype=np.float32)

    def __len__(self) -> int:
        return int(self.n_nodes.shape[0])

    def extents(self, idx) -> tuple:
        """(nodes, hyperedges, incidences) of the batch made of molecules ``idx``."""
        idx = np.asarray(idx, dtype=np.int64)
        return int(self.n_nodes[idx].sum()), int(self.n_he[idx].sum()), int(self.n_inc[idx].sum())

    # what fit.BucketedLoader asks a store for (GraphStore answers with two extents instead of three)
    SPARE = (1, 1, 1)                   # slots a padded batch needs beyond its molecules' (the padding molecule's own)

    def count_columns(self) -> tuple:
        """Per-molecule counts, one array per extent of a batch."""
        return self.n_nodes, self.n_he, self.n_inc

    @staticmethod
    def bucket(ext, quantum: int) -> tuple:
        """The static extents of the bucket that holds a batch of extents ``ext``."""
        return bucket_sizes(ext[0], ext[1], ext[2], quantum)

    @staticmethod
    def ladder_step(quantum: int) -> tuple:
        """Distance between neighbouring rungs of the loader's bucket ladder, per extent."""
        return quantum, quantum, 2 * quantum

    def empty_staging(self, tgt, n_graphs: int, pin: bool = False) -> "HBatch":
        """An empty packed staging batch of extents ``tgt`` for ``collate(out=...)``."""
        return HBatch.empty_packed(tgt[0], tgt[1], tgt[2], n_graphs, pin=pin)

    def to_device(self, device) -> "DeviceMolStore":
        """The store in ``device``'s memory: uploaded once, batches assembled there by two kernel launches
        (``DeviceMolStore``).  A CPU device raises ``HipLibraryError``: there is no fallback."""
        return DeviceMolStore(self, device)

    @staticmethod
    def _ranges(starts, counts):
        """Concatenation of arange(starts[i], starts[i] + counts[i]) and the owner i of every element."""
        total = int(counts.sum())
        owner = np.repeat(np.arange(counts.shape[0], dtype=np.int64), counts)
        first = np.concatenate(([0], np.cumsum(counts)[:-1]))
        return starts[owner] + (np.arange(total, dtype=np.int64) - first[owner]), owner

    def collate(self, idx, pad_to: Optional[tuple] = None, out: Optional["HBatch"] = None) -> "HBatch":
        """The batch of molecules ``idx`` (HData.__inc__ offsets, data/utils.py:172-178), optionally padded to the
        static extents ``pad_to`` = (nodes, hyperedges, incidences) exactly as ``pad_batch`` does (one dummy molecule
        owns the padding, padded incidences are null), optionally written into the tensors of ``out`` (a packed,
        pinned staging batch of those extents).

        Assembled by the library's host-side ``hb_collate`` (csrc/collate.hip: a molecule's rows are contiguous in the
        store, so a batch is a few memcpy's per molecule): ~25 us for a 256-molecule QM9 batch, against ~1.2 ms for the
        numpy gathers of ``collate_numpy`` (kept as the restatement the tests compare it with, bit for bit)."""
        from . import hip
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        B = idx.shape[0]
        if B and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError("collate: molecule index outside the store")
        n_tot, h_tot, z_tot = self.extents(idx) if (pad_to is None or out is None) else (None, None, None)
        if pad_to is None:
            PN, PM, PZ, PB = n_tot, h_tot, z_tot, B
        else:
            PN, PM, PZ = (int(v) for v in pad_to)
            PB = B + 1
        if out is None:
            t = lambda shape, dt: torch.empty(shape, dtype=dt)
            out = HBatch(x=t((PN, 9), torch.int64), pos=t((PN, 3), torch.float32), edge_index0=t((PZ,), torch.int64),
                         edge_index1=t((PZ,), torch.int64), edge_attr=t((PM, 1), torch.int64), n_e=t((PB,), torch.int64),
                         e_order=t((PM,), torch.int64), batch=t((PN,), torch.int64), y=t((PB,), torch.float32))
        a = hip.HbCollate()
        a.B, a.n_mols, a.idx = B, len(self), idx.ctypes.data
        for name, ptr in self._checked_pointers().items():
            setattr(a, name, ptr)
        a.PN, a.PM, a.PZ, a.padded = PN, PM, PZ, 0 if pad_to is None else 1
        shapes = dict(x=(PN, 9), pos=(PN, 3), edge_index0=(PZ,), edge_index1=(PZ,), edge_attr=(PM, 1), n_e=(PB,), e_order=(PM,),
                      batch=(PN,), y=(PB,))
        for name, shp in shapes.items():
            ten = getattr(out, name)
            want = torch.float32 if name in ("pos", "y") else torch.int64
            if tuple(ten.shape) != shp or ten.dtype != want or not ten.is_contiguous() or ten.device.type != "cpu":
                raise ValueError(f"collate: out.{name} must be a contiguous CPU {want} tensor of shape {shp}")
            setattr(a, "out_" + name, ten.data_ptr())
        counts = np.zeros(3, dtype=np.int64)
        a.out_counts = counts.ctypes.data
        rc = hip.lib().hb_collate(ctypes.byref(a))
        if rc == hip.EQH_ERR_RANGE and pad_to is not None:       # the extents do not fit (indices were checked above)
            raise ValueError("collate: pad_to must exceed the batch (nodes and hyperedges strictly)")
        hip.check(rc, "hb_collate")
        if pad_to is not None:
            out.num_real_graphs = B
        out.num_nodes, out.num_hyperedges, out.num_graphs = PN, PM, PB
        return out

    _ARRAYS = ("node_off", "he_off", "inc_off", "x", "pos", "v", "e", "edge_attr", "e_order", "y")

    def _checked_pointers(self) -> dict:
        """Addresses of the store's arrays for ``hb_collate``, which memcpy's whole rows by them: a store whose arrays have
        another dtype, width or length (a processed file with a different feature layout re-seated into a MolStore by hand)
        must fail HERE, not read the wrong rows or run past the end.  Checked once per set of array objects."""
        key = tuple(id(getattr(self, n)) for n in self._ARRAYS)
        cached = getattr(self, "_ptr_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        n_mols = len(self)
        for name in ("node_off", "he_off", "inc_off"):
            arr = getattr(self, name)
            if arr.dtype != np.int64 or arr.shape != (n_mols + 1,) or not arr.flags.c_contiguous:
                raise ValueError(f"MolStore.{name} must be a C-contiguous int64 array of {n_mols + 1} offsets")
        N, M, Z = int(self.node_off[-1]), int(self.he_off[-1]), int(self.inc_off[-1])
        want = dict(x=(np.int64, (N, 9)), pos=(np.float32, (N, 3)), v=(np.int64, (Z,)), e=(np.int64, (Z,)),
                    edge_attr=(np.int64, (M, 1)), e_order=(np.int64, (M,)), y=(np.float32, (n_mols,)))
        ptrs = {}
        for name in self._ARRAYS:
            arr = getattr(self, name)
            if name in want:
                dt, shape = want[name]
                if arr.dtype != dt or tuple(arr.shape) != shape or not arr.flags.c_contiguous:
                    raise ValueError(f"MolStore.{name} must be a C-contiguous {np.dtype(dt).name} array of shape {shape}, got "
                                     f"{arr.dtype} {tuple(arr.shape)}{'' if arr.flags.c_contiguous else ' (strided)'}")
            ptrs[name] = arr.ctypes.data if arr.size else None
        self._ptr_cache = (key, ptrs)
        return ptrs

    def collate_numpy(self, idx, pad_to: Optional[tuple] = None, out: Optional["HBatch"] = None) -> "HBatch":
        """``collate`` by numpy gathers driven by cumsum offsets (rounds 2-4's implementation; the restatement
        tests/test_fit.py compares the native assembly with)."""
        idx = np.asarray(idx, dtype=np.int64)
        B = idx.shape[0]
        n, h, z = self.n_nodes[idx], self.n_he[idx], self.n_inc[idx]
        src_n, own_n = self._ranges(self.node_off[idx], n)
        src_h, _ = self._ranges(self.he_off[idx], h)
        src_z, own_z = self._ranges(self.inc_off[idx], z)
        N, M, Z = src_n.shape[0], src_h.shape[0], src_z.shape[0]
        node_base = np.concatenate(([0], np.cumsum(n)[:-1]))
        he_base = np.concatenate(([0], np.cumsum(h)[:-1]))
        if pad_to is None:
            PN, PM, PZ, PB = N, M, Z, B
        else:
            PN, PM, PZ = (int(v) for v in pad_to)
            PB = B + 1
            if PN <= N or PM <= M or PZ < Z:
                raise ValueError("collate: pad_to must exceed the batch (nodes and hyperedges strictly)")
        if out is None:
            t = lambda shape, dt: torch.empty(shape, dtype=dt)
            out = HBatch(x=t((PN, 9), torch.int64), pos=t((PN, 3), torch.float32), edge_index0=t((PZ,), torch.int64),
                         edge_index1=t((PZ,), torch.int64), edge_attr=t((PM, 1), torch.int64), n_e=t((PB,), torch.int64),
                         e_order=t((PM,), torch.int64), batch=t((PN,), torch.int64), y=t((PB,), torch.float32))
        a = lambda name: getattr(out, name).numpy()
        a("x")[:N] = self.x[src_n]
        a("pos")[:N] = self.pos[src_n]
        a("batch")[:N] = own_n
        a("edge_index0")[:Z] = self.v[src_z] + node_base[own_z]
        a("edge_index1")[:Z] = self.e[src_z] + he_base[own_z]
        a("edge_attr")[:M] = self.edge_attr[src_h]
        a("e_order")[:M] = self.e_order[src_h]
        a("n_e")[:B] = h
        a("y")[:B] = self.y[idx]
        if pad_to is not None:
            pn = PN - N
            a("x")[N:] = 0
            far = a("pos")[N:]
            far[:] = 0.0
            far[:, 0] = 1.0e4 + 10.0 * np.arange(pn, dtype=np.float32)      # as pad_batch: 10 A apart, 10^4 A away
            a("batch")[N:] = B
            a("edge_index0")[Z:] = -1
            a("edge_index1")[Z:] = -1
            a("edge_attr")[M:] = 0
            a("e_order")[M:] = 0
            a("n_e")[B] = PM - M
            a("y")[B] = 0.0
            out.num_real_graphs = B
        out.num_nodes, out.num_hyperedges, out.num_graphs = PN, PM, PB
        return out


def bucket_sizes(n_nodes: int, n_hyperedges: int, n_inc: int, quantum: int = 128):
    """Static shapes for hipGraph replay: round each extent up to a multiple of ``quantum`` with
    at least one spare slot (the padding molecule needs a node and a hyperedge of its own).  The quantum
    trades padded rows (every kernel and GEMM of the step works on them: 128 is <= 2.8 % of a 256-molecule
    QM9 batch) against the number of distinct shape buckets, each of which is captured once (~0.3 s)."""
    up = lambda v: -(-(v + 1) // quantum) * quantum
    return up(n_nodes), up(n_hyperedges), up(n_inc)


def pad_batch(b: HBatch, n_nodes: int, n_hyperedges: int, n_inc: int) -> HBatch:
    """Pad a batch to fixed extents with ONE extra dummy molecule (graph id B) that owns every
    padded node and hyperedge.  Padded atoms sit 10 A apart on a line 10^4 A away, so no real atom
    ever selects one as a neighbour (each real atom has >= 16 real candidates) and the 5 A radius mask
    drops them; padded rows never mix with real rows in any aggregation, and the loss is taken over the
    first B outputs only — real-molecule outputs and all parameter gradients are unchanged for models
    without batch statistics (LayerNorm models: egnn_equihnns, equiformer_equihnns).

    Padded INCIDENCES are null: both coordinates are -1, which the CSR builders drop (out-of-range keys),
    so no aggregation ever visits them and the padded nodes / hyperedges have no incidences at all.
    (Spreading them over the few padded rows instead gave those rows 20-40 incidences each against 2-3
    for real rows, and the wavefront that owned them ran 10x longer than the rest of the launch: 112 us
    for a backward kernel that needs 10.)  `HyperIndex` keeps them at -1 in its int32 gather copies, which the row-gather
    kernel reads as zero rows (zero gradient for null incidences on the unfused per-incidence path too)."""
    N, M, nnz, B = b.x.shape[0], b.edge_attr.shape[0], b.edge_index0.shape[0], b.y.shape[0]
    if n_nodes <= N or n_hyperedges <= M or n_inc < nnz:
        raise ValueError("pad_batch: target extents must exceed the batch (nodes and hyperedges strictly)")
    dev = b.x.device
    pn, pm, pz = n_nodes - N, n_hyperedges - M, n_inc - nnz
    far = torch.zeros((pn, 3), dtype=b.pos.dtype, device=dev)
    far[:, 0] = 1.0e4 + 10.0 * torch.arange(pn, device=dev, dtype=b.pos.dtype)
    cat = torch.cat
    zl = lambda n, like: torch.zeros((n, *like.shape[1:]), dtype=like.dtype, device=dev)
    iv = torch.full((pz,), -1, device=dev)
    ie = torch.full((pz,), -1, device=dev)
    out = HBatch(
        x=cat((b.x, zl(pn, b.x))), pos=cat((b.pos, far)),
        edge_index0=cat((b.edge_index0, iv.to(b.edge_index0.dtype))),
        edge_index1=cat((b.edge_index1, ie.to(b.edge_index1.dtype))),
        edge_attr=cat((b.edge_attr, zl(pm, b.edge_attr))),
        n_e=cat((b.n_e, torch.tensor([pm], dtype=b.n_e.dtype, device=dev))),
        e_order=cat((b.e_order, zl(pm, b.e_order))),
        batch=cat((b.batch, torch.full((pn,), B, dtype=b.batch.dtype, device=dev))),
        y=cat((b.y, zl(1, b.y))),
        num_nodes=n_nodes, num_hyperedges=n_hyperedges, num_graphs=B + 1)
    out.num_real_graphs = B
    return out


def synth_molecule(rng: np.random.Generator, flavour: str = "qm9",
                   n_atoms: Optional[int] = None, force_conj: Optional[bool] = None) -> HMol:
    mu, sigma, n_max, p_conj = FLAVOURS[flavour]
    if n_atoms is None:
        n = int(np.clip(np.rint(rng.normal(mu, sigma)), 3, n_max))
    else:
        n = int(n_atoms)
    x = np.stack([rng.integers(0, d, size=n) for d in ATOM_FEATURE_DIMS], axis=1).astype(np.int64)

    # bonds: random spanning tree + a few ring-closing bonds
    bonds = []
    parent = np.zeros(n, dtype=np.int64)
    for a in range(1, n):
        p = int(rng.integers(0, a))
        parent[a] = p
        bonds.append((p, a))
    have = set(bonds)
    for _ in range(int(np.rint(0.08 * n))):
        a, b = sorted(int(t) for t in rng.choice(n, size=2, replace=False))
        if (a, b) not in have:
            have.add((a, b))
            bonds.append((a, b))
    nb = len(bonds)
    v = np.empty(2 * nb, dtype=np.int64)
    e = np.empty(2 * nb, dtype=np.int64)
    for i, (a, b) in enumerate(bonds):
        v[2 * i], v[2 * i + 1] = a, b
        e[2 * i] = e[2 * i + 1] = i
    edge_attr = rng.integers(0, 4, size=(nb, 1)).astype(np.int64)
    e_order = np.full((nb,), 2, dtype=np.int64)

    conj = (rng.random() < p_conj) if force_conj is None else force_conj
    if conj and n >= 3:
        k = int(rng.integers(3, min(8, n) + 1))
        v = np.concatenate([v, np.arange(k, dtype=np.int64)])
        e = np.concatenate([e, np.full((k,), nb, dtype=np.int64)])
        edge_attr = np.concatenate([edge_attr, np.full((1, 1), 5, dtype=np.int64)], 0)
        e_order = np.concatenate([e_order, np.array([k], dtype=np.int64)])

    # coordinates: chain growth along the spanning tree, then centred
    pos = np.zeros((n, 3), dtype=np.float64)
    for a in range(1, n):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        # bond length 1.4 A +- 0.1: a constant length would make the squared distances of all
        # bonded pairs EXACTLY equal in fp32, and torch.topk's choice among exact ties at the
        # k-th neighbour is implementation-defined (see tests: test_knn_ties_prefer_lower_index)
        pos[a] = pos[parent[a]] + (1.4 + 0.1 * rng.uniform(-1.0, 1.0)) * u
    pos -= pos.mean(0, keepdims=True)
    return HMol(x=x, pos=pos.astype(np.float32), edge_index0=v, edge_index1=e,
                edge_attr=edge_attr, e_order=e_order, y=float(rng.normal()))


def synth_batch(batch_size: int, seed: int, flavour: str = "qm9") -> HBatch:
    """Seeded synthetic batch.  Pure host code, deterministic per seed."""
    rng = np.random.default_rng(seed)
    return collate([synth_molecule(rng, flavour) for _ in range(batch_size)])


def shard_indices(n_items: int, rank: int, world_size: int, seed: int, epoch: int = 0,
                  shuffle: bool = True) -> List[int]:
    """DistributedSampler semantics (the Lightning default the reference relies on,
    main.py:271-283): a shared shuffled permutation, padded to a multiple of the world
    size, strided by rank."""
    return shard_permutation(n_items, world_size, seed, epoch, shuffle)[rank::world_size].tolist()


def shard_permutation(n_items: int, world_size: int, seed: int, epoch: int = 0, shuffle: bool = True) -> np.ndarray:
    """The epoch's shared permutation, padded to a multiple of the world size: rank r's shard is ``[r::world_size]``
    (every rank can therefore see what every other rank will draw -- ``fit.BucketedLoader.plan``)."""
    perm = np.random.default_rng(seed + epoch).permutation(n_items) if shuffle else np.arange(n_items)
    total = -(-n_items // world_size) * world_size
    reps = -(-total // max(n_items, 1))
    return np.concatenate([perm] * reps)[:total] if total > n_items else perm


# ------------------------------------------------------------------------------------------------------------------
# 2-D molecular graphs (the baselines of baseline_2d.py: PyG ``Data(x, edge_index, edge_attr, y)``, ogb mol2graph)
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class GBatch:
    """A PyG ``Batch`` of 2-D molecular graphs with the fields GNN_2D reads:
        x          [N, 9]  int64   ogb atom features
        edge_index [2, E]  int64   (source, target) per directed edge, node ids offset per molecule
        edge_attr  [E, F]  int64   ogb bond features (F = 3: type, stereo, conjugated; qm9_g keeps the type only)
        batch      [N]     int64   molecule id per atom (sorted)
        y          [B]     float32 regression target"""
    x: torch.Tensor
    edge_index: torch.Tensor
    edge_attr: torch.Tensor
    batch: torch.Tensor
    y: torch.Tensor
    num_nodes: int = 0
    num_edges: int = 0
    num_graphs: int = 0

    def to(self, device, non_blocking: bool = False) -> "GBatch":
        flat = getattr(self, "_flat", None)
        if flat is not None:   # packed: ONE transfer, then the same views over the new buffer
            return self._from_flat(flat.to(device, non_blocking=non_blocking), self._layout)
        kw = {}
        for f in fields(self):
            v = getattr(self, f.name)
            kw[f.name] = v.to(device, non_blocking=non_blocking) if torch.is_tensor(v) else v
        out = GBatch(**kw)
        if hasattr(self, "num_real_graphs"):
            out.num_real_graphs = self.num_real_graphs
        return out

    @staticmethod
    def _plan(spec):
        """(layout, bytes) of the tensors ``spec`` = ((name, shape, dtype), ...) in one flat buffer, 256-byte aligned slots"""
        layout, total = [], 0
        for name, shape, dtype in spec:
            layout.append((name, total, tuple(shape), dtype))
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
            total += (nbytes + 255) // 256 * 256
        return tuple(layout), max(total, 256)

    def packed(self) -> "GBatch":
        """The same batch with every tensor field a view into ONE flat byte buffer (256-byte aligned slots), as
        ``HBatch.packed``: host-to-device staging and the refresh of a captured graph's static inputs are one copy."""
        names = [f.name for f in fields(self) if torch.is_tensor(getattr(self, f.name))]
        layout, total = self._plan([(n, getattr(self, n).shape, getattr(self, n).dtype) for n in names])
        out = self._from_flat(torch.empty(total, dtype=torch.uint8, device=self.x.device), layout)
        for n in names:
            getattr(out, n).copy_(getattr(self, n))
        return out

    @classmethod
    def empty_packed(cls, n_nodes: int, n_edges: int, n_bond_features: int, n_graphs: int, pin: bool = False,
                     device=None) -> "GBatch":
        """An uninitialised packed host batch of the given extents (one flat buffer, optionally pinned): the staging buffer
        a loader thread collates into (``GraphStore.collate(out=...)``).  ``device``: the same layout in that device's
        memory (what a ``DeviceGraphStore`` collates into)."""
        spec = (("x", (n_nodes, 9), torch.int64), ("edge_index", (2, n_edges), torch.int64),
                ("edge_attr", (n_edges, n_bond_features), torch.int64), ("batch", (n_nodes,), torch.int64),
                ("y", (n_graphs,), torch.float32))
        layout, total = cls._plan(spec)
        flat = torch.empty(total, dtype=torch.uint8, device=device)
        if pin and device is None:
            flat = flat.pin_memory()
        proto = cls(**{name: torch.empty(0) for name, _, _ in spec}, num_nodes=n_nodes, num_edges=n_edges, num_graphs=n_graphs)
        return proto._from_flat(flat, layout)

    def _from_flat(self, flat, layout) -> "GBatch":
        kw = {f.name: getattr(self, f.name) for f in fields(self) if not torch.is_tensor(getattr(self, f.name))}
        for n, off, shape, dtype in layout:
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
            kw[n] = flat[off:off + nbytes].view(dtype).view(shape)
        out = GBatch(**kw)
        out._flat, out._layout = flat, layout
        if hasattr(self, "num_real_graphs"):
            out.num_real_graphs = self.num_real_graphs
        return out


@dataclass
class GMol:
    x: np.ndarray            # [n, 9] int64
    edge_index: np.ndarray   # [2, e] int64, local atom ids
    edge_attr: np.ndarray    # [e, F] int64
    y: float


def collate_graphs(mols: Sequence[GMol]) -> GBatch:
    """PyG ``Batch.from_data_list``: edge_index offset by the atoms of the molecules before, ``batch`` = molecule id."""
    n = np.array([m.x.shape[0] for m in mols], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    F = mols[0].edge_attr.shape[1] if mols else 1
    x = np.concatenate([m.x for m in mols], 0) if mols else np.zeros((0, 9), np.int64)
    ei = np.concatenate([m.edge_index + s for m, s in zip(mols, start)], 1) if mols else np.zeros((2, 0), np.int64)
    ea = np.concatenate([m.edge_attr.reshape(-1, F) for m in mols], 0) if mols else np.zeros((0, F), np.int64)
    batch = np.repeat(np.arange(len(mols), dtype=np.int64), n)
    y = np.array([m.y for m in mols], dtype=np.float32)
    t = torch.from_numpy
    return GBatch(x=t(np.ascontiguousarray(x, np.int64)), edge_index=t(np.ascontiguousarray(ei, np.int64)),
                  edge_attr=t(np.ascontiguousarray(ea, np.int64)), batch=t(batch), y=t(y), num_nodes=int(x.shape[0]),
                  num_edges=int(ei.shape[1]), num_graphs=len(mols))


class GraphStore:
    """A dataset of 2-D molecules (the reference's ``*_g`` datasets) as a structure of arrays, the counterpart of
    ``MolStore``: the concatenated fields plus per-molecule offsets, so that a batch is assembled without a Python loop over
    molecules (the library's host-side ``gb_collate``).  Field semantics as GBatch / PyG ``Data``; ``src`` / ``dst`` are
    the two rows of ``edge_index`` with atom ids LOCAL to their molecule; all molecules share one bond-feature width F."""

    def __init__(self, mols: Sequence[GMol]):
        mols = list(mols)
        widths = {int(m.edge_attr.shape[1]) if m.edge_attr.ndim == 2 else 1 for m in mols}
        if len(widths) > 1:
            raise ValueError(f"GraphStore: the molecules disagree on the number of bond features: {sorted(widths)}")
        F = widths.pop() if widths else 1
        cat = lambda xs, dt, shape, ax=0: (np.ascontiguousarray(np.concatenate(xs, ax), dtype=dt) if len(xs)
                                           else np.zeros(shape, dt))
        ei = cat([m.edge_index.reshape(2, -1) for m in mols], np.int64, (2, 0), 1)
        self._seat(n_nodes=np.array([m.x.shape[0] for m in mols], dtype=np.int64),
                   n_edges=np.array([m.edge_index.shape[1] for m in mols], dtype=np.int64),
                   x=cat([m.x for m in mols], np.int64, (0, 9)), src=np.ascontiguousarray(ei[0]),
                   dst=np.ascontiguousarray(ei[1]), edge_attr=cat([m.edge_attr.reshape(-1, F) for m in mols], np.int64, (0, F)),
                   y=np.array([m.y for m in mols], dtype=np.float32), F=F)

    @classmethod
    def from_arrays(cls, n_nodes, n_edges, x, src, dst, edge_attr, y) -> "GraphStore":
        """A store over arrays that are already concatenated (a processed dataset file: reader.read_processed_graph):
        per-molecule counts, x [N, 9], local src / dst [E], edge_attr [E, F], y [n_mols].  Arrays of the right dtype and
        layout are kept as they are, not copied."""
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        edge_attr = c(edge_attr, np.int64)
        if edge_attr.ndim != 2:
            raise ValueError("GraphStore: edge_attr must be [E, F]")
        st = cls.__new__(cls)
        st._seat(n_nodes=c(n_nodes, np.int64), n_edges=c(n_edges, np.int64), x=c(x, np.int64), src=c(src, np.int64),
                 dst=c(dst, np.int64), edge_attr=edge_attr, y=c(y, np.float32), F=int(edge_attr.shape[1]))
        st._checked_pointers()
        return st

    def subset(self, idx) -> "GraphStore":
        """The store of molecules ``idx`` (a train / valid / test split), by array gathers."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError("subset: molecule index outside the store")
        rows = lambda off, cnt: MolStore._ranges(off[idx], cnt[idx])[0]
        a, e = rows(self.node_off, self.n_nodes), rows(self.edge_off, self.n_edges)
        return GraphStore.from_arrays(self.n_nodes[idx], self.n_edges[idx], self.x[a], self.src[e], self.dst[e],
                                      self.edge_attr[e], self.y[idx])

    def _seat(self, n_nodes, n_edges, x, src, dst, edge_attr, y, F):
        off = lambda c: np.concatenate(([0], np.cumsum(c))).astype(np.int64)
        self.n_nodes, self.n_edges = n_nodes, n_edges
        self.node_off, self.edge_off = off(n_nodes), off(n_edges)
        self.x, self.src, self.dst, self.edge_attr, self.y, self.F = x, src, dst, edge_attr, y, F

    def __len__(self) -> int:
        return int(self.n_nodes.shape[0])

    def extents(self, idx) -> tuple:
        """(atoms, edges) of the batch made of molecules ``idx``."""
        idx = np.asarray(idx, dtype=np.int64)
        return int(self.n_nodes[idx].sum()), int(self.n_edges[idx].sum())

    # what fit.BucketedLoader asks a store for (MolStore answers with three extents, this one with two)
    SPARE = (1, 0)                      # slots a padded batch needs beyond its molecules': the padding molecule's atom

    def count_columns(self) -> tuple:
        return self.n_nodes, self.n_edges

    @staticmethod
    def bucket(ext, quantum: int) -> tuple:
        return graph_bucket_sizes(ext[0], ext[1], quantum)

    @staticmethod
    def ladder_step(quantum: int) -> tuple:
        return quantum, 2 * quantum

    def empty_staging(self, tgt, n_graphs: int, pin: bool = False) -> "GBatch":
        return GBatch.empty_packed(tgt[0], tgt[1], self.F, n_graphs, pin=pin)

    def to_device(self, device) -> "DeviceGraphStore":
        """The store in ``device``'s memory (``DeviceGraphStore``).  A CPU device raises ``HipLibraryError``."""
        return DeviceGraphStore(self, device)

    def collate(self, idx, pad_to: Optional[tuple] = None, out: Optional["GBatch"] = None) -> "GBatch":
        """The batch of molecules ``idx`` (what ``collate_graphs`` returns for them), optionally padded to the static
        extents ``pad_to`` = (atoms, edges) exactly as ``pad_graph_batch`` does, optionally written into the tensors of
        ``out`` (a packed, pinned staging batch of those extents).  Assembled by the library's host-side ``gb_collate``
        (csrc/collate.hip); ``collate_graphs`` + ``pad_graph_batch`` are the restatement the tests compare it with, bit
        for bit."""
        from . import hip
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        B, F = idx.shape[0], self.F
        if B and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError("collate: molecule index outside the store")
        if pad_to is None:
            PN, PE = self.extents(idx)
            PB = B
        else:
            PN, PE = (int(v) for v in pad_to)
            PB = B + 1
        if out is None:
            t = lambda shape, dt: torch.empty(shape, dtype=dt)
            out = GBatch(x=t((PN, 9), torch.int64), edge_index=t((2, PE), torch.int64), edge_attr=t((PE, F), torch.int64),
                         batch=t((PN,), torch.int64), y=t((PB,), torch.float32))
        a = hip.GbCollate()
        a.B, a.n_mols, a.idx = B, len(self), idx.ctypes.data
        for name, ptr in self._checked_pointers().items():
            setattr(a, name, ptr)
        a.F, a.PN, a.PE, a.padded = F, PN, PE, 0 if pad_to is None else 1
        shapes = dict(x=(PN, 9), edge_index=(2, PE), edge_attr=(PE, F), batch=(PN,), y=(PB,))
        for name, shp in shapes.items():
            ten = getattr(out, name)
            want = torch.float32 if name == "y" else torch.int64
            if tuple(ten.shape) != shp or ten.dtype != want or not ten.is_contiguous() or ten.device.type != "cpu":
                raise ValueError(f"collate: out.{name} must be a contiguous CPU {want} tensor of shape {shp}")
            setattr(a, "out_" + name, ten.data_ptr())
        counts = np.zeros(2, dtype=np.int64)
        a.out_counts = counts.ctypes.data
        rc = hip.lib().gb_collate(ctypes.byref(a))
        if rc == hip.EQH_ERR_RANGE and pad_to is not None:       # the extents do not fit (indices were checked above)
            raise ValueError("collate: pad_to must exceed the batch (atoms strictly)")
        hip.check(rc, "gb_collate")
        if pad_to is not None:
            out.num_real_graphs = B
        out.num_nodes, out.num_edges, out.num_graphs = PN, PE, PB
        return out

    _ARRAYS = ("node_off", "edge_off", "x", "src", "dst", "edge_attr", "y")

    def _checked_pointers(self) -> dict:
        """Addresses of the store's arrays for ``gb_collate``, which copies whole rows by them: arrays of another dtype,
        width or length must fail HERE, not read the wrong rows or run past the end.  Checked once per set of array
        objects (and bond-feature width)."""
        key = tuple(id(getattr(self, n)) for n in self._ARRAYS) + (self.F,)
        cached = getattr(self, "_ptr_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        n_mols = len(self)
        for name in ("node_off", "edge_off"):
            arr = getattr(self, name)
            if arr.dtype != np.int64 or arr.shape != (n_mols + 1,) or not arr.flags.c_contiguous:
                raise ValueError(f"GraphStore.{name} must be a C-contiguous int64 array of {n_mols + 1} offsets")
            if int(arr[0]) != 0 or (n_mols and int(np.diff(arr).min()) < 0):
                raise ValueError(f"GraphStore.{name} must start at 0 and not decrease")
        N, E = int(self.node_off[-1]), int(self.edge_off[-1])
        want = dict(x=(np.int64, (N, 9)), src=(np.int64, (E,)), dst=(np.int64, (E,)), edge_attr=(np.int64, (E, int(self.F))),
                    y=(np.float32, (n_mols,)))
        ptrs = {}
        for name in self._ARRAYS:
            arr = getattr(self, name)
            if name in want:
                dt, shape = want[name]
                if arr.dtype != dt or tuple(arr.shape) != shape or not arr.flags.c_contiguous:
                    raise ValueError(f"GraphStore.{name} must be a C-contiguous {np.dtype(dt).name} array of shape {shape}, got "
                                     f"{arr.dtype} {tuple(arr.shape)}{'' if arr.flags.c_contiguous else ' (strided)'}")
            ptrs[name] = arr.ctypes.data if arr.size else None
        self._ptr_cache = (key, ptrs)
        return ptrs


# ------------------------------------------------------------------------------------------------------------------
# device-resident stores: the dataset uploaded once, batches assembled by two kernel launches (csrc/collate_dev.hip)
# ------------------------------------------------------------------------------------------------------------------
class _DeviceStore:
    """What ``DeviceMolStore`` and ``DeviceGraphStore`` share.  The store's arrays are device tensors of the host store's
    dtypes (the offsets too: the kernels index the arrays by them); the per-molecule counts and offsets ALSO stay on the host
    as numpy arrays, so ``extents`` / ``count_columns`` -- all ``fit.BucketedLoader.plan`` asks -- never touch the device.
    ``collate`` enqueues ``hb_collate_dev`` / ``gb_collate_dev`` on the current stream: no allocation beyond the output (none
    with ``out``), no synchronisation, no host read."""

    _COLUMNS: tuple = ()     # ((count name, offset name), ...): one per extent of a batch
    _ROWS: dict = {}         # array name -> the column whose offsets index its rows
    _HOST = None             # the host store class (its bucket / ladder / SPARE rules are this one's)
    _MIN_SPARE: tuple = ()   # rows a padded extent needs beyond the batch's own (hb_collate's "must exceed" rule)

    def __init__(self, host, device):
        from . import hip
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.HipLibraryError(f"{type(host).__name__}.to_device({str(device)!r}): a device store lives in the memory "
                                      "of an MI355X (HIP) device and is collated by its kernels; there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        host._checked_pointers()                 # dtypes, widths and lengths against the offsets, once, before the upload
        for _, off in self._COLUMNS:             # the kernels index the arrays by the offsets: they must not run backwards
            arr = getattr(host, off)
            if int(arr[0]) != 0 or (len(host) and int(np.diff(arr).min()) < 0):
                raise ValueError(f"{type(host).__name__}.{off} must start at 0 and not decrease")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self._seat_device(device, {c: np.ascontiguousarray(getattr(host, c)) for c, _ in self._COLUMNS},
                          {n: up(getattr(host, n)) for n in (*self._ROWS, "y")})

    def _seat_device(self, device, counts: dict, tensors: dict):
        self.device = device
        for (cname, oname) in self._COLUMNS:
            c = counts[cname]
            setattr(self, cname, c)
            setattr(self, oname, np.concatenate(([0], np.cumsum(c))).astype(np.int64))
        self._offsets = torch.from_numpy(np.stack([getattr(self, o) for _, o in self._COLUMNS])).to(device)
        for name, t in tensors.items():
            setattr(self, name, t)

    def __len__(self) -> int:
        return int(getattr(self, self._COLUMNS[0][0]).shape[0])

    def extents(self, idx) -> tuple:
        idx = np.asarray(idx, dtype=np.int64)
        return tuple(int(getattr(self, c)[idx].sum()) for c, _ in self._COLUMNS)

    def count_columns(self) -> tuple:
        return tuple(getattr(self, c) for c, _ in self._COLUMNS)

    def bucket(self, ext, quantum: int) -> tuple:
        return self._HOST.bucket(ext, quantum)

    def ladder_step(self, quantum: int) -> tuple:
        return self._HOST.ladder_step(quantum)

    @property
    def SPARE(self) -> tuple:
        return self._HOST.SPARE

    def subset(self, idx):
        """The device store of molecules ``idx`` (a train / valid / test split): the rows are chosen on the host from the
        offsets and gathered on the device."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError("subset: molecule index outside the store")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.device)
        rows = [up(MolStore._ranges(getattr(self, o)[idx], getattr(self, c)[idx])[0]) for c, o in self._COLUMNS]
        st = type(self).__new__(type(self))
        if hasattr(self, "F"):
            st.F = self.F
        tensors = {n: getattr(self, n).index_select(0, rows[col]) for n, col in self._ROWS.items()}
        tensors["y"] = self.y.index_select(0, up(idx))
        st._seat_device(self.device, {c: np.ascontiguousarray(getattr(self, c)[idx]) for c, _ in self._COLUMNS}, tensors)
        torch.cuda.current_stream(self.device).synchronize()    # (a loader collates on a stream of its own: gathers done first)
        return st

    def _index(self, idx):
        """(device int64 [B], host array or None) of a batch's molecule indices: a host array is range-checked and uploaded, a
        device tensor is trusted (callers pass slices of a permutation the host built)."""
        if torch.is_tensor(idx) and idx.is_cuda:
            if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous() or idx.device != self.device:
                raise ValueError(f"collate: a device index must be a contiguous int64 vector on {self.device}")
            return idx, None
        host = np.ascontiguousarray(idx.numpy() if torch.is_tensor(idx) else idx, dtype=np.int64).reshape(-1)
        if host.shape[0] and (int(host.min()) < 0 or int(host.max()) >= len(self)):
            raise IndexError("collate: molecule index outside the store")
        return torch.from_numpy(host).to(self.device), host

    def _extents_for(self, dev_idx, host_idx, pad_to, misfit: str):
        """The output extents, from the HOST counts; ``pad_to`` that does not fit raises before any launch.  (A device
        index with ``pad_to`` is trusted to fit -- the loader's plan chose the bucket from the same counts; the kernels
        never write past the extents and report a misfit in ``out._counts[-1]``.  A device index without ``pad_to`` is
        read back once: the only synchronising form, which no loader uses.)"""
        if pad_to is not None and host_idx is None:
            return tuple(int(v) for v in pad_to)
        if host_idx is None:
            host_idx = dev_idx.cpu().numpy()
            if host_idx.shape[0] and (int(host_idx.min()) < 0 or int(host_idx.max()) >= len(self)):
                raise IndexError("collate: molecule index outside the store")
        tot = self.extents(host_idx)
        if pad_to is None:
            return tot
        ext = tuple(int(v) for v in pad_to)
        if len(ext) != len(tot) or any(p < t + s for p, t, s in zip(ext, tot, self._MIN_SPARE)):
            raise ValueError(misfit)
        return ext

    def _scratch(self, out, n_graphs: int, query):
        """The collate workspace and the counts word of an output batch, allocated once per batch object"""
        need = int(query(n_graphs))
        ws = getattr(out, "_collate_ws", None)
        if ws is None or ws.numel() < need or ws.device != self.device:
            out._collate_ws = ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            out._counts = torch.zeros(4, dtype=torch.int64, device=self.device)
        return ws, out._counts

    def _bind_outputs(self, a, out, shapes: dict, floats: tuple):
        for name, shp in shapes.items():
            ten = getattr(out, name)
            want = torch.float32 if name in floats else torch.int64
            if (not torch.is_tensor(ten) or tuple(ten.shape) != shp or ten.dtype != want or not ten.is_contiguous()
                    or ten.device != self.device):
                raise ValueError(f"collate: out.{name} must be a contiguous {want} tensor of shape {shp} on {self.device}")
            setattr(a, "out_" + name, ten.data_ptr() or None)


class DeviceMolStore(_DeviceStore):
    """``MolStore.to_device(device)``: the hypergraph dataset in device memory.  ``collate`` writes the bytes
    ``MolStore.collate`` writes for the same ``idx`` and ``pad_to`` (tests/test_hip_device_collate.py: bit for bit), by the two
    launches of ``hb_collate_dev``; ``fit.BucketedLoader`` takes it in place of the host store and then runs without a
    producer thread, pinned staging or a per-batch host-to-device copy."""

    _COLUMNS = (("n_nodes", "node_off"), ("n_he", "he_off"), ("n_inc", "inc_off"))
    _ROWS = {"x": 0, "pos": 0, "v": 2, "e": 2, "edge_attr": 1, "e_order": 1}
    _HOST = MolStore
    _MIN_SPARE = (1, 1, 0)  # nodes and hyperedges strictly (the padding molecule's own), incidences may fill their extent

    def empty_staging(self, tgt, n_graphs: int, pin: bool = False) -> "HBatch":
        """An empty packed DEVICE batch of extents ``tgt`` for ``collate(out=...)`` (``pin`` has no meaning here)."""
        out = HBatch.empty_packed(tgt[0], tgt[1], tgt[2], n_graphs, device=self.device)
        from . import hip
        self._scratch(out, n_graphs, hip.lib().hb_collate_dev_workspace_bytes)
        return out

    def collate(self, idx, pad_to: Optional[tuple] = None, out: Optional["HBatch"] = None) -> "HBatch":
        from . import hip
        dev_idx, host_idx = self._index(idx)
        B = int(dev_idx.shape[0])
        PN, PM, PZ = self._extents_for(dev_idx, host_idx, pad_to,
                                       "collate: pad_to must exceed the batch (nodes and hyperedges strictly)")
        PB = B + (0 if pad_to is None else 1)
        if out is None:
            t = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
            out = HBatch(x=t((PN, 9), torch.int64), pos=t((PN, 3), torch.float32), edge_index0=t((PZ,), torch.int64),
                         edge_index1=t((PZ,), torch.int64), edge_attr=t((PM, 1), torch.int64), n_e=t((PB,), torch.int64),
                         e_order=t((PM,), torch.int64), batch=t((PN,), torch.int64), y=t((PB,), torch.float32))
        a = hip.HbCollateDev()
        self._bind_outputs(a, out, dict(x=(PN, 9), pos=(PN, 3), edge_index0=(PZ,), edge_index1=(PZ,), edge_attr=(PM, 1),
                                        n_e=(PB,), e_order=(PM,), batch=(PN,), y=(PB,)), ("pos", "y"))
        ws, counts = self._scratch(out, PB, hip.lib().hb_collate_dev_workspace_bytes)
        a.B, a.n_mols, a.idx = B, len(self), dev_idx.data_ptr() or None
        off = self._offsets
        a.node_off, a.he_off, a.inc_off = (off[k].data_ptr() for k in range(3))
        for name in self._ROWS:
            setattr(a, name, getattr(self, name).data_ptr() or None)
        a.y = self.y.data_ptr() or None
        a.PN, a.PM, a.PZ, a.padded = PN, PM, PZ, 0 if pad_to is None else 1
        a.out_counts, a.workspace, a.workspace_bytes = counts.data_ptr(), ws.data_ptr(), ws.numel()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            hip.check(hip.lib().hb_collate_dev(ctypes.byref(a), stream), "hb_collate_dev")
        out._collate_idx = dev_idx          # (keeps an uploaded index alive until the batch is collated into again)
        if pad_to is not None:
            out.num_real_graphs = B
        out.num_nodes, out.num_hyperedges, out.num_graphs = PN, PM, PB
        return out


class DeviceGraphStore(_DeviceStore):
    """``GraphStore.to_device(device)``: the 2-D graph dataset in device memory, collated by ``gb_collate_dev`` into the bytes
    ``GraphStore.collate`` writes."""

    _COLUMNS = (("n_nodes", "node_off"), ("n_edges", "edge_off"))
    _ROWS = {"x": 0, "src": 1, "dst": 1, "edge_attr": 1}
    _HOST = GraphStore
    _MIN_SPARE = (1, 0)     # atoms strictly, edges may fill their extent

    def __init__(self, host, device):
        self.F = int(host.F)
        super().__init__(host, device)

    def empty_staging(self, tgt, n_graphs: int, pin: bool = False) -> "GBatch":
        out = GBatch.empty_packed(tgt[0], tgt[1], self.F, n_graphs, device=self.device)
        from . import hip
        self._scratch(out, n_graphs, hip.lib().gb_collate_dev_workspace_bytes)
        return out

    def collate(self, idx, pad_to: Optional[tuple] = None, out: Optional["GBatch"] = None) -> "GBatch":
        from . import hip
        dev_idx, host_idx = self._index(idx)
        B, F = int(dev_idx.shape[0]), self.F
        PN, PE = self._extents_for(dev_idx, host_idx, pad_to, "collate: pad_to must exceed the batch (atoms strictly)")
        PB = B + (0 if pad_to is None else 1)
        if out is None:
            t = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
            out = GBatch(x=t((PN, 9), torch.int64), edge_index=t((2, PE), torch.int64), edge_attr=t((PE, F), torch.int64),
                         batch=t((PN,), torch.int64), y=t((PB,), torch.float32))
        a = hip.GbCollateDev()
        self._bind_outputs(a, out, dict(x=(PN, 9), edge_index=(2, PE), edge_attr=(PE, F), batch=(PN,), y=(PB,)), ("y",))
        ws, counts = self._scratch(out, PB, hip.lib().gb_collate_dev_workspace_bytes)
        a.B, a.n_mols, a.idx = B, len(self), dev_idx.data_ptr() or None
        a.node_off, a.edge_off = (self._offsets[k].data_ptr() for k in range(2))
        for name in self._ROWS:
            setattr(a, name, getattr(self, name).data_ptr() or None)
        a.y = self.y.data_ptr() or None
        a.F, a.PN, a.PE, a.padded = F, PN, PE, 0 if pad_to is None else 1
        a.out_counts, a.workspace, a.workspace_bytes = counts.data_ptr(), ws.data_ptr(), ws.numel()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            hip.check(hip.lib().gb_collate_dev(ctypes.byref(a), stream), "gb_collate_dev")
        out._collate_idx = dev_idx
        if pad_to is not None:
            out.num_real_graphs = B
        out.num_nodes, out.num_edges, out.num_graphs = PN, PE, PB
        return out


def graph_bucket_sizes(n_nodes: int, n_edges: int, quantum: int = 128):
    """Static extents of a padded 2-D batch: at least one padded atom (the padding molecule's)."""
    return -(-(n_nodes + 1) // quantum) * quantum, -(-n_edges // quantum) * quantum


def pad_graph_batch(b: GBatch, n_nodes: int, n_edges: int) -> GBatch:
    """Pad to fixed extents with ONE extra molecule (id B) that owns every padded atom; padded edges join padded atoms
    only (a ring over them), so no real row ever reads a padded one.  Real molecules keep identical outputs, gradients
    and -- with the real-row mask of layers.real_row_mask -- BatchNorm statistics."""
    N, E, B = b.x.shape[0], b.edge_index.shape[1], b.y.shape[0]
    if n_nodes <= N or n_edges < E:
        raise ValueError("pad_graph_batch: target extents must exceed the batch (atoms strictly)")
    dev = b.x.device
    pn, pe = n_nodes - N, n_edges - E
    k = torch.arange(pe, dtype=torch.int64, device=dev)
    pad_ei = torch.stack((N + k % pn, N + (k + 1) % pn))
    out = GBatch(x=torch.cat((b.x, torch.zeros((pn, b.x.shape[1]), dtype=b.x.dtype, device=dev))),
                 edge_index=torch.cat((b.edge_index, pad_ei.to(b.edge_index.dtype)), 1),
                 edge_attr=torch.cat((b.edge_attr, torch.zeros((pe, b.edge_attr.shape[1]), dtype=b.edge_attr.dtype,
                                                               device=dev))),
                 batch=torch.cat((b.batch, torch.full((pn,), B, dtype=b.batch.dtype, device=dev))),
                 y=torch.cat((b.y, torch.zeros(1, dtype=b.y.dtype, device=dev))),
                 num_nodes=n_nodes, num_edges=n_edges, num_graphs=B + 1)
    out.num_real_graphs = getattr(b, "num_real_graphs", B)
    return out


def synth_graph(rng: np.random.Generator, flavour: str = "qm9") -> GMol:
    """2-D graph of one synth_molecule: its bonds in both directions (ogb mol2graph order: (i, j) then (j, i)),
    1 bond column (qm9_g: the bond type) or 3 (pcqm_g / molecule_g: type, stereo, conjugated)."""
    m = synth_molecule(rng, flavour)
    bond = m.e_order == 2
    nb = int(bond.sum())
    pairs = m.edge_index0[: 2 * nb].reshape(nb, 2)
    ei = np.empty((2, 2 * nb), dtype=np.int64)
    ei[0, 0::2], ei[1, 0::2] = pairs[:, 0], pairs[:, 1]
    ei[0, 1::2], ei[1, 1::2] = pairs[:, 1], pairs[:, 0]
    cols = [m.edge_attr[:nb, 0]]
    if flavour != "qm9":
        cols += [rng.integers(0, 6, size=nb), rng.integers(0, 2, size=nb)]
    attr = np.repeat(np.stack(cols, 1).astype(np.int64), 2, axis=0)
    return GMol(x=m.x, edge_index=ei, edge_attr=attr, y=m.y)


def synth_graph_batch(batch_size: int, seed: int, flavour: str = "qm9") -> GBatch:
    """Seeded synthetic 2-D batch (qm9: 1 bond column; pcqm: 3).  Pure host code, deterministic per seed."""
    rng = np.random.default_rng(seed)
    return collate_graphs([synth_graph(rng, flavour) for _ in range(batch_size)])
