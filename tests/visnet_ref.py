"""Float64 restatement of the reference ViSNet front-end (visnet_layer.py as equihnn_visnet.py configures it), written
from its documented semantics on plain torch (CPU, any dtype) for the ViSNet tests.  ``radius_graph`` stands in for
torch_cluster's CUDA radius_graph (loop=True, max_num_neighbors=16): for each target i, the atoms j of i's molecule in
ascending index, i included, whose fp32 squared distance summed in x, y, z order is strictly below r^2; the search stops
after 16 kept atoms; edges ordered by target then source; edge_index[0] = source j, edge_index[1] = target i."""
import math

import torch

K, CUTOFF = 16, 5.0
VIS_WEIGHT_SCALE = 0.15


def radius_graph(pos, batch, r=CUTOFF, k=K, n_real=None):
    """``n_real``: atoms at index >= n_real (a padded batch's dummy molecule) keep only their self-loop."""
    p = pos.detach().to(torch.float32).cpu()
    b = batch.cpu()
    N = p.shape[0]
    n_real = N if n_real is None else int(n_real)
    src, dst = [], []
    r2 = torch.tensor(r, dtype=torch.float32) * torch.tensor(r, dtype=torch.float32)
    ordered = bool((b[1:] >= b[:-1]).all())             # a sorted batch vector: each molecule is one index range
    if ordered:
        lo = torch.searchsorted(b, b, right=False).tolist()
        hi = torch.searchsorted(b, b, right=True).tolist()
    for i in range(N):
        if i >= n_real:
            src.append(i)
            dst.append(i)
            continue
        same = torch.arange(lo[i], hi[i]) if ordered else torch.nonzero(b == b[i]).reshape(-1)
        d = p[same] - p[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = same[d2 < r2][:k]
        src += keep.tolist()
        dst += [i] * keep.numel()
    return torch.tensor([src, dst], dtype=torch.long)


def _cut(d):
    return 0.5 * (torch.cos(d * math.pi / CUTOFF) + 1.0) * (d < CUTOFF).to(d.dtype)


def _sphere(v):
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    s3 = math.sqrt(3.0)
    return torch.stack([x, y, z, s3 * x * z, s3 * x * y, y * y - 0.5 * (x * x + z * z), s3 * y * z,
                        s3 / 2.0 * (z * z - x * x)], -1)


def visnet(sd, z, pos, batch, prefix="", n_real=None, dtype=torch.float64, num_layers=6, with_repr=False, vec0=None):
    """Per-atom output [N, C] of ViSNet(hidden_channels=C, lmax=2, max_num_neighbors=16, num_layers=num_layers) with the
    state dict ``sd`` (tensors that require grad are used as they are, so gradients flow back to them).  ``with_repr``:
    return (output, x, vec) with the representation model's pair as well.  ``vec0`` [N, 8, C]: the vector features the
    first layer starts from (the model's own start is zero)."""
    P = lambda n: sd[prefix + n]
    rm = "representation_model."
    z = z.cpu()
    N = z.shape[0]

    def emb(name):
        out = 0
        for f in range(z.shape[1]):
            out = out + P(f"{name}.atom_embedding_list.{f}.weight")[z[:, f]]
        return out

    def lin(x, name, bias=True):
        y = x @ P(name + ".weight").t()
        return y + P(name + ".bias") if bias else y

    def ln(x, name):
        return torch.nn.functional.layer_norm(x, (x.shape[-1],), P(name + ".weight"), P(name + ".bias"), 1e-5)

    silu = torch.nn.functional.silu
    ei = radius_graph(pos, batch, n_real=n_real)
    src, dst = ei[0], ei[1]
    posd = pos.detach().cpu().to(dtype)
    vec_e = posd[src] - posd[dst]
    mask = src != dst
    w = torch.zeros(src.numel(), dtype=dtype)
    w[mask] = torch.norm(vec_e[mask], dim=-1)
    means, betas = P(rm + "distance_expansion.means"), P(rm + "distance_expansion.betas")
    rbf = _cut(w).unsqueeze(-1) * torch.exp(-betas * (torch.exp((5.0 / CUTOFF) * (-w)).unsqueeze(-1) - means) ** 2)
    vec_e = vec_e.clone()
    vec_e[mask] = vec_e[mask] / torch.norm(vec_e[mask], dim=1).unsqueeze(1)
    sh = _sphere(vec_e)

    x = emb(rm + "embedding")
    ne = rm + "neighbor_embedding."
    Wn = lin(rbf[mask], ne + "distance_proj") * _cut(w[mask]).unsqueeze(-1)
    xn = emb(ne + "embedding")
    xn = torch.zeros_like(xn).index_add(0, dst[mask], xn[src[mask]] * Wn)
    x = lin(torch.cat([x, xn], 1), ne + "combine")
    C = x.shape[1]
    D = C // 8
    vec = torch.zeros(N, 8, C, dtype=dtype) if vec0 is None else vec0
    f = (x[dst] + x[src]) * lin(rbf, rm + "edge_embedding.edge_proj")
    L = num_layers
    for l in range(L):
        p = f"{rm}vis_mp_layers.{l}."
        xl = ln(x, p + "layernorm")
        q = lin(xl, p + "q_proj").view(-1, 8, D)
        k = lin(xl, p + "k_proj").view(-1, 8, D)
        v = lin(xl, p + "v_proj").view(-1, 8, D)
        dk = silu(lin(f, p + "dk_proj")).view(-1, 8, D)
        dv = silu(lin(f, p + "dv_proj")).view(-1, 8, D)
        vec1, vec2, vec3 = torch.split(lin(vec, p + "vec_proj", False), C, dim=-1)
        vec_dot = (vec1 * vec2).sum(dim=1)
        attn = silu((q[dst] * k[src] * dk).sum(-1)) * _cut(w).unsqueeze(1)
        vj = ((v[src] * dv) * attn.unsqueeze(2)).view(-1, C)
        s1, s2 = torch.split(silu(lin(vj, p + "s_proj")), C, dim=1)
        vecj = vec[src] * s1.unsqueeze(1) + s2.unsqueeze(1) * sh.unsqueeze(2)
        xa = torch.zeros(N, C, dtype=dtype).index_add(0, dst, vj)
        vo = torch.zeros(N, 8, C, dtype=dtype).index_add(0, dst, vecj)
        o1, o2, o3 = torch.split(lin(xa, p + "o_proj"), C, dim=1)
        dx = vec_dot * o2 + o3
        dvec = vec3 * o1.unsqueeze(1) + vo
        if l < L - 1:
            def rej(a, d):
                return a - (a * d.unsqueeze(2)).sum(dim=1, keepdim=True) * d.unsqueeze(2)
            w1 = rej(lin(vec, p + "w_trg_proj", False)[dst], sh)
            w2 = rej(lin(vec, p + "w_src_proj", False)[src], -sh)
            f = f + silu(lin(f, p + "f_proj")) * (w1 * w2).sum(dim=1)
        x = x + dx
        vec = vec + dvec
    x = ln(x, rm + "out_norm")
    x_repr = x
    v = vec
    for bb in range(2):
        p = f"output_model.output_network.{bb}."
        v1 = torch.linalg.vector_norm(lin(v, p + "vec1_proj", False), dim=-2)
        v2 = lin(v, p + "vec2_proj", False)
        h = lin(silu(lin(torch.cat([x, v1], -1), p + "update_net.0")), p + "update_net.2")
        x, v = torch.split(h, C, dim=-1)
        v = v.unsqueeze(1) * v2
        x = silu(x)
    out = (x + v.sum() * 0) * P("std")
    return (out, x_repr, vec) if with_repr else out


# ----------------------------------------------------------------------------------------------------------------------
# the five vis_* operators on plain torch, over the kept edges of a slot table
# ----------------------------------------------------------------------------------------------------------------------
class EdgeList:
    """The kept edges of a [N, 16] slot table, in edge-id order: ``src`` / ``dst`` [n] (atom ids), ``eid`` [n] (slot ids
    16 i + s), and the per-slot ``cut`` [16 N] and ``sh`` [16 N, 8] the operators read."""

    def __init__(self, N, src, dst, eid, cut, sh):
        self.N, self.E, self.src, self.dst, self.eid, self.cut, self.sh = int(N), K * int(N), src, dst, eid, cut, sh

    def rows(self, a0, a1):
        """The edges of atoms [a0, a1), a range of whole molecules, renumbered from 0."""
        m = (self.dst >= a0) & (self.dst < a1)
        return EdgeList(a1 - a0, self.src[m] - a0, self.dst[m] - a0, self.eid[m] - K * a0, self.cut[K * a0:K * a1],
                        self.sh[K * a0:K * a1])

    def to(self, dtype):
        return EdgeList(self.N, self.src, self.dst, self.eid, self.cut.to(dtype), self.sh.to(dtype))


class _AbsSilu(torch.autograd.Function):
    """|silu(t)| forward; backward the two terms of silu'(t) = s + t s (1 - s), s = sigmoid(t), by their absolute values
    (they cancel at t = -1.28)."""

    @staticmethod
    def forward(ctx, t):
        ctx.save_for_backward(t)
        return torch.nn.functional.silu(t).abs()

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        s = torch.sigmoid(t)
        return g * (s * (1 + t.abs() * (1 - s)))


def _act(t, magnitude):
    return _AbsSilu.apply(t) if magnitude else torch.nn.functional.silu(t)


# Each reference takes ``magnitude``: with it, every term enters by its absolute value -- an activation as |silu|, with
# |silu'| as its derivative, a harmonic as |sh|, a difference as a sum -- so that on inputs whose linear operands (q, k,
# v, vec, wt, ws, x, W and the upstream gradients) were made non-negative by the caller, an output element, and a
# gradient element after backward, is the sum of the absolute values of the terms that make up the plain element: the
# scale A of a per-element rounding bound.
def nbr_ref(G, x, W, magnitude=False):
    m = G.src != G.dst
    C = x.shape[1]
    return torch.zeros(G.N, C, dtype=x.dtype).index_add(
        0, G.dst[m], x[G.src[m]] * (W[G.eid[m]] * G.cut[G.eid[m]].unsqueeze(-1)))


def eemb_ref(G, x, W, magnitude=False):
    f = torch.zeros(G.E, x.shape[1], dtype=x.dtype)
    return f.index_put((G.eid,), (x[G.dst] + x[G.src]) * W[G.eid])


def attn_ref(G, q, k, v, dkr, dvr, magnitude=False):
    C = q.shape[1]
    D = C // 8
    src, dst, eid = G.src, G.dst, G.eid
    pre = (q[dst] * k[src] * _act(dkr[eid], magnitude)).view(-1, 8, D).sum(-1)
    a = _act(pre, magnitude) * G.cut[eid].unsqueeze(-1)
    u_e = ((v[src] * _act(dvr[eid], magnitude)).view(-1, 8, D) * a.unsqueeze(-1)).view(-1, C)
    u = torch.zeros(G.E, C, dtype=q.dtype).index_put((eid,), u_e)
    return u, torch.zeros(G.N, C, dtype=q.dtype).index_add(0, dst, u_e)


def vec_ref(G, vec, sr, magnitude=False):
    C = vec.shape[2]
    sh = G.sh.abs() if magnitude else G.sh
    s = _act(sr[G.eid], magnitude)
    msg = vec[G.src] * s[:, :C].unsqueeze(1) + s[:, C:].unsqueeze(1) * sh[G.eid].unsqueeze(2)
    return torch.zeros(G.N, 8, C, dtype=vec.dtype).index_add(0, G.dst, msg)


def eupd_ref(G, wt, ws, fr, magnitude=False):
    C = wt.shape[2]
    sign = 1.0 if magnitude else -1.0

    def rej(a, d):
        return a + sign * (a * d.unsqueeze(2)).sum(dim=1, keepdim=True) * d.unsqueeze(2)

    d = G.sh[G.eid]
    d, nd = (d.abs(), d.abs()) if magnitude else (d, -d)
    df = _act(fr[G.eid], magnitude) * (rej(wt[G.dst], d) * rej(ws[G.src], nd)).sum(1)
    return torch.zeros(G.E, C, dtype=wt.dtype).index_put((G.eid,), df)


def restore_visnet_buffers(model):
    """Put the ViSNet buffers back to their constructed values after common.fill_state_dict (which fills every floating
    tensor): ExpNormalSmearing means / betas, the VecLayerNorm weights (ones), ViSNet.mean (0) and .std (1)."""
    start = torch.exp(torch.tensor(-CUTOFF))
    sd = model.state_dict()
    new = {}
    for k, v in sd.items():
        if k.endswith("distance_expansion.means"):
            new[k] = torch.linspace(start, 1, v.numel()).to(v.dtype)
        elif k.endswith("distance_expansion.betas"):
            new[k] = torch.tensor([(2 / v.numel() * (1 - start)) ** -2] * v.numel()).to(v.dtype)
        elif k.endswith("vec_layernorm.weight") or k.endswith("vec_out_norm.weight"):
            new[k] = torch.ones_like(v)
        elif k.endswith("visnet_layer.mean"):
            new[k] = torch.zeros_like(v)
        elif k.endswith("visnet_layer.std"):
            new[k] = torch.ones_like(v)
    model.load_state_dict(new, strict=False)


def fill_visnet_model(model, seed, fill_state_dict):
    """common.fill_state_dict for a model holding a ViSNet (whose 0-dim ``mean`` / ``std`` buffers it cannot fill), then
    restore_visnet_buffers."""
    vis = [m for m in model.modules() if hasattr(m, "representation_model") and hasattr(m, "std")]
    for m in vis:
        m.mean, m.std = m.mean.reshape(1), m.std.reshape(1)
    fill_state_dict(model, seed)
    for m in vis:
        m.mean, m.std = m.mean.reshape(()), m.std.reshape(())
    restore_visnet_buffers(model)
    with torch.no_grad():      # (at fill_state_dict's 1 / sqrt(fan_in) scale the 6 layers' quadratic terms overflow)
        for m in vis:
            for n, p in m.named_parameters():
                if p.dim() == 2 and "embedding." not in n:
                    p.mul_(VIS_WEIGHT_SCALE)
