"""The SE(3)-Transformer front-end of ``se3_transformer_equihnns`` restated in plain torch, any dtype, from its semantics
(se3_transformer_layer.py:1378-1693 at heads=2, depth=2, dim_head=32, num_degrees=2, radius 5, 16 neighbours, mask all
true, one cloud over the whole batch).  No kernel, no fused path, the per-edge radial weights formed as written: the
operand-level oracle of tests/test_hip_se3t.py and, in float64, what tests/test_se3t_host.py pins to the reference's own
float64 run.  Features are in the reference's layout, [N, C, m].

Only the closed-form Q_J matrices are shared with the package (equihgnn_amd.se3_transformer.q_matrices; pinned to the
reference's values by tests/test_se3t_host.py).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from equihgnn_amd.se3_transformer import q_matrices

HEADS, DIM_HEAD, MID = 2, 32, 128
PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1))


def edge_graph(pos, k=16, radius=5.0):
    """Self-excluded k = min(k, N - 1) nearest by true distance (ties: lowest index, as a stable sort gives), the radius
    mask, and rel = pos_i - pos_j.  -> nbr [N, K] int64, dist [N, K], mask [N, K] bool, rel [N, K, 3]."""
    n = pos.shape[0]
    k = min(k, n - 1)
    rel_all = pos[:, None, :] - pos[None, :, :]
    d = rel_all.norm(dim=-1)
    d = d.masked_fill(torch.eye(n, dtype=torch.bool), float("inf"))
    dist, nbr = torch.sort(d, dim=-1, stable=True)
    dist, nbr = dist[:, :k], nbr[:, :k]
    rel = torch.gather(rel_all, 1, nbr[..., None].expand(-1, -1, 3))
    return nbr, dist, dist <= radius, rel


def real_sh(rel):
    """Y_0 [.., 1], Y_1 [.., 3], Y_2 [.., 5] of the direction of ``rel`` in the reference's convention
    (get_spherical_from_cartesian: cartesian x, y, z = components 2, 0, 1; theta = pi - beta; tesseral harmonics with the
    Condon-Shortley phase), written in cartesian form.  A zero vector reads as the direction (0, 1, 0), which is what
    atan2(0, 0) = 0 gives there."""
    r = rel.norm(dim=-1, keepdim=True)
    zero = r == 0
    u = torch.where(zero, torch.zeros_like(rel), rel / r.clamp(min=1e-300 if rel.dtype == torch.float64 else 1e-30))
    u = torch.where(zero.expand_as(u), torch.tensor([0.0, 1.0, 0.0], dtype=rel.dtype).expand_as(u), u)
    cy, cz, cx = u[..., 0], u[..., 1], u[..., 2]
    n0, n1, n2 = math.sqrt(1 / (4 * math.pi)), math.sqrt(3 / (4 * math.pi)), math.sqrt(5 / (4 * math.pi))
    s3 = math.sqrt(3.0)
    y0 = torch.full_like(cx, n0)[..., None]
    y1 = -n1 * torch.stack((cy, cz, cx), -1)
    y2 = n2 * torch.stack((s3 * cx * cy, s3 * cy * cz, 1.5 * cz * cz - 0.5, s3 * cx * cz, 0.5 * s3 * (cx * cx - cy * cy)), -1)
    return y0, y1, y2


def basis(rel):
    """{(di, do): [.., mo, mi, F]} with F = 2 min(di, do) + 1: K_J = Y_J Q_J^T stacked over J (basis.py:223-245)."""
    q = q_matrices(rel.dtype)
    ys = real_sh(rel)
    out = {}
    for di, do in PAIRS:
        ks = []
        for j in range(abs(di - do), di + do + 1):
            ks.append(ys[j] @ q[(di, do, j)].T)                      # [.., mo * mi]
        out[(di, do)] = torch.stack(ks, -1).view(*rel.shape[:-1], 2 * do + 1, 2 * di + 1, len(ks))
    return out


def trunk(sd, p, dist):
    """RadialFunc.net[0..5]: Linear(1,128) -> LayerNorm -> GELU -> Linear(128,128) -> LayerNorm -> GELU."""
    h = dist[..., None] * sd[p + "rp.net.0.weight"][:, 0] + sd[p + "rp.net.0.bias"]
    h = F.gelu(F.layer_norm(h, (MID,), sd[p + "rp.net.1.weight"], sd[p + "rp.net.1.bias"]))
    h = h @ sd[p + "rp.net.3.weight"].T + sd[p + "rp.net.3.bias"]
    return F.gelu(F.layer_norm(h, (MID,), sd[p + "rp.net.4.weight"], sd[p + "rp.net.4.bias"]))


def pair_kernel_apply(h, w3, b3, bas, xj):
    """One PairwiseConv as written: R = reshape(W3 h + b3) [.., O, I, F], kernel[(o,mo),(i,mi)] = sum_f R[o,i,f] B[mo,mi,f],
    out[o, mo] = sum_(i,mi) kernel x_j[i, mi].  h [.., 128], bas [.., mo, mi, F], xj [.., I, mi] -> [.., O, mo]."""
    i, f = xj.shape[-2], bas.shape[-1]
    r = (h @ w3.T + b3).view(*h.shape[:-1], -1, i, f)
    return torch.einsum("...oif,...pqf,...iq->...op", r, bas, xj)


def conv(sd, p, feats, graph, bas, degs_out, pool, self_interaction):
    nbr, dist, mask, _ = graph
    out = {}
    for do in degs_out:
        acc = 0
        for di in sorted(feats):
            pp = f"{p}kernel_unary.({di},{do})."
            acc = acc + pair_kernel_apply(trunk(sd, pp, dist), sd[pp + "rp.net.6.weight"], sd[pp + "rp.net.6.bias"],
                                          bas[(di, do)], feats[di][nbr])
        if pool:
            acc = masked_mean(acc, mask)
        out[do] = acc
    if self_interaction:
        for d in out:
            key = f"{p}self_interact.weights.{d}"
            if key in sd and d in feats:
                out[d] = out[d] + linear(feats[d], sd[key])
    return out


def masked_mean(t, mask):
    """se3_transformer/utils.py::masked_mean over the neighbour slots: t [N, K, ...], mask [N, K]."""
    m = mask.view(*mask.shape, *([1] * (t.dim() - 2)))
    cnt = mask.sum(1).view(-1, *([1] * (t.dim() - 2)))
    mean = t.masked_fill(~m, 0.0).sum(1) / cnt.clamp(min=1).to(t.dtype)
    return mean.masked_fill(cnt == 0, 0.0)


def linear(x, w):
    return torch.einsum("...dm,de->...em", x, w)


def norm_se3(x, scale, eps=1e-12):
    """NormSE3: x [.., C, m], scale [1, 1, C] (or [C])."""
    norm = x.norm(dim=-1, keepdim=True).clamp(min=eps)
    return F.gelu(norm[..., 0] * scale.reshape(-1))[..., None] * (x / norm)


def attention_core(q, k_self, k_edge, v_self, v_edge, mask):
    """One degree: q / k_self / v_self [N, 64, m], k_edge / v_edge [N, K, 64, m], mask [N, K] -> ([N, 64, m], logits)."""
    n, _, m = q.shape
    qh = q.view(n, HEADS, DIM_HEAD, m)
    k = torch.cat((k_self[:, None], k_edge), 1).view(n, -1, HEADS, DIM_HEAD, m)
    v = torch.cat((v_self[:, None], v_edge), 1).view(n, -1, HEADS, DIM_HEAD, m)
    sim = torch.einsum("nhdm,njhdm->nhj", qh, k) * DIM_HEAD ** -0.5
    keep = F.pad(mask, (1, 0), value=True)[:, None, :]
    sim = sim.masked_fill(~keep, -torch.finfo(sim.dtype).max)
    out = torch.einsum("nhj,njhdm->nhdm", sim.softmax(-1), v)
    return out.reshape(n, HEADS * DIM_HEAD, m), sim


def attention_block(sd, p, x, graph, bas):
    f = {d: norm_se3(x[d], sd[f"{p}prenorm.transform.{d}.scale"]) for d in x}
    a = p + "attn."
    q = {d: linear(f[d], sd[f"{a}to_q.weights.{d}"]) for d in f}
    v = conv(sd, a + "to_v.", f, graph, bas, (0, 1), False, False)
    k = conv(sd, a + "to_k.", f, graph, bas, (0, 1), False, False)
    out = {}
    for d in f:
        ks, vs = linear(f[d], sd[f"{a}to_self_k.weights.{d}"]), linear(f[d], sd[f"{a}to_self_v.weights.{d}"])
        o, _ = attention_core(q[d], ks, k[d], vs, v[d], graph[2])
        out[d] = x[d] + linear(o, sd[f"{a}to_out.weights.{d}"])
    return out


def feedforward_block(sd, p, x):
    out = {}
    for d in x:
        h = linear(norm_se3(x[d], sd[f"{p}prenorm.transform.{d}.scale"]), sd[f"{p}feedforward.project_in.weights.{d}"])
        h = norm_se3(h, sd[f"{p}feedforward.nonlin.transform.{d}.scale"])
        out[d] = x[d] + linear(h, sd[f"{p}feedforward.project_out.weights.{d}"])
    return out


def front_end(sd, feats, pos, prefix="se3_transformer_layer.", depth=2, taps=None):
    """feats [N, C], pos [N, 3] -> [N, C]; ``taps`` (a dict) receives conv_in0/1, block{i}_0/1 and front_end."""
    graph = edge_graph(pos)
    bas = basis(graph[3])
    x = conv(sd, prefix + "conv_in.", {0: feats[..., None]}, graph, bas, (0, 1), True, True)
    if taps is not None:
        taps["conv_in0"], taps["conv_in1"] = x[0], x[1]
    for i in range(depth):
        x = attention_block(sd, f"{prefix}net.blocks.{i}.0.", x, graph, bas)
        x = feedforward_block(sd, f"{prefix}net.blocks.{i}.1.", x)
        if taps is not None:
            taps[f"block{i}_0"], taps[f"block{i}_1"] = x[0], x[1]
    out = conv(sd, prefix + "conv_out.", x, graph, bas, (0,), True, True)[0][..., 0]
    if taps is not None:
        taps["front_end"] = out
    return out
