"""GPU: the se3t_* kernels (csrc/se3t.hip) against the float64 restatement tests/se3t_ref.py, forward and backward.

Bounds.  The kernels are fp32 (unit roundoff u = 6e-8).  A pair output is a sum of up to Q * 128 = 1152 products on top of a
node-level product over I <= 256 channels; with random signs the error grows like sqrt(n) u ~ 2e-6 of the typical term, and
the bound is 2e-5 of the largest entry of the float64 result (a factor 10 over that estimate; the rule of the other operator
tests).  The softmax multiplies a logit's absolute error into a relative one, so the attention bound adds 4 |logit|_max u.
The basis is a handful of operations on unit vectors: 1e-6 absolute."""
import numpy as np
import pytest
import torch

import se3t_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 2e-5
OFF = {(0, 0): (0, 1, 1, 1), (0, 1): (1, 3, 1, 1), (1, 0): (4, 1, 3, 1), (1, 1): (7, 3, 3, 3)}     # offset, mo, mi, F


def _rand(*shape, seed):
    # (float32-representable values: both sides start from the same numbers)
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float().double()


def _close(got, ref, what, tol=TOL):
    """Asserts the max-norm bound; returns error / bound."""
    ref = ref.detach()
    err = float((got.detach().cpu().double() - ref).abs().max())
    assert err <= tol * float(ref.abs().max()) + 1e-30, (what, err, float(ref.abs().max()))
    return err / (tol * float(ref.abs().max()) + 1e-30)


def _qtab():
    from equihgnn_amd.se3_transformer import q_table
    return q_table().to(DEV)


def _basis_rows(rel):
    """[.., 34] in the kernel's layout from the restatement's basis dict."""
    bas = se3t_ref.basis(rel)
    return torch.cat([bas[p].reshape(*rel.shape[:-1], -1) for p in ((0, 0), (0, 1), (1, 0), (1, 1))], -1)


def _cloud(n, seed):
    pos = _rand(n, 3, seed=seed) * 2.4                  # some pairs beyond the radius of 5
    pos[1] = pos[0] + torch.tensor([0.0, 0.0, 1.3])     # exactly along +z (and -z seen from atom 1)
    pos[3] = pos[2] + torch.tensor([1.1, 0.7, 0.0])     # in the xy-plane
    return pos.float().double()                          # float32-representable coordinates


@pytest.mark.parametrize("n", [5, 70])
def test_edge_basis(n):
    from equihgnn_amd import ops
    pos = _cloud(n, 3)
    nbr, dist, mask, rel = se3t_ref.edge_graph(pos)
    k = nbr.shape[1]
    g_nbr, _ = ops.knn(pos.float().to(DEV), k, 1)
    assert torch.equal(g_nbr.cpu().long(), nbr)
    d, maskf, meanw, basis = ops.se3t_edge_basis(pos.float().to(DEV), g_nbr, 5.0, _qtab())
    assert float((d.cpu().double().view(n, k) - dist).abs().max()) <= 1e-5
    assert torch.equal(maskf.cpu() > 0, mask)
    want_w = mask.double() / mask.sum(1, keepdim=True).clamp(min=1)
    assert float((meanw.cpu().double() - want_w).abs().max()) <= 1e-6
    assert float((basis.cpu().double().view(n, k, 34) - _basis_rows(rel)).abs().max()) <= 1e-6
    if n == 70:
        assert (~mask).any() and mask.any()


def _table(n, k, seed):
    """A neighbour table in which atom 0 is nobody's neighbour and a mask whose row 3 is empty."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(1, n - 1, (n, k), generator=g)                  # 1 .. n - 2, then skip the atom itself
    nbr = cand + (cand >= torch.arange(n)[:, None]).long()
    mask = torch.rand(n, k, generator=g) < 0.7
    mask[3] = False
    mask[min(4, n - 1)] = True
    return nbr, mask


def _graph(n, k, seed):
    """_table and its transposed CSR."""
    from equihgnn_amd import ops
    nbr, mask = _table(n, k, seed)
    csr = ops.csr_build(nbr.reshape(-1).to(torch.int32).to(DEV), None, n)
    return nbr, mask, csr


def _node_weights(w3, b3, o, i, f):
    w = w3.view(o, i, f, 128).permute(1, 2, 3, 0).reshape(i, f * 128 * o)
    b = b3.view(o, i, f).permute(1, 2, 0).reshape(i, f * o)
    return w, b


def _pair_case(pair, i, o, n, k, seed):
    from equihgnn_amd import ops
    off, mo, mi, f = OFF[pair]
    nbr, mask, csr = _graph(n, k, seed)
    x = _rand(n, i, mi, seed=seed + 1)                                   # the reference's layout [N, I, mi]
    h = _rand(n, k, 128, seed=seed + 2)
    w3 = (_rand(o * i * f, 128, seed=seed + 3) / 128 ** 0.5).float().double()
    b3 = (_rand(o * i * f, seed=seed + 4) * 0.1).float().double()
    rows = _rand(n, k, 34, seed=seed + 5)
    bas = rows[..., off:off + mo * mi * f].reshape(n, k, mo, mi, f)
    leaves64 = [t.clone().requires_grad_(True) for t in (x, h, w3, b3)]
    x64, h64, w64, b64 = leaves64
    edge64 = se3t_ref.pair_kernel_apply(h64, w64, b64, bas, x64[nbr])    # [N, K, O, mo]
    pool64 = se3t_ref.masked_mean(edge64, mask)                          # [N, O, mo]
    meanw = (mask.double() / mask.sum(1, keepdim=True).clamp(min=1)).float().to(DEV)
    worst = 0.0                                                          # (the largest error / bound, returned)
    for pooled, ref in ((False, edge64.reshape(n * k, o, mo)), (True, pool64)):
        leaves = [t.float().to(DEV).requires_grad_(True) for t in (x, h, w3, b3)]
        xg, hg, wg, bg = leaves
        w, b = _node_weights(wg, bg, o, i, f)
        xc = xg.transpose(1, 2).reshape(n * mi, i)                       # component-major rows (n, mi)
        out = ops.se3t_pair(hg.reshape(n * k, 128), xc @ w, xc @ b, rows.float().to(DEV).reshape(n * k, 34), pair, o,
                            csr.rowptr, csr.perm, meanw if pooled else None)
        out = out.transpose(1, 2)                                        # [*, O, mo]
        worst = max(worst, _close(out, ref, ("fwd", pooled)))
        up = _rand(*ref.shape, seed=seed + 6)
        g64 = torch.autograd.grad((ref * up).sum(), leaves64, retain_graph=True)
        g32 = torch.autograd.grad((out * up.float().to(DEV)).sum(), leaves)
        for name, a, c in zip("x h w3 b3".split(), g64, g32):
            worst = max(worst, _close(c, a, ("bwd", name, pooled)))
        if pooled:
            assert float(out[3].abs().max()) == 0                        # every slot masked: the clamped count, a zero mean
            assert float(g32[1].view(n, k, 128)[3].abs().max()) == 0
    return worst


# (32, 32) / (32, 64): one partial 64-column block; (256, 64): the full node-level K loop and a whole block
@pytest.mark.parametrize("io", [(32, 32), (32, 64), (256, 64)])
@pytest.mark.parametrize("pair", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_pair_ragged_tile(pair, io):
    _pair_case(pair, io[0], io[1], 37, 16, 11)       # 592 edges: sender rows of 16 k + r entries, a ragged last tile


@pytest.mark.parametrize("pair", [(0, 0), (1, 1)])
def test_pair_small_cloud(pair):
    _pair_case(pair, 32, 32, 5, 4, 12)               # k = 4


def _attn_inputs(n, k, m, big, seed):
    """(mask [N, K], [q, kself, kedge, vself, vedge] in the reference's layout, float32-representable)"""
    if n > 4:
        _, mask = _table(n, k, seed)
    else:                                            # (_graph plants rows 3 and 4: a cloud of two to four atoms draws its own)
        mask = torch.rand(n, k, generator=torch.Generator().manual_seed(seed)) < 0.7
    mask[0] = False                                  # only the self slot survives
    mask[1] = False
    mask[1, k // 2] = True                           # a single valid neighbour slot
    amp = (80 / m ** 0.5) ** 0.5 if big else 1.0                         # |q . k| * 32^-0.5 ~ 80
    ts = [_rand(n, 64, m, seed=seed + 1) * amp, _rand(n, 64, m, seed=seed + 2) * amp, _rand(n, k, 64, m, seed=seed + 3) * amp,
          _rand(n, 64, m, seed=seed + 4), _rand(n, k, 64, m, seed=seed + 5)]
    return mask, [t.float().double() for t in ts]


def _attn_case(n, k, m, big, seed):
    from equihgnn_amd import ops
    mask, ts = _attn_inputs(n, k, m, big, seed)
    l64 = [t.clone().requires_grad_(True) for t in ts]
    ref, sim = se3t_ref.attention_core(l64[0], l64[1], l64[2], l64[3], l64[4], mask)
    lmax = float(sim.detach()[sim.detach() > -1e30].abs().max())
    if big:
        assert lmax > 60
    tol = TOL + 4 * lmax * 2.0 ** -24
    l32 = [t.float().to(DEV).requires_grad_(True) for t in ts]
    cm = lambda t: t.transpose(-1, -2).reshape(-1, m, 64)                # component-major [*, m, 64]
    out = ops.se3t_attn(cm(l32[0]), cm(l32[1]), cm(l32[2]), cm(l32[3]), cm(l32[4]), mask.float().to(DEV), 32 ** -0.5)
    out = out.transpose(1, 2)
    worst = _close(out, ref, "fwd", tol)
    assert float((out[0] - l32[3][0]).abs().max()) <= tol * float(ref.abs().max())      # all masked: the self value
    up = _rand(*ref.shape, seed=seed + 6)
    g64 = torch.autograd.grad((ref * up).sum(), l64)
    g32 = torch.autograd.grad((out * up.float().to(DEV)).sum(), l32)
    for name, a, c in zip("q kself kedge vself vedge".split(), g64, g32):
        worst = max(worst, _close(c, a, ("bwd", name), tol))
    assert float(g32[2][0].abs().max()) == 0 and float(g32[4][0].abs().max()) == 0      # masked slots get no gradient
    return mask, g32, worst


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("nk", [(37, 16), (5, 4)])
def test_attention(nk, m, big):
    _attn_case(nk[0], nk[1], m, big, 21)


@pytest.mark.parametrize("c", [32, 320])
@pytest.mark.parametrize("m", [1, 3])
def test_norm_with_a_zero_row(m, c):
    from equihgnn_amd import ops
    x = _rand(37, c, m, seed=31)
    x[5] = 0.0                                        # the clamp: norm 0 < 1e-12
    s = (1.0 + 0.1 * _rand(1, 1, c, seed=32)).float().double()
    x64, s64 = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
    ref = se3t_ref.norm_se3(x64, s64)
    x32, s32 = x.float().to(DEV).requires_grad_(True), s.float().to(DEV).requires_grad_(True)
    out = ops.se3t_norm(x32.transpose(1, 2).contiguous(), s32).transpose(1, 2)
    _close(out, ref, "fwd")
    assert float(out[5].abs().max()) == 0
    up = _rand(*ref.shape, seed=33)
    g64 = torch.autograd.grad((ref * up).sum(), (x64, s64))
    g32 = torch.autograd.grad((out * up.float().to(DEV)).sum(), (x32, s32))
    _close(g32[0], g64[0], "dx")
    _close(g32[1], g64[1], "dscale")
    assert torch.isfinite(g32[0]).all()


def test_extents_beyond_the_grid_caps():
    """Row counts above every kernel's grid cap (pair / attention: 2048 workgroups x 4 rows; norm: 4096 / 256 workgroups;
    edge basis: 1024 x 256 edges): the capped grids loop."""
    from equihgnn_amd import ops
    n, k = 8300, 4
    _pair_case((0, 0), 16, 16, n, k, 41)
    _attn_case(n, k, 1, False, 42)
    x = _rand(n, 32, 3, seed=43)
    ref = se3t_ref.norm_se3(x, torch.ones(32, dtype=torch.float64))
    out = ops.se3t_norm(x.float().to(DEV).transpose(1, 2).contiguous(), torch.ones(1, 1, 32, device=DEV)).transpose(1, 2)
    _close(out, ref, "norm")
    n, k = 17000, 16                                  # 272 000 edges
    g = torch.Generator().manual_seed(44)
    pos = (_rand(n, 3, seed=45) * 3).float()
    nbr = (torch.arange(n)[:, None] + torch.randint(1, n, (n, k), generator=g)) % n
    rel = pos.double()[:, None] - pos.double()[nbr]
    d, maskf, meanw, basis = ops.se3t_edge_basis(pos.to(DEV), nbr.to(torch.int32).to(DEV), 5.0, _qtab())
    assert float((d.cpu().double().view(n, k) - rel.norm(dim=-1)).abs().max()) <= 1e-5
    assert float((basis.cpu().double().view(n, k, 34) - _basis_rows(rel)).abs().max()) <= 1e-6
    near = (rel.norm(dim=-1) - 5.0).abs() > 1e-4      # (slots within rounding of the radius may fall either way)
    assert torch.equal((maskf.cpu() > 0)[near], (rel.norm(dim=-1) <= 5.0)[near])
