"""Plain-torch restatement of the hypergraph row operators (ops/rows.py, ops/aggregate.py, ops.colsum), written as
explicit sums and products from their documented semantics: no F.layer_norm, no F.batch_norm, no autograd.  Every function
takes the inputs, the upstream gradient and a ``dtype`` and returns a dict with the output and every gradient, so the same
text evaluated in float32 is "the reference alone" (what test_hip_row_bounds.py sets its constants from).

``magnitude=True`` returns, under the same keys, A per element: the sum of the absolute values of the element's terms.
Every term is replaced by its absolute value and every subtraction becomes an addition; masks (ReLU, row mask, index
structure) and the statistics mu and rstd are kept.  For LayerNorm:
    A(d) = |r| + |mu|,  A(xhat) = A(d) rstd,  A(y) = A(xhat) |gamma| + |beta|,
    A(dx) = rstd (|g gamma| + mean|g gamma| + A(xhat) mean(|g gamma| A(xhat))) where the ReLU passed, 0 elsewhere,
    A(dgamma) = sum_r |g| A(xhat),  A(dbeta) = sum_r |g|.
A reduction's A is the sum of its entries' A, divided by the degree for the mean (degree 0 counts as 1, as in
torch_scatter).  Indices are int64 vectors: ``v``/``ia`` the source (node) row of an entry, ``e``/``ib`` its hyperedge row."""
import torch


def _v(t, m):
    """a term"""
    return t.abs() if m else t


def _sub(a, b, m):
    """a - b"""
    return a + b if m else a - b


def _seg(vals, idx, n):
    """out[i] = sum_{p: idx[p] = i} vals[p], in the order of p"""
    return torch.zeros((n,) + tuple(vals.shape[1:]), dtype=vals.dtype).index_add_(0, idx, vals)


def _deg(idx, n, dtype):
    """(degree, degree clamped to >= 1) as [n, 1] columns"""
    d = torch.bincount(idx, minlength=n).to(dtype)[:, None]
    return d, d.clamp(min=1)


def _ln_fwd(r, gamma, beta, eps, m):
    """(xhat, rstd, y) of LayerNorm over the last dim of ``r`` (the rows after their ReLU)."""
    C = r.shape[-1]
    mu = r.sum(-1, keepdim=True) / C
    d = r - mu
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / C + eps)
    xhat = (r.abs() + mu.abs() if m else d) * rstd
    return xhat, rstd, xhat * _v(gamma, m) + _v(beta, m)


def _ln_bwd(xhat, rstd, gamma, g, pos, m):
    """dx of LayerNorm (+ the ReLU mask ``pos`` in front of it) for the upstream gradient ``g`` (already |.| with m)."""
    C = xhat.shape[-1]
    gg = g * _v(gamma, m)
    m1 = gg.sum(-1, keepdim=True) / C
    m2 = (gg * xhat).sum(-1, keepdim=True) / C
    return rstd * _sub(_sub(gg, m1, m), xhat * m2, m) * pos


def layer_norm_rows(x, gamma, beta, g, eps=1e-5, dtype=torch.float64, magnitude=False):
    m = magnitude
    x, gamma, beta, g = (t.to(dtype) for t in (x, gamma, beta, g))
    xhat, rstd, y = _ln_fwd(x, gamma, beta, eps, m)
    ga = _v(g, m)
    return {"y": y, "dx": _ln_bwd(xhat, rstd, gamma, ga, torch.ones_like(x), m), "dgamma": (ga * xhat).sum(0),
            "dbeta": ga.sum(0)}


def bias_relu_ln(h, bias, gamma, beta, g, eps=1e-5, dtype=torch.float64, magnitude=False):
    m = magnitude
    h, bias, gamma, beta, g = (t.to(dtype) for t in (h, bias, gamma, beta, g))
    pre = h + bias
    pos = (pre > 0).to(dtype)
    xhat, rstd, y = _ln_fwd(pre * pos, gamma, beta, eps, m)
    ga = _v(g, m)
    dh = _ln_bwd(xhat, rstd, gamma, ga, pos, m)
    return {"y": y, "dh": dh, "dbias": dh.sum(0), "dgamma": (ga * xhat).sum(0), "dbeta": ga.sum(0)}


def gather_ln_reduce(h, bias, gamma, beta, v, e, n_out, g, mean, eps=1e-5, dtype=torch.float64, magnitude=False):
    """out[j] = reduce_{p: e[p] = j} LayerNorm(relu(h[v[p]] + bias)); g [n_out, C]."""
    m = magnitude
    h, bias, gamma, beta, g = (t.to(dtype) for t in (h, bias, gamma, beta, g))
    deg, den = _deg(e, n_out, dtype)
    if not mean:
        den = torch.ones_like(den)
    pre = h + bias
    pos = (pre > 0).to(dtype)
    xhat, rstd, _ = _ln_fwd(pre * pos, gamma, beta, eps, m)
    out = _v(gamma, m) * (_seg(xhat[v], e, n_out) / den) + _v(beta, m) * (deg / den)      # gamma and beta factor out of the sum
    gs = _seg((_v(g, m) / den)[e], v, h.shape[0])           # the gradient of y, one row per source row
    dh = _ln_bwd(xhat, rstd, gamma, gs, pos, m)
    return {"out": out, "dh": dh, "dbias": dh.sum(0), "dgamma": (gs * xhat).sum(0), "dbeta": gs.sum(0)}


def incidence_ln_reduce(pa, qb, gamma, beta, ia, ib, okey, n_out, g, mean, eps=1e-5, dtype=torch.float64,
                        magnitude=False):
    """out[j] = reduce_{p: okey[p] = j} LayerNorm(relu(pa[ia[p]] + qb[ib[p]])); g [n_out, C]."""
    m = magnitude
    pa, qb, gamma, beta, g = (t.to(dtype) for t in (pa, qb, gamma, beta, g))
    deg, den = _deg(okey, n_out, dtype)
    if not mean:
        den = torch.ones_like(den)
    pre = pa[ia] + qb[ib]
    pos = (pre > 0).to(dtype)
    xhat, rstd, _ = _ln_fwd(pre * pos, gamma, beta, eps, m)
    out = _v(gamma, m) * (_seg(xhat, okey, n_out) / den) + _v(beta, m) * (deg / den)       # gamma and beta factor out of the sum
    gp = (_v(g, m) / den)[okey]                              # the gradient of y, one row per incidence
    dpre = _ln_bwd(xhat, rstd, gamma, gp, pos, m)
    return {"out": out, "dpa": _seg(dpre, ia, pa.shape[0]), "dqb": _seg(dpre, ib, qb.shape[0]),
            "dgamma": (gp * xhat).sum(0), "dbeta": gp.sum(0)}


def batch_norm_rows(x, mask, gamma, beta, running_mean, running_var, g, relu, momentum=0.1, eps=1e-5,
                    dtype=torch.float64, magnitude=False):
    """Training-mode BatchNorm1d whose statistics count the rows with mask [R] = 1 (None: all) and are applied to every
    row, the ReLU behind it with ``relu``; the running buffers after the call (running_var takes the unbiased
    variance).  The gradients are those of that function: every row's g enters dgamma, dbeta and, through the statistics,
    the dx of the counted rows."""
    m = magnitude
    x, gamma, beta, rm, rv, g = (t.to(dtype) for t in (x, gamma, beta, running_mean, running_var, g))
    mk = (torch.ones(x.shape[0]) if mask is None else mask).to(dtype)[:, None]
    n = mk.sum()
    mean = (mk * x).sum(0) / n
    d = x - mean
    var = (mk * d * d).sum(0) / n
    rstd = 1.0 / torch.sqrt(var + eps)
    gate = (d * rstd * gamma + beta > 0).to(dtype) if relu else torch.ones_like(x)
    xhat = (x.abs() + mean.abs() if m else d) * rstd
    y = (xhat * _v(gamma, m) + _v(beta, m)) * gate
    ga = _v(g, m) * gate
    dbeta = ga.sum(0)
    dgamma = (ga * xhat).sum(0)
    dx = rstd * _v(gamma, m) * _sub(_sub(ga, mk * dbeta / n, m), mk * xhat * dgamma / n, m)
    unb = var * (n / (n - 1))
    return {"y": y, "dx": dx, "dgamma": dgamma, "dbeta": dbeta,
            "running_mean": _v(rm, m) + momentum * _sub(_v(mean, m), _v(rm, m), m),
            "running_var": _v(rv, m) + momentum * _sub(unb, _v(rv, m), m)}


def reduce_gathered(src, v, e, n_out, g, mean, dtype=torch.float64, magnitude=False):
    """out[j] = reduce_{p: e[p] = j} src[v[p]]"""
    src, g = _v(src.to(dtype), magnitude), _v(g.to(dtype), magnitude)
    deg, den = _deg(e, n_out, dtype)
    if not mean:
        den = torch.ones_like(den)
    return {"out": _seg(src[v], e, n_out) / den, "dsrc": _seg((g / den)[e], v, src.shape[0])}


def reduce_entries(src, key, n_out, g, mean, dtype=torch.float64, magnitude=False):
    """out[j] = reduce_{p: key[p] = j} src[p]"""
    src, g = _v(src.to(dtype), magnitude), _v(g.to(dtype), magnitude)
    deg, den = _deg(key, n_out, dtype)
    if not mean:
        den = torch.ones_like(den)
    return {"out": _seg(src, key, n_out) / den, "dsrc": (g / den)[key]}


def gather_rows(src, key, g, dtype=torch.float64, magnitude=False):
    """out[p] = src[key[p]]"""
    src, g = _v(src.to(dtype), magnitude), _v(g.to(dtype), magnitude)
    return {"out": src[key], "dsrc": _seg(g, key, src.shape[0])}


def row_weights(deg, mode, dtype):
    """w_r of colsum and residual_mix: 1 (mode 0), [row non-empty] (1), the row length (2); ``deg`` int64 [R]."""
    if mode == 0:
        return torch.ones(deg.shape[0], 1, dtype=dtype)
    return ((deg > 0) if mode == 1 else deg).to(dtype)[:, None]


def colsum(x, deg=None, mode=0, scale=1.0, dtype=torch.float64, magnitude=False):
    """scale sum_r w_r x[r]"""
    x = _v(x.to(dtype), magnitude)
    w = row_weights(deg if deg is not None else torch.zeros(x.shape[0], dtype=torch.int64), mode, dtype)
    return {"out": abs(scale) * (w * x).sum(0) if magnitude else scale * (w * x).sum(0)}


def residual_mix(x0, bias, deg, mode, alpha, g, dtype=torch.float64, magnitude=False):
    """out = alpha x0 + (1 - alpha) w_r bias"""
    m = magnitude
    x0, bias, g = (_v(t.to(dtype), m) for t in (x0, bias, g))
    w = row_weights(deg, mode, dtype)
    a, b = (abs(alpha), abs(1.0 - alpha)) if m else (alpha, 1.0 - alpha)
    return {"out": a * x0 + b * w * bias, "dx0": a * g, "dbias": b * (w * g).sum(0)}
