"""Row-panel kernels (csrc/panel.hip): weights packed once per step into bf16 planes in MFMA operand order, conv-sized
dense products fused with the row-wise work either side of them.

Part of equihgnn_amd.ops (host-side operators over libequihgnn_hip.so; no CPU fallback).
"""
from __future__ import annotations

import functools
import threading

import torch

from .. import hip, precision
from ._base import (_ptr, _row_view, _stream)

PANEL_WIDTHS = (64, 128, 256)


# The matmul precision of the panel kernels (precision.panel_products(): 6 unless set_float32_matmul_precision(mode, panels=True)).
# panel_pack lays down three planes unless its caller asks for fewer (the operators here pack panel_planes(): what their mode's
# products read).  A product call reads the mode at call time unless it is given `products`; the planes of its images are worked
# out from their SIZE (an image of K x N holds K N 2 bytes per plane: nothing travels beside the tensor that a clone or a slice
# could lose), the images of one call must agree, and the library refuses an image that holds fewer planes than the products
# read.  The backward pass of an autograd node multiplies as its forward pass did, whatever the mode has become in between (its
# images were packed for that count): `backward_as_forward` pins the count for the call.
_PIN = threading.local()


def _products(products=None) -> int:
    if products is not None:
        return int(products)
    pinned = getattr(_PIN, "products", None)
    return precision.panel_products() if pinned is None else pinned


FULL_IMAGES = False     # measurement aid (tools/bench_matmul_precision.py --full-images): the operators pack three planes under every mode


def panel_planes(products=None) -> int:
    """bf16 planes that the operators pack for ``products`` (default: the current mode's) partial products: what they read."""
    return 3 if FULL_IMAGES else precision.PLANES[_products(products)]


def _image_planes(what: str, *images) -> int:
    """The bf16 planes of the images of one call.  ``images``: (image tensor or None, K, N) -- an image of a K x N operand with p
    planes has exactly K N 2 p bytes.  Raises if a size is no whole number of planes in 1..3 or the images disagree."""
    found = set()
    for img, K, N in images:
        if img is None:
            continue
        p, rest = divmod(img.numel() * img.element_size(), K * N * 2)
        if rest or p not in (1, 2, 3):
            raise ValueError(f"{what}: an image of {img.numel() * img.element_size()} bytes is no {K} x {N} operand of 1, 2 or 3 bf16 planes")
        found.add(p)
    if len(found) > 1:
        raise ValueError(f"{what}: the images of one call must hold the same number of planes, not {sorted(found)}")
    return found.pop() if found else 3


def backward_as_forward(fn):
    """Decorator of an autograd Function's ``backward`` whose forward pass stored ``ctx.products = _products()``: the panel
    products inside it take that count (pinned for this thread -- autograd runs it on a thread of its own)."""
    @functools.wraps(fn)
    def backward(ctx, *grads):
        before = getattr(_PIN, "products", None)
        _PIN.products = ctx.products
        try:
            return fn(ctx, *grads)
        finally:
            _PIN.products = before
    return backward


def panel_supported(C: int) -> bool:
    return C in PANEL_WIDTHS


def panel_pack(items, out=None, k_major: bool = False, planes: int = 3):
    """Pack weights for the panel kernels in ONE launch.  ``items`` = [(w, trans)] or [[(w, trans), ...]]: a 2-D fp32 weight
    view ``w`` (unit inner stride) used as B[k][n] = w[n, k] (``trans`` True: x @ w.T) or B[k][n] = w[k, n] (False: dy @ w);
    an inner list stacks its weights along K in one image; (w, trans, n_pad): N zero-padded up to n_pad columns.  Returns one uint8 image tensor per item (views of ``out`` if
    given: a uint8 device buffer of at least panel_pack_bytes(items) bytes).  ``k_major``: the image order the x6 GEMM's pre-split
    B operand takes ([k / 32][tile][k half][plane][lane]) instead of the panel kernels' [tile][k / 16][plane][lane].
    ``planes``: bf16 planes per image, 3 (the default, which serves every mode), 2 or 1: the leading planes only -- a caller
    that multiplies under a reduced mode passes panel_planes(); a ``k_major`` image always has three."""
    L = hip.lib()
    planes = 3 if k_major else int(planes)
    if planes not in (1, 2, 3):
        raise ValueError(f"panel_pack: planes must be 1, 2 or 3, not {planes}")
    groups = [it if isinstance(it, list) else [it] for it in items]
    sizes = []
    for g in groups:
        ks = [(it[0].shape[1] if it[1] else it[0].shape[0]) for it in g]
        ns = {(it[2] if len(it) > 2 else (it[0].shape[0] if it[1] else it[0].shape[1])) for it in g}
        if len(ns) != 1:
            raise ValueError("panel_pack: weights stacked along K must share their N")
        sizes.append((sum(ks), ns.pop()))
    total = sum(K * N * 2 * planes for K, N in sizes)
    dev = groups[0][0][0].device
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=dev)
    elif out.numel() < total or out.dtype != torch.uint8:
        raise ValueError("panel_pack: output buffer too small")
    n = sum(len(g) for g in groups)
    arr = (hip.HgPanelPack * n)()
    keep, views, off, i = [], [], 0, 0
    for g, (K, N) in zip(groups, sizes):
        img = out[off:off + K * N * 2 * planes]
        views.append(img)
        k0 = 0
        for it in g:
            w, tr = it[0], it[1]
            w = _row_view(w.detach(), "panel_pack: w")
            keep.append(w)
            kk = w.shape[1] if tr else w.shape[0]
            if kk % 16 or N % 32:
                raise ValueError(f"panel_pack: K = {kk} must be a multiple of 16 and N = {N} of 32")
            arr[i].w, arr[i].ld, arr[i].dst = w.data_ptr(), w.stride(0), img.data_ptr()
            arr[i].K, arr[i].N, arr[i].trans, arr[i].kstep0, arr[i].ksteps_total = kk, N, 1 if tr else 0, k0 // 16, K // 16
            arr[i].n_valid = w.shape[0] if tr else w.shape[1]
            arr[i].k_major = 1 if k_major else 0
            arr[i].planes = planes
            k0 += kk
            i += 1
        off += K * N * 2 * planes
    hip.check(L.hg_panel_pack(n, arr, _stream(dev)), "hg_panel_pack")
    return views


def panel_pack_bytes(items, planes: int = 3) -> int:
    groups = [it if isinstance(it, list) else [it] for it in items]
    return sum(sum((it[0].shape[1] if it[1] else it[0].shape[0]) for it in g)
               * (g[0][2] if len(g[0]) > 2 else (g[0][0].shape[0] if g[0][1] else g[0][0].shape[1])) * 2 * planes for g in groups)


def panel_gemm(a, wpack, C: int, alpha: float = 1.0, d=None, beta: float = 1.0, bias=None, relu: bool = False, out=None,
               products=None):
    """act(alpha * a @ B + beta * d + bias) for a [rows, C] and a packed [C x C] image (hg_panel_gemm_f32_p)."""
    a = _row_view(a, "panel_gemm: a")
    rows = a.shape[0]
    if a.shape[1] != C or not panel_supported(C):
        raise ValueError(f"panel_gemm: a must be [rows, {C}] with C in {PANEL_WIDTHS}")
    if out is None:
        out = torch.empty((rows, C), dtype=torch.float32, device=a.device)
    if d is not None:
        d = _row_view(d, "panel_gemm: d")
    hip.check(hip.lib().hg_panel_gemm_f32_p(_ptr(a), a.stride(0), rows, C, _ptr(wpack), float(alpha),
                                            _ptr(d) if d is not None else None, d.stride(0) if d is not None else 0, float(beta),
                                            _ptr(bias) if bias is not None else None, 1 if relu else 0, _ptr(out), out.stride(0),
                                            _products(products), _image_planes("panel_gemm", (wpack, C, C)), _stream(a.device)), "hg_panel_gemm_f32_p")
    return out


def panel_stream_supported(K: int, N: int) -> bool:
    return bool(hip.lib().hg_panel_stream_supported(int(K), int(N)))


def panel_stream_gemm(a, w, trans_b: bool = True, alpha: float = 1.0, d=None, beta: float = 1.0, bias=None, relu: bool = False, out=None):
    """act(alpha * a @ op(w) + beta * d + bias) for MANY rows a [rows, K] and a small weight (``trans_b``: w [N, K], an
    nn.Linear weight used as x W^T; else w [K, N], an input gradient dY W), K in {64, 128, 256}, N in {128, 256}: the weight is
    packed into the bf16 planes of the current mode (one launch) and the persistent row-panel kernel streams the rows
    (hg_panel_stream_gemm_f32_p)."""
    a = _row_view(a, "panel_stream_gemm: a")
    rows, K = a.shape
    N = w.shape[0] if trans_b else w.shape[1]
    if (w.shape[1] if trans_b else w.shape[0]) != K or not panel_stream_supported(K, N):
        raise ValueError(f"panel_stream_gemm: a [{rows}, {K}] x weight {tuple(w.shape)} (trans_b={trans_b}) is not a supported shape")
    products = _products()
    (img,) = panel_pack([(w, bool(trans_b))], planes=panel_planes(products))
    if out is None:
        out = torch.empty((rows, N), dtype=torch.float32, device=a.device)
    if d is not None and d is not out:
        d = _row_view(d, "panel_stream_gemm: d")
    if bias is not None:
        bias = bias.detach().contiguous()
    hip.check(hip.lib().hg_panel_stream_gemm_f32_p(_ptr(a), a.stride(0), rows, K, N, _ptr(img), float(alpha),
                                                   _ptr(d) if d is not None else None, d.stride(0) if d is not None else 0, float(beta),
                                                   _ptr(bias) if bias is not None else None, 1 if relu else 0, _ptr(out), out.stride(0),
                                                   products, _image_planes("panel_stream_gemm", (img, K, N)), _stream(a.device)), "hg_panel_stream_gemm_f32_p")
    return out


def _stage_images(stage: int, C: int) -> dict:
    """operand slot -> (K, N) of the weight image a hg_conv_panel stage takes there (include/equihgnn_hip.h)"""
    sq = (C, C)
    if stage == hip.HG_CONV_B1:
        return {"w0": (2 * C, C), "w1": sq, "w2": sq, "w3": sq}
    if stage == hip.HG_EGNN_NODE_F:
        return {"w0": (C + 16, C), "w1": (C + 16, C), "w2": (2 * C, C)}
    if stage == hip.HG_EGNN_NODE_B:
        return {"w0": sq, "w1": sq, "w2": (2 * C, C + 32)}
    return {"w0": sq, "w1": sq, "w2": sq, "w3": sq}


_CP_PTRS = ("in0", "in1", "in2", "in3", "rowptr", "col", "wq", "w0", "w1", "w2", "w3", "b0", "g0", "be0", "b1", "g1", "be1",
            "bias_out", "out0", "out1", "out2", "out3", "out4", "out5", "slab", "slab2", "acc_out", "dbias", "dgamma", "dbeta",
            "dbias2", "dgamma2", "dbeta2", "g_inc", "be_inc", "out6", "signal")


_SD_PROBS = ("p_inc", "p3", "p_x", "p1")
_SD_PTRS = ("seed_inc", "perm", "seed3", "seed_x", "seed1")


def conv_panel(stage: int, rows: int, C: int, device, eps: float = 1e-5, scale: float = 1.0, relu: bool = False,
               acc_first: bool = False, tail: bool = False, accumulate: bool = False, ld0: int = 0, eps_inc: float = 1e-5,
               products=None, drop=None, stack_drop=None, **tensors):
    """One hg_conv_panel stage (include/equihgnn_hip.h lists the operands of each); ``tensors``: name -> device tensor or None.
    ``products``: 6, 3 or 1 partial products per fp32 product (default: the current mode's).
    ``drop`` = (p_inc, seed_inc, perm, p, seed): training dropout of HG_CONV_F3 / HG_CONV_B3 (hg_conv_panel_drop) -- p_inc, an
    int64 seed tensor on the device and the CSR's perm for F3's incidence prologue, p and its seed for the stage's LayerNorm.
    With both probabilities 0 this is the call without the argument.
    ``stack_drop`` = {p_inc, seed_inc, perm, p3, seed3, p_x, seed_x, p1, seed1} (missing keys: 0 / None): the sites of an S-tail
    stack stage under dropout (hg_conv_stack_drop: HG_CONV_F1, _F3, _B1, _B3; include/equihgnn_hip.h says which stage reads
    which).  The entry is called only when a probability is not 0; otherwise this is the call without the argument."""
    a = hip.HgConvPanel()
    a.products = _products(products)
    a.planes = _image_planes(f"conv_panel(stage {stage})", *((tensors.get(k), K, N) for k, (K, N) in _stage_images(stage, C).items()))
    a.rows, a.C, a.eps, a.scale, a.eps_inc = rows, C, float(eps), float(scale), float(eps_inc)
    a.relu, a.acc_first, a.tail, a.accumulate, a.ld0 = int(relu), int(acc_first), int(tail), int(accumulate), int(ld0)
    for k, t in tensors.items():
        if k not in _CP_PTRS:
            raise TypeError(f"conv_panel: unknown operand {k}")
        if t is not None:
            setattr(a, k, t.data_ptr())
    if drop is not None and (float(drop[0]) != 0.0 or float(drop[3]) != 0.0):
        d = hip.HgConvDrop()
        d.p_inc, d.p = float(drop[0]), float(drop[3])
        for k, t in (("seed_inc", drop[1]), ("perm", drop[2]), ("seed", drop[4])):
            if t is not None:
                setattr(d, k, t.data_ptr())
        hip.check(hip.lib().hg_conv_panel_drop(stage, a, d, _stream(device)), f"hg_conv_panel_drop(stage {stage})")
        return
    if stack_drop is not None and any(float(stack_drop.get(k) or 0.0) != 0.0 for k in _SD_PROBS):
        if drop is not None:
            raise TypeError("conv_panel: drop and stack_drop are two entry points, pass one")
        d = hip.HgConvStackDrop()
        for k in _SD_PROBS:
            setattr(d, k, float(stack_drop.get(k) or 0.0))
        for k in _SD_PTRS:
            if stack_drop.get(k) is not None:
                setattr(d, k, stack_drop[k].data_ptr())
        hip.check(hip.lib().hg_conv_stack_drop(stage, a, d, _stream(device)), f"hg_conv_stack_drop(stage {stage})")
        return
    hip.check(hip.lib().hg_conv_panel(stage, a, _stream(device)), f"hg_conv_panel(stage {stage})")


def conv_panel_slab(rows: int, C: int, device):
    """A slab for the vector gradients of an HG_CONV_B3 / HG_CONV_B1 stage (parked until defer_flush while deferred)."""
    from ._base import _workspace
    return _workspace(max(hip.lib().hg_conv_panel_slab_bytes(rows, C), 16), device)
