"""The stamps build of the panel kernels (equihgnn_amd/libequihgnn_panel_stamps.so: build.PANEL_SOURCES with -DPN_STAMPS, loaded
beside the product library by bench.py and tools/panel_prologues.py).  The library is linked from objects of its own that
are compiled beside the product's; if it stamps nothing, tools/panel_prologues.measure raises and bench.py falls back to a
recorded profile without failing, so nothing else in the suite would notice.  One launch of a product (hg_panel_gemm_f32) and one of an MHNNConv stage
(HG_CONV_F2) must both leave their stamps, and must compute what the product library computes, bit for bit.

C = 64 and 33 rows: two panels, the second with one live row -- the smallest size with a full and a ragged panel.  C = 64 is
two column tiles of 32, one per multiplying wavefront, with 8 or with 4 wavefronts per panel; stamp 3 sits behind the MFMA
loop, so only those two write it."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C, ROWS, NODES = 64, 33, 40


def _stamped(L, launch, outs):
    """run `launch` on library L with a fresh stamp buffer; returns (stamps [2, 8, 16], the outputs' clones)"""
    buf = torch.zeros(2 * 8 * 16, dtype=torch.int64, device=DEV)
    for o in outs:
        o.fill_(float("nan"))
    assert L.hg_panel_debug_stamps(ctypes.c_void_p(buf.data_ptr())) == 0
    assert launch(L) == 0
    torch.cuda.synchronize()
    return buf.cpu().reshape(2, 8, 16), [o.clone() for o in outs]


def _check_stamps(st, nw):
    for wg in range(2):
        for w in range(nw):
            phases = st[wg, w, [0, 1, 2, 4, 5]]
            assert (phases != 0).all(), (wg, w, st[wg, w])
            assert (phases[1:] >= phases[:-1]).all(), (wg, w, st[wg, w])
            assert (st[wg, w, 3] != 0) == (w < min(nw, C // 32)), (wg, w, st[wg, w])
    assert (st[:, :, 6:] == 0).all() and (st[:, nw:, :] == 0).all()


def test_product_and_conv_stage_of_the_stamps_build_stamp_and_compute_what_the_product_computes():
    from equihgnn_amd import build, hip, ops
    L = hip.load(build.STAMPS_LIB, partial=True)
    nw = int(L.hg_panel_waves())
    assert nw in (4, 8)
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, device=DEV, generator=g)
    (img,) = ops.panel_pack([(rn(C, C) * C ** -0.5, True)])
    bias = rn(C)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # a product: out = x W^T
    x, out = rn(ROWS, C), torch.empty(ROWS, C, device=DEV)
    gemm = lambda lib: lib.hg_panel_gemm_f32(x.data_ptr(), C, ROWS, C, img.data_ptr(), 1.0, None, 0, 0.0, None, 0, out.data_ptr(), C, stream)
    # a stage of MHNNConv, F2: hbar[e] = mean of h1n over the hyperedge's nodes, qb = hbar W^T + bias; hyperedges of one and two nodes
    deg = 1 + torch.arange(ROWS) % 2
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).to(torch.int32).to(DEV)
    col = torch.randint(0, NODES, (int(deg.sum()),), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(DEV)
    h1n, hbar, qb = rn(NODES, C), torch.empty(ROWS, C, device=DEV), torch.empty(ROWS, C, device=DEV)
    a = hip.HgConvPanel()
    for k, v in dict(in0=h1n, rowptr=rowptr, col=col, w0=img, bias_out=bias, out0=hbar, out1=qb).items():
        setattr(a, k, v.data_ptr())
    a.rows, a.C, a.eps, a.eps_inc, a.scale = ROWS, C, 1e-5, 1e-5, 1.0
    f2 = lambda lib: lib.hg_conv_panel(hip.HG_CONV_F2, a, stream)
    try:
        for launch, outs in ((gemm, [out]), (f2, [hbar, qb])):
            st, got = _stamped(L, launch, outs)
            _check_stamps(st, nw)
            assert launch(hip.lib()) == 0
            torch.cuda.synchronize()
            for o, s in zip(outs, got):
                assert torch.isfinite(o).all() and torch.equal(o, s), "the stamps build must not change arithmetic"
    finally:
        assert L.hg_panel_debug_stamps(ctypes.c_void_p(0)) == 0
