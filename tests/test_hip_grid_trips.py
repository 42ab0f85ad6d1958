"""Every grid-capped kernel past its cap: the second trip of each grid-stride loop and both sides of each switch in the rows
a wavefront takes, through the public ops (and trainer.FlatAdam) the models call.

Almost every row kernel is launched through eqh_grid_for(work, per_block, cap) and strides over the rest; the backward
kernels of incidence.hip instead give a wavefront a range of rows that grows with the row count.  Below the cap a loop
body runs once, and a second trip is where an accumulator that is not cleared, a prefetch past the end, a wrong stride
or a dropout decision keyed by the trip would show.  Sizes: the first second-trip size + one full workgroup + 1 (full
workgroups, a ragged one and idle ones in the second trip); both sides of a switch; the smallest width the operator takes.

Reference: the same operation in float64 on the host over EVERY row, forward and every gradient, as the operator's own
test does.  The 8-frame tensors (67 M outputs) take float64 on the device, as test_hip_gnn2d does at 70 000 atoms; where
even that is seconds (eigh3, swiglu, the 524 801-row gather) the input is a block of 37 rows repeated (block-diagonally
with its index structure), one period goes against float64 and every row must equal its twin bit for bit.  Outputs land on
poisoned (NaN) memory and are asserted finite; rows that must be zero are asserted == 0.0.  Every case counts the calls of
its native entry points (_count) and fails if the wrapper routed the shape elsewhere.  With p > 0 the keep matrix is
checked bit for bit against ops.dropout_mean on ones with the same seed (_keep_of: every dropout kernel hashes
(seed, flat element index)) and the backward against float64 with that mask; periodicity is used at p = 0 only.

Tolerances: outputs and per-row gradients take the tolerance of the operator's existing float64 test (named in each case).
A parameter gradient summed over all rows takes the larger of that tolerance and 4 x the error of the unfused fp32 torch
composition on the same device against float64, relative to the largest reference entry (_summed_limit; 4: the slab
reductions sum in another order).  [fp32: ...] below is the largest such error measured on an MI355X for the case; 4 x
each of them is below the existing tolerance, so the existing tolerances are what is asserted today.

The capped launches of equihgnn_amd/csrc (file:line; rows or elements per workgroup x cap; first size that takes a second
trip or crosses a switch; where it is covered).  K = test_hip_kernels.py, X = test_hip_extents.py.

incidence.hip
  :853 k_inc_fwd, :876 k_inc_fwd_col, :969 k_gather_ln_fwd, :920 k_rowln_fwd<RELU>, :1207 k_rowln_fwd<!RELU> and their DROP
       forms                     4 x 4096; 16 385 rows    here: test_incidence_ln_reduce_past_the_forward_cap,
                                                          test_gather_ln_reduce_past_the_forward_cap, test_dense_rows_* (16 389 rows);
                                                          NV = 2 with DROP (C = 320, p = 0.25): the *_at_two_float4_per_lane cases and
                                                          gather [C320_drop]                                        [fp32: 4.0e-7]
  :893 k_inc_bwd_both (inc_bwd_body)  bwd_rpw >= 2 from 2049 rows a side    here: test_incidence_backward_around_its_rows_per_wavefront_
                                                          switch (2048 / 2049), rpw = 9 in the 16 389-row cases     [fp32: 1.8e-7]
  :946,:1238 k_rowln_bwd         rowln_blocks: 16 x 256, 16 x 2048 past 65 536 rows; 4097 rows, switch 65 536 / 65 537
                                                          here: test_dense_rows_* [bwd_256_blocks / bwd_2048_blocks]  [fp32: 2.7e-7]
  :998 k_gather_ln_bwd           gl_rpw >= 2 from 8193 source rows (K::test_gather_ln_reduce_matches_float64_reference[*-9000-256]),
                                 capped at 64 from 524 288: blocks grow past 1024
                                                          here: test_gather_ln_reduce_backward_at_its_rows_per_wavefront_cap [fp32: 2.2e-6]
rmsnorm.hip
  :122 k_rms_fwd 4 x 4096; 16 385 rows.  :150 k_rms_bwd rn_blocks 16 x 256; 4097 rows
                                                          here: test_rms_norm_rows_past_both_caps                   [fp32: 1.7e-7]
ln_rowdot.hip
  :211 k_ln_rowdot_fwd 4 x 4096; 16 385 rows              test_hip_faformer_geom.py::test_ln_rowdot_matches_float64[20000-256-2-False], and here
  :248 k_ln_rowdot_bwd lr_blocks as rowln_blocks          here: test_ln_rowdot_around_the_backward_switch           [fp32: 1.7e-6]
faformer_ew.hip
  :214,:228 k_swiglu_drop_*      256 float4 x 8192; 8 388 609 outputs    here: test_swiglu_dropout_past_its_cap
  :243,:246 k_drop_mean_fwd<8>/<0>   same, float4 of output   here: test_dropout_mean_past_its_caps
  :279 k_drop_mean_bwd_f8c256<false>   4 rows x 8192; 32 769 rows       here: test_dropout_mean_past_its_caps[f8c256-plain]
  :312 k_drop_mean_bwd_f8c256<true> (the bias rider)   dm_colsum_blocks (:290) 4 rows x 4096; 16 385 rows
                                                          here: test_dropout_mean_past_its_caps[f8c256-bias_rider]  [fp32: 6.6e-7]
  :282 k_drop_mean_bwd<false>    256 float4 of dx x 8192; 8 388 609 floats of dx    here: test_dropout_mean_past_its_caps[general-plain]
  :315 k_drop_mean_bwd<true> (the bias rider)   dm_colsum_blocks 256 float4 x 4096; 4 194 305 floats of dx
                                                          here: test_dropout_mean_past_its_caps[general-bias_rider] [fp32: 6.6e-7]
  :258 k_dropout_add             256 float4 x 8192; 8 388 609 floats    here: test_dropout_add_past_its_cap
  :646 k_frame_pre_fwd, :688 k_frame_hidden_fwd 4 x 8192; 32 769 rows.  :668 k_frame_pre_bwd, :724 k_frame_hidden_bwd<false>
       (per-row bases), fp_blocks (:635) 32 x 1024; 32 769 rows
                                                          here: test_frame_pre_past_both_caps, test_frame_hidden_past_both_caps[rows-*] [fp32: 2.3e-6]
  :729 k_frame_hidden_bwd<true>  (the vector form: bias + extra * wx inside the kernel; a second slab region behind
       blocks x FH_SLAB for d bias and d wx)   fp_blocks 32 x 1024; 32 769 rows
                                                          here: test_frame_hidden_past_both_caps[vector-*]          [fp32: 2.1e-6]
  :1175 k_rowdot_fwd, :1233 k_gate_fwd 4 x 8192; 32 769 rows.  :1207,:1266 backwards, rd_blocks (:1158) 64 x 1024; 65 537 rows
                                                          here: test_rowdot_past_both_caps, test_gate_rows_past_both_caps [fp32: 1.6e-6]
  :1422 k_edge_hidden_fwd 4 x 8192; 32 769 nodes.  :1452 k_edge_hidden_bwd eh_blocks (:1408) 4 x 1024; 4097 nodes
                                                          here: test_edge_hidden_past_both_caps                     [fp32: 4.2e-7]
attn_pool.hip
  :176 k_attn_pool_fwd 4 x 2048; 8193 nodes.  :206 k_attn_pool_bwd ap_blocks (:157) 8 x 512; 4097 nodes
                                                          here: test_attn_pool_past_both_caps                       [fp32: 5.1e-6]
rowgemm.hip
  :657 the streaming kernels     one row per workgroup, no cap          not reachable (uncapped grid)
  :717,:774 k_rowgemm_fwd_lds / _bwd_z_lds   1 x 2048; 2049 rows        here: test_rowgemm_past_its_caps[lds]
  :735,:791 k_rowgemm_fwd / _bwd_z 4 x 4096; 16 385 rows.  :813 k_rowgemm_bwd_w 4 x 2048; 8193 rows
                                                          here: test_rowgemm_past_its_caps[generic]
  :797 k_rowgemm_bwd_w_lds       1 x 2048                 not reachable (its shapes, Kd = 64 with L = 64 / 256 and Kd = 192 / 256 with
                                                          L = 64, are taken by the streaming kernels first: stream_shape, rowgemm.hip:760;
                                                          only under EQH_ROWGEMM_LDS=1, which stream_on, rowgemm.hip:642, reads once)
radial.hip
  :517 k_radial_fwd_mfma         rm_blocks 128 edges x 512; 65 537      here: test_radial_trunk_past_the_forward_cap    [fp32: 3.4e-6]
  :552 k_radial_bwd_mfma         rm_bwd_blocks 128 x 256; 32 769        K::test_radial_trunk_matches_float64_reference[36864], and here
  :519,:554 k_radial_fwd / _bwd  rt_blocks 64 x 256       not reachable (rt_mfma_on, radial.hip:490: only under EQH_RADIAL_READLANE=1)
se3t.hip
  :492 edge_basis 256 x 1024 edges; :526,:552 pair fwd / bwd, :579,:598 attn fwd / bwd 4 x 2048 atoms; :615 norm fwd 1 x 4096 rows
                                                          test_hip_se3t.py::test_extents_beyond_the_grid_caps
  :535 k_se3t_pool               256 x 2048; 524 289 outputs            here: test_se3t_pooled_pair_past_the_pool_cap
  :636 k_se3t_norm_bwd           st_norm_blocks (:482) 8 x 256; 2049 rows   here: test_se3t_norm_backward_past_its_cap  [fp32: 1.8e-7]
segment_reduce.hip
  :97 k_segment_reduce           256 / LPR rows x 4096 (LPR = 16 at C = 64: 65 537 rows); :145 k_entry_weights 256 x 1024; 262 145 entries
                                                          here: test_reduce_gathered_past_the_row_and_entry_caps
embed.hip
  :136 k_embed_fwd               256 / LPR nodes x 4096   X::test_atom_encoder_backward_counts (8.4 M nodes, forward exact)
csr_build.hip
  :483 k_hist, k_fill            256 x 2048; 524 289 entries.  :488 k_clear 256 x 1024; 262 144 rows
                                                          here: test_csr_build_past_the_entry_passes_cap
  :509 k_sort_rows, :607 k_sort_rows_batch 4 x 4096; 16 385 rows    K::test_csr_build_matches_stable_sort[100000-40000-5],
                                                          K::test_csr_build_batch_matches_stable_sort
  :628 k_index_aux               256 x 1024; 262 145 items              here: test_index_aux_past_its_cap
eigh3.hip
  :37 k_eigh3                    128 x 4096; 524 289 matrices           here: test_eigh3_past_its_cap
optim.hip
  :170 k_adam                    16 floats x 256 x 2048; n > 8 388 608 (the prefetched second pass)
                                                          here: test_flat_adam_second_pass_ragged_quad_and_tail
  :195 k_copy_many               4096 floats x 256 per tensor; 1 048 577 floats    here: test_copy_many_past_its_cap
dense_aux.hip
  :286 k_residual_mix            256 float4 x 4096; 1 048 577 float4    here: test_residual_mix_past_its_cap            [fp32: 1.9e-7]
  :298,:311 k_pack_fwd / k_pack_bwd   256 x 2048; 524 289 elements      here: test_egnn_pack_weights_past_its_cap
  :201,:229 k_colsum*            32 rows per chunk, one chunk per workgroup    X::test_colsum_around_its_grid
common.h
  :40 eqh_k_zero                 256 x 1024; 262 145 floats   not reachable (every caller clears one parameter's gradient, tens of
                                                          thousands of floats at most, and most only for an empty input)
  :122,:130 eqh_k_reduce_slabs   64 x 2048; 131 073 elements  here: test_accumulate_past_the_reduction_cap (one slab, eqh_accumulate);
                                                          the 2-D form: K::test_wgrad_matches_float64[3000-2176-256] (557 056 elements)
egnn_edge.hip
  :939 k_edge_fwd_x3, :1010 k_edge_fwd   2 or 4 nodes x 256; 513 / 1025 atoms    K::test_egnn_edge_fused_matches_float64_reference[1283-576-6]
  :1077 k_edge_bwd_prep          prep_blocks (:1027) 4 x 2048; 8193 atoms   here: test_egnn_edge_past_the_backward_prep_cap   [fp32: 2.4e-6]
gnn2d.hip
  :245 k_edge_msg_fwd 256 / (C / 4) rows x 16 384; :282 the backward, bwd_blocks (:198) 32 x 2048; 65 537 rows
                                                          test_hip_gnn2d.py::test_edge_msg_large_n_matches_float64 (70 000 atoms, C = 300)
  :229 k_edge_codes              256 x 4096; 1 048 577 edges            here: test_edge_codes_past_their_cap
faformer_geom.hip
  :443 k_moments (moments_grid :433, the partial table the centre-mix and cloud-frame passes read)   256 x 128; 32 769 rows
                                                          test_hip_faformer_geom.py::test_centre_mix_matches_float64[70000-True],
                                                          ::test_cloud_frame_matches_the_unfused_frame[70000-False]
  :455-:554 k_centre_mix_*, k_cloud_frame_*, k_edge_frame_*, k_attn_logits_*, k_elw_*: cap 1 << 30
                                                          not reachable (2^30 workgroups of 128 or 256 rows)
knn.hip :162 4 x 2048                                     K::test_counted_knn_and_csr_build_match_the_plain_pair[9000-16-1], X::test_knn_around_the_grid_limit
pool_pair.hip :120, :139                                  test_hip_pool_pair.py::test_forward_around_its_grid_caps, ::test_backward_around_its_grid_caps
visnet.hip :600 row_grid, GRID_CAP 16 384                 test_hip_visnet_extents.py (CAP_SIZES)
panel.hip, gemm_x6.hip, wgrad.hip, bn_rows.hip, readout.hip, knn_grid.hip, collate.hip, small_mm.hip, edge_geom.hip
                                                          no eqh_grid_for and none of the block-count helpers: not listed here
                                                          (K::test_panel_*, K::test_gemm_x6_*, K::test_wgrad_*; their limits in X)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_models as O  # noqa: E402
from test_hip_extents import _release  # noqa: E402
from test_hip_kernels import _np_csr  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional


def _ops():
    from equihgnn_amd import ops
    return ops


def _poison(*numels):
    """_poison of test_hip_extents for several blocks at once: freed blocks of NaNs that the next allocations of those sizes
    come back holding, so a row a kernel never writes stays NaN."""
    t = [torch.full((n,), float("nan"), dtype=torch.float32, device=DEV) for n in numels]
    del t


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _keep_of(shape, p, seed):
    """The keep factors (0 or 1 / (1 - p)) of a tensor of ``shape``: ops.dropout_mean on ones, averaging over one frame, with
    the same seed -- every dropout kernel hashes (seed, flat element index)."""
    n = int(np.prod(shape))
    return _ops().dropout_mean(torch.ones(n // shape[-1], 1, shape[-1], device=DEV), p, seed).reshape(shape)


def _count(monkeypatch, *names):
    """Count the calls of the native entry points ``names`` (the attributes of the loaded library every wrapper looks up)."""
    from equihgnn_amd import hip
    lib, calls = hip.lib(), {n: 0 for n in names}
    for n in names:
        def counted(*a, _n=n, _inner=getattr(lib, n)):
            calls[_n] += 1
            return _inner(*a)
        monkeypatch.setattr(lib, n, counted, raising=True)
    return calls


def _ran(calls):
    """every counted entry point was called"""
    assert all(c > 0 for c in calls.values()), calls


def _rows_close(got, ref, atol, rtol, what):
    """every entry of ``got`` (device fp32) within atol + rtol |ref| of the float64 ``ref`` (host); NaN (a row never
    written onto the poisoned block) fails"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, what
    assert bool(torch.isfinite(got).all()), (what, "rows left unwritten")
    over = (got - ref).abs() - (atol + rtol * ref.abs())
    assert float(over.max()) <= 0.0, (what, float(over.max()), int(over.argmax()) // max(1, ref.shape[-1]))


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp(min=1e-9))


def _summed_limit(name, existing, got32, ref):
    """The limit of a gradient summed over all rows: the larger of the existing test's tolerance and 4 x the error of the
    unfused fp32 torch composition on the same device, relative to the largest reference entry (4: the slab reductions
    sum in another order)."""
    e32 = _rel(got32, ref)
    print(f"    {name}: fp32 torch composition {e32:.2e}")
    return max(existing, 4.0 * e32)


def _compare(tag, outs, refs, grads, rgrads, grads32, per_row, summed, out_tol, row_tol, sum_tol):
    """Outputs and per-row gradients at the operator's own tolerances, the summed parameter gradients at _summed_limit."""
    for (name, o), r in zip(outs, refs):
        _rows_close(o, r.detach(), out_tol[0], out_tol[1], (tag, name))
    for name in per_row:
        err = _rel(grads[name], rgrads[name])
        print(f"{tag} {name}: {err:.2e}")
        assert bool(torch.isfinite(grads[name]).all()), (tag, name)
        assert err < row_tol, (tag, name, err)
    for name in summed:
        lim = _summed_limit(f"{tag} {name}", sum_tol, grads32[name], rgrads[name])
        err = _rel(grads[name], rgrads[name])
        print(f"{tag} {name}: {err:.2e} (limit {lim:.2e})")
        assert err <= lim, (tag, name, err, lim)


# ---- k_rowln_fwd<RELU> / <!RELU>, k_rowln_bwd (incidence.hip): 4 rows x 4096 forward; rowln_blocks 256 <-> 2048 -----------------
def _dense_case(R, C, relu, p, monkeypatch):
    ops = _ops()
    g = torch.Generator().manual_seed(R + C)
    h = torch.randn(R, C, generator=g) - (0.0 if relu else 0.5)
    b = 0.3 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = torch.randn(R, C, generator=g)
    seed = _seed(9000 + R + C)
    s = 1.0 / (1.0 - p)
    names = ((("hg_bias_relu_ln_drop_fwd", "hg_bias_relu_ln_drop_bwd") if p > 0 else ("hg_bias_relu_ln_fwd", "hg_bias_relu_ln_bwd"))
             if relu else ("hg_layer_norm_fwd", "hg_layer_norm_bwd"))
    calls = _count(monkeypatch, *names)
    keep = None
    if p > 0:       # the keep matrix of every row, second-trip rows included, bit for bit
        keep = _keep_of((R, C), p, seed)
        _poison(R * C)
        got = ops.bias_relu_ln(h.to(DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                               p=p, seed=seed)
        assert torch.equal(got, keep)
        del got

    def run(t, fused, kp):
        if fused:
            _poison(R * C)
            if relu:
                out = ops.bias_relu_ln(t[0], t[1], t[2], t[3], p=p, seed=seed) if p > 0 else ops.bias_relu_ln(t[0], t[1], t[2], t[3])
            else:
                out = ops.layer_norm_rows(t[0], t[2], t[3])
            _poison(R * C)
        else:
            out = F.layer_norm(torch.relu(t[0] + t[1]) if relu else t[0], (C,), t[2], t[3], 1e-5)
            if kp is not None:
                out = out * kp.to(out)
        (out * w.to(out)).sum().backward()
        return out

    t64 = [x.double().requires_grad_(True) for x in (h, b, gamma, beta)]
    ref = run(t64, False, None if keep is None else keep.cpu())
    d = [x.to(DEV).requires_grad_(True) for x in (h, b, gamma, beta)]
    out = run(d, True, None)
    d32 = [x.to(DEV).requires_grad_(True) for x in (h, b, gamma, beta)]
    run(d32, False, keep)
    torch.cuda.synchronize()
    _ran(calls)
    keys = ("dh", "dbias", "dgamma", "dbeta") if relu else ("dh", "dgamma", "dbeta")
    pick = (0, 1, 2, 3) if relu else (0, 2, 3)
    _compare(f"dense relu={relu} R={R} C={C} p={p}", [("out", out)], [ref], {k: d[i].grad for k, i in zip(keys, pick)},
             {k: t64[i].grad for k, i in zip(keys, pick)}, {k: d32[i].grad for k, i in zip(keys, pick)}, ("dh",), keys[1:],
             (2e-5 * s, 1e-5), 3e-5 * s, 3e-5 * s)
    _release()


@pytest.mark.parametrize("R", [16384 + 4 + 1, 65536, 65537], ids=["fwd_second_trip", "bwd_256_blocks", "bwd_2048_blocks"])
@pytest.mark.parametrize("relu", [True, False], ids=["bias_relu_ln", "layer_norm_rows"])
def test_dense_rows_past_the_forward_cap_and_around_the_backward_switch(R, relu, monkeypatch):
    """ops.bias_relu_ln / ops.layer_norm_rows at C = 64 against float64 on every row; tolerances of
    test_bias_relu_ln_matches_float64_reference / test_layer_norm_rows_matches_float64_reference."""
    _dense_case(R, 64, relu, 0.0, monkeypatch)


def test_dense_rows_with_dropout_at_two_float4_per_lane(monkeypatch):
    """k_rowln_fwd / k_rowln_bwd <NV = 2, RELU, DROP> (C = 320, p = 0.25) past the forward cap: the keep matrix bit for bit,
    forward and backward against float64 with that mask; tolerances of test_bias_relu_ln_dropout_matches_float64_reference."""
    _dense_case(16384 + 4 + 1, 320, True, 0.25, monkeypatch)


# ---- k_gather_ln_fwd (4 x 4096 output rows), k_gather_ln_bwd (gl_rpw rows per wavefront) -------------------------------------------
@pytest.mark.parametrize("C,p", [(64, 0.0), (320, 0.25)], ids=["C64", "C320_drop"])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_gather_ln_reduce_past_the_forward_cap(C, p, reduce, monkeypatch):
    """ops.gather_ln_reduce with 16 389 output rows (a long row and an empty row among the five of the second trip) over
    16 400 source rows (gl_rpw = 3), float64 on every row; tolerances of test_gather_ln_reduce_matches_float64_reference
    (x 1 / (1 - p) as test_gather_ln_reduce_dropout_matches_float64_reference)."""
    ops = _ops()
    M, N = 16384 + 4 + 1, 16400
    nnz = 3 * N
    g = torch.Generator().manual_seed(N + C)
    v = torch.randint(0, N, (nnz,), generator=g)
    e = torch.randint(0, M, (nnz,), generator=g)
    v[v == N - 2] = N - 1                                  # source row N - 2 is never gathered
    e[e == M - 2] = M - 1                                  # output row M - 2 (second trip) is empty
    v[:150] = 3                                            # a source row with 150 entries
    e[200:300] = M - 4                                     # an output row of the second trip with 100 entries
    h, b = torch.randn(N, C, generator=g), 0.3 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = torch.randn(M, C, generator=g)
    seed = _seed(2000 + C)
    s = 1.0 / (1.0 - p)
    calls = _count(monkeypatch, *(("hg_gather_ln_reduce_drop_fwd", "hg_gather_ln_reduce_drop_bwd") if p > 0
                                  else ("hg_gather_ln_reduce_fwd", "hg_gather_ln_reduce_bwd")))
    by_v = ops.csr_build(v.to(DEV), e.to(DEV), N)
    by_e = ops.csr_build(e.to(DEV), v.to(DEV), M)
    keep = None
    if p > 0:
        keep = _keep_of((N, C), p, seed)
        # one entry per output row: the row IS the keep row of its source, second trip included
        src = torch.randint(0, N, (M,), generator=g).to(DEV)
        one = ops.csr_build(torch.arange(M, device=DEV), src, M)
        one_t = ops.csr_build(src, torch.arange(M, device=DEV), N)
        _poison(M * C)
        got = ops.gather_ln_reduce(h.to(DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                                   one, one_t, reduce, p=p, seed=seed)
        assert torch.equal(got, keep[src])
        del got

    def run(t, fused, kp):
        if fused:
            _poison(M * C)
            out = ops.gather_ln_reduce(t[0], t[1], t[2], t[3], by_e, by_v, reduce, p=p, seed=seed) if p > 0 \
                else ops.gather_ln_reduce(t[0], t[1], t[2], t[3], by_e, by_v, reduce)
            _poison(N * C)
        else:
            y = F.layer_norm(torch.relu(t[0] + t[1]), (C,), t[2], t[3], 1e-5)
            if kp is not None:
                y = y * kp.to(y)
            out = O.segment_reduce(y[v.to(y.device)], e.to(y.device), M, reduce)
        (out * w.to(out)).sum().backward()
        return out

    t64 = [x.double().requires_grad_(True) for x in (h, b, gamma, beta)]
    ref = run(t64, False, None if keep is None else keep.cpu())
    d = [x.to(DEV).requires_grad_(True) for x in (h, b, gamma, beta)]
    out = run(d, True, None)
    d32 = [x.to(DEV).requires_grad_(True) for x in (h, b, gamma, beta)]
    run(d32, False, keep)
    torch.cuda.synchronize()
    _ran(calls)
    assert float(out[M - 2].detach().abs().max()) == 0.0
    assert float(d[0].grad[N - 2].abs().max()) == 0.0
    keys = ("dh", "dbias", "dgamma", "dbeta")
    _compare(f"gather_ln C={C} {reduce} p={p}", [("out", out)], [ref], {k: x.grad for k, x in zip(keys, d)},
             {k: x.grad for k, x in zip(keys, t64)}, {k: x.grad for k, x in zip(keys, d32)}, ("dh",), keys[1:],
             (3e-5 * s, 1e-5), 3e-5 * s, 3e-5 * s)
    _release()


# ---- k_inc_fwd / k_inc_fwd_col (4 x 4096 output rows), inc_bwd_body through k_inc_bwd_both (bwd_rpw rows per wavefront) -------------
def _incidence_case(N, M, C, path, reduce, p, monkeypatch):
    """ops.incidence_ln_reduce over N node rows and M hyperedge rows, 3 N incidences: a row of 70 incidences in the first
    workgroup and another three rows before the end, an empty row next to the last on both sides."""
    ops = _ops()
    nnz = 3 * N
    g = torch.Generator().manual_seed(N + C)
    v = torch.randint(0, N, (nnz,), generator=g)
    e = torch.randint(0, M, (nnz,), generator=g)
    v[v == N - 2] = N - 1
    e[e == M - 2] = M - 1
    v[:70] = 3
    v[70:140] = N - 4
    pa, qb = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    by_b = path == "rows_are_b"
    R = M if by_b else N
    w = torch.randn(R, C, generator=g)
    seed = _seed(3000 + C)
    s = 1.0 / (1.0 - p)
    fwd = "hg_incidence_ln_reduce" + ("_drop" if p > 0 else "") + ("_fwd" if path == "generic" else "_fwd_col")
    calls = _count(monkeypatch, fwd, "hg_incidence_ln_reduce_drop_bwd" if p > 0 else "hg_incidence_ln_reduce_bwd")
    by_v = ops.csr_build(v.to(DEV), e.to(DEV), N)
    by_e = ops.csr_build(e.to(DEV), v.to(DEV), M)
    v32, e32 = v.to(DEV).int(), e.to(DEV).int()
    okey = {"generic": v.to(DEV).int(), "rows_are_a": v32, "rows_are_b": e32}[path]
    keep = _keep_of((nnz, C), p, seed) if p > 0 else None
    if p > 0:
        # one incidence per output row: the row IS the keep row of that incidence (positions 0 .. R - 1 of the same hash)
        zeros, ones = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        ar = torch.arange(R, device=DEV)
        oth = torch.randint(0, M if not by_b else N, (R,), generator=g).to(DEV)
        a1, b1 = (oth, ar) if by_b else (ar, oth)
        ca, cb = ops.csr_build(a1, b1, N), ops.csr_build(b1, a1, M)
        a32, b32 = a1.int(), b1.int()
        ok1 = {"generic": ar.int(), "rows_are_a": a32, "rows_are_b": b32}[path]
        _poison(R * C)
        got = ops.incidence_ln_reduce(pa.to(DEV), qb.to(DEV), zeros, ones, a32, b32, ca, cb, cb if by_b else ca, ok1, reduce,
                                      p=p, seed=seed)
        assert torch.equal(got, keep[:R])
        del got

    def run(t, fused, kp):
        if fused:
            _poison(R * C)
            kw = dict(p=p, seed=seed) if p > 0 else {}
            out = ops.incidence_ln_reduce(t[0], t[1], t[2], t[3], v32, e32, by_v, by_e, by_e if by_b else by_v, okey, reduce, **kw)
            _poison(N * C, M * C)
        else:
            dv = t[0].device
            hh = F.layer_norm(torch.relu(t[0][v.to(dv)] + t[1][e.to(dv)]), (C,), t[2], t[3], 1e-5)
            if kp is not None:
                hh = hh * kp.to(hh)
            out = O.segment_reduce(hh, (e if by_b else v).to(dv), R, reduce)
        (out * w.to(out)).sum().backward()
        return out

    t64 = [x.double().requires_grad_(True) for x in (pa, qb, gamma, beta)]
    ref = run(t64, False, None if keep is None else keep.cpu())
    d = [x.to(DEV).requires_grad_(True) for x in (pa, qb, gamma, beta)]
    out = run(d, True, None)
    d32 = [x.to(DEV).requires_grad_(True) for x in (pa, qb, gamma, beta)]
    run(d32, False, keep)
    torch.cuda.synchronize()
    _ran(calls)
    assert float(out[R - 2].detach().abs().max()) == 0.0
    assert float(d[0].grad[N - 2].abs().max()) == 0.0 and float(d[1].grad[M - 2].abs().max()) == 0.0
    keys = ("dpa", "dqb", "dgamma", "dbeta")
    _compare(f"incidence N={N} C={C} {path} {reduce} p={p}", [("out", out)], [ref], {k: x.grad for k, x in zip(keys, d)},
             {k: x.grad for k, x in zip(keys, t64)}, {k: x.grad for k, x in zip(keys, d32)}, ("dpa", "dqb"), keys[2:],
             (3e-5 * s, 1e-5), 2e-5 * s, 2e-5 * s)
    _release()


@pytest.mark.parametrize("path", ["generic", "rows_are_a", "rows_are_b"])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_incidence_ln_reduce_past_the_forward_cap(path, reduce, monkeypatch):
    """16 389 rows per side at C = 64 (bwd_rpw = 9), every forward form; tolerances of
    test_incidence_ln_reduce_matches_float64_reference."""
    _incidence_case(16384 + 4 + 1, 16384 + 4 + 1, 64, path, reduce, 0.0, monkeypatch)


@pytest.mark.parametrize("rows", [2048, 2049], ids=["one_row_per_wave", "two_rows_per_wave"])
def test_incidence_backward_around_its_rows_per_wavefront_switch(rows, monkeypatch):
    """bwd_rpw = 1 at 2048 rows per side and 2 at 2049, where the last workgroup of each side has three idle wavefronts."""
    _incidence_case(rows, rows, 64, "rows_are_a", "mean", 0.0, monkeypatch)


@pytest.mark.parametrize("path", ["generic", "rows_are_a"])
def test_incidence_ln_reduce_with_dropout_at_two_float4_per_lane(path, monkeypatch):
    """k_inc_fwd / k_inc_fwd_col / k_inc_bwd_both <NV = 2, DROP> (C = 320, p = 0.25) past the forward cap; tolerances of
    test_incidence_ln_reduce_dropout_matches_float64_reference."""
    _incidence_case(16384 + 4 + 1, 16384 + 4 + 1, 320, path, "mean", 0.25, monkeypatch)


# ---- k_rms_fwd (4 x 4096 rows), k_rms_bwd (16 x 256 rows) -------------------------------------------------------------------------
def test_rms_norm_rows_past_both_caps(monkeypatch):
    """ops.rms_norm_rows at 16 389 rows of 64 (a zero row in the second trip); tolerances of
    test_rms_norm_rows_matches_float64_reference."""
    ops = _ops()
    R, C, eps = 16384 + 4 + 1, 64, 1e-12
    g = torch.Generator().manual_seed(R + C)
    t, gam, w = torch.randn(R, C, generator=g), 1 + 0.3 * torch.randn(C, 1, generator=g), torch.randn(R, C, generator=g)
    t[R - 3] = 0.0
    calls = _count(monkeypatch, "eqf_rms_norm_fwd", "eqf_rms_norm_bwd")

    def run(x, gm, fused):
        if fused:
            _poison(R * C)
            out = ops.rms_norm_rows(x, gm, eps)
            _poison(R * C)
        else:
            out = x / (x.norm(dim=-1, keepdim=True) * (C ** -0.5)).clamp(min=eps) * gm[:, 0]
        (out * w.to(out)).sum().backward()
        return out

    td, gd = t.double().requires_grad_(True), gam.double().requires_grad_(True)
    ref = run(td, gd, False)
    tm, gm = t.to(DEV).requires_grad_(True), gam.to(DEV).requires_grad_(True)
    out = run(tm, gm, True)
    t32, g32 = t.to(DEV).requires_grad_(True), gam.to(DEV).requires_grad_(True)
    run(t32, g32, False)
    torch.cuda.synchronize()
    _ran(calls)
    _rows_close(out, ref.detach(), 2e-6, 2e-6, "rms out")
    assert float(out[R - 3].detach().abs().max()) == 0.0
    live = torch.ones(R, dtype=torch.bool)
    live[R - 3] = False                                  # the zero row: gradient of size 1 / eps, compared relatively
    got = tm.grad.cpu().double()
    assert bool(torch.isfinite(got).all())
    assert float((got[R - 3] - td.grad[R - 3]).abs().max() / td.grad[R - 3].abs().max()) < 1e-5
    err = float((got[live] - td.grad[live]).abs().max() / td.grad[live].abs().max())
    print(f"rms dt: {err:.2e}")
    assert err < 2e-5, err
    lim = _summed_limit("rms dg", 2e-5, g32.grad, gd.grad)
    errg = _rel(gm.grad, gd.grad)
    print(f"rms dg: {errg:.2e} (limit {lim:.2e})")
    assert errg <= lim, (errg, lim)
    _release()


# ---- k_ln_rowdot_fwd (4 x 4096 rows), k_ln_rowdot_bwd (lr_blocks 256 <-> 2048) -------------------------------------------------------
@pytest.mark.parametrize("R", [65536, 65537], ids=["bwd_256_blocks", "bwd_2048_blocks"])
def test_ln_rowdot_around_the_backward_switch(R, monkeypatch):
    """ops.ln_rowdot at C = 64, J = 2 with the alias's gradient and a strided upstream gradient; tolerances of
    test_ln_rowdot_matches_float64."""
    ops = _ops()
    C, J = 64, 2
    g = torch.Generator().manual_seed(R + C + J)
    x = torch.randn(R, C, generator=g) * 2 + 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    U, cb = torch.randn(J, C, generator=g), torch.randn(J, generator=g)
    wx, wl, wa = torch.randn(R, 2 * C, generator=g), torch.randn(R, J, generator=g), torch.randn(R, C, generator=g)
    calls = _count(monkeypatch, "faf_ln_rowdot_fwd", "faf_ln_rowdot_bwd")

    def run(t, fused):
        if fused:
            _poison(R * C)
            xe, le, xa = ops.ln_rowdot(t[0], t[1], t[2], t[3], t[4], 1e-5)
            _poison(R * C)
        else:
            xe = F.layer_norm(t[0], (C,), t[1], t[2], 1e-5)
            le, xa = xe @ t[3].T + t[4], t[0]
        ((torch.cat((xe, xe), 1) * wx.to(xe)).sum() + (le * wl.to(xe)).sum() + (xa * wa.to(xe)).sum()).backward()
        return xe, le

    t64 = [a.double().requires_grad_(True) for a in (x, gamma, beta, U, cb)]
    xe64, le64 = run(t64, False)
    d = [a.to(DEV).requires_grad_(True) for a in (x, gamma, beta, U, cb)]
    xe, le = run(d, True)
    d32 = [a.to(DEV).requires_grad_(True) for a in (x, gamma, beta, U, cb)]
    run(d32, False)
    torch.cuda.synchronize()
    _ran(calls)
    _rows_close(xe, xe64.detach(), 2e-5, 1e-5, "xe")
    _rows_close(le, le64.detach(), 3e-4, 1e-5, "le")
    keys = ("dx", "dgamma", "dbeta", "dU", "dcb")
    _compare(f"ln_rowdot R={R}", [], [], {k: a.grad for k, a in zip(keys, d)}, {k: a.grad for k, a in zip(keys, t64)},
             {k: a.grad for k, a in zip(keys, d32)}, ("dx",), keys[1:], None, 3e-5, 3e-5)
    _release()


# ---- k_adam (optim.hip): 16 floats x 256 threads x 2048 workgroups per pass ------------------------------------------------------------
def test_flat_adam_second_pass_ragged_quad_and_tail(monkeypatch):
    """trainer.FlatAdam over n = 8 388 608 + 16 x 256 + 3 floats -- a second (prefetched) pass of two workgroups' worth, a
    ragged quad and a ragged tail -- three steps against torch.optim.Adam on the device, with weight decay, the gradient and a
    second buffer cleared by the kernel; tolerances of test_flat_adam_matches_torch_adam.  64 guard floats behind each buffer."""
    from equihgnn_amd.trainer import FlatAdam
    n, guard, nz = 8388608 + 16 * 256 + 3, 64, 4 * (256 * 2048 + 256 + 1)
    mark = 7.25
    gen = torch.Generator(device=DEV).manual_seed(2)
    bufs = [torch.full((n + guard,), mark, device=DEV) for _ in range(4)]      # param, grad, exp_avg, exp_avg_sq
    also = torch.full((nz + guard,), mark, device=DEV)
    w0 = torch.randn(n, generator=gen, device=DEV)
    bufs[0][:n] = w0
    bufs[2][:n] = 0.0
    bufs[3][:n] = 0.0
    p1 = torch.nn.Parameter(bufs[0][:n])
    p2 = torch.nn.Parameter(w0.clone())
    p1.grad = bufs[1][:n]
    o1 = FlatAdam(p1, lr=1e-2, weight_decay=0.1)
    o1.state[p1]["exp_avg"], o1.state[p1]["exp_avg_sq"] = bufs[2][:n], bufs[3][:n]
    o1.zero_grad_in_step, o1.zero_also = True, (lambda: also[:nz])
    o2 = torch.optim.Adam([p2], lr=1e-2, weight_decay=0.1)
    calls = _count(monkeypatch, "eqh_adam_step")
    for t in range(3):
        gr = torch.randn(n, generator=gen, device=DEV) * (0.5 + t)
        p1.grad.copy_(gr)
        p2.grad = gr
        also[:nz] = 1.0 + t
        o1.sync_lr()
        o1.step()
        o2.step()
        a, b = p1.detach(), p2.detach()
        assert bool(torch.isfinite(a).all())
        over = (a - b).abs() - (2e-7 + 2e-6 * b.abs())
        assert float(over.max()) <= 0.0, (t, float(over.max()), int(over.argmax()))
        assert float(p1.grad.abs().max()) == 0.0 and float(also[:nz].abs().max()) == 0.0, t
    assert calls["eqh_adam_step"] == 3
    assert o1.state[p1]["step_block"].tolist() == [3, 0]
    for buf in bufs:
        assert bool((buf[n:] == mark).all())
    assert bool((also[nz:] == mark).all())
    del bufs, also, p1, p2, o1, o2, w0, gr
    _release()


# ---- csr_build.hip: the passes over the entries (256 x 2048) ---------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [300, 40000, 262144 + 256 + 1])
def test_csr_build_past_the_entry_passes_cap(n_rows, monkeypatch):
    """524 288 + 257 entries (k_hist / k_fill take a second trip: one full workgroup and one entry) against the stable sort,
    bit for bit, on poisoned index arrays; over 300 rows, 40 000 rows, and as many rows as take the counter clear (k_clear,
    256 x 1024) round again."""
    ops = _ops()
    nnz = 524288 + 257
    rng = np.random.default_rng(n_rows)
    key = rng.integers(0, n_rows, size=nnz)
    other = rng.integers(0, 1000, size=nnz)
    calls = _count(monkeypatch, "hg_csr_build")
    t = [torch.full((nnz,), -7, dtype=torch.int32, device=DEV) for _ in range(2)]   # perm and col come back holding -7
    del t
    csr = ops.csr_build(torch.from_numpy(key).to(DEV), torch.from_numpy(other).to(DEV), n_rows)
    rp, perm, col = _np_csr(key, other, n_rows)
    assert np.array_equal(csr.rowptr.cpu().numpy(), rp)
    assert np.array_equal(csr.perm.cpu().numpy(), perm)
    assert np.array_equal(csr.col.cpu().numpy(), col)
    csr2 = ops.csr_build(torch.from_numpy(key).to(DEV), None, n_rows, col_div=3)
    assert np.array_equal(csr2.col.cpu().numpy(), perm // 3)
    assert calls["hg_csr_build"] == 2
    _release()


# ---- k_segment_reduce (256 / LPR rows x 4096; LPR = 16 at C = 64), k_entry_weights (256 x 1024 entries) ---------------------------
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_reduce_gathered_past_the_row_and_entry_caps(reduce, monkeypatch):
    """ops.reduce_gathered over 65 553 rows per side (65 536 + 16 + 1) and 262 412 entries (> 262 144 + 256 + 1: the mean's
    entry weights), forward and the weighted backward against float64; tolerances of
    test_reduce_gathered_and_gather_rows_vs_oracle."""
    ops = _ops()
    N = M = 65536 + 16 + 1
    C, nnz = 64, 4 * N + 200
    g = torch.Generator().manual_seed(7)
    v, e = torch.randint(0, N, (nnz,), generator=g), torch.randint(0, M, (nnz,), generator=g)
    v[v == N - 2] = N - 1
    e[e == M - 2] = M - 1
    X, w = torch.randn(N, C, generator=g), torch.randn(M, C, generator=g)
    calls = _count(monkeypatch, "hg_segment_reduce_f32", *(("hg_entry_weights", "hg_segment_reduce_w_f32") if reduce == "mean" else ()))
    Xc = X.double().requires_grad_(True)
    ref = O.segment_reduce(Xc[v], e, M, reduce)
    (ref * w.double()).sum().backward()
    by_e, by_v = ops.csr_build(e.to(DEV), v.to(DEV), M), ops.csr_build(v.to(DEV), e.to(DEV), N)
    Xd = X.to(DEV).requires_grad_(True)
    _poison(M * C)
    out = ops.reduce_gathered(Xd, by_e, by_v, reduce)
    _poison(N * C)
    (out * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _ran(calls)
    _rows_close(out, ref.detach(), 1e-5, 1e-5, "out")
    _rows_close(Xd.grad, Xc.grad, 2e-5, 1e-5, "dX")
    assert float(out[M - 2].detach().abs().max()) == 0.0 and float(Xd.grad[N - 2].abs().max()) == 0.0
    _release()


# ---- k_rowdot_* / k_gate_* (faformer_ew.hip): 4 x 8192 rows forward, rd_blocks 64 x 1024 rows backward ---------------------------------
@pytest.mark.parametrize("passthrough", [False, True], ids=["plain", "passthrough"])
def test_rowdot_past_both_caps(passthrough, monkeypatch):
    """ops.rowdot at 65 536 + 64 + 1 rows of 64, J = 2; tolerances of test_rowdot_matches_float64."""
    ops = _ops()
    R, C, J = 65536 + 64 + 1, 64, 2
    g = torch.Generator().manual_seed(R + C + J)
    x, U, b = torch.randn(R, C, generator=g), torch.randn(J, C, generator=g), torch.randn(J, generator=g)
    wy, wx = torch.randn(R, J, generator=g), torch.randn(R, C, generator=g)
    calls = _count(monkeypatch, "faf_rowdot_fwd", "faf_rowdot_bwd")

    def run(t, fused):
        if fused:
            _poison(R * J)
            y = ops.rowdot(t[0], t[1], t[2], passthrough=passthrough)
            y, xp = y if passthrough else (y, None)
            _poison(R * C)
        else:
            y, xp = t[0] @ t[1].T + t[2], (t[0] if passthrough else None)
        ((y * wy.to(y)).sum() + ((xp * wx.to(y)).sum() if passthrough else 0.0)).backward()
        return y

    t64 = [a.double().requires_grad_(True) for a in (x, U, b)]
    ref = run(t64, False)
    d = [a.to(DEV).requires_grad_(True) for a in (x, U, b)]
    y = run(d, True)
    d32 = [a.to(DEV).requires_grad_(True) for a in (x, U, b)]
    run(d32, False)
    torch.cuda.synchronize()
    _ran(calls)
    keys = ("dx", "dU", "db")
    _compare(f"rowdot passthrough={passthrough}", [("y", y)], [ref], {k: a.grad for k, a in zip(keys, d)},
             {k: a.grad for k, a in zip(keys, t64)}, {k: a.grad for k, a in zip(keys, d32)}, ("dx",), keys[1:],
             (3e-5, 1e-5), 3e-5, 3e-5)
    _release()


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gate_rows_past_both_caps(p, monkeypatch):
    """ops.gate_rows at 65 601 rows of 64 with a residual; the keep matrix comes from ops.dropout_mean on ones with the same
    seed (as test_gate_rows_matches_float64, whose tolerances these are)."""
    ops = _ops()
    R, C = 65536 + 64 + 1, 64
    g = torch.Generator().manual_seed(R + C)
    x, w, b = torch.randn(R, C, generator=g), 0.2 * torch.randn(1, C, generator=g), torch.randn(1, generator=g)
    res, wo = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
    seed = _seed(987654321)
    keep = ops.dropout_mean(torch.ones(R, 1, C, device=DEV), p, seed) if p > 0 else torch.ones(R, C, device=DEV)
    calls = _count(monkeypatch, "faf_gate_fwd", "faf_gate_bwd")

    def run(t, fused):
        if fused:
            _poison(R * C)
            out = ops.gate_rows(t[0], t[1], t[2], t[3], p, seed)
            _poison(R * C, R * C)
        else:
            xd = t[0] * keep.to(t[0])
            out = xd * torch.sigmoid(xd @ t[1].reshape(-1, 1) + t[2]) + t[3]
        (out * wo.to(out)).sum().backward()
        return out

    t64 = [a.double().requires_grad_(True) for a in (x, w, b, res)]
    ref = run(t64, False)
    d = [a.to(DEV).requires_grad_(True) for a in (x, w, b, res)]
    out = run(d, True)
    d32 = [a.to(DEV).requires_grad_(True) for a in (x, w, b, res)]
    run(d32, False)
    torch.cuda.synchronize()
    _ran(calls)
    keys = ("dx", "dw", "db", "dres")
    _compare(f"gate p={p}", [("out", out)], [ref], {k: a.grad for k, a in zip(keys, d)}, {k: a.grad for k, a in zip(keys, t64)},
             {k: a.grad for k, a in zip(keys, d32)}, ("dx", "dres"), ("dw", "db"), (3e-5, 1e-5), 3e-5, 3e-5)
    _release()


# ---- k_attn_pool_fwd (4 x 2048 nodes), k_attn_pool_bwd (ap_blocks: 8 x 512 nodes) ---------------------------------------------------
def test_attn_pool_past_both_caps(monkeypatch):
    """ops.attn_pool at 8192 + 4 + 1 nodes (a node with every neighbour masked in the second trip); tolerances of
    test_attn_pool_matches_float64_reference."""
    ops = _ops()
    N = 8192 + 4 + 1
    g = torch.Generator().manual_seed(N)
    K, D, V, v_off, scale, slope = 16, 104, 48, 56, 48 ** -0.5, 0.1
    me, edge = torch.randn(N, D, generator=g), torch.randn(N * K, D, generator=g)
    mask = torch.rand(N, K, generator=g) < 0.7
    mask[0] = False
    mask[N - 2] = False
    wl, wv, wo = 0.5 * torch.randn(1, 4, generator=g), torch.randn(V, V, generator=g) / V ** 0.5, torch.randn(N, V, generator=g)
    calls = _count(monkeypatch, "eqf_attn_pool_fwd", "eqf_attn_pool_bwd")

    def run(t, fused):
        if fused:
            _poison(N * V)
            out = ops.attn_pool(t[0], t[1], mask.float().to(DEV), t[2], t[3], v_off, scale, slope)
            _poison(N * D, N * K * D)
        else:
            mk = mask.to(t[0].device)
            inter = torch.cat((t[0][:, None, :], t[1].view(N, K, D)), 1)
            logits = F.linear(F.leaky_relu(inter[..., :4], slope), t[2]) * scale
            keep = F.pad(mk, (1, 0), value=True)[..., None]
            attn = logits.masked_fill(~keep, -torch.finfo(logits.dtype).max).softmax(dim=1)
            out = (attn * (F.silu(inter[..., v_off:]) @ t[3])).sum(1)
        (out * wo.to(out)).sum().backward()
        return out

    t64 = [z.double().requires_grad_(True) for z in (me, edge, wl, wv)]
    ref = run(t64, False)
    d = [z.to(DEV).requires_grad_(True) for z in (me, edge, wl, wv)]
    out = run(d, True)
    d32 = [z.to(DEV).requires_grad_(True) for z in (me, edge, wl, wv)]
    run(d32, False)
    torch.cuda.synchronize()
    _ran(calls)
    keys = ("dme", "dedge", "dw_logit", "dwv")
    _compare("attn_pool", [("out", out)], [ref], {k: a.grad for k, a in zip(keys, d)}, {k: a.grad for k, a in zip(keys, t64)},
             {k: a.grad for k, a in zip(keys, d32)}, ("dme", "dedge"), ("dw_logit", "dwv"), (2e-5, 2e-5), 3e-5, 3e-5)
    assert float(d[1].grad[:, 4:v_off].abs().max()) == 0.0 and float(d[0].grad[:, 4:v_off].abs().max()) == 0.0
    _release()


# ---- k_residual_mix (dense_aux.hip): 256 float4 x 4096 -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_residual_mix_past_its_cap(mode, monkeypatch):
    """ops.residual_mix at 65 536 + 16 + 1 rows of 64 (1 048 576 float4 + one workgroup + 16); tolerances of
    test_residual_mix_matches_float64; the bias gradient is summed over all rows (ops.colsum): measured limit."""
    ops = _ops()
    R, C, a = 65536 + 16 + 1, 64, 0.3
    g = torch.Generator().manual_seed(mode)
    x0, b, w = torch.randn(R, C, generator=g), torch.randn(C, generator=g), torch.randn(R, C, generator=g)
    lens = torch.randint(0, 4, (R,), generator=g)
    rowptr = torch.cat((torch.zeros(1, dtype=torch.int64), lens.cumsum(0))).int().to(DEV)
    rw = ((lens > 0) if mode == 1 else lens).double()[:, None]
    calls = _count(monkeypatch, "hg_residual_mix_f32")
    t = [v.double().requires_grad_(True) for v in (x0, b)]
    ref = a * t[0] + (1 - a) * rw * t[1]
    (ref * w.double()).sum().backward()
    d = [v.to(DEV).requires_grad_(True) for v in (x0, b)]
    _poison(R * C)
    out = ops.residual_mix(d[0], d[1], rowptr, mode, a)
    _poison(R * C)
    (out * w.to(DEV)).sum().backward()
    d32 = [v.to(DEV).requires_grad_(True) for v in (x0, b)]
    ((a * d32[0] + (1 - a) * rw.float().to(DEV) * d32[1]) * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _ran(calls)
    _rows_close(out, ref.detach(), 1e-6, 1e-6, "out")
    _rows_close(d[0].grad, t[0].grad, 1e-6, 1e-6, "dx0")
    lim = _summed_limit(f"residual_mix mode={mode} db", 0.0, d32[1].grad, t[1].grad) * float(t[1].grad.abs().max())
    over = (d[1].grad.cpu().double() - t[1].grad).abs() - torch.clamp(2e-4 + 1e-5 * t[1].grad.abs(), min=lim)
    assert float(over.max()) <= 0.0, float(over.max())
    _release()


# ---- k_eigh3: 128 matrices x 4096 ----------------------------------------------------------------------------------------------------
def test_eigh3_past_its_cap(monkeypatch):
    """ops.eigh3 on 524 288 + 128 + 1 matrices: a block of 37 repeated (LAPACK on half a million 3 x 3 problems takes seconds;
    the kernel works on one matrix per thread with no state between matrices, so equal inputs give equal bits): every
    result equals its twin in the first period bit for bit, and the first period meets test_eigh3_matches_lapack_up_to_sign."""
    ops = _ops()
    B, P = 524288 + 128 + 1, 37
    g = torch.Generator().manual_seed(0)
    x = torch.randn(P, 12, 3, generator=g)
    x[:3, 3:] = 0
    cov = torch.bmm(x.transpose(1, 2), x)
    calls = _count(monkeypatch, "geo_eigh3")
    big = cov.repeat((B + P - 1) // P, 1, 1)[:B].contiguous().to(DEV)
    _poison(B * 9)
    vd = ops.eigh3(big)
    torch.cuda.synchronize()
    _ran(calls)
    assert bool(torch.isfinite(vd).all())
    assert torch.equal(vd, vd[:P].repeat((B + P - 1) // P, 1, 1)[:B])
    w_ref, v_ref = torch.linalg.eigh(cov.double(), UPLO="U")
    v = vd[:P].cpu().double()
    gap_ok = ((w_ref[:, 1] - w_ref[:, 0]) > 1e-3 * w_ref[:, 2]) & ((w_ref[:, 2] - w_ref[:, 1]) > 1e-3 * w_ref[:, 2])
    assert int(gap_ok.sum()) >= 30
    assert float((1 - (v * v_ref).sum(1).abs()[gap_ok]).max()) < 1e-5
    assert float((torch.bmm(v.transpose(1, 2), v) - torch.eye(3, dtype=torch.double)).abs().max()) < 1e-5
    assert float((torch.bmm(cov.double(), v) - v * w_ref.unsqueeze(1)).abs().max() / cov.abs().max()) < 1e-5
    _release()


# ---- the elementwise kernels of faformer_ew.hip: 256 float4 x 8192 -------------------------------------------------------------------
def test_swiglu_dropout_past_its_cap(monkeypatch):
    """ops.swiglu_dropout on [65 536 + 8 + 1, 256] (2 097 152 float4 of output, one more workgroup and 32).  p = 0: a block of 37
    rows repeated, the first period against float64 (tolerances of test_faformer_elementwise_kernels), every row and gradient
    row equal to its twin bit for bit (an elementwise kernel: no state between elements).  p = 0.25: the output is the
    p = 0 output times the keep matrix and the backward that of the masked upstream gradient, bit for bit."""
    ops = _ops()
    R, H, P = 65536 + 8 + 1, 128, 37
    g = torch.Generator().manual_seed(3)
    blk, wb = torch.randn(P, 2 * H, generator=g), torch.randn(P, H, generator=g)
    k = (R + P - 1) // P
    calls = _count(monkeypatch, "faf_swiglu_dropout_fwd", "faf_swiglu_dropout_bwd")
    t = blk.double().requires_grad_(True)
    a, b = t.chunk(2, -1)
    ref = F.silu(a) * b
    (ref * wb.double()).sum().backward()
    pre, w = blk.repeat(k, 1)[:R].contiguous().to(DEV), wb.repeat(k, 1)[:R].contiguous().to(DEV)
    d = pre.clone().requires_grad_(True)
    _poison(R * H)
    out = ops.swiglu_dropout(d, 0.0)
    _poison(R * 2 * H)
    (out * w).sum().backward()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d.grad).all())
    assert torch.equal(out.detach(), out.detach()[:P].repeat(k, 1)[:R]) and torch.equal(d.grad, d.grad[:P].repeat(k, 1)[:R])
    _rows_close(out[:P], ref.detach(), 2e-6, 2e-6, "out")
    _rows_close(d.grad[:P], t.grad, 5e-6, 1e-5, "dpre")
    p, seed = 0.25, _seed(77)
    keep = _keep_of((R, H), p, seed)
    assert sorted(keep.unique().tolist()) == [0.0, float(np.float32(1.0) / np.float32(1.0 - p))]
    d2 = pre.clone().requires_grad_(True)
    _poison(R * H)
    o1 = ops.swiglu_dropout(d2, p, seed)
    _poison(R * 2 * H)
    (o1 * w).sum().backward()
    assert torch.equal(o1.detach(), out.detach() * keep)
    d3 = pre.clone().requires_grad_(True)
    (ops.swiglu_dropout(d3, 0.0) * (w * keep)).sum().backward()
    assert torch.equal(d2.grad, d3.grad)
    torch.cuda.synchronize()
    _ran(calls)
    _release()


@pytest.mark.parametrize("rider", [True, False], ids=["bias_rider", "plain"])
@pytest.mark.parametrize("R,F_,C", [(32768 + 4 + 1, 8, 256), (131072 + 16 + 1, 3, 64)], ids=["f8c256", "general"])
def test_dropout_mean_past_its_caps(R, F_, C, rider, monkeypatch):
    """ops.dropout_mean past the forward's 2 097 152 float4 of output and the backward's 32 768 rows
    (k_drop_mean_bwd_f8c256) / 2 097 152 float4 of dx (k_drop_mean_bwd): without a bias the <false> forms on 8192
    workgroups (faf_dropout_mean_bwd), with the bias rider the <true> forms on dm_colsum_blocks' 4096
    (faf_dropout_mean_bwd_colsum).  Float64 on the device over every row (an average of F values: the host would spend
    seconds on the 67 M-element input); the masks are the keep factors of the flat index.  Tolerances of
    test_faformer_elementwise_kernels: the forward 1e-6 + 1e-6 |ref| at p = 0 and 2e-6 + 1e-5 |ref| with dropout, dx
    1e-7 + 1e-6 |ref|; the bias gradient (summed over R F rows) at the measured limit."""
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(R)
    x = torch.randn(R, F_, C, generator=g, device=DEV)
    w = torch.randn(R, C, generator=g, device=DEV)
    seed = _seed(24681357)
    calls = _count(monkeypatch, "faf_dropout_mean_fwd", "faf_dropout_mean_bwd_colsum" if rider else "faf_dropout_mean_bwd")
    for p in (0.0, 0.25):
        keep = _keep_of((R, F_, C), p, seed) if p > 0 else None
        calls["faf_dropout_mean_fwd"] = 0                  # (_keep_of is a forward call of its own)
        bias = torch.zeros(C, device=DEV, requires_grad=True) if rider else None
        xd = x.clone().requires_grad_(True)
        _poison(R * C)
        out = ops.dropout_mean(xd, p, seed, bias=bias)
        _poison(R * F_ * C)
        (out * w).sum().backward()
        assert calls["faf_dropout_mean_fwd"] == 1, calls
        xk = x.double() if keep is None else x.double() * keep.double()
        ref = xk.mean(-2)
        atol, rtol = (1e-6, 1e-6) if p == 0 else (2e-6, 1e-5)
        over = (out.detach().double() - ref).abs() - (atol + rtol * ref.abs())
        print(f"dropout_mean {R}x{F_}x{C} p={p} out: {float((out.detach().double() - ref).abs().max()):.2e}")
        assert bool(torch.isfinite(out).all()) and float(over.max()) <= 0.0, (p, float(over.max()))
        dref = (w.double()[:, None, :] / F_).expand(R, F_, C) * (1.0 if keep is None else keep.double())
        over = (xd.grad.double() - dref).abs() - (1e-7 + 1e-6 * dref.abs())
        assert bool(torch.isfinite(xd.grad).all()) and float(over.max()) <= 0.0, (p, float(over.max()))
        if rider:
            bref = dref.sum((0, 1))
            b32 = ((w[:, None, :] / F_).expand(R, F_, C) * (1.0 if keep is None else keep)).sum((0, 1))
            e32 = float((b32.double() - bref).abs().max() / bref.abs().max())
            err = float((bias.grad.double() - bref).abs().max() / bref.abs().max())
            lim = max(2e-6 * max(1.0, (R * F_) ** 0.5 / 30), 4.0 * e32)       # the first: test_dropout_mean_backward_carries_...
            print(f"dropout_mean {R}x{F_}x{C} p={p} dbias: {err:.2e} (fp32 torch sum {e32:.2e}, limit {lim:.2e})")
            assert err <= lim, (p, err, lim)
        del keep, xd, out, xk, ref, dref, over
    torch.cuda.synchronize()
    _ran(calls)
    assert calls["faf_dropout_mean_bwd_colsum" if rider else "faf_dropout_mean_bwd"] == 2, calls
    _release()


def test_dropout_add_past_its_cap(monkeypatch):
    """ops.dropout_add on 8 388 608 + 1024 + 4 floats: p = 0 is exactly res + x; with p = 0.25 the keep factors equal those
    ops.dropout_mean gives for the same flat indices (another kernel, another loop) bit for bit, the kept fraction is
    within 5 sigma in the second trip too, and the backward applies the same factors."""
    ops = _ops()
    n, p, seed = 8388608 + 1024 + 4, 0.25, _seed(97)
    g = torch.Generator(device=DEV).manual_seed(n)
    x, res, w = (torch.randn(n, generator=g, device=DEV) for _ in range(3))
    calls = _count(monkeypatch, "faf_dropout_add")
    _poison(n)
    assert torch.equal(ops.dropout_add(x, res, 0.0), x + res)
    keep = ops.dropout_mean(torch.ones(n // 4, 1, 4, device=DEV), p, seed).reshape(-1)
    _poison(n)
    assert torch.equal(ops.dropout_add(torch.ones(n, device=DEV), None, p, seed), keep)
    q = round(p * 65536) / 65536
    for part in (keep[:8388608], keep[8388608:]):
        assert abs(float((part != 0).double().mean()) - (1 - q)) <= 5 * (q * (1 - q) / part.numel()) ** 0.5
    xd, rd = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    _poison(n)
    out = ops.dropout_add(xd, rd, p, seed)
    assert torch.equal(out.detach(), x * keep + res)
    _poison(n)
    (out * w).sum().backward()
    assert torch.equal(xd.grad, w * keep) and torch.equal(rd.grad, w)
    torch.cuda.synchronize()
    _ran(calls)
    _release()


# ---- k_frame_pre_* / k_frame_hidden_* (4 x 8192 rows forward, fp_blocks 32 x 1024 rows backward) ---------------------------------------
def _sign_frames(dtype):
    return torch.tensor([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=dtype, device=DEV)


def test_frame_pre_past_both_caps(monkeypatch):
    """ops.frame_pre at 32 768 + 32 + 1 rows with a broadcast bias: [E, 8, 256] against float64 on the device over every
    row (67 M outputs); tolerances of test_frame_pre_matches_float64_reference, d W3 and d bias (summed over all rows and
    frames) at the measured limit."""
    ops = _ops()
    E = 32768 + 32 + 1
    g = torch.Generator(device=DEV).manual_seed(9)
    y, w3, base = (torch.randn(*s, generator=g, device=DEV) for s in ((E, 3), (256, 3), (256,)))
    wo = torch.randn(E, 8, 256, generator=g, device=DEV)
    calls = _count(monkeypatch, "faf_frame_pre_fwd", "faf_frame_pre_bwd")

    def run(t, fused):
        if fused:
            _poison(E * 8 * 256)
            out = ops.frame_pre(t[0], t[1], t[2])
            _poison(E * 3, E * 256)
        else:
            out = F.linear(t[0].unsqueeze(-2) * _sign_frames(t[0].dtype), t[1]) + t[2]
        (out * wo.to(out)).sum().backward()
        return out.detach()

    t64 = [z.double().requires_grad_(True) for z in (y, w3, base)]
    ref = run(t64, False)
    d = [z.clone().requires_grad_(True) for z in (y, w3, base)]
    out = run(d, True)
    d32 = [z.clone().requires_grad_(True) for z in (y, w3, base)]
    run(d32, False)
    torch.cuda.synchronize()
    _ran(calls)
    over = (out.double() - ref).abs() - (1e-5 + 1e-5 * ref.abs())
    assert bool(torch.isfinite(out).all()) and float(over.max()) <= 0.0, float(over.max())
    del over, ref, out
    keys = ("dy", "dw3", "dbase")
    _compare("frame_pre", [], [], {k: a.grad for k, a in zip(keys, d)}, {k: a.grad.cpu() for k, a in zip(keys, t64)},
             {k: a.grad for k, a in zip(keys, d32)}, ("dy",), keys[1:], None, 2e-5, 2e-5)
    _release()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("form", ["rows", "vector"])
def test_frame_hidden_past_both_caps(form, p, monkeypatch):
    """ops.frame_hidden at 32 801 rows against float64 on the device over every row, with per-row bases
    (k_frame_hidden_bwd<false>) and in the vector form, where the row of a point is bias + extra * wx formed inside the
    kernel and d bias / d wx leave through a second slab region behind the blocks x FH_SLAB of the first
    (k_frame_hidden_bwd<true>).  With p = 0.1 the masks are the keep factors of the [E, 8, 128] hidden tensor.
    Tolerances of the float64 branch of test_frame_hidden_matches_the_three_kernel_composition (whose 5e-5 also bounds the
    vector form's seven gradients there), x 1 / (1 - p) with dropout (every kept value carries it)."""
    ops = _ops()
    E = 32768 + 32 + 1
    vec = form == "vector"
    g = torch.Generator(device=DEV).manual_seed(E)
    y, w3 = torch.randn(E, 3, generator=g, device=DEV), 0.5 * torch.randn(256, 3, generator=g, device=DEV)
    base = 0.5 * torch.randn(*((256,) if vec else (E, 256)), generator=g, device=DEV)
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g, device=DEV), 0.3 * torch.randn(128, generator=g, device=DEV)
    wgt = torch.randn(E, 8, 128, generator=g, device=DEV)
    extra, wx = torch.rand(E, 1, generator=g, device=DEV) * 4, 0.3 * torch.randn(256, generator=g, device=DEV)
    seed, s = _seed(123456789), 1.0 / (1.0 - p)
    keep = _keep_of((E, 8, 128), p, seed) if p > 0 else None
    calls = _count(monkeypatch, "faf_frame_hidden_fwd", "faf_frame_hidden_bwd")

    def run(t, fused):
        if fused:
            _poison(E * 8 * 128)
            out = ops.frame_hidden(t[0], t[1], t[2], t[3], t[4], 1e-5, p, seed, *t[5:])
            _poison(E * 3, E * 256)
        else:
            rows = torch.addcmul(t[2], t[5], t[6]) if vec else t[2]
            pre = torch.einsum("efd,hd->efh", t[0][:, None, :] * _sign_frames(t[0].dtype)[None], t[1]) + rows[:, None, :]
            hid = F.silu(pre[..., :128]) * pre[..., 128:]
            if keep is not None:
                hid = hid * keep.to(hid)
            out = F.layer_norm(hid, (128,), t[3], t[4], 1e-5)
        (out * wgt.to(out)).sum().backward()
        return out.detach()

    leaves = (y, w3, base, gamma, beta) + ((extra, wx) if vec else ())
    t64 = [z.double().requires_grad_(True) for z in leaves]
    ref = run(t64, False)
    d = [z.clone().requires_grad_(True) for z in leaves]
    out = run(d, True)
    d32 = [z.clone().requires_grad_(True) for z in leaves]
    run(d32, False)
    torch.cuda.synchronize()
    _ran(calls)
    over = (out.double() - ref).abs() - (3e-5 * s + 1e-5 * ref.abs())
    assert bool(torch.isfinite(out).all()) and float(over.max()) <= 0.0, float(over.max())
    del over, ref, out
    keys = ("dy", "dw3", "dbias", "dgamma", "dbeta", "dextra", "dwx") if vec else ("dy", "dw3", "dbase", "dgamma", "dbeta")
    per_row = ("dy", "dextra") if vec else ("dy", "dbase")
    _compare(f"frame_hidden {form} p={p}", [], [], {k: a.grad for k, a in zip(keys, d)}, {k: a.grad.cpu() for k, a in zip(keys, t64)},
             {k: a.grad for k, a in zip(keys, d32)}, per_row, tuple(k for k in keys if k not in per_row), None, 5e-5 * s, 5e-5 * s)
    _release()


# ---- k_gather_ln_bwd at the gl_rpw cap: 64 rows per wavefront x 8 wavefronts, block count growing past 524 288 source rows ------------
def test_gather_ln_reduce_backward_at_its_rows_per_wavefront_cap(monkeypatch):
    """ops.gather_ln_reduce over 524 288 + 512 + 1 source rows (gl_rpw = 64 with 1026 workgroups, the last holding one row) and
    411 307 output rows.  The index is a block of 37 source rows, 29 output rows and 111 entries repeated down the diagonal;
    the 30 source rows behind the last block have no entry.  Both kernels sum a row's entries in CSR order whatever the
    wavefront's range holds (entries fetched past a row's end carry weight 0), so every output row and every dh row must
    equal its twin in the first block bit for bit; the first block is compared with float64 at the tolerances of
    test_gather_ln_reduce_matches_float64_reference, the three parameter gradients (blocks x the block's) at the measured
    limit."""
    ops = _ops()
    C, Pn, Pm, nb = 64, 37, 29, 111
    N = 524288 + 512 + 1
    k = N // Pn
    M = k * Pm
    g = torch.Generator().manual_seed(N)
    vb, eb = torch.randint(0, Pn, (nb,), generator=g), torch.randint(0, Pm - 1, (nb,), generator=g)   # the block's last output row is empty
    vb[vb == 5] = 6                                                                                   # and source row 5 unused
    vb[:70], eb[20:90] = 3, 11                                                                        # rows longer than 64 entries
    hb, b = torch.randn(Pn, C, generator=g), 0.3 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    wb = torch.randn(Pm, C, generator=g)
    calls = _count(monkeypatch, "hg_gather_ln_reduce_fwd", "hg_gather_ln_reduce_bwd")
    t = [x.double().requires_grad_(True) for x in (hb, b, gamma, beta)]
    ref = O.segment_reduce(F.layer_norm(torch.relu(t[0] + t[1]), (C,), t[2], t[3], 1e-5)[vb], eb, Pm, "mean")
    (ref * wb.double()).sum().backward()
    blocks = torch.arange(k, device=DEV)
    v = (vb.to(DEV)[None, :] + Pn * blocks[:, None]).reshape(-1)
    e = (eb.to(DEV)[None, :] + Pm * blocks[:, None]).reshape(-1)
    by_v, by_e = ops.csr_build(v, e, N), ops.csr_build(e, v, M)
    h = torch.cat((hb.repeat(k, 1), torch.randn(N - k * Pn, C, generator=g))).to(DEV)
    w = wb.repeat(k, 1).to(DEV)
    d = [x.clone().to(DEV).requires_grad_(True) for x in (h, b, gamma, beta)]
    _poison(M * C)
    out = ops.gather_ln_reduce(d[0], d[1], d[2], d[3], by_e, by_v, "mean")
    _poison(N * C)
    (out * w).sum().backward()
    d32 = [x.clone().to(DEV).requires_grad_(True) for x in (h, b, gamma, beta)]
    (O.segment_reduce(F.layer_norm(torch.relu(d32[0] + d32[1]), (C,), d32[2], d32[3], 1e-5)[v], e, M, "mean") * w).sum().backward()
    torch.cuda.synchronize()
    _ran(calls)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d[0].grad).all())
    assert torch.equal(out.detach(), out.detach()[:Pm].repeat(k, 1))
    assert torch.equal(d[0].grad[:k * Pn], d[0].grad[:Pn].repeat(k, 1))
    assert float(d[0].grad[k * Pn:].abs().max()) == 0.0 and float(d[0].grad[5].abs().max()) == 0.0
    assert float(out[Pm - 1].detach().abs().max()) == 0.0
    _rows_close(out[:Pm], ref.detach(), 3e-5, 1e-5, "out")
    err = _rel(d[0].grad[:Pn], t[0].grad)
    assert err < 3e-5, err
    for name, x, x32, r in zip(("dbias", "dgamma", "dbeta"), d[1:], d32[1:], t[1:]):
        lim = _summed_limit(f"gather_ln cap {name}", 3e-5, x32.grad, k * r.grad)
        err = _rel(x.grad, k * r.grad)
        print(f"gather_ln cap {name}: {err:.2e} (limit {lim:.2e})")
        assert err <= lim, (name, err, lim)
    _release()


# ---- rowgemm.hip: the LDS kernels (1 row x 2048) and the generic ones (4 rows x 4096 forward / dz, 4 x 2048 dw) -----------------------
@pytest.mark.parametrize("R,Kd,L", [(2048 + 1 + 1, 64, 80), (16384 + 4 + 1, 16, 16)], ids=["lds", "generic"])
def test_rowgemm_past_its_caps(R, Kd, L, monkeypatch):
    """ops.rowgemm with two entries per row on average (an empty row and a long one in the second trip) at shapes the streaming
    kernels (one row per workgroup, uncapped) do not take; tolerances of test_rowgemm_matches_float64_reference."""
    ops = _ops()
    g = torch.Generator().manual_seed(R)
    E = 2 * R
    key = torch.randint(0, R, (E,), generator=g)
    key[key == R - 2] = R - 1
    key[:40] = R - 3
    z = torch.randn(E, Kd, generator=g)
    w = torch.randn(R, Kd, L, generator=g) / Kd ** 0.5
    dout = torch.randn(E, L, generator=g)
    calls = _count(monkeypatch, "hg_rowgemm_fwd", "hg_rowgemm_bwd")
    z64, w64 = z.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = torch.einsum("ek,ekl->el", z64, w64[key])
    (ref * dout.double()).sum().backward()
    csr = ops.csr_build(key.to(DEV), None, R)
    zd, wd = z.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    _poison(E * L)
    out = ops.rowgemm(zd, wd, csr.rowptr, csr.perm)
    _poison(E * Kd, R * Kd * L)
    (out * dout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _ran(calls)
    _rows_close(out, ref.detach(), 2e-5, 1e-5, "out")
    _rows_close(zd.grad, z64.grad, 5e-5, 1e-5, "dz")
    _rows_close(wd.grad, w64.grad, 5e-5, 1e-5, "dw")
    assert float(wd.grad[R - 2].abs().max()) == 0.0
    _release()


# ---- k_edge_hidden_fwd (4 x 8192 nodes), k_edge_hidden_bwd (eh_blocks: 4 x 1024 nodes) -----------------------------------------------
def test_edge_hidden_past_both_caps(monkeypatch):
    """ops.edge_hidden at 32 768 + 4 + 1 nodes with 16 neighbours against float64 on the device over every row (67 M outputs;
    the neighbour lists are a kNN of random points, so dB is a scattered sum).  The existing test compares with the
    unfused fp32 composition only; the float64 tolerances are those of the same LayerNorm(SwiGLU) tail in
    test_frame_hidden_matches_the_three_kernel_composition."""
    ops = _ops()
    N, K = 32768 + 4 + 1, 16
    g = torch.Generator(device=DEV).manual_seed(N)
    A, B = torch.randn(N, 256, generator=g, device=DEV), torch.randn(N, 256, generator=g, device=DEV)
    Cf = torch.randn(N, K, 256, generator=g, device=DEV)
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g, device=DEV), 0.3 * torch.randn(128, generator=g, device=DEV)
    wgt = torch.randn(N, K, 128, generator=g, device=DEV)
    nbr, _ = ops.knn(torch.randn(N, 3, generator=g, device=DEV), K, 1)
    csr_t = ops.csr_build(nbr.reshape(-1), None, N)
    calls = _count(monkeypatch, "faf_edge_hidden_fwd", "faf_edge_hidden_bwd")

    def run(t, fused):
        if fused:
            _poison(N * K * 128)
            out = ops.edge_hidden(t[0], t[1], t[2], nbr, csr_t, t[3], t[4], 1e-5, 0.0, None)
            _poison(N * 256, N * 256, N * K * 256)
        else:
            pre = t[0].unsqueeze(1) + t[1][nbr.reshape(-1).long()].view(N, K, 256) + t[2]
            out = F.layer_norm(F.silu(pre[..., :128]) * pre[..., 128:], (128,), t[3], t[4], 1e-5)
        (out * wgt.to(out)).sum().backward()
        return out.detach()

    t64 = [z.double().requires_grad_(True) for z in (A, B, Cf, gamma, beta)]
    ref = run(t64, False)
    d = [z.clone().requires_grad_(True) for z in (A, B, Cf, gamma, beta)]
    out = run(d, True)
    d32 = [z.clone().requires_grad_(True) for z in (A, B, Cf, gamma, beta)]
    run(d32, False)
    torch.cuda.synchronize()
    _ran(calls)
    over = (out.double() - ref).abs() - (3e-5 + 1e-5 * ref.abs())
    assert bool(torch.isfinite(out).all()) and float(over.max()) <= 0.0, float(over.max())
    del over, ref, out
    keys = ("dA", "dB", "dCf", "dgamma", "dbeta")
    _compare("edge_hidden", [], [], {k_: a.grad for k_, a in zip(keys, d)}, {k_: a.grad.cpu() for k_, a in zip(keys, t64)},
             {k_: a.grad for k_, a in zip(keys, d32)}, ("dA", "dB", "dCf"), ("dgamma", "dbeta"), None, 5e-5, 5e-5)
    _release()


# ---- radial.hip: rm_blocks (128 edges x 512), rm_bwd_blocks (128 x 256) -------------------------------------------------------------
def test_radial_trunk_past_the_forward_cap(monkeypatch):
    """ops.radial_trunk at 65 536 + 128 + 1 edges (test_radial_trunk_matches_float64_reference stops at 36 864: past the
    backward's 32 768, short of the forward's 65 536); its tolerances, the six parameter gradients at the measured limit."""
    ops = _ops()
    from equihgnn_amd.equiformer import Radial
    E = 65536 + 128 + 1
    torch.manual_seed(E)
    rad = Radial(4, 4)
    g = torch.Generator().manual_seed(E + 1)
    for p in rad.parameters():
        p.data.add_(0.3 * torch.randn(p.shape, generator=g))
    rad.rp[2].beta.copy_(0.1 * torch.randn(64, generator=g))
    dist = 0.8 + 4.0 * torch.rand(E, 1, generator=g)
    w = torch.randn(E, 64, generator=g)
    calls = _count(monkeypatch, "eqf_radial_trunk_fwd", "eqf_radial_trunk_bwd")
    ref, r32 = Radial(4, 4).double(), Radial(4, 4)
    ref.load_state_dict({k: v.double() for k, v in rad.state_dict().items()})
    r32.load_state_dict(rad.state_dict())
    r32 = r32.to(DEV)
    h, h32 = dist.double(), dist.to(DEV)
    for i in range(6):
        h, h32 = ref.rp[i](h), r32.rp[i](h32)
    (h * w.double()).sum().backward()
    (h32 * w.to(DEV)).sum().backward()
    rp = rad.to(DEV).rp
    _poison(E * 64)
    out = ops.radial_trunk(dist.to(DEV), rp[0], rp[2], rp[3], rp[5])
    (out * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _ran(calls)
    _rows_close(out, h.detach(), 2e-5, 2e-5, "out")
    for name, pick in (("weight", (0, 3)), ("bias", (0, 3)), ("gamma", (2, 5))):
        for i in pick:
            mine, theirs, fp32 = (getattr(m.rp[i], name).grad for m in (rad, ref, r32))
            lim = _summed_limit(f"radial rp[{i}].{name}", 5e-5, fp32, theirs)
            err = _rel(mine, theirs)
            print(f"radial rp[{i}].{name}: {err:.2e} (limit {lim:.2e})")
            assert err <= lim, (i, name, err, lim)
    _release()


# ---- k_index_aux (csr_build.hip): 256 x 1024 items ------------------------------------------------------------------------------------
def test_index_aux_past_its_cap(monkeypatch):
    """ops.index_aux over 262 144 + 256 + 1 incidences with the two CSRs' entry weights and a counter buffer of the same
    length to clear: every output is exact (casts, flags, 1 / degree)."""
    ops = _ops()
    nnz = 262144 + 256 + 1
    n_nodes, n_edges = 90001, 85003
    rng = np.random.default_rng(5)
    vertex, edges = rng.integers(0, n_nodes - 3, size=nnz), rng.integers(0, n_edges - 2, size=nnz)
    batch = np.sort(rng.integers(0, 700, size=n_nodes))
    vt, et = torch.from_numpy(vertex).to(DEV), torch.from_numpy(edges).to(DEV)
    by_v, by_e = ops.csr_build(vt, et, n_nodes), ops.csr_build(et, vt, n_edges)
    zero_buf = torch.full((nnz,), 9, dtype=torch.int32, device=DEV)
    calls = _count(monkeypatch, "hg_index_aux")
    _poison(nnz, nnz, n_nodes, n_edges)
    v32, e32, b32, has_v, has_e = ops.index_aux(vt, et, torch.from_numpy(batch).to(DEV), n_nodes, n_edges, by_v.rowptr, by_e.rowptr,
                                                by_v, by_e, zero_buf)
    torch.cuda.synchronize()
    _ran(calls)
    assert np.array_equal(v32.cpu().numpy(), vertex) and np.array_equal(e32.cpu().numpy(), edges)
    assert np.array_equal(b32.cpu().numpy(), batch)
    deg_v, deg_e = np.bincount(vertex, minlength=n_nodes), np.bincount(edges, minlength=n_edges)
    assert np.array_equal(has_v.cpu().numpy(), (deg_v > 0).astype(np.float32))
    assert np.array_equal(has_e.cpu().numpy(), (deg_e > 0).astype(np.float32))
    assert int(zero_buf.abs().max()) == 0
    for csr, deg in ((by_v, deg_e), (by_e, deg_v)):       # 1 / (the entry's row length in the OTHER CSR)
        want = np.float32(1.0) / np.maximum(deg[csr.col.cpu().numpy()], 1).astype(np.float32)
        assert np.array_equal(csr.entry_w.cpu().numpy(), want)
    _release()


# ---- se3t.hip: k_se3t_pool (256 x 2048 outputs), k_se3t_norm_bwd (st_norm_blocks: 8 rows x 256) ------------------------------------
def test_se3t_pooled_pair_past_the_pool_cap(monkeypatch):
    """ops.se3t_pair, edge-level and pooled, at 8192 + 4 + 1 atoms with O = 64: the pool writes 524 288 + 256 + 64 outputs
    (test_extents_beyond_the_grid_caps of test_hip_se3t pools 132 800).  The case, reference and bound of test_hip_se3t."""
    import test_hip_se3t as S
    calls = _count(monkeypatch, "se3t_pair_fwd", "se3t_pair_bwd")
    S._pair_case((0, 0), 16, 64, 8192 + 4 + 1, 4, 51)
    _ran(calls)
    _release()


@pytest.mark.parametrize("m", [1, 3])
def test_se3t_norm_backward_past_its_cap(m, monkeypatch):
    """ops.se3t_norm forward and backward at 4096 + 1 + 1 rows of 32 channels (forward: one row per workgroup x 4096;
    backward: 8 rows x 256 workgroups, so every workgroup comes round again) with a zero row in the second trip; reference and
    bound of test_norm_with_a_zero_row, the scale's gradient (summed over all rows) at the measured limit."""
    import se3t_ref
    from test_hip_se3t import TOL, _close, _rand
    ops = _ops()
    n, c = 4096 + 1 + 1, 32
    x = _rand(n, c, m, seed=31)
    x[n - 2] = 0.0
    s = (1.0 + 0.1 * _rand(1, 1, c, seed=32)).float().double()
    up = _rand(n, c, m, seed=33)
    calls = _count(monkeypatch, "se3t_norm_fwd", "se3t_norm_bwd")
    x64, s64 = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
    ref = se3t_ref.norm_se3(x64, s64)
    g64 = torch.autograd.grad((ref * up).sum(), (x64, s64))
    x32, s32 = x.float().to(DEV).requires_grad_(True), s.float().to(DEV).requires_grad_(True)
    _poison(n * c * m)
    out = ops.se3t_norm(x32.transpose(1, 2).contiguous(), s32).transpose(1, 2)
    _poison(n * c * m)
    g32 = torch.autograd.grad((out * up.float().to(DEV)).sum(), (x32, s32))
    xt, st = x.float().to(DEV).requires_grad_(True), s.float().to(DEV).requires_grad_(True)
    gt = torch.autograd.grad((se3t_ref.norm_se3(xt, st) * up.float().to(DEV)).sum(), (xt, st))
    torch.cuda.synchronize()
    _ran(calls)
    _close(out, ref, "fwd")
    assert float(out[n - 2].abs().max()) == 0 and bool(torch.isfinite(out).all())
    _close(g32[0], g64[0], "dx")
    assert bool(torch.isfinite(g32[0]).all())
    lim = _summed_limit(f"se3t_norm m={m} dscale", TOL, gt[1], g64[1])
    err = _rel(g32[1], g64[1])
    print(f"se3t_norm m={m} dscale: {err:.2e} (limit {lim:.2e})")
    assert err <= lim, (err, lim)
    _release()


# ---- eqh_k_reduce_slabs (common.h): 64 elements x 2048 ------------------------------------------------------------------------------
def test_accumulate_past_the_reduction_cap(monkeypatch):
    """The slab reduction takes 64 elements per workgroup on at most 2048 workgroups; every slab a kernel here writes is
    narrower than 131 072 elements, but eqh_accumulate (ops._hand_out: a fresh gradient added onto a parameter's persistent
    accumulator) sends a whole tensor through it as one slab.  131 072 + 64 + 1 elements, eagerly and deferred: one exact
    fp32 addition per element."""
    from equihgnn_amd import ops
    from equihgnn_amd.ops import _base
    n = 131072 + 64 + 1
    g = torch.Generator(device=DEV).manual_seed(n)
    calls = _count(monkeypatch, "eqh_accumulate")
    for deferred in (False, True):
        grad, acc = torch.randn(n, generator=g, device=DEV), torch.randn(n + 64, generator=g, device=DEV)
        want = acc.clone()
        want[:n] += grad
        if deferred:
            ops.defer_begin(DEV)
        try:
            assert _base._hand_out([grad], [acc[:n]]) == [None]
        finally:
            if deferred:
                ops.defer_flush(DEV)
        torch.cuda.synchronize()
        assert torch.equal(acc, want), deferred
    assert calls["eqh_accumulate"] == 2, calls                 # (_hand_out adds with torch when its guard refuses a pair)
    _release()


# ---- egnn_edge.hip: k_edge_bwd_prep (prep_blocks: 4 nodes x 2048) -------------------------------------------------------------------
def test_egnn_edge_past_the_backward_prep_cap(monkeypatch):
    """ops.egnn_edge at 8192 + 4 + 1 atoms, Hp = 64 (the forward kernels and the two backward products loop from 1025
    atoms, which test_egnn_edge_fused_matches_float64_reference[1283-576-6] passes; the preparation pass not before 8193),
    with a hub every atom lists; that test's reference and tolerances, the three weight gradients at the measured limit."""
    from equihgnn_amd import hip
    ops = _ops()
    N, Hp = 8192 + 4 + 1, 64
    g = torch.Generator().manual_seed(N)
    ab, wd = torch.randn(N, 2 * Hp, generator=g), torch.randn(Hp, generator=g) * 0.3
    w2, b2 = torch.randn(16, Hp, generator=g) / Hp ** 0.5, torch.randn(16, generator=g) * 0.1
    nbr = torch.randint(0, N, (N, 16), generator=g)
    nbr[:, 0] = torch.arange(N)
    nbr[:, 5] = 3
    d2, dm = torch.rand(N, 16, generator=g) * 3, torch.randn(N, 16, generator=g)
    calls = _count(monkeypatch, *(n for n in ("egnn_edge_fwd", "egnn_edge_fwd_p", "egnn_edge_bwd", "egnn_edge_bwd_p")
                                  if n in hip.SIGNATURES))

    def run(t, fused):
        if fused:
            _poison(N * 16)
            m = ops.egnn_edge(t[0], t[1], t[2], t[3], nbr.to(DEV).int(), d2.to(DEV), ops.csr_build(nbr.reshape(-1).to(DEV), None, N))
            _poison(N * 2 * Hp)
        else:
            dv = t[0].device
            h = t[0][:, None, :Hp] + t[0][:, Hp:][nbr.to(dv)] + d2.to(t[0])[..., None] * t[1]
            m = F.silu(F.silu(h) @ t[2].T + t[3]).sum(1)
        (m * dm.to(m)).sum().backward()
        return m.detach()

    t64 = [x.double().requires_grad_(True) for x in (ab, wd, w2, b2)]
    ref = run(t64, False)
    d = [x.to(DEV).requires_grad_(True) for x in (ab, wd, w2, b2)]
    m = run(d, True)
    d32 = [x.to(DEV).requires_grad_(True) for x in (ab, wd, w2, b2)]
    run(d32, False)
    torch.cuda.synchronize()
    assert sum(c for n, c in calls.items() if "fwd" in n) >= 1 and sum(c for n, c in calls.items() if "bwd" in n) >= 1, calls
    keys = ("dab", "dwd", "dw2", "db2")
    _compare("egnn_edge", [("m", m)], [ref], {k: x.grad for k, x in zip(keys, d)}, {k: x.grad for k, x in zip(keys, t64)},
             {k: x.grad for k, x in zip(keys, d32)}, ("dab",), keys[1:], (2e-6 * max(float(ref.abs().max()), 1.0), 1e-5), 2e-5, 2e-5)
    _release()


# ---- k_pack_fwd / k_pack_bwd (dense_aux.hip): 256 x 2048 elements -------------------------------------------------------------------
def test_egnn_pack_weights_past_its_cap(monkeypatch):
    """ops.egnn_pack_weights at H = 1025 padded to Hp = 1088, C = 256 (577 728 packed elements forward, 560 675 backward;
    the cap is 524 288): the edge kernel's operand layout is a rearrangement with zero padding and its backward the inverse
    one, so both are compared bit for bit with index expressions."""
    ops = _ops()
    H, Hp, C = 1025, 1088, 256
    g = torch.Generator(device=DEV).manual_seed(H)
    w1, b1, w2 = (torch.randn(*sh, generator=g, device=DEV).requires_grad_(True) for sh in ((H, 2 * C + 1), (H,), (16, H)))
    ups = [torch.randn(*sh, generator=g, device=DEV) for sh in ((2 * Hp, C), (2 * Hp,), (Hp,), (16, Hp))]
    calls = _count(monkeypatch, "egnn_pack_weights_fwd", "egnn_pack_weights_bwd")
    _poison(2 * Hp * C, 2 * Hp, Hp, 16 * Hp)
    outs = ops.egnn_pack_weights(w1, b1, w2, Hp)
    _poison(H * (2 * C + 1), H, 16 * H)
    sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    torch.cuda.synchronize()
    _ran(calls)
    w_cat, b_cat, wd, w2p = (o.detach() for o in outs)
    pad = torch.zeros(Hp - H, C, device=DEV)
    assert torch.equal(w_cat, torch.cat((w1.detach()[:, :C], pad, w1.detach()[:, C:2 * C], pad)))
    assert torch.equal(b_cat, torch.cat((b1.detach(), torch.zeros(2 * Hp - H, device=DEV))))
    assert torch.equal(wd, torch.cat((w1.detach()[:, 2 * C], torch.zeros(Hp - H, device=DEV))))
    assert torch.equal(w2p, torch.cat((w2.detach(), torch.zeros(16, Hp - H, device=DEV)), 1))
    assert torch.equal(w1.grad, torch.cat((ups[0][:H], ups[0][Hp:Hp + H], ups[2][:H, None]), 1))
    assert torch.equal(b1.grad, ups[1][:H]) and torch.equal(w2.grad, ups[3][:, :H])
    _release()


# ---- k_copy_many (optim.hip): 4096 floats x 256 workgroups per tensor ------------------------------------------------------------------
def test_copy_many_past_its_cap(monkeypatch):
    """ops.copy_many with one tensor of 1 048 576 + 4096 + 1 floats among small ones, into a flat buffer at an offset that
    keeps the float4 body (and at one that does not): exact copies, the floats around them untouched."""
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(3)
    calls = _count(monkeypatch, "eqh_copy_many")
    for first in (8, 5):
        srcs = [torch.randn(n, generator=g, device=DEV) for n in (256, 1048576 + 4096 + 1, 7)]      # (first = 8: the big one lands 16-byte aligned)
        flat = torch.full((first + sum(t.numel() for t in srcs) + 64,), 3.5, device=DEV)
        dsts, off = [], first
        for t in srcs:
            dsts.append(flat[off:off + t.numel()])
            off += t.numel()
        ops.copy_many(dsts, srcs)
        torch.cuda.synchronize()
        for d, t in zip(dsts, srcs):
            assert torch.equal(d, t)
        assert bool((flat[:first] == 3.5).all()) and bool((flat[off:] == 3.5).all())
    assert calls["eqh_copy_many"] == 2, calls
    _release()


# ---- k_edge_codes (gnn2d.hip): 256 x 4096 edges -----------------------------------------------------------------------------------
def test_edge_codes_past_their_cap(monkeypatch):
    """ops.gnn2d.GraphIndex over 1 048 576 + 256 + 1 bonds of 5000 atoms: both edge CSRs against the stable sort and the packed
    bond codes (table row of feature f in byte f, out-of-range values clamped) against the same expression in numpy, exactly."""
    from equihgnn_amd.ops.gnn2d import BOND_FEATURE_DIMS, GraphIndex, bond_offsets
    N, E, F_ = 5000, 1048576 + 256 + 1, 3
    rng = np.random.default_rng(E)
    src, dst = rng.integers(0, N, size=E), rng.integers(0, N, size=E)
    attr = np.stack([rng.integers(-1, d + 1, size=E) for d in BOND_FEATURE_DIMS], 1)       # -1 and d: clamped
    calls = _count(monkeypatch, "hg_edge_codes")
    t = [torch.full((E,), -7, dtype=torch.int32, device=DEV) for _ in range(2)]
    del t
    gi = GraphIndex(torch.from_numpy(np.stack((src, dst))).to(DEV), torch.from_numpy(attr).to(DEV),
                    torch.zeros(N, dtype=torch.int64, device=DEV), N, 1)
    torch.cuda.synchronize()
    assert calls["hg_edge_codes"] == 2
    offs, _ = bond_offsets(F_)
    packed = sum((offs[f] + np.clip(attr[:, f], 0, BOND_FEATURE_DIMS[f] - 1)) << (8 * f) for f in range(F_))
    for csr, code, key, other in ((gi.by_dst, gi.code_dst, dst, src), (gi.by_src, gi.code_src, src, dst)):
        rp, perm, col = _np_csr(key, other, N)
        assert np.array_equal(csr.rowptr.cpu().numpy(), rp) and np.array_equal(csr.perm.cpu().numpy()[:E], perm)
        assert np.array_equal(csr.col.cpu().numpy()[:E], col)
        assert np.array_equal(code.cpu().numpy()[:E], packed[perm])
    _release()
