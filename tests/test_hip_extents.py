"""The kernels at the edges of their grids: shapes just below and just above the limits the C entry points enforce
(EQH_ERR_RANGE), through the public ops the models call.  Inputs are small integers (or dyadic values), so every fp32
sum is exact and the float64 reference is compared bit for bit, millions of rows deep; results land on poisoned (NaN)
memory or onto a sentinel, so rows a kernel never wrote show up.

Every guard, the model path that could reach it, and its case -- (a) the models cannot reach it, (b) the ops layer
routes around it, (c) a latent failure:

====================================  ==================================  =============================================  ====
guard                                 limit                               model path                                     case
====================================  ==================================  =============================================  ====
wgrad.hip:656 hg_wgrad_skinny_f32     K <= 64 x 65 535 = 4 194 240 rows   ops.linear weight gradient of a <= 16-column   (c)
                                                                          block into an accumulator (the EGNN m_i
                                                                          block): fixed, _wgrad_skinny declines past it
embed.hip:164 hg_embed_sum_bwd        N <= 128 x 65 535 = 8 388 480       AtomEncoder / BondEncoder backward (every      (c)
                                      nodes                               model): fixed, the kernel runs 65 535 chunks
                                                                          per launch, as many launches as needed
dense_aux.hip:201,229 hg_colsum_*     R <= 32 x 65 535 = 2 097 120 rows   bias gradients: ops.colsum sums more than      (b)
                                                                          2 000 000 rows with torch (so the kernel's
                                                                          last chunk row is never reached)
small_mm.hip:187 hg_small_mm_batch    m, n <= 65 536                      merged weight products: model widths           (a)
rmsnorm.hip:139 eqf_rms_norm_*        C <= 1024                           Equiformer FiberNorm: norm0 / norm1 send       (b)
                                                                          wider rows to torch
rmsnorm.hip:139 eqf_rms_norm_*        rows < 2^31                         >= 32 GB per operand                           (a)
egnn_edge.hip:872 check_common        N x 2 Hp < 2^33                     EGNN edge MLP, ~3.9 M atoms at C = 256: ab     (c)
                                                                          alone is 34 GB there at any width, past this
                                                                          suite's memory budget; open (the edge kernels
                                                                          need 64-bit offsets for it), no test
egnn_edge.hip:873 check_common        N x 16 < 2^31                       134 M atoms: ab > 288 GB                       (a)
egnn_edge.hip:909,930 LDS caps        Hp-wide tiles in 160 KiB            width only (Hp ~ 4 C): thousands of channels   (a)
knn.hip:158 geo_knn                   N < 2^31 / 3                        715 M atoms                                    (a)
knn_grid.hip:354 geo_knn_grid         N <= 65 536                         ops.knn "auto" takes the brute force above     (b)
gemm_x6.hip:770,827 hg_gemm_x6_batch  m < 2^31 - 256, tiles < 2^31        Linears: 2^31 rows x K >= 64 floats            (a)
bn_rows.hip:226 bn_check              R < 2^31                            MHNN BatchNorm: >= 32 GB per operand           (a)
segment_reduce.hip:118                rows < 2^31 - 1                     aggregations                                   (a)
rowgemm.hip:686                       rows < 2^31 - 1                     Equiformer radial products                     (a)
incidence.hip:737                     rows < 2^31 - 1                     MHNN incidence gathers                         (a)
panel.hip                             rows < 2^31 - 64                    MHNN / EGNN row panels                         (a)
  (conv_panel_launch, hg_panel_sum, hg_panel_multi, hg_panel_stream_gemm_f32_p, hg_panel_gemm_f32_p)
gnn2d.hip:208                         N < 2^31 - 1                        GNN_2D message passing                         (a)
====================================  ==================================  =============================================  ====

The row guards cannot be met: 2^31 rows of the models' widths are hundreds of GB per operand.  R x C >= 2^31 elements
is reachable (~10 M rows of 256), so their element offsets were read: segment_reduce, rowgemm, incidence and gnn2d widen
the row index to int64 before every multiply by the width, panel.hip forms (int64_t) row * ld; none needed a fix.  No
test here crosses 2^31 elements (8.6 GB per operand, past the budget of one suite test)."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SKINNY_LIMIT = 64 * 65535      # rows hg_wgrad_skinny_f32 takes: 64 per workgroup row, 65 535 workgroup rows


def _poison(numel):
    """Leave a freed block of ``numel`` NaNs in the caching allocator: the next allocation of that size comes back holding
    NaN, so a row a kernel never writes stays NaN."""
    t = torch.full((numel,), float("nan"), dtype=torch.float32, device=DEV)
    del t


def _release():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _signs(shape, seed):
    """Entries in {-1, 0, 1}: any fp32 sum of fewer than 2^23 of them is exact, in any order."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randint(0, 3, shape, generator=g, device=DEV, dtype=torch.int8) - 1).to(torch.float32)


# ---- hg_wgrad_skinny_f32 (wgrad.hip): 64 rows per workgroup row, grid.y <= 65 535 -------------------------------------------------
def _skinny_case(K, O, J, deferred, monkeypatch):
    """ops.linear over the column block [8, 8 + J) of a weight with a persistent accumulator (the m_i block of the EGNN node
    MLP): the block's gradient dy^T x is added onto a sentinel of 0.5.  Returns what _wgrad_skinny answered, call by call."""
    from equihgnn_amd import ops
    from equihgnn_amd.ops import grads

    took = []
    inner = grads._wgrad_skinny

    def counted(dy2, x2, tgt):
        took.append(inner(dy2, x2, tgt))
        return took[-1]

    monkeypatch.setattr(grads, "_wgrad_skinny", counted)
    w = torch.nn.Parameter(torch.zeros(O, 8 + J + 8, device=DEV))
    w._eqh_gbuf = torch.full((O, 8 + J + 8), 0.5, device=DEV)
    x = _signs((K, J), 1)
    dy = _signs((K, O), 2)
    y = ops.linear(x, w, cols=(8, 8 + J))
    if deferred:
        ops.defer_begin(DEV)
    try:
        y.backward(dy)
    finally:                                    # (a failure must not leave the deferral window open for the next test)
        if deferred:
            ops.defer_flush(DEV)
    torch.cuda.synchronize()
    assert w.grad is None                       # all of it went into the accumulator
    ref = dy.double().t() @ x.double() + 0.5    # |sums| <= K < 2^23: exact in fp32, and so is + 0.5
    got = w._eqh_gbuf
    assert torch.equal(got[:, 8:8 + J].double(), ref)
    assert torch.equal(got[-1, 8:8 + J].double(), ref[-1])      # the last output row (in the partial 64-column block)
    assert bool((got[:, :8] == 0.5).all()) and bool((got[:, 8 + J:] == 0.5).all())
    monkeypatch.setattr(grads, "_wgrad_skinny", inner)
    del w, x, dy, y, ref, got
    _release()
    return took


@pytest.mark.parametrize("deferred", [False, True], ids=["eager", "deferred"])
def test_skinny_wgrad_at_its_last_workgroup_row(deferred, monkeypatch):
    """65 535 chunks of 64 rows, the last holding a single row: the skinny kernel takes it and the sum is exact."""
    K = SKINNY_LIMIT - 63
    assert (K + 63) // 64 == 65535
    assert _skinny_case(K, 72, 9, deferred, monkeypatch) == [True]


@pytest.mark.parametrize("deferred", [False, True], ids=["eager", "deferred"])
def test_skinny_wgrad_past_its_grid(deferred, monkeypatch):
    """One row past the limit: the skinny kernel declines (no EQH_ERR_RANGE) and the next path adds the same exact sum."""
    assert _skinny_case(SKINNY_LIMIT + 1, 72, 9, deferred, monkeypatch) == [False]


@pytest.mark.parametrize("deferred", [False, True], ids=["eager", "deferred"])
def test_skinny_wgrad_keeps_the_baseline_m_i_block(deferred, monkeypatch):
    """The m_i block of the EGNN node MLP at the BASELINE batch (4736 rows x 16 columns into 512 outputs) still goes to
    the skinny kernel: counted calls, not timing."""
    assert _skinny_case(4736, 512, 16, deferred, monkeypatch) == [True]


# ---- hg_embed_sum_bwd (embed.hip): 128 nodes per workgroup row -------------------------------------------------------------------
@pytest.mark.parametrize("N", [128 * 65535 - 127, 128 * 65535 + 129], ids=["last_chunk", "past_one_grid"])
def test_atom_encoder_backward_counts(N):
    """AtomEncoder forward and backward with 65 535 node chunks (the last holding one node) and past them.  With integer
    tables the forward is exact; with d out = 1 the gradient of table f, row v, is the number of nodes whose feature f is v."""
    from equihgnn_amd.batch import ATOM_FEATURE_DIMS
    from equihgnn_amd.layers import AtomEncoder

    C = 4
    enc = AtomEncoder(C).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(N)
    with torch.no_grad():
        for e in enc.atom_embedding_list:
            e.weight.copy_(torch.randint(-8, 9, e.weight.shape, generator=g, device=DEV).float())
    x = torch.stack([torch.randint(0, d, (N,), generator=g, device=DEV) for d in ATOM_FEATURE_DIMS], 1)
    x[-1] = torch.tensor([d - 1 for d in ATOM_FEATURE_DIMS], device=DEV)   # the last node selects every table's last row
    _poison(N * C)
    out = enc(x)
    with torch.no_grad():
        ref = sum(e.weight.double()[x[:, f]] for f, e in enumerate(enc.atom_embedding_list))
        assert torch.equal(out.double(), ref)
        assert torch.equal(out[-1].double(), ref[-1])
    del ref
    _poison(sum(ATOM_FEATURE_DIMS) * C)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    for f, (d, e) in enumerate(zip(ATOM_FEATURE_DIMS, enc.atom_embedding_list)):
        cnt = torch.bincount(x[:, f], minlength=d).double()
        assert int(cnt[-1]) >= 1
        assert torch.equal(e.weight.grad.double(), cnt[:, None].expand(d, C)), f
    del enc, x, out
    _release()


# ---- hg_colsum_f32 / hg_colsum_batch_f32 (dense_aux.hip): 32 rows per chunk, <= 65 535 chunks --------------------------------------
@pytest.mark.parametrize("R", [2_000_000, 2_000_001, 32 * 65535 + 1], ids=["last_kernel_shape", "first_torch", "past_grid"])
@pytest.mark.parametrize("deferred", [False, True], ids=["eager", "deferred"])
def test_colsum_around_its_grid(R, deferred):
    """ops.colsum (bias gradients) on both sides of its 2 000 000-row switch and past the kernel's 2 097 120 rows: the sum is
    exact, added onto a sentinel (eagerly, and through the deferred batched launch) or written to poisoned memory."""
    from equihgnn_amd import ops

    C = 36
    x = _signs((R, C), R)
    x[-1] = 1.0
    into = torch.full((C,), 0.5, device=DEV)
    if deferred:
        ops.defer_begin(DEV)
    try:
        assert ops.colsum(x, into=into) is None
    finally:
        if deferred:
            ops.defer_flush(DEV)
    torch.cuda.synchronize()
    ref = x.double().sum(0)
    assert torch.equal(into.double(), ref + 0.5)
    _poison(C)
    got = ops.colsum(x)
    assert torch.equal(got.double(), ref)
    del x, into, got
    _release()


# ---- geo_knn_grid (knn_grid.hip): at most 65 536 points; ops.knn("auto") takes the brute-force search above ---------------------
@pytest.mark.parametrize("N", [65536, 65537], ids=["grid_max", "brute_past_grid"])
def test_knn_around_the_grid_limit(N):
    """ops.knn (mode 0: squared distance, self included) on integer coordinates: distances are exact and neighbours are
    ordered by (distance, index); both equal a float64 search over all pairs, the last query included."""
    from equihgnn_amd import ops

    k = 16
    g = torch.Generator(device=DEV).manual_seed(N)
    pos = torch.randint(0, 48, (N, 3), generator=g, device=DEV).float()
    nbr, key = ops.knn(pos, k, 0)
    torch.cuda.synchronize()
    p64 = pos.double()
    sq = (p64 * p64).sum(1)
    idx = torch.arange(N, device=DEV, dtype=torch.int64)
    for q0 in range(0, N, 4096):
        q1 = min(q0 + 4096, N)
        d2 = sq[q0:q1, None] + sq[None, :] - 2.0 * (p64[q0:q1] @ p64.t())          # integers: exact in float64
        order = (d2.to(torch.int64) * N + idx).topk(k, dim=1, largest=False).values  # (distance, index)
        del d2
        assert torch.equal(nbr[q0:q1].to(torch.int64), order % N), q0
        assert torch.equal(key[q0:q1].double(), (order // N).double()), q0
        del order
    del pos, nbr, key
    _release()


# ---- eqf_rms_norm_* (rmsnorm.hip): C <= 1024; FiberNorm sends wider rows to torch ------------------------------------------------
@pytest.mark.parametrize("C", [1024, 1028], ids=["kernel_max", "torch_past"])
def test_fiber_norm_around_its_width_limit(C):
    """FiberNorm.norm0 at the kernel's widest row and one float4 past it: rows of {-1, 0, 1} (the last all zero, clamped by
    eps) with a dyadic gain, the output and the gain's gradient against float64."""
    from equihgnn_amd.equiformer import FiberNorm

    R = 3000
    norm = FiberNorm([C]).to(DEV)
    with torch.no_grad():
        norm.transforms[0].copy_(torch.randint(1, 8, (C, 1), device=DEV).float() / 4)
    t = _signs((R, C), C)
    t[-1] = 0.0
    t.requires_grad_(True)
    out = norm.norm0(t)
    td, gd = t.detach().double(), norm.transforms[0].detach().double()[:, 0]
    rms = (td.norm(dim=-1, keepdim=True) * C ** -0.5).clamp(min=norm.eps)
    ref = td / rms * gd
    assert float((out.detach().double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    assert float(out.detach()[-1].abs().max()) == 0.0
    dy = _signs((R, C), C + 1)
    out.backward(dy)
    dg_ref = (dy.double() * td / rms).sum(0)
    assert float((norm.transforms[0].grad.double()[:, 0] - dg_ref).abs().max()) <= 1e-5 * float(dg_ref.abs().max())
    del norm, t, out, dy
    _release()
