"""CPU-side checks of the drop-in boundary: the shared library loads and exports every symbol
include/equihgnn_hip.h declares, the ctypes table derived from the header matches a second reading of it and the
compiler's struct layout, argument validation works without a GPU, and the product refuses to run on CPU tensors
(no fallback)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "equihgnn_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b([a-z_0-9]+)\s*\([^;{]*\)\s*;", text)))


def declared_argument_counts():
    """name -> number of parameters of every function the header declares (a reader independent of equihgnn_amd.hip)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {name: 0 if args.strip() == "void" else args.count(",") + 1
            for name, args in re.findall(r"\b([a-z_0-9]+)\s*\(([^;{]*)\)\s*;", text)}


def vis_entry_points():
    """name -> [(C type, parameter name)] of every vis_* function the header declares"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(vis_[a-z_0-9]+)\s*\(([^;{]*)\)\s*;", text):
        out[name] = [(m.group(1).replace(" ", ""), m.group(2)) for m in
                     (re.fullmatch(r"\s*(?:const\s+)?(\w+\s*\*?)\s*(\w+)\s*", a) for a in args.split(","))]
    return out


STRUCTS = ("HgSmallMM", "HgGemmProblem", "HgPanelPack", "HgConvPanel", "HgPanelMulti", "HgPanelSum", "HbCollate")


def test_header_declares_functions():
    names = declared_functions()
    assert "hg_segment_reduce_f32" in names and "geo_knn" in names and len(names) >= 8


def test_library_exports_every_declared_symbol():
    from equihgnn_amd import build, hip

    build.build(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in declared_functions():
        assert hasattr(handle, name), f"{name} declared in the header but not exported"
    assert sorted(hip.SIGNATURES) == declared_functions()
    assert hip.lib().eqh_version() >= 1


def test_signatures_take_the_header_argument_counts():
    from equihgnn_amd import hip

    counts = declared_argument_counts()
    assert sorted(counts) == sorted(hip.SIGNATURES)
    assert {n: len(hip.SIGNATURES[n][1]) for n in counts} == counts


def test_struct_layout_matches_the_compiler(tmp_path):
    """sizeof of every argument struct and offsetof / sizeof of every field, as the host compiler lays them out, against
    the derived ctypes.Structure classes: a field swapped, dropped or mistyped is caught here, before a kernel reads it."""
    from equihgnn_amd import build, hip

    lines, want = [], {}
    for s in STRUCTS:
        cls = getattr(hip, s)
        lines.append(f'std::printf("{s} %zu\\n", sizeof({s}));')
        want[s] = str(ctypes.sizeof(cls))
        for f, _ in cls._fields_:
            lines.append(f'std::printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)nullptr)->{f}));')
            want[f"{s}.{f}"] = f"{getattr(cls, f).offset} {getattr(cls, f).size}"
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "equihgnn_hip.h"\nint main() {\n' + "\n".join(lines)
                   + "\nreturn 0;\n}\n")
    subprocess.check_call([build._hipcc(), "-x", "c++", "-I", build.INCLUDE, str(src), "-o", str(exe)])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got == want


def test_constants_match_the_header():
    from equihgnn_amd import hip

    text = open(HEADER).read()
    defines = dict(re.findall(r"#define (EQH_\w+) \(?(-?\d+)\)?", text))
    (enum,) = re.findall(r"enum \{([^}]*)\}", text)
    stages = dict(re.findall(r"(\w+) = (\d+)", enum))
    assert sorted(defines) == ["EQH_ERR_ALIGN", "EQH_ERR_ARG", "EQH_ERR_LAUNCH", "EQH_ERR_RANGE", "EQH_OK"]
    assert list(stages) == ["HG_CONV_F1", "HG_CONV_F2", "HG_CONV_F3", "HG_CONV_B3", "HG_CONV_B1", "HG_EGNN_NODE_F",
                            "HG_EGNN_NODE_B"]
    for name, value in {**defines, **stages}.items():
        assert getattr(hip, name) == int(value), name
    assert hip.EQH_ERR_RANGE == -3 and hip.HG_CONV_F1 == 1 and hip.HG_EGNN_NODE_B == 7


def test_header_reader_maps_each_c_type_and_refuses_the_rest():
    from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_size_t, c_void_p

    from equihgnn_amd import hip

    structs, sigs, consts = hip.parse_header(
        "#define EQH_X (-9)\n"
        "enum { STAGE_A = 1, STAGE_B = 2 };\n"
        "/* a comment */ typedef struct Tag {\n    int32_t n, k;\n    const void* w[3];\n    const float *in0, *in1;\n} S;\n"
        "int f(int a, int32_t b, int64_t c, size_t d, float e, const float* const* g, void** h,\n"
        "      const S* s, float* __restrict__ p, const uint8_t* m);\n"
        "const char* name(int code);\n"
        "void nothing(void);\n")
    S = structs["S"]
    assert [(n, t) for n, t in S._fields_ if n != "w"] == [("n", c_int32), ("k", c_int32), ("in0", c_void_p), ("in1", c_void_p)]
    assert [n for n, _ in S._fields_] == ["n", "k", "w", "in0", "in1"]
    w = dict(S._fields_)["w"]
    assert (w._type_, w._length_) == (c_void_p, 3)
    assert sigs == {"f": (c_int32, [c_int32, c_int32, c_int64, c_size_t, c_float, c_void_p, POINTER(c_void_p), POINTER(S),
                                    c_void_p, c_void_p]),
                    "name": (c_char_p, [c_int32]),
                    "nothing": (None, [])}
    assert consts == {"EQH_X": -9, "STAGE_A": 1, "STAGE_B": 2}
    # no silent c_void_p: an unknown scalar, a pointer to an unknown type, a struct by value, an unreadable declaration
    # (uint8_t is known as a pointer's target -- faf_edge_frame_fwd's mask -- but not as a value)
    for snippet, line, decl in (("int f(int a,\n      double x);", 2, "double x"),
                                ("typedef struct {\n    int32_t n;\n    double x;\n} T;", 3, "double x"),
                                ("int f(uint8_t v);", 1, "uint8_t v"),
                                ("int f(double* p);", 1, "double* p"),
                                ("int f(unsigned int n);", 1, "unsigned int n"),
                                ("typedef struct {\n    int32_t n;\n} T;\nint f(T t);", 4, "T t"),
                                ("int f(int n);\ntypedef int32_t idx_t;", 2, "typedef int32_t idx_t"),
                                ("int f(void (*cb)(int));", 1, "cb")):
        with pytest.raises(ValueError, match=rf"^snippet\.h:{line}: cannot bind `.*{re.escape(decl)}"):
            hip.parse_header(snippet, "snippet.h")


def test_partial_load_of_a_diagnostic_build():
    """hip.load(partial=True) types what a build of some of the sources exports; the full rule refuses that build."""
    from equihgnn_amd import build, hip

    build.build(verbose=False)
    L = hip.load(build.STAMPS_LIB, partial=True)
    assert list(L.hg_conv_panel.argtypes) == hip.SIGNATURES["hg_conv_panel"][1]
    assert L.hg_conv_panel_slab_bytes.restype is ctypes.c_size_t
    with pytest.raises(hip.HipLibraryError, match="does not export"):
        hip.load(build.STAMPS_LIB)


def test_argument_validation_without_gpu():
    from equihgnn_amd import hip

    L = hip.lib()
    assert L.hg_csr_build_workspace_bytes(100, 10) > 0
    assert L.hg_csr_build_workspace_bytes(-1, 10) == 0
    # null pointers / bad shapes are rejected before anything is launched
    assert L.hg_segment_reduce_f32(None, None, None, None, None, 4, 64, 0, None) == -1
    assert L.geo_knn(None, 10, 0, 0, None, None, None) == -1
    assert L.geo_knn(None, 10, 16, 5, None, None, None) == -1
    assert b"argument" in L.eqh_error_string(-1)
    with pytest.raises(hip.HipLibraryError):
        hip.check(-2, "demo")
    # the 11 vis_* entries: width and extent are checked before any pointer is read, pointers before any launch
    vis = vis_entry_points()
    assert len(vis) == 11
    held = ctypes.create_string_buffer(64)       # an address that is never read: every call below names a null pointer too
    for name, params in vis.items():
        fn = getattr(L, name)

        def call(N, C=64, null=None, name=name, params=params, fn=fn):
            args = []
            for ctype, arg in params:
                if ctype.endswith("*"):
                    filled = null is not None and arg != null and arg != "stream"
                    args.append(ctypes.addressof(held) if filled else None)
                else:
                    args.append({"N": N, "C": C, "cutoff": 5.0}[arg])
            assert null is None or null in [a for _, a in params], null
            return fn(*args)

        assert call(0) == hip.EQH_OK, name
        assert call(4) == hip.EQH_ERR_ARG, name
        assert call(-1) == hip.EQH_ERR_ARG, name
        assert call(2 ** 27) == hip.EQH_ERR_RANGE, name                  # 16 N = 2^31
        assert call(2 ** 27 - 1) == hip.EQH_ERR_ARG, name                # the largest N in range: on to the pointers
        for ctype, arg in params:
            if ctype.endswith("*") and arg not in ("n_real", "stream"):  # (n_real may be null: an unpadded batch)
                assert call(4, null=arg) == hip.EQH_ERR_ARG, (name, arg)
        if name != "vis_radius_graph":
            for C in (12, 520, 0, -8):
                assert call(4, C) == hip.EQH_ERR_ARG, (name, C)
                assert call(0, C) == hip.EQH_ERR_ARG, (name, C)
            assert call(2 ** 27, 520) == hip.EQH_ERR_ARG, name
            for C in (8, 72, 512):
                assert call(0, C) == hip.EQH_OK, (name, C)


def test_se3t_argument_validation_without_gpu():
    """The se3t_* entries refuse in the order of csrc/se3t.hip: extents and shapes (st_pair_check), then null pointers, then
    alignment, then the pooled form's own conditions -- all before a launch.  Every call below is refused by a check that
    comes before any launch; ``held`` is an address that is never read (each call that names it is refused first)."""
    from equihgnn_amd import hip

    L = hip.lib()
    ARG, RANGE, ALIGN, OK = hip.EQH_ERR_ARG, hip.EQH_ERR_RANGE, hip.EQH_ERR_ALIGN, hip.EQH_OK
    buf = ctypes.create_string_buffer(256)
    held = (ctypes.addressof(buf) + 15) & ~15
    big = 2 ** 31

    def fwd(h=held, G=held, GB=held, coef=held, cstride=34, rowptr=held, perm=held, N=4, E=64, MO=3, Q=9, O=64, meanw=None, K=16,
            out=held, accumulate=0, ws=None, ws_bytes=0):
        return L.se3t_pair_fwd(h, G, GB, coef, cstride, rowptr, perm, N, E, MO, Q, O, meanw, K, out, accumulate, ws, ws_bytes, None)

    def bwd(h=held, G=held, coef=held, cstride=34, rowptr=held, perm=held, N=4, E=64, MO=3, Q=9, O=64, dout=held, meanw=None,
            K=16, dh=held, dG=held, dGB=held):
        return L.se3t_pair_bwd(h, G, coef, cstride, rowptr, perm, N, E, MO, Q, O, dout, meanw, K, dh, dG, dGB, None)

    for f in (fwd, bwd):
        for bad in (dict(MO=2), dict(MO=0), dict(Q=2), dict(Q=27), dict(cstride=26), dict(MO=1, Q=3, cstride=2), dict(K=0),
                    dict(K=17), dict(N=big), dict(E=big), dict(N=-1), dict(E=-1)):
            assert f(**bad) == ARG, (f.__name__, bad)
        for O in (8, 24, 1040, 0):
            assert f(O=O) == RANGE, (f.__name__, O)
        assert f(O=1040, MO=2) == ARG, f.__name__                      # the shape is looked at before the width
        assert f(N=0, E=0) == OK and f(N=0, E=0, O=1024, MO=1, Q=1, cstride=1, K=1) == OK, f.__name__
    assert fwd(E=0) == OK
    for name in ("h", "G", "GB", "coef", "rowptr", "perm", "out"):
        assert fwd(**{name: None}) == ARG, name
    for name in ("h", "G", "coef", "rowptr", "perm", "dout", "dh", "dG", "dGB"):
        assert bwd(**{name: None}) == ARG, name
        assert bwd(E=0, **{name: None}) == ARG, name                   # (no edges, some atoms: dG and dGB are still written)
    for name in ("h", "G", "GB", "out"):
        for shift in (4, 8, 12):
            assert fwd(**{name: held + shift}) == ALIGN, (name, shift)
    for name in ("G", "dout"):
        assert bwd(**{name: held + 4}) == ALIGN, name
    assert fwd(h=None, G=held + 4) == ARG                               # a null pointer is refused before the alignment
    # the pooled form: E = N K, a workspace of se3t_pair_fwd_workspace_bytes; accumulate only with it
    need = L.se3t_pair_fwd_workspace_bytes(64, 3, 64, 1)
    assert need == 64 * 3 * 64 * 4 and L.se3t_pair_fwd_workspace_bytes(64, 3, 64, 0) == 0
    assert fwd(accumulate=1) == ARG
    assert fwd(meanw=held, E=63, ws=held, ws_bytes=need) == ARG and bwd(meanw=held, E=63) == ARG
    assert fwd(meanw=held, K=8, ws=held, ws_bytes=need) == ARG
    assert fwd(meanw=held, ws=None, ws_bytes=need) == ARG
    assert fwd(meanw=held, ws=held + 4, ws_bytes=need) == ARG
    assert fwd(meanw=held, ws=held, ws_bytes=need - 1) == ARG and fwd(meanw=held, ws=held, ws_bytes=0) == ARG
    assert fwd(meanw=held, accumulate=1, ws=held, ws_bytes=need - 4) == ARG

    def attn_fwd(N=4, K=16, M=3, null=None):
        p = [None if i == null else held for i in range(8)]
        return L.se3t_attn_fwd(*p[:6], N, K, M, 0.25, p[6], p[7], None)

    def attn_bwd(N=4, K=16, M=3, null=None):
        p = [None if i == null else held for i in range(12)]
        return L.se3t_attn_bwd(*p[:7], N, K, M, 0.25, *p[7:], None)

    for f, n_ptr in ((attn_fwd, 8), (attn_bwd, 12)):
        for bad in (dict(M=2), dict(M=0), dict(K=17), dict(K=0), dict(N=-1), dict(N=big)):
            assert f(**bad) == ARG, (f.__name__, bad)
        assert f(N=0) == OK, f.__name__
        for i in range(n_ptr):
            assert f(null=i) == ARG, (f.__name__, i)

    assert L.se3t_norm_fwd(held, held, 4, 3, 0, 1e-12, held, None) == ARG
    assert L.se3t_norm_fwd(held, held, 4, 2, 64, 1e-12, held, None) == ARG
    assert L.se3t_norm_fwd(held, held, -1, 3, 64, 1e-12, held, None) == ARG
    assert L.se3t_norm_fwd(None, None, 0, 3, 64, 1e-12, None, None) == OK
    for i in range(3):
        p = [None if j == i else held for j in range(3)]
        assert L.se3t_norm_fwd(p[0], p[1], 4, 3, 64, 1e-12, p[2], None) == ARG, i
    need = L.se3t_norm_bwd_workspace_bytes(37, 1024)
    assert need >= 1024 * 4 and need % (1024 * 4) == 0 and L.se3t_norm_bwd_workspace_bytes(37, 0) == 0

    def norm_bwd(R=37, M=3, C=1024, null=None, ws_bytes=need):
        p = [None if i == null else held for i in range(6)]              # x, scale, dy, dx, dscale, workspace
        return L.se3t_norm_bwd(p[0], p[1], p[2], R, M, C, 1e-12, p[3], p[4], p[5], ws_bytes, None)

    for bad in (dict(C=0), dict(M=2), dict(R=-1), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert norm_bwd(**bad) == ARG, bad
    for i in range(6):
        assert norm_bwd(null=i) == ARG, i

    def basis(N=4, K=16, null=None):
        p = [None if i == null else held for i in range(7)]              # pos, nbr, qtab, dist, maskf, meanw, basis
        return L.se3t_edge_basis(p[0], p[1], N, K, 5.0, p[2], p[3], p[4], p[5], p[6], None)

    for bad in (dict(K=17), dict(K=0), dict(N=-1), dict(N=big)):
        assert basis(**bad) == ARG, bad
    assert basis(N=0) == OK
    for i in range(7):
        assert basis(null=i) == ARG, i


def test_visnet_rejects_unsupported_widths():
    from equihgnn_amd.visnet import ViS_MP, ViSNet

    with pytest.raises(ValueError, match=r"hidden channels \(got 12\) must be evenly divisible by the number of "
                                         r"attention heads \(got 8\)"):
        ViS_MP(8, 12, 5.0)
    with pytest.raises(ValueError, match=r"at most 512 hidden channels \(got 520\)"):
        ViS_MP(8, 520, 5.0)
    with pytest.raises(ValueError, match=r"at most 512 hidden channels \(got 520\)"):
        ViSNet(hidden_channels=520, lmax=2, max_num_neighbors=16)
    assert ViS_MP(8, 512, 5.0).head_dim == 64


def test_no_cpu_fallback():
    from equihgnn_amd import hip, ops

    with pytest.raises(hip.HipLibraryError):
        ops.csr_build(torch.zeros(4, dtype=torch.int64), None, 2)
    with pytest.raises(hip.HipLibraryError):
        ops.knn(torch.zeros(20, 3), 16, 0)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "equihgnn_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), fn


def test_registry_contract():
    from equihgnn_amd import models  # noqa: F401  (registers)
    from equihgnn_amd.registry import create_model, registry

    assert registry.get_model_class("egnn_equihnns") is models.EGNNEquiHNNS
    assert registry.get_model_class("nope") is None
    with pytest.raises(ValueError):
        create_model("nope")
    with pytest.raises(ValueError):
        registry.register_model("mhnnm")(object)


def test_state_dict_matches_reference_names():
    """The fixture's grad_names are the reference's named_parameters()."""
    from common import golden_args, load_case

    from equihgnn_amd import models

    for name in ("mhnnm_c64_train", "egnn_equihnns_c64", "equiformer_equihnns_c64", "mhnn_c64", "mhnns_c64",
                 "egnn_equihnn_c64", "egnn_equihnnm_c64", "faformer_equihnns_c64"):
        case = load_case(name)
        method = str(case["meta_method"])
        m = models.MODELS[method](1, golden_args(method, int(case["meta_hidden"])))
        assert sorted(n for n, _ in m.named_parameters()) == sorted(str(n) for n in case["grad_names"])


def test_gemm_x6_tile_choice_is_a_valid_configuration_and_sizes_its_workspace():
    """hg_gemm_x6_choose_tile (the cost estimate behind tile = 0) on host only: a valid tile id for any shape, the big
    configurations for the shapes they were built for, and hg_gemm_x6_workspace_bytes(tile = 0) equal to the chosen
    configuration's own need (the launch re-derives the same choice)."""
    import random

    from equihgnn_amd import hip
    L = hip.lib()
    rng = random.Random(7)

    def prob(m, n, k, ta=0, tb=1):
        pr = (hip.HgGemmProblem * 1)()
        q = pr[0]
        q.m, q.n, q.k, q.trans_a, q.trans_b = m, n, k, ta, tb
        return pr

    for _ in range(300):
        m, n, k = rng.choice([1, 77, 256, 4736, 31232, 250000, 1971840]), 4 * rng.randint(1, 4200), 4 * rng.randint(1, 20000)
        ta = rng.randint(0, 1)
        pr = prob(m if not ta else 4 * ((m + 3) // 4), n, k, ta, rng.randint(0, 1))
        tile = L.hg_gemm_x6_choose_tile(1, pr, 1)
        assert tile in (64, 128, 256, 512, 513), (m, n, k, tile)
        assert L.hg_gemm_x6_workspace_bytes(1, pr, 0) == L.hg_gemm_x6_workspace_bytes(1, pr, tile)
        assert L.hg_gemm_x6_choose_tile(1, pr, 0) in (64, 128, 256, 512, 513)
    assert L.hg_gemm_x6_choose_tile(1, prob(245760, 256, 256), 1) == 512          # [246 k x 256].[256 x 256]: 128 x 256 tiles
    assert L.hg_gemm_x6_choose_tile(1, prob(1971840, 128, 256, 0, 0), 1) == 513    # N = 128: 256 x 128
    assert L.hg_gemm_x6_choose_tile(1, prob(77, 132, 36, 0, 0), 1) == 64
    assert L.hg_gemm_x6_workspace_bytes(1, prob(256, 256, 245760, 1, 0), 0) > 0     # a deep weight gradient is split along k
    assert L.hg_gemm_x6_workspace_bytes(1, prob(245760, 256, 256), 0) == 0
