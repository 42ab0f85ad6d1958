"""The wavefront, MFMA and activation primitives of equihgnn_amd/csrc have ONE definition each, in a header (wave.h,
mfma.h, act.h): a reduction's definition fixes its summation order, so a private copy in a .hip file is a kernel family
that can silently start to round differently from its twins.  Plain text search over the sources, no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "equihgnn_amd", "csrc")
SHARED = ("dpp_move", "wave_sum", "row16_sum", "bcast", "mfma16", "sigmoid_fast")


def sources(*patterns):
    return {os.path.basename(p): open(p).read() for pat in patterns for p in sorted(glob.glob(os.path.join(CSRC, pat)))}


def files_naming(word):
    return sorted(name for name, text in sources("*.hip", "*.h").items() if word in text)


def test_builtins_are_wrapped_once():
    assert files_naming("__builtin_amdgcn_update_dpp") == ["wave.h"]
    assert files_naming("__builtin_amdgcn_mfma_f32_16x16x4f32") == ["mfma.h"]


def test_no_hip_file_defines_a_shared_primitive():
    hip = sources("*.hip")
    assert len(hip) >= 26
    # a definition: the name, a parameter list, then the opening brace of a body
    define = re.compile(r"\b(%s)\s*\([^;{}()]*\)\s*\{" % "|".join(SHARED))
    found = {name: sorted(set(define.findall(text))) for name, text in hip.items() if define.search(text)}
    assert found == {}


def test_each_shared_primitive_is_defined_once_in_a_header():
    headers = sources("*.h")
    for word in SHARED:
        define = re.compile(r"\b%s\s*\([^;{}()]*\)\s*\{" % word)
        assert sum(len(define.findall(text)) for text in headers.values()) == 1, word
