"""Which build of the match-finder kernels a batch launch takes (lz77_hooks_build, moonbit-flate_amd/csrc/
deflate_plan.h), on the CPU: the product instantiations, whose batch loop carries no test hook, unless the call has set
"debug_stall_batch" or "debug_drop_window_push" -- then, and only then, the HOOKS instantiations.  tests/host_model/
lz77_hooks_rule_model.cpp includes the header the driver includes; the driver's one use of the rule is checked in its
source, and that the two builds give the same bytes is tests/test_gpu_lz77_hot_loop.py's to show."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "lz77_hooks_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "deflate_plan.h"), os.path.join(CSRC, "flate_common.h"), os.path.join(INC, "flate_hip.h")]
LIB = os.path.join(HERE, "host_model", "liblz77_hooks_rule_model.so")


@pytest.fixture(scope="module")
def rule():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (LIB, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, SRC, "-o", tmp])
        os.replace(tmp, LIB)
    L = C.CDLL(LIB)
    L.hooks_build_model.argtypes = [C.c_uint32, C.c_uint32]
    L.hooks_build_model.restype = C.c_int
    return L.hooks_build_model


VALUES = [0, 1, 2, 3, 0x7fffffff, 0x80000000, 0xffffffff]


def test_no_option_set_is_the_product_build(rule):
    assert rule(0, 0) == 0


def test_either_option_alone_or_both_is_the_hooks_build(rule):
    for stall in VALUES:
        for drop in VALUES:
            assert rule(stall, drop) == int(stall != 0 or drop != 0), (stall, drop)


def test_the_driver_asks_the_rule_once_with_the_two_options():
    text = open(os.path.join(CSRC, "flate_api_deflate.hip")).read()
    assert len(re.findall(r"lz77_hooks_build\(", text)) == 1
    assert "lz77_hooks_build(c->inject_stall, c->inject_drop_push)" in text
    # every stream kernel it launches is picked by that one answer: no launch names a build outright
    for kernel in ("lz77_wave_kernel", "lz77_guest_kernel", "lz77_wave_dict_kernel", "lz77_guest_dict_kernel"):
        uses = [st for st in text.split(";") if kernel + "<" in st]
        assert uses and all(re.search(r"=\s*hooks\s*\?", st) for st in uses), (kernel, uses)
