"""csrc/device/dispatch.h maps run-time scene properties to the compile-time
switches of the traced kernels.  A stand-alone C++17 program over the header
alone (host compiler, no HIP) prints what every input dispatches to; each
printed constant is decltype(X)::value, i.e. usable in a template-id.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "cudatracerlib_amd", "csrc", "device")

# the shading levels of common.h: lean, full, env, alpha, mat
ALL_LEVELS = (0, 1, 2, 3, 4)
NO_TRACE_LEVELS = (0, 1, 2, 4)   # kernels that never trace have no alpha instantiation
PROBED = range(-1, 7)

SRC = r"""
#include "dispatch.h"

#include <cstdio>

template <int... L>
void levels(const char* tag) {
    for (int full = -1; full < 7; full++) {
        const bool hit = ctl::with_level<L...>(
            full, [&](auto FU) { std::printf("%s %d call %d\n", tag, full, (int)decltype(FU)::value); });
        std::printf("%s %d hit %d\n", tag, full, (int)hit);
    }
}

int main() {
    for (int i = 0; i < 8; i++) {
        const bool stats = i & 4, single = i & 2, wide = i & 1;
        ctl::with_tree(stats, single, wide, [&](auto ST, auto SG, auto WD) {
            std::printf("tree3 %d %d %d call %d %d %d\n", stats, single, wide, (int)decltype(ST)::value,
                        (int)decltype(SG)::value, (int)decltype(WD)::value);
        });
    }
    for (int i = 0; i < 4; i++) {
        const bool single = i & 2, wide = i & 1;
        ctl::with_tree(single, wide, [&](auto SG, auto WD) {
            std::printf("tree2 %d %d call %d %d\n", single, wide, (int)decltype(SG)::value, (int)decltype(WD)::value);
        });
    }
    levels<0, 1, 2, 3, 4>("all");
    levels<0, 1, 2, 4>("notrace");
    return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("dispatch")
    src, exe = d / "dispatch_probe.cpp", d / "dispatch_probe"
    src.write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", DEVICE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return [tuple(x if i == 0 or x in ("call", "hit") else int(x) for i, x in enumerate(ln.split()))
            for ln in out.splitlines()]


def test_header_is_plain_cxx():
    text = open(os.path.join(DEVICE, "dispatch.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<type_traits>"]


def test_tree_with_stats(lines):
    calls = [ln for ln in lines if ln[0] == "tree3"]
    assert len(calls) == 8                                    # f exactly once per input
    assert len({ln[1:4] for ln in calls}) == 8
    for _, stats, single, wide, _, ST, SG, WD in calls:
        assert (ST, SG) == (stats, single)
        assert WD == (0 if stats else wide)                   # a stats launch runs the binary tree
    triples = {ln[5:] for ln in calls}
    assert len(triples) == 6 and not any(ST and WD for ST, _, WD in triples)


def test_tree_without_stats(lines):
    calls = [ln for ln in lines if ln[0] == "tree2"]
    assert len(calls) == 4
    for _, single, wide, _, SG, WD in calls:
        assert (SG, WD) == (single, wide)
    assert len({ln[4:] for ln in calls}) == 4


@pytest.mark.parametrize("tag,listed", [("all", ALL_LEVELS), ("notrace", NO_TRACE_LEVELS)])
def test_levels(lines, tag, listed):
    for full in PROBED:
        calls = [ln[3] for ln in lines if ln[:3] == (tag, full, "call")]
        hit = [ln[3] for ln in lines if ln[:3] == (tag, full, "hit")]
        if full in listed:
            assert calls == [full] and hit == [1]             # once, with that constant
        else:
            assert calls == [] and hit == [0]                 # nothing called, and reported
