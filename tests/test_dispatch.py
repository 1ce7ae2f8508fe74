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

# the shading levels of dispatch.h: lean, full, env, alpha, mat, lights, media
ALL_LEVELS = (0, 1, 2, 3, 4, 5, 6)
TRACE_LEVELS = (0, 1, 2, 3, 4, 5)         # the path kernels of ctl_trace.hip's code object
MEDIA_LEVELS = (6,)                       # ... and of path_media.hip's
NO_TRACE_LEVELS = (0, 1, 2, 4, 5, 6)      # kernels that never trace have no alpha instantiation
PROBED = range(-1, 9)

# level: (ALPHA, ENV, EXT, DELTA_LIGHTS, MEDIA, no-trace level)
TABLE = {
    0: (0, 0, 0, 0, 0, 0),
    1: (0, 0, 0, 0, 0, 1),
    2: (1, 1, 0, 0, 0, 2),
    3: (1, 0, 0, 0, 0, 1),
    4: (1, 1, 1, 0, 0, 4),
    5: (1, 1, 1, 1, 0, 5),
    6: (1, 1, 1, 1, 1, 6),
}

SRC = r"""
#include "dispatch.h"

#include <cstdio>

template <int... L>
void levels(const char* tag) {
    for (int full = -1; full < 9; full++) {
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
    levels<0, 1, 2, 3, 4, 5, 6>("all");
    levels<0, 1, 2, 3, 4, 5>("trace");
    levels<6>("media");
    levels<0, 1, 2, 4, 5, 6>("notrace");
    for (int l = 0; l < ctl::kShadeLevelCount; l++)
        std::printf("row %d %d %d %d %d %d %d\n", l, (int)ctl::level_alpha(l), (int)ctl::level_env(l),
                    (int)ctl::level_ext(l), (int)ctl::level_delta_lights(l), (int)ctl::level_media(l),
                    ctl::level_no_trace(l));
    for (int i = 0; i < 64; i++) {
        const bool shaded = i & 1, alpha = i & 2, env = i & 4, ext = i & 8, delta = i & 16, volume = i & 32;
        std::printf("scene %d %d %d %d %d %d %d\n", shaded, alpha, env, ext, delta, volume,
                    ctl::scene_level(shaded, alpha, env, ext, delta, volume));
    }
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


@pytest.mark.parametrize("tag,listed", [("all", ALL_LEVELS), ("notrace", NO_TRACE_LEVELS), ("trace", TRACE_LEVELS),
                                        ("media", MEDIA_LEVELS)])
def test_levels(lines, tag, listed):
    for full in PROBED:
        calls = [ln[3] for ln in lines if ln[:3] == (tag, full, "call")]
        hit = [ln[3] for ln in lines if ln[:3] == (tag, full, "hit")]
        if full in listed:
            assert calls == [full] and hit == [1]             # once, with that constant
        else:
            assert calls == [] and hit == [0]                 # nothing called, and reported


def test_level_table(lines):
    rows = {ln[1]: ln[2:] for ln in lines if ln[0] == "row"}
    assert rows == TABLE                                      # every level, and no other
    # the two level lists are what the table says: a no-trace level maps to itself, and
    # ctl_trace.hip's and path_media.hip's lists split the levels by MEDIA
    assert tuple(sorted({row[5] for row in TABLE.values()})) == NO_TRACE_LEVELS
    assert all(TABLE[nt][5] == nt for nt in NO_TRACE_LEVELS)
    assert tuple(l for l in ALL_LEVELS if TABLE[l][4]) == MEDIA_LEVELS
    assert tuple(l for l in ALL_LEVELS if not TABLE[l][4]) == TRACE_LEVELS


def test_scene_level(lines):
    got = {ln[1:7]: ln[7] for ln in lines if ln[0] == "scene"}
    assert len(got) == 64
    # media > lights > mat > env > alpha > full > lean
    for (shaded, alpha, env, ext, delta, volume), level in got.items():
        want = 6 if volume else 5 if delta else 4 if ext else 2 if env else 3 if alpha else 1 if shaded else 0
        assert level == want, (shaded, alpha, env, ext, delta, volume)
