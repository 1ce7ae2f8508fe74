"""dispatch.h with the sensor level: scene_level without a sensor is the function it was (restated here from
the precedence media > lights > mat > env > alpha > full > lean), any scene with another sensor than the
perspective one runs kShadeSensors, and the new row carries every flag the media row carries."""
import os
import shutil
import subprocess

import pytest

DEVICE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cudatracerlib_amd", "csrc", "device")

SRC = r"""
#include "dispatch.h"

#include <cstdio>

int main() {
    std::printf("ids %d %d %d %d\n", (int)ctl::kShadeMedia, (int)ctl::kShadeSensors, ctl::kShadeLevelCount, ctl::kLevelRows);
    for (int l = -1; l <= ctl::kLevelRows; l++)
        std::printf("row %d %d %d %d %d %d %d %d %d\n", l, (int)ctl::shade_level_known(l), (int)ctl::level_alpha(l),
                    (int)ctl::level_env(l), (int)ctl::level_ext(l), (int)ctl::level_delta_lights(l),
                    (int)ctl::level_media(l), (int)ctl::level_sensors(l), ctl::level_no_trace(l));
    for (int i = 0; i < 128; i++) {
        const bool shaded = i & 1, alpha = i & 2, env = i & 4, ext = i & 8, delta = i & 16, volume = i & 32, sensor = i & 64;
        std::printf("scene %d %d %d %d %d %d %d %d %d\n", shaded, alpha, env, ext, delta, volume, sensor,
                    ctl::scene_level(shaded, alpha, env, ext, delta, volume, sensor),
                    sensor ? -1 : ctl::scene_level(shaded, alpha, env, ext, delta, volume));
    }
    for (int full = -1; full < 10; full++) {
        const bool hit = ctl::with_level<ctl::kShadeSensors>(full, [&](auto FU) { std::printf("only %d call %d\n", full, (int)decltype(FU)::value); });
        std::printf("only %d hit %d\n", full, (int)hit);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    d = tmp_path_factory.mktemp("dispatch_sensors")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", DEVICE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return [tuple(x if not x.lstrip("-").isdigit() else int(x) for x in ln.split()) for ln in out.splitlines()]


def parent_scene_level(shaded, alpha, env, ext, delta, volume):
    return 6 if volume else 5 if delta else 4 if ext else 2 if env else 3 if alpha else 1 if shaded else 0


def test_scene_level_without_a_sensor_is_the_parents(lines):
    got = [ln for ln in lines if ln[0] == "scene" and not ln[7]]
    assert len(got) == 64 and len({ln[1:7] for ln in got}) == 64
    for _, shaded, alpha, env, ext, delta, volume, _, level, default_arg in got:
        assert level == default_arg == parent_scene_level(shaded, alpha, env, ext, delta, volume)


def test_any_scene_with_a_sensor_runs_the_sensor_level(lines):
    got = [ln for ln in lines if ln[0] == "scene" and ln[7]]
    assert len(got) == 64
    assert all(ln[8] == 7 for ln in got)


def test_the_sensor_row_carries_what_media_carries(lines):
    ids = [ln for ln in lines if ln[0] == "ids"][0]
    assert ids[1:] == (6, 7, 7, 8)
    rows = {ln[1]: ln[2:] for ln in lines if ln[0] == "row"}
    known, *media = rows[6]
    known7, *sensors = rows[7]
    assert known == known7 == 1
    assert media[:5] == [1, 1, 1, 1, 1] and media[5] == 0 and media[6] == 6
    assert sensors[:5] == media[:5] and sensors[5] == 1 and sensors[6] == 7       # its own no-trace kernels
    assert all(rows[l][6] == 0 for l in range(7))                                  # no lower level has the switch
    assert rows[-1][0] == 0 and rows[8][0] == 0 and rows[8][1:7] == (0,) * 6 and rows[8][7] == 8


def test_with_level_instantiates_the_sensor_level_alone(lines):
    for full in range(-1, 10):
        calls = [ln[3] for ln in lines if ln[:3] == ("only", full, "call")]
        hit = [ln[3] for ln in lines if ln[:3] == ("only", full, "hit")]
        assert (calls, hit) == (([7], [1]) if full == 7 else ([], [0]))
