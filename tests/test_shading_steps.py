"""The integrators' shared hit-shading steps are stated once (csrc/device/shading.h,
beside traverse.h's material index): no integrator file restates the fill_dg
call, the material index, the emitter choice or the wave-aggregated cursor claim."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "cudatracerlib_amd", "csrc", "device")


def _sources():
    files = sorted(p for ext in ("*.hip", "*.h") for p in glob.glob(os.path.join(DEVICE, ext)))
    assert len(files) >= 16 and os.path.join(DEVICE, "shading.h") in files
    return {os.path.basename(p): open(p).read() for p in files}


def _lines_with(text, needle):
    return [f"{i}: {ln.strip()}" for i, ln in enumerate(text.splitlines(), 1) if needle in ln]


def test_surface_step_only_in_shading_and_traverse():
    found = [f"{name}:{hit}" for name, text in _sources().items() if name not in ("shading.h", "traverse.h")
             for needle in ("fill_dg(", ".material_offset") for hit in _lines_with(text, needle)]
    assert not found, "the surface at a hit is shading.h's surface_at:\n" + "\n".join(found)


def test_light_cdf_upper_bound_stated_once():
    search = re.compile(r"sample\.x\s*<\s*S\.light_cdf\[")
    found = [f"{name}:{i}" for name, text in _sources().items()
             for i, ln in enumerate(text.splitlines(), 1) if search.search(ln)]
    assert len(found) == 1 and found[0].startswith("shading.h:"), found


def test_cursor_claims_go_through_wave_claim():
    found = [f"{name}:{hit}" for name, text in _sources().items() if name.endswith(".hip") and name != "prim.hip"
             for hit in _lines_with(text, "atomicAdd(cursor")]
    assert not found, "claim slots through common.h's wave_claim:\n" + "\n".join(found)
    # prim_kernel's fixed 64-per-wave fetch is the one other claim
    assert len(_lines_with(_sources()["prim.hip"], "atomicAdd(cursor")) == 1
