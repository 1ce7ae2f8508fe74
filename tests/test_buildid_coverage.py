"""Every file libctl_trace.so is compiled from is in the source fingerprint
(buildid.py): the persistent path kernels' loop lives in a file of its own,
included as the body of two kernel templates, and those templates in a header
that two code objects include; a profile of that kernel must not be matched to
a binary built from an edited loop or header."""
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from buildid import source_fingerprint  # noqa: E402

CSRC = os.path.join("cudatracerlib_amd", "csrc")


def _copy_sources(dst):
    shutil.copytree(os.path.join(ROOT, CSRC), os.path.join(dst, CSRC))
    shutil.copy(os.path.join(ROOT, "cudatracerlib_amd", "Makefile"), os.path.join(dst, "cudatracerlib_amd"))
    os.makedirs(os.path.join(dst, "include"))
    shutil.copy(os.path.join(ROOT, "include", "ctl_trace.h"), os.path.join(dst, "include"))


def test_every_csrc_file_changes_the_fingerprint(tmp_path):
    dst = str(tmp_path)
    _copy_sources(dst)
    base = source_fingerprint(ROOT)
    assert source_fingerprint(dst) == base
    rel = [os.path.relpath(os.path.join(d, n), dst) for d, _, names in os.walk(os.path.join(dst, CSRC)) for n in names]
    assert os.path.join(CSRC, "device", "persistent_loop.h") in rel
    assert os.path.join(CSRC, "device", "path_kernels.h") in rel
    for r in sorted(rel):
        path = os.path.join(dst, r)
        with open(path, "rb") as f:
            kept = f.read()
        with open(path, "ab") as f:
            f.write(b"\n")
        assert source_fingerprint(dst) != base, r
        with open(path, "wb") as f:
            f.write(kept)
    assert source_fingerprint(dst) == base
