"""csrc/device/devmem.h owns the device layer's device and pinned memory.  A
stand-alone C++17 program (host compiler, AddressSanitizer + UBSan) drives the
real header over a stand-in hip/hip_runtime.h that is backed by malloc, counts
live allocations, records the sizes asked for and can fail the k-th
allocation.  A source check keeps raw allocation calls out of every other
file of the device layer.  No GPU."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "cudatracerlib_amd", "csrc", "device")

# only what devmem.h uses
FAKE_HIP = r"""
#pragma once
#include <cstddef>
#include <cstdlib>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
struct FakeEvent { int id; };
typedef FakeEvent* hipEvent_t;
enum : unsigned { hipHostMallocDefault = 0, hipEventDefault = 0, hipEventDisableTiming = 2 };

struct FakeHip {
    long live_dev = 0, live_host = 0, live_ev = 0;
    long frees = 0;
    int fail_in = 0;                 // k > 0: the k-th allocation from now fails
    hipError_t last = hipSuccess;
    std::vector<size_t> sizes;       // bytes of every allocation asked for, failed ones included
};
inline FakeHip& fake() { static FakeHip f; return f; }

inline hipError_t fake_alloc(void** p, size_t bytes, long& live) {
    FakeHip& f = fake();
    f.sizes.push_back(bytes);
    if (f.fail_in > 0 && --f.fail_in == 0) {
        *p = nullptr;
        return f.last = hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    live++;
    return hipSuccess;
}
inline hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes, fake().live_dev); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_alloc(p, bytes, fake().live_host); }
inline hipError_t hipFree(void* p) { std::free(p); fake().live_dev--; fake().frees++; return hipSuccess; }
inline hipError_t hipHostFree(void* p) { std::free(p); fake().live_host--; fake().frees++; return hipSuccess; }
inline hipError_t hipGetLastError() { const hipError_t e = fake().last; fake().last = hipSuccess; return e; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = new FakeEvent{0}; fake().live_ev++; return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t e) { delete e; fake().live_ev--; return hipSuccess; }
"""

SRC = r"""
#include "devmem.h"

#include <cstdint>
#include <cstdio>

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

template <class A>
int array_checks(long& live) {
    FakeHip& f = fake();
    const long frees0 = f.frees;
    {
        A a;
        CHECK(a.get() == nullptr && a.cap() == 0 && !a);
        CHECK(a.fits(0) && !a.fits(1));
        f.sizes.clear();
        CHECK(a.grow(10, 64) == hipSuccess);
        CHECK(f.sizes.size() == 1 && f.sizes[0] == 10 * sizeof(*a.get()) + 64);   // n * sizeof(T) + pad
        CHECK(a.cap() == 10 && a && live == 1);
        auto* const p = a.get();
        CHECK(a.fits(10) && a.fits(3) && !a.fits(11));
        CHECK(a.get() == p);                                     // fitting: the pointer is kept
        p[9] = {};                                               // the last element is inside the allocation
        CHECK(a.grow(25) == hipSuccess);                         // frees the old one first
        CHECK(f.sizes.back() == 25 * sizeof(*a.get()) && a.cap() == 25 && live == 1 && f.frees == frees0 + 1);
        // a failed grow: empty, capacity 0, the error consumed; a later grow succeeds
        f.fail_in = 1;
        CHECK(a.grow(40, 16) == hipErrorOutOfMemory);
        CHECK(f.sizes.back() == 40 * sizeof(*a.get()) + 16);
        CHECK(a.get() == nullptr && a.cap() == 0 && !a && !a.fits(1) && live == 0);
        CHECK(f.last == hipSuccess && hipGetLastError() == hipSuccess);
        CHECK(a.grow(40, 16) == hipSuccess && a.cap() == 40 && live == 1);
        // move construction and move assignment: one owner at a time, one free each
        auto* const q = a.get();
        A b(std::move(a));
        CHECK(b.get() == q && b.cap() == 40 && a.get() == nullptr && a.cap() == 0 && live == 1);
        A c;
        CHECK(c.grow(5) == hipSuccess && live == 2);
        const long frees1 = f.frees;
        c = std::move(b);                                        // frees c's own, takes b's
        CHECK(c.get() == q && c.cap() == 40 && b.get() == nullptr && live == 1 && f.frees == frees1 + 1);
        A& self = c;
        c = std::move(self);                                     // self-assignment keeps it
        CHECK(c.get() == q && live == 1);
        c.reset();
        CHECK(c.get() == nullptr && c.cap() == 0 && live == 0 && f.frees == frees1 + 2);
        CHECK(c.grow(7) == hipSuccess && live == 1);
    }                                                            // the destructor frees
    CHECK(live == 0);
    return 0;
}

int pool_checks() {
    FakeHip& f = fake();
    {
        ctl::DevPool pool;
        float* x = nullptr;
        uint64_t* y = nullptr;
        char* z = nullptr;
        f.sizes.clear();
        CHECK(pool.alloc(&x, 3, 64) == hipSuccess && pool.alloc(&y, 5, 16) == hipSuccess && pool.alloc(&z, 9) == hipSuccess);
        CHECK(f.sizes.size() == 3 && f.sizes[0] == 3 * 4 + 64 && f.sizes[1] == 5 * 8 + 16 && f.sizes[2] == 9);
        CHECK(x && y && z && f.live_dev == 3);
        int* w = reinterpret_cast<int*>(0x10);
        f.fail_in = 1;
        CHECK(pool.alloc(&w, 4, 64) == hipErrorOutOfMemory);     // not remembered, the error consumed, *p untouched
        CHECK(w == reinterpret_cast<int*>(0x10) && f.live_dev == 3 && f.last == hipSuccess);
        const long frees0 = f.frees;
        pool.release(y);                                         // exactly that entry
        CHECK(f.live_dev == 2 && f.frees == frees0 + 1);
        pool.release(y);                                         // no longer the pool's: nothing happens
        CHECK(f.live_dev == 2 && f.frees == frees0 + 1);
        x[2] = 1.0f; z[8] = 1;                                   // the others are still alive (ASan would object)
        pool.clear();
        CHECK(f.live_dev == 0 && f.frees == frees0 + 3);
        CHECK(pool.alloc(&x, 2) == hipSuccess && pool.alloc(&y, 2) == hipSuccess && f.live_dev == 2);
    }                                                            // the destructor frees all of them
    CHECK(f.live_dev == 0);
    return 0;
}

int event_checks() {
    FakeHip& f = fake();
    {
        ctl::Event e, never;
        CHECK(!static_cast<hipEvent_t>(e));
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && static_cast<hipEvent_t>(e) && f.live_ev == 1);
        CHECK(!static_cast<hipEvent_t>(never));
    }
    CHECK(f.live_ev == 0);
    return 0;
}

int main() {
    if (array_checks<ctl::DevArray<double>>(fake().live_dev)) return 1;
    CHECK(fake().live_host == 0);
    if (array_checks<ctl::PinnedArray<uint16_t>>(fake().live_host)) return 1;
    if (pool_checks() || event_checks()) return 1;
    CHECK(fake().live_dev == 0 && fake().live_host == 0 && fake().live_ev == 0);
    std::printf("devmem ok\n");
    return 0;
}
"""


def test_owners_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text(FAKE_HIP)
    src, exe = tmp_path / "devmem_probe.cpp", tmp_path / "devmem_probe"
    src.write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(tmp_path), "-I", DEVICE, str(src), "-o", str(exe)],
                   check=True)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("devmem ok"), r.stdout + r.stderr


def test_header_includes():
    text = open(os.path.join(DEVICE, "devmem.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes[0] == "<hip/hip_runtime.h>"
    assert includes[1:] and all(re.fullmatch(r"<[a-z_]+>", inc) for inc in includes[1:])   # standard headers only
    assert "namespace ctl" in text and "__global__" not in text and "__device__" not in text


def test_no_raw_allocation_outside_devmem():
    files = [p for ext in ("*.hip", "*.h") for p in glob.glob(os.path.join(DEVICE, ext))
             if os.path.basename(p) != "devmem.h"]
    assert len(files) >= 15
    raw = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(")
    found = [f"{os.path.basename(p)}:{i}: {ln.strip()}" for p in sorted(files)
             for i, ln in enumerate(open(p).read().splitlines(), 1) if raw.search(ln)]
    assert not found, "allocate through devmem.h's owners:\n" + "\n".join(found)
