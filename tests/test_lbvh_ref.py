"""The numpy restatement of the device mesh builder (tests/lbvh_ref.py) builds
well-formed, tight trees that traverse to the truth: this pins the specification
the GPU tests (test_gpu_mesh_rebuild.py) compare the device against byte for byte.
CPU only."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import camera_rays, oracle_trace, random_rays
from lbvh_cases import ALL, desc_with_trees, mesh, restate, single_scene

SENT = 0x76543210
_CACHE = {}


def case(ctl, name):
    """(positions, restated trees, compiled single-node desc), built once per mesh."""
    if name not in _CACHE:
        P = mesh(name)
        s = single_scene(ctl, P)
        _CACHE[name] = (P, restate(ctl, P), s.compile(), s)
    return _CACHE[name][:3]


@pytest.mark.parametrize("name", ALL)
def test_restated_tree_is_well_formed(ctl, name):
    P, R, d = case(ctl, name)
    n = P.shape[0]
    A = ctl._abi
    nodes = np.ascontiguousarray(R["nodes"])
    arr = (A.BVHNode * nodes.shape[0]).from_buffer_copy(nodes.tobytes())
    bin_bound, _ = ctl.bvh_stack_bound(arr)     # throws on a malformed tree
    assert bin_bound == R["bin_bound"]
    # every triangle once, each the last of its leaf
    assert np.array_equal(np.sort(R["idx"] >> 1), np.arange(n, dtype=np.uint32))
    assert np.all(R["idx"] & 1)
    # leaves in child words: every entry once
    words = nodes.view(np.int32)[:, 12:14].ravel()
    leaves = ~words[(words < 0)]
    assert np.array_equal(np.sort(leaves), np.arange(n))
    assert nodes.view(np.uint32)[0, 14] == 0xffffffff and np.all(nodes[:, 15] == 0)
    if n == 1:
        assert words[1] == SENT
    if R["wide"] is not None:
        W = R["wide"]
        child = W.view(np.int32)[:, 24:28]
        assert np.all(W.view(np.uint32)[:, 28:32] == 0)
        lf = (child < 0)
        codes = ~child[lf]
        assert np.all((codes & 7) == 1)
        assert np.array_equal(np.sort(codes >> 3), np.arange(n))
        inner = child[(child >= 0) & (child != SENT)]
        assert np.array_equal(np.sort(inner), np.arange(1, W.shape[0]))   # every node but the root is one node's child
        empty = child == SENT
        for f in range(6):
            assert np.all(np.isnan(W[:, 4 * f:4 * f + 4][empty]))
        # the 4-wide stack bound of the restatement is the tree's (1 + sum(children - 1) along a path)
        below = np.zeros(W.shape[0], np.int64)
        order, best = [0], 0
        below[0] = 1
        while order:
            k = order.pop()
            used = int((child[k] != SENT).sum())
            here = below[k] + max(used - 1, 0)
            best = max(best, here)
            for c in child[k]:
                if c >= 0 and c != SENT:
                    below[c] = here
                    order.append(int(c))
        assert best == R["wide_bound"]


@pytest.mark.parametrize("name", ALL)
def test_child_boxes_are_exact(ctl, name):
    """Every stored child box is the exact min / max of the triangles under it."""
    P, R, d = case(ctl, name)
    n = P.shape[0]
    if n == 1:
        V = P.reshape(3, 3)
        assert np.array_equal(R["nodes"][0, [0, 2, 8]], V.min(0)) and np.array_equal(R["nodes"][0, [1, 3, 9]], V.max(0))
        return
    V = P[R["order"]].reshape(n, 3, 3)
    lo, hi = V.min(1), V.max(1)
    kids = R["kids"]
    # entries under each node: a post-order accumulation over the range ends (Karras ranges are contiguous)
    first = np.zeros(n - 1, np.int64)
    last = np.zeros(n - 1, np.int64)
    done = np.zeros(n - 1, bool)
    stack = [0]
    while stack:
        x = stack[-1]
        pend = [int(k) >> 2 for k in kids[x] if k >= 0 and not done[int(k) >> 2]]
        if pend:
            stack.extend(pend)
            continue
        stack.pop()
        ends = [(~int(k), ~int(k)) if k < 0 else (first[int(k) >> 2], last[int(k) >> 2]) for k in kids[x]]
        first[x], last[x] = min(e[0] for e in ends), max(e[1] for e in ends)
        done[x] = True
    nodes = R["nodes"]
    slot = {0: ([0, 2, 8], [1, 3, 9]), 1: ([4, 6, 10], [5, 7, 11])}
    for x in range(n - 1):
        for q in range(2):
            k = int(kids[x, q])
            a, b = (~k, ~k) if k < 0 else (first[k >> 2], last[k >> 2])
            assert np.array_equal(nodes[x, slot[q][0]], lo[a:b + 1].min(0)), (x, q)
            assert np.array_equal(nodes[x, slot[q][1]], hi[a:b + 1].max(0)), (x, q)
    assert np.array_equal(R["box"], np.concatenate([lo.min(0), hi.max(0)]))


# random rays from inside the scene box and camera rays from above (a flat mesh's box holds
# only rays in its plane); fewer on the large mesh: the brute-force scan is n x rays
def _rays(d, n):
    k, side = (1000, 32) if n > 10000 else (5000, 56)
    cam = camera_rays(d, side, side, seed=12)
    cam[:, 3] = float(d.ray_eps)
    return np.ascontiguousarray(np.concatenate([random_rays(d, k, seed=11, tmin=float(d.ray_eps)), cam]))


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("mode", ["binary", "wide"])
def test_restated_tree_traverses_to_brute_force(ctl, orc, name, mode):
    """oracle_trace over a desc carrying the restated arrays finds what a scan of
    every triangle finds.  The float slab test may drop a sliver of rays: at most
    1 in 1000, none on the axis-aligned grid."""
    P, R, d = case(ctl, name)
    keep = []
    d2 = desc_with_trees(ctl, d, R["nodes"], R["woop"], R["idx"], keep=keep)
    rays = _rays(d2, P.shape[0])
    tie = 0
    if mode == "wide":
        _, _, sc = ctl.host_wide_trees(d)
        W = np.ascontiguousarray(R["wide"])
        wbase = np.zeros(1, np.uint32)
        orc.oracle_set_wide(C.byref(d2), oracle.ptr(W), W.shape[0], oracle.ptr(wbase), 1, oracle.ptr(sc), sc.shape[0])
        tie = oracle.TRAVERSE_WIDE
    t, u, v, tri, node, st = oracle_trace(orc, d2, rays, mode=0, tie=tie)
    bt = np.zeros(rays.shape[0], np.float32)
    btri = np.zeros(rays.shape[0], np.uint32)
    orc.oracle_brute_force(C.byref(d2), rays.shape[0], oracle.ptr(rays), oracle.ptr(bt), oracle.ptr(btri), 0)
    differ = int((t != bt).sum())
    print(f"{name} {mode}: {differ} of {rays.shape[0]} rays differ from brute force, {(btri != 0xFFFFFFFF).sum()} hit")
    assert (btri != 0xFFFFFFFF).sum() >= 50
    assert differ <= (0 if name == "flat" else rays.shape[0] // 1000)
