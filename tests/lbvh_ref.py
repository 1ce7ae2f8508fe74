"""numpy (fp32) restatement of the device mesh builder (csrc/device/lbvh.hip,
ctl_scene_rebuild_mesh): for a position array, every byte the device must
produce -- binary nodes, Woop records, index words, 4-wide nodes, mesh box and
the two stack bounds.  Test infrastructure; each step is vectorised over the
triangles / nodes of a level, so 70 k triangles take seconds.

Steps (the device file's header states them in full):
  box    per triangle min / max of the vertices, + 0.0f; proxy c = lo + hi
  key    q = (c - cb_lo) / (cb_hi - cb_lo) (0 on zero extent), 21-bit codes,
         63-bit Morton key, x highest
  sort   stable, ascending, by key (equal keys keep triangle order)
  tree   Karras 2012 over delta = clz64(key_i ^ key_j) | 64 + clz32(i ^ j)
  fit    child boxes by min / max; area 2 (dx dy + dy dz + dz dx); height
  wide   greedy collapse by level (open the inner child of largest area, a tie
         to the lowest slot; the opened slot takes child 0, child 1 the first
         free slot); wide index = exclusive prefix sum over the binary node
         index of "starts a wide node"
"""
import numpy as np

SENT = 0x76543210
F32 = np.float32


def _clz64(x):
    """Leading zeros of non-zero uint64 values."""
    x = x.astype(np.uint64).copy()
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(64 - s)) == 0
        n += m * s
        x = np.where(m, x << np.uint64(s), x)
    return n


def _spread3(v):
    x = v.astype(np.uint64) & np.uint64(0x1fffff)
    x = (x | x << np.uint64(32)) & np.uint64(0x1f00000000ffff)
    x = (x | x << np.uint64(16)) & np.uint64(0x1f0000ff0000ff)
    x = (x | x << np.uint64(8)) & np.uint64(0x100f00f00f00f00f)
    x = (x | x << np.uint64(4)) & np.uint64(0x10c30c30c30c30c3)
    x = (x | x << np.uint64(2)) & np.uint64(0x1249249249249249)
    return x


def tri_boxes(P):
    V = np.ascontiguousarray(P, F32).reshape(-1, 3, 3)
    lo = (V.min(axis=1) + F32(0)).astype(F32)
    hi = (V.max(axis=1) + F32(0)).astype(F32)
    return lo, hi


def morton_keys(lo, hi):
    c = (lo + hi).astype(F32)
    cb_lo, cb_hi = c.min(axis=0), c.max(axis=0)
    ext = (cb_hi - cb_lo).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ((c - cb_lo).astype(F32) / ext).astype(F32)
    q = np.where(ext == 0, F32(0), q).astype(F32)
    code = np.minimum((q * F32(2097152.0)).astype(F32).astype(np.uint32), np.uint32(0x1fffff))
    return _spread3(code[:, 0]) << np.uint64(2) | _spread3(code[:, 1]) << np.uint64(1) | _spread3(code[:, 2])


def _delta(keys, i, j):
    n = keys.size
    ok = (j >= 0) & (j < n)
    jj = np.clip(j, 0, n - 1)
    x = keys[i] ^ keys[jj]
    same = x == 0
    ij = (i ^ jj).astype(np.uint64)
    d = np.where(same, 64 + _clz64(np.where(ij == 0, np.uint64(1), ij)) - 32, _clz64(np.where(same, np.uint64(1), x)))
    return np.where(ok, d, -1)


def karras(keys):
    """Child words (n - 1, 2) int64 of the inner nodes; child 0 the left range."""
    n = keys.size
    i = np.arange(n - 1, dtype=np.int64)
    d = np.where(_delta(keys, i, i + 1) > _delta(keys, i, i - 1), 1, -1).astype(np.int64)
    dmin = _delta(keys, i, i - d)
    lmax = np.full(n - 1, 2, np.int64)
    while True:
        grow = _delta(keys, i, i + lmax * d) > dmin
        if not grow.any():
            break
        lmax = np.where(grow, lmax * 2, lmax)
    l = np.zeros(n - 1, np.int64)
    t = lmax // 2
    while (t >= 1).any():
        act = t >= 1
        take = act & (_delta(keys, i, i + (l + t) * d) > dmin)
        l = np.where(take, l + t, l)
        t = t // 2
    j = i + l * d
    dnode = _delta(keys, i, j)
    s = np.zeros(n - 1, np.int64)
    t = (l + 1) >> 1
    act = np.ones(n - 1, bool)
    while act.any():
        take = act & (_delta(keys, i, i + (s + t) * d) > dnode)
        s = np.where(take, s + t, s)
        act = act & (t > 1)
        t = (t + 1) >> 1
    g = i + s * d + np.where(d < 0, -1, 0)
    first, last = np.minimum(i, j), np.maximum(i, j)
    c0 = np.where(first == g, ~g, 4 * g)
    c1 = np.where(last == g + 1, ~(g + 1), 4 * (g + 1))
    return np.stack([c0, c1], 1)


def _area(lo, hi):
    d = (hi - lo).astype(F32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (F32(2.0) * (((dx * dy).astype(F32) + (dy * dz).astype(F32)).astype(F32) + (dz * dx).astype(F32)).astype(F32)).astype(F32)


def build(positions, woop_set, wide=True):
    """positions: (n, 9) float32; woop_set(v0, v1, v2) -> (n, 12) float32 (ctl.woop_set).
    Returns a dict: nodes (max(n - 1, 1), 16) float32, woop (n, 12) float32, idx (n,) uint32,
    wide (n_wide, 32) float32 or None, box (6,) float32, bin_bound, wide_bound, order (the
    triangle of every entry), kids (n - 1, 2) int64."""
    P = np.ascontiguousarray(positions, F32).reshape(-1, 9)
    n = P.shape[0]
    lo, hi = tri_boxes(P)
    if n == 1:
        order = np.zeros(1, np.int64)
    else:
        keys = morton_keys(lo, hi)
        order = np.argsort(keys, kind="stable").astype(np.int64)
        keys = keys[order]
    Ps = P[order]
    llo, lhi = lo[order], hi[order]
    out = {"order": order, "idx": (order.astype(np.uint32) << np.uint32(1)) | np.uint32(1),
           "woop": np.ascontiguousarray(woop_set(Ps[:, 0:3], Ps[:, 3:6], Ps[:, 6:9]), F32).reshape(n, 12)}
    nan = np.uint32(0x7fc00000)
    if n == 1:
        nodes = np.zeros((1, 16), F32)
        nodes[0, 0:4] = [llo[0, 0], lhi[0, 0], llo[0, 1], lhi[0, 1]]
        nodes[0, 8:10] = [llo[0, 2], lhi[0, 2]]
        nodes.view(np.uint32)[0, 12:15] = [0xffffffff, SENT, 0xffffffff]
        out.update(nodes=nodes, box=np.concatenate([llo[0], lhi[0]]), bin_bound=1, wide_bound=1 if wide else 0,
                   kids=np.zeros((0, 2), np.int64), wide=None)
        if wide:
            w = np.zeros((1, 32), F32)
            wu = w.view(np.uint32)
            wu[0, 0:24] = nan
            for f in range(6):
                w[0, 4 * f] = (lhi if f & 1 else llo)[0, f >> 1]
            wu[0, 24:28] = [np.uint32(~np.int64(1) & 0xffffffff), SENT, SENT, SENT]
            out["wide"] = w
        return out
    ni = n - 1
    kids = karras(keys)
    leaf = kids < 0
    # parents and depths, level by level from the root
    parent = np.full(ni, -1, np.int64)
    depth = np.full(ni, -1, np.int64)
    depth[0] = 0
    front = np.array([0], np.int64)
    lv = 0
    while front.size:
        k = kids[front]
        inner = ~leaf[front]
        ch = (k[inner] >> 2)
        parent[ch] = np.repeat(front, 2).reshape(-1, 2)[inner]
        lv += 1
        depth[ch] = lv
        front = ch
    assert (depth >= 0).all(), "restated tree: a node is not reached from the root"
    # fit, deepest level first
    nlo = np.zeros((ni, 3), F32)
    nhi = np.zeros((ni, 3), F32)
    height = np.zeros(ni, np.int64)
    clo = np.zeros((ni, 2, 3), F32)
    chi = np.zeros((ni, 2, 3), F32)
    for dlev in range(int(depth.max()), -1, -1):
        x = np.nonzero(depth == dlev)[0]
        hh = np.zeros((x.size, 2), np.int64)
        for q in range(2):
            k = kids[x, q]
            lf = k < 0
            e = np.where(lf, ~k, 0)
            c = np.where(lf, 0, k >> 2)
            clo[x, q] = np.where(lf[:, None], llo[e], nlo[c])
            chi[x, q] = np.where(lf[:, None], lhi[e], nhi[c])
            hh[:, q] = np.where(lf, 0, height[c])
        nlo[x] = np.minimum(clo[x, 0], clo[x, 1])
        nhi[x] = np.maximum(chi[x, 0], chi[x, 1])
        height[x] = 1 + hh.max(axis=1)
    area = _area(nlo, nhi)
    nodes = np.zeros((ni, 16), F32)
    nodes[:, 0] = clo[:, 0, 0]; nodes[:, 1] = chi[:, 0, 0]; nodes[:, 2] = clo[:, 0, 1]; nodes[:, 3] = chi[:, 0, 1]
    nodes[:, 4] = clo[:, 1, 0]; nodes[:, 5] = chi[:, 1, 0]; nodes[:, 6] = clo[:, 1, 1]; nodes[:, 7] = chi[:, 1, 1]
    nodes[:, 8] = clo[:, 0, 2]; nodes[:, 9] = chi[:, 0, 2]; nodes[:, 10] = clo[:, 1, 2]; nodes[:, 11] = chi[:, 1, 2]
    nu = nodes.view(np.uint32)
    nu[:, 12] = (kids[:, 0] & 0xffffffff).astype(np.uint32)
    nu[:, 13] = (kids[:, 1] & 0xffffffff).astype(np.uint32)
    nu[:, 14] = np.where(parent < 0, 0xffffffff, 4 * parent).astype(np.uint32)
    out.update(nodes=nodes, box=np.concatenate([nlo[0], nhi[0]]), bin_bound=1 + int(height[0]), kids=kids,
               wide=None, wide_bound=0)
    if not wide:
        return out
    # greedy collapse, level by level
    flag = np.zeros(ni, np.int64)
    wk = np.full((ni, 4), SENT, np.int64)
    front = np.array([0], np.int64)
    below = np.array([1], np.int64)
    bound = 0
    while front.size:
        m = front.size
        K = np.full((m, 4), SENT, np.int64)
        K[:, 0:2] = kids[front]
        nk = np.full(m, 2, np.int64)
        rows = np.arange(m)
        for _ in range(2):
            slot = np.arange(4)[None, :]
            inner = (slot < nk[:, None]) & (K >= 0)
            a = np.where(inner, area[np.where(inner, K >> 2, 0)], F32(-1.0))
            best = np.argmax(a, axis=1)
            has = inner.any(axis=1)
            r = rows[has]
            c = K[r, best[r]] >> 2
            K[r, best[r]] = kids[c, 0]
            K[r, nk[r]] = kids[c, 1]
            nk[r] += 1
        here = below + nk - 1
        bound = max(bound, int(here.max()))
        flag[front] = 1
        wk[front] = K
        nxt = (np.arange(4)[None, :] < nk[:, None]) & (K >= 0)
        front = (K[nxt] >> 2)
        below = np.repeat(here, 4).reshape(-1, 4)[nxt]
    widx = np.cumsum(flag) - flag
    b = np.nonzero(flag)[0]
    W = np.zeros((b.size, 32), F32)
    Wu = W.view(np.uint32)
    for q in range(4):
        k = wk[b, q]
        empty = k == SENT
        lf = (k < 0)
        e = np.where(lf, ~k, 0)
        c = np.where(lf | empty, 0, k >> 2)
        blo = np.where(lf[:, None], llo[e], nlo[c])
        bhi = np.where(lf[:, None], lhi[e], nhi[c])
        for ax in range(3):
            W[:, 8 * ax + q] = blo[:, ax]
            W[:, 8 * ax + 4 + q] = bhi[:, ax]
        for f in range(6):
            Wu[empty, 4 * f + q] = nan
        code = np.where(empty, SENT, np.where(lf, ~((e << 3) | 1), widx[c]))
        Wu[:, 24 + q] = (code & 0xffffffff).astype(np.uint32)
    out.update(wide=W, wide_bound=bound)
    return out
