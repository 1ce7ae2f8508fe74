"""The host block sampler (ctl_block_sampler_*, csrc/host/block_sampler.cpp)
against a numpy restatement of VarianceBlockSampler's formulas: get_w1 / get_w2,
the min/max normalisation, weight = (0.85 w1n + 0.15 w2n) * userWeight^2, the
descending order with the documented tie and NaN rules, and MixedBlockIterate's
list.  No GPU."""
import numpy as np
import pytest

f32 = np.float32


def make_info(ctl, n, seed=0):
    """n records with distinct, well separated weights."""
    rng = np.random.default_rng(seed)
    a = np.zeros(n, ctl.BLOCK_INFO_DTYPE)
    npx = 1024
    a["num_pixels_var"] = npx
    a["num_pixels_e"] = npx
    a["block_var_i"] = (rng.permutation(n) + 1).astype(f32) * f32(3.0)     # distinct w1
    mean = rng.random(n).astype(f32) + f32(0.5)
    spread = (rng.permutation(n) + 1).astype(f32) * f32(0.01)               # distinct w2
    a["block_e_i"] = mean * f32(npx)
    a["block_e_i2"] = (mean * mean + spread) * f32(npx)
    return a


def np_weights(info, user):
    """fp32, operation by operation as TmpBlockInfo::getWeight x userWeight^2."""
    with np.errstate(all="ignore"):
        nv = info["num_pixels_var"]
        w1 = np.where(nv == 0, f32(0), np.sqrt(info["block_var_i"] / np.maximum(nv, 1).astype(f32))).astype(f32)
        ne = info["num_pixels_e"].astype(f32)
        e = info["block_e_i"] / ne
        w2 = np.sqrt(info["block_e_i2"] / ne - e * e).astype(f32)
        # min / max by comparison: a NaN term never wins
        lo1, hi1, lo2, hi2 = np.fmin.reduce(w1), np.fmax.reduce(w1), np.fmin.reduce(w2), np.fmax.reduce(w2)
        w1n = (w1 - lo1) / (hi1 - lo1)
        w2n = (w2 - lo2) / (hi2 - lo2)
        lam = f32(0.85)
        return ((lam * w1n + (f32(1) - lam) * w2n) * (user * user)).astype(f32)


def np_order(w):
    """Descending weight; NaN below every number; ties by ascending id."""
    key = np.where(np.isnan(w), -np.inf, w.astype(np.float64))
    return np.lexsort((np.arange(w.size), -key)).astype(np.uint32)


def np_list(order, n, passes_done, fd, fw, variance=True):
    if not variance or passes_done < 10:
        return np.arange(n, dtype=np.uint32)
    return np.concatenate([order[:n // fw], np.arange(passes_done % fd, n, fd, dtype=np.uint32)]).astype(np.uint32)


@pytest.mark.parametrize("w,h,ts", [(96, 64, 32), (224, 160, 32)])          # 6 and 35 blocks
@pytest.mark.parametrize("fractions", [(2, 4), (3, 2), (1, 1)])
def test_lists_and_ranking(ctl, w, h, ts, fractions):
    s = ctl.BlockSampler(w, h, ts, "variance")
    n = s.num_blocks
    assert n in (6, 35)
    fd, fw = fractions
    s.set_fractions(fd, fw)
    user = np.ones(n, f32)
    user[1] = 0.0
    user[n - 2] = 3.0
    s.set_user_weight(1 % s.blocks_x, 1 // s.blocks_x, 0.0)
    s.set_user_weight((n - 2) % s.blocks_x, (n - 2) // s.blocks_x, 3.0)
    order = np.arange(n, dtype=np.uint32)
    rendered = np.zeros(n, np.uint32)
    for done in range(13):
        want = np_list(order, n, done, fd, fw)
        got = s.blocks()
        assert np.array_equal(got, want), (done, got, want)
        counts = s.tile_samples()
        assert counts.dtype == np.uint8
        assert np.array_equal(counts, np.bincount(want, minlength=n))
        if done in (0, 9):
            assert np.array_equal(got, np.arange(n))
        if done >= 10 and fractions == (2, 4):
            assert got.size == n // 4 + (n - done % 2 + 1) // 2 < n
            assert got[n // 4] == done % 2                       # the deterministic stride rotates
            both = np.intersect1d(got[:n // 4], got[n // 4:])
            assert np.all(counts[both] == 2)
        if done >= 10 and fractions == (1, 1):
            assert np.all(counts == 2)                           # every block in both halves
        info = make_info(ctl, n, seed=done)
        s.add_pass(info)
        rendered += np.bincount(want, minlength=n).astype(np.uint32)
        wts = np_weights(info, user)
        assert np.unique(wts[user > 0]).size == int((user > 0).sum())   # distinct, as the case needs
        assert np.array_equal(s.weights().view(np.uint32), wts.view(np.uint32))
        order = np_order(wts)
        assert np.array_equal(s.passes_done(), rendered)
    assert order[0] == np.argmax(np.where(np.isnan(wts), -1, wts))
    s.start_new_rendering()
    assert np.array_equal(s.blocks(), np.arange(n))
    assert not s.passes_done().any()
    s.close()


def ranked(ctl, info, n_x):
    """The order the sampler holds after 10 passes of `info`, read through a list
    that is the whole order (frac_weighted 1) followed by every block."""
    n = info.size
    s = ctl.BlockSampler(32 * n_x, 32 * (n // n_x), 32, "variance")
    s.set_fractions(1, 1)
    for _ in range(10):
        s.add_pass(info)
    got = s.blocks()
    assert np.array_equal(got[n:], np.arange(n))
    wts = s.weights()
    s.close()
    return got[:n], wts


def test_equal_weights_rank_by_ascending_id(ctl):
    info = make_info(ctl, 6, seed=3)
    info[4] = info[1]                     # two equal weights
    order, wts = ranked(ctl, info, 3)
    assert wts[4] == wts[1]
    assert np.array_equal(order, np_order(np_weights(info, np.ones(6, f32))))
    assert list(order).index(1) + 1 == list(order).index(4)


def test_all_equal_blocks_give_nan_weights_in_id_order(ctl):
    info = make_info(ctl, 6, seed=1)
    info[:] = info[2]                     # max == min in both terms: 0 / 0
    order, wts = ranked(ctl, info, 3)
    assert np.isnan(wts).all()
    assert np.array_equal(order, np.arange(6))


def test_nan_weight_ranks_below_every_number(ctl):
    info = make_info(ctl, 6, seed=2)
    info["block_e_i"][0] = np.nan         # a pixel without a variance sample: NaN sums
    info["block_e_i2"][0] = np.nan
    order, wts = ranked(ctl, info, 3)
    assert np.isnan(wts[0]) and not np.isnan(wts[1:]).any()
    assert order[-1] == 0
    assert np.array_equal(order, np_order(np_weights(info, np.ones(6, f32))))


def test_block_without_variance_pixels(ctl):
    info = make_info(ctl, 6, seed=4)
    info["num_pixels_var"][3] = 0         # get_w1 = 0: the minimum of the first term
    info["block_var_i"][3] = 0.0
    order, wts = ranked(ctl, info, 3)
    want = np_weights(info, np.ones(6, f32))
    assert np.array_equal(wts.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(order, np_order(want))


def test_uniform_sampler(ctl):
    s = ctl.BlockSampler(96, 64, 32, "uniform")
    for _ in range(12):
        assert np.array_equal(s.blocks(), np.arange(6))
        s.add_pass()
    assert np.array_equal(s.passes_done(), np.full(6, 12))
    s.close()


def test_capacity_and_bad_arguments(ctl):
    import ctypes as C
    L = ctl.lib()
    s = ctl.BlockSampler(96, 64, 32, "variance")
    out = np.full(6, 0xAAAAAAAA, np.uint32)
    n = C.c_uint32(0)
    assert L.ctl_block_sampler_blocks(s._h, out.ctypes.data, 5, C.byref(n)) != 0
    assert n.value == 6 and np.all(out == 0xAAAAAAAA)            # reports n, writes nothing
    assert L.ctl_block_sampler_blocks(s._h, out.ctypes.data, 6, C.byref(n)) == 0
    assert np.array_equal(out, np.arange(6))
    assert L.ctl_block_sampler_blocks(s._h, out.ctypes.data, 6, None) != 0
    with pytest.raises(ctl.CTLError):
        s.set_fractions(0, 4)
    with pytest.raises(ctl.CTLError):
        s.set_fractions(2, 0)
    with pytest.raises(ctl.CTLError):
        s.set_user_weight(3, 0, 1.0)
    with pytest.raises(ctl.CTLError):
        s.set_user_weight(0, 2, 1.0)
    with pytest.raises(ctl.CTLError):
        s.add_pass(make_info(ctl, 5))                            # one record per block
    with pytest.raises(ctl.CTLError):
        s.add_pass()                                             # the variance sampler needs them
    assert L.ctl_block_sampler_tile_samples(s._h, None) != 0
    assert L.ctl_block_sampler_weights(s._h, None) != 0
    assert L.ctl_block_sampler_passes_done(None, out.ctypes.data) != 0
    s.close()
    for args in [(0, 64, 32, "variance"), (96, 0, 32, "variance"), (96, 64, 0, "variance"), (96, 64, 32, 7)]:
        with pytest.raises(ctl.CTLError):
            ctl.BlockSampler(*args)


def test_block_info_layout(ctl):
    import ctypes as C
    assert C.sizeof(ctl._abi.BlockInfo) == 20 == ctl.BLOCK_INFO_DTYPE.itemsize      # TmpBlockInfo
    for name, _ in ctl._abi.BlockInfo._fields_:
        assert getattr(ctl._abi.BlockInfo, name).offset == ctl.BLOCK_INFO_DTYPE.fields[name][1]
