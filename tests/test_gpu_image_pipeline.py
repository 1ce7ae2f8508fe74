"""GPU image pipeline (ctl_image_pipeline, ctl_image_luminance) against the numpy
restatement in image_pipeline_ref.py, on synthetic framebuffers and variance
records.  Every comparison with the restatement is on bytes."""
import numpy as np
import pytest

import image_pipeline_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

f32 = np.float32
BOX, GAUSSIAN, MITCHELL, LANCZOS, TRIANGLE, NLM = 1, 2, 3, 4, 5, 16
NLM_DIRECT = 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pt(ctl, dev):
    t = ctl.PathTracer(0)
    yield t
    t.close()


def run(pt, dev, fb, w, h, filt=None, tonemap=None, var=None, splat=0.0, num_passes=0, filtered=True):
    """ctl_image_pipeline on host arrays -> (rgba uint32, filtered RGBE uint32 or None)"""
    d_fb = torch.from_numpy(np.ascontiguousarray(fb, f32)).to(dev)
    d_var = torch.from_numpy(np.ascontiguousarray(var, f32)).to(dev) if var is not None else None
    d_out = torch.full((w * h,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    d_flt = torch.full((w * h,), 0x5a5a5a5a, dtype=torch.int32, device=dev) if filtered else None
    pt.image_pipeline(d_fb.data_ptr(), w, h, d_out.data_ptr(), filter=filt, tonemap=tonemap,
                      var_ptr=d_var.data_ptr() if d_var is not None else None,
                      filtered_ptr=d_flt.data_ptr() if d_flt is not None else None, splat_scale=splat,
                      num_passes=num_passes)
    torch.cuda.synchronize()
    return (d_out.cpu().numpy().view(np.uint32), d_flt.cpu().numpy().view(np.uint32) if filtered else None)


def random_fb(w, h, seed, scale=0.9):
    """PixelData records: weighted sums, a splat term, some pixels without samples"""
    rng = np.random.default_rng(seed)
    n = w * h
    fb = np.zeros((n, 7), f32)
    fb[:, 6] = rng.integers(0, 5, n).astype(f32)
    fb[:, 0:3] = rng.random((n, 3), dtype=f32) * f32(scale) * np.maximum(fb[:, 6:7], 1)
    fb[:, 3:6] = rng.random((n, 3), dtype=f32) * f32(0.1)
    return fb


def hdr_fb(w, h, seed):
    """colours spanning 1e-3 .. 1e3"""
    rng = np.random.default_rng(seed)
    n = w * h
    fb = np.zeros((n, 7), f32)
    fb[:, 6] = 4
    lum = 10.0 ** rng.uniform(-3, 3, (n, 1))
    fb[:, 0:3] = (lum * rng.uniform(0.3, 1.0, (n, 3)) * 4).astype(f32)
    return fb


# ---- 1. neither filter nor process -----------------------------------------

def test_no_filter_no_process_is_image_resolve(pt, dev):
    w, h = 37, 21
    fb = random_fb(w, h, 1)
    d_fb = torch.from_numpy(fb).to(dev)
    want = torch.zeros(w * h, dtype=torch.int32, device=dev)
    pt.image_resolve(d_fb.data_ptr(), w, h, want.data_ptr(), splat_scale=0.25)
    got, flt = run(pt, dev, fb, w, h, splat=0.25)
    assert np.array_equal(got, want.cpu().numpy().view(np.uint32))
    assert np.array_equal(got, ref.resolve(fb, 0.25))
    assert (flt == 0x5a5a5a5a).all()          # this branch has no filtered stage


# ---- 2. canonical filters ---------------------------------------------------

CANONICAL = [(BOX, {}), (GAUSSIAN, {}), (GAUSSIAN, dict(a=2.0)), (MITCHELL, {}), (LANCZOS, {}), (TRIANGLE, {})]


@pytest.mark.parametrize("widths", [None, (1.5, 2.25)])
@pytest.mark.parametrize("ftype,params", CANONICAL)
def test_canonical_filters_match_restatement(ctl, pt, dev, ftype, params, widths):
    w, h = 37, 21
    fb = random_fb(w, h, 2)
    kw = dict(params)
    if widths:
        kw.update(x_width=widths[0], y_width=widths[1])
    f = ctl.image_filter(ftype, **kw)
    rgba, flt = run(pt, dev, fb, w, h, filt=f, splat=0.25)
    want = ref.canonical_filter(fb, w, h, 0.25, f)
    assert np.array_equal(flt, want)
    assert np.array_equal(rgba, ref.finish(want, w, h, None))
    if not (ftype == GAUSSIAN and not params):   # the reference's default alpha (-2): every weight 0, 0 / 0
        assert (want != ref.rgbe_encode(ref.pixel_to_spectrum(fb, 0.25))).sum() > w * h // 2
    # the context's own filtered scratch gives the same picture
    rgba2, _ = run(pt, dev, fb, w, h, filt=f, splat=0.25, filtered=False)
    assert np.array_equal(rgba2, rgba)


def test_box_of_half_a_pixel_is_the_pixel(ctl, pt, dev):
    w, h = 37, 21
    fb = random_fb(w, h, 3)
    _, flt = run(pt, dev, fb, w, h, filt=ctl.image_filter(BOX, 0.5, 0.5), splat=0.25)
    assert np.array_equal(flt, ref.rgbe_encode(ref.pixel_to_spectrum(fb, 0.25)))


# ---- 3. non-local means -----------------------------------------------------

def nlm_inputs(w, h, seed):
    """A smooth ramp with one hard edge plus noise; variance records built directly: a
    zero-variance corner, a few records without variance samples (NaN variance), one
    variance above the half range (infinity)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    base = 0.2 + 0.6 * xs / w + np.where(xs > 0.6 * w, 0.8, 0.0)
    col = base[..., None] * np.array([1.0, 0.8, 0.6]) + rng.normal(0, 0.05, (h, w, 3))
    n = w * h
    fb = np.zeros((n, 7), f32)
    fb[:, 6] = 8
    fb[:, 0:3] = (np.clip(col, 0, None).reshape(n, 3) * 8).astype(f32)
    fb[:, 3:6] = (rng.random((n, 3)) * 0.01).astype(f32)
    var = np.zeros((n, 11), f32)
    N = 8
    mean = (base.reshape(n) * 0.8).astype(f32)
    v = (0.5 * (1 + 0.4 * rng.random(n))).astype(f32)
    var[:, 8] = mean * N
    var[:, 9] = (v + mean * mean) * N
    nsv = np.full(n, N, np.int32)
    zero = ((xs < max(w // 4, 2)) & (ys < max(h // 3, 2))).reshape(n)
    var[zero, 8], var[zero, 9] = 4.0, 2.0                  # mean 0.5 exactly: variance 0
    special = rng.choice(np.flatnonzero(~zero), 2 + n // 300, replace=False)
    nsv[special[1:]] = 0                                   # no variance samples: NaN
    var[special[0], 8], var[special[0], 9] = 0.0, 8.0e5    # variance 1e5 > 65504: half infinity
    var[:, 10] = nsv.view(f32)
    return fb, var


_WEIGHTS = {}


def ref_weights(key, fb, var, w, h, splat, k=0.45, s2=0.005):
    if key not in _WEIGHTS:
        _WEIGHTS[key] = ref.nlm_weights(fb, var, w, h, splat, k, s2)
    return _WEIGHTS[key]


@pytest.mark.parametrize("w,h", [(40, 24), (16, 16), (5, 4), (33, 17)])
def test_nlm_matches_restatement_both_variants(ctl, pt, dev, w, h):
    fb, var = nlm_inputs(w, h, 11)
    wts = ref_weights(("A", w, h), fb, var, w, h, 0.25)
    want, C_p = ref.nlm_apply(fb, wts, w, h, 0.25)
    if w * h >= 256:
        ref.nlm_check_non_vacuous(fb, wts, want, C_p, w, h, 0.25)
    got = {}
    for flags in (0, NLM_DIRECT):
        for per in (1, 25):          # fused, and through the weight buffer
            f = ctl.image_filter(NLM, update_periodicity=per, flags=flags)
            rgba, flt = run(pt, dev, fb, w, h, filt=f, var=var, splat=0.25, num_passes=0)
            assert np.array_equal(flt, want), (flags, per, int((flt != want).sum()))
            assert np.array_equal(rgba, ref.finish(want, w, h, None))
            got[(flags, per)] = flt
    assert np.array_equal(got[(0, 1)], got[(NLM_DIRECT, 1)])


# ---- 4. weight reuse --------------------------------------------------------

def test_nlm_weight_reuse_rule(ctl, dev):
    w, h = 40, 24
    A, var = nlm_inputs(w, h, 11)
    B, _ = nlm_inputs(w, h, 12)
    Cc, _ = nlm_inputs(w, h, 13)
    wA = ref_weights(("A", w, h), A, var, w, h, 0.25)
    wB = ref_weights(("B", w, h), B, var, w, h, 0.25)
    wC = ref_weights(("C", w, h), Cc, var, w, h, 0.25)
    ap = lambda fb, wt: ref.nlm_apply(fb, wt, w, h, 0.25)[0]
    assert not np.array_equal(ap(B, wA), ap(B, wB))      # kept and fresh weights are told apart
    assert not np.array_equal(ap(Cc, wB), ap(Cc, wC))
    t = ctl.PathTracer(0)                                # its own context: a fresh filter state
    try:
        f = ctl.image_filter(NLM, update_periodicity=25)
        call = lambda fb, p, ww=w, hh=h, v=var, ff=f: run(t, dev, fb, ww, hh, filt=ff, var=v, splat=0.25, num_passes=p)[1]
        assert np.array_equal(call(A, 1), ap(A, wA))     # first call computes
        assert np.array_equal(call(B, 2), ap(B, wA))     # pass-1 weights on the current image
        assert np.array_equal(call(Cc, 3), ap(Cc, wA))
        assert np.array_equal(call(B, 7), ap(B, wB))     # a jump recomputes
        assert np.array_equal(call(Cc, 8), ap(Cc, wB))
        assert np.array_equal(call(A, 24), ap(A, wA))    # jump
        assert np.array_equal(call(B, 25), ap(B, wB))    # consecutive, but 25 % 25 == 0
        assert np.array_equal(call(Cc, 26), ap(Cc, wB))
        w2, h2 = 33, 17                                  # consecutive pass, another size
        D, var2 = nlm_inputs(w2, h2, 11)
        wD = ref_weights(("A", w2, h2), D, var2, w2, h2, 0.25)
        assert np.array_equal(call(D, 27, w2, h2, var2), ref.nlm_apply(D, wD, w2, h2, 0.25)[0])
        # periodicity 1: every call recomputes (and invalidates what was kept)
        f1 = ctl.image_filter(NLM, update_periodicity=1)
        assert np.array_equal(call(A, 1, ff=f1), ap(A, wA))
        assert np.array_equal(call(B, 2, ff=f1), ap(B, wB))
        assert np.array_equal(call(Cc, 3, ff=f1), ap(Cc, wC))
        assert np.array_equal(call(A, 4), ap(A, wA))     # back to 25: consecutive, but nothing valid is kept
        assert np.array_equal(call(B, 5), ap(B, wA))
    finally:
        t.close()


# ---- 5. luminance -----------------------------------------------------------

@pytest.mark.parametrize("w,h", [(37, 21), (300, 200)])
def test_luminance_fixed_order(pt, dev, w, h):
    rgbe = ref.rgbe_encode(ref.pixel_to_spectrum(hdr_fb(w, h, 5), 0.0))
    rgbe[3] = 0                                            # a black pixel: the minimum
    d = torch.from_numpy(rgbe.view(np.int32)).to(dev)
    a = pt.image_luminance(d.data_ptr(), w, h)
    b = pt.image_luminance(d.data_ptr(), w, h)
    got = np.array(list(a.avg_color) + [a.min_lum, a.max_lum, a.avg_lum, a.avg_log_lum], f32)
    again = np.array(list(b.avg_color) + [b.min_lum, b.max_lum, b.avg_lum, b.avg_log_lum], f32)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    r = ref.luminance(rgbe, w, h)
    want = np.array(list(r["avg_color"]) + [r["min_lum"], r["max_lum"], r["avg_lum"], r["avg_log_lum"]], f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    # min and max are exact
    L, Y, lg = ref.luminance_terms(rgbe)
    assert got[3] == Y.min() == 0 and got[4] == Y.max()
    # each mean within Higham's bound gamma_k sum|term| / n of the fp64 mean of the fp32 terms; k = the
    # longest chain of additions of the documented order, + 2 for the division (or reciprocal and product)
    n = w * h
    k = ref.ordered_sum(Y)[1] + 2
    u = 2.0 ** -24
    gamma = k * u / (1 - k * u)
    for val, terms in [(got[0], L[:, 0]), (got[1], L[:, 1]), (got[2], L[:, 2]), (got[5], Y)]:
        t64 = terms.astype(np.float64)
        assert abs(float(val) - t64.sum() / n) <= gamma * np.abs(t64).sum() / n
    t64 = lg.astype(np.float64)
    m, dm = t64.sum() / n, gamma * np.abs(t64).sum() / n
    assert abs(float(got[6]) - np.exp(m)) <= np.exp(m) * (np.expm1(dm) + u * np.exp(dm))


# ---- 6. tone map ------------------------------------------------------------

@pytest.mark.parametrize("key,burn", [(0.18, 0.0), (0.5, 0.7)])
@pytest.mark.parametrize("with_filter", [False, True])
def test_tonemap_matches_restatement(ctl, pt, dev, key, burn, with_filter):
    w, h = 37, 21
    fb = hdr_fb(w, h, 6)
    f = ctl.image_filter(GAUSSIAN, a=2.0) if with_filter else None
    rgba, flt = run(pt, dev, fb, w, h, filt=f, tonemap=ctl.Tonemap(key, burn))
    want_flt = ref.canonical_filter(fb, w, h, 0.0, f) if with_filter else ref.rgbe_encode(ref.pixel_to_spectrum(fb, 0.0))
    assert np.array_equal(flt, want_flt)
    want = ref.finish(want_flt, w, h, (key, burn))
    assert np.array_equal(rgba, want)
    by = np.stack([(want >> s) & 0xff for s in (0, 8, 16)], -1)
    assert by.min() < 32 and by.max() > 200 and len(np.unique(by)) > 100    # a picture, not a clipped one
    rgba2, _ = run(pt, dev, fb, w, h, filt=f, tonemap=ctl.Tonemap(key, burn), filtered=False)
    assert np.array_equal(rgba2, rgba)


def test_tonemap_of_a_black_image(ctl, pt, dev):
    w, h = 37, 21
    fb = np.zeros((w * h, 7), f32)
    rgba, flt = run(pt, dev, fb, w, h, tonemap=ctl.Tonemap(0.18, 0.0))
    assert (flt == 0).all()
    assert np.array_equal(rgba, ref.finish(flt, w, h, (0.18, 0.0)))
    assert (rgba == 0xff000000).all()        # 0 * inf = NaN goes through to_u8 as 0


# ---- 7. refusals ------------------------------------------------------------

def test_refusals_leave_the_context_usable(ctl, dev):
    w, h = 16, 16
    fb, var = nlm_inputs(w, h, 11)
    t = ctl.PathTracer(0)
    try:
        d_fb = torch.from_numpy(fb).to(dev)
        d_var = torch.from_numpy(var).to(dev)
        d_out = torch.zeros(w * h, dtype=torch.int32, device=dev)
        nan, inf = float("nan"), float("inf")

        def refused(match, filt=None, fbp=d_fb.data_ptr(), outp=d_out.data_ptr(), varp=d_var.data_ptr(), ww=w, hh=h):
            with pytest.raises(ctl.CTLError, match=match) as e:
                t.image_pipeline(fbp, ww, hh, outp, filter=filt, var_ptr=varp)
            assert "status 1" in str(e.value)            # CTL_ERR_INVALID

        refused("unknown filter type", ctl.image_filter(7, 1.0, 1.0))
        refused("unknown filter type", ctl.image_filter(0, 1.0, 1.0))
        for bad in (0.0, -1.0, nan, inf):
            refused("width", ctl.image_filter(BOX, bad, 1.0))
            refused("width", ctl.image_filter(TRIANGLE, 2.0, bad))
        refused("needs d_var", ctl.image_filter(NLM), varp=None)
        refused("update_periodicity", ctl.image_filter(NLM, update_periodicity=0))
        for bad in (-0.5, nan):
            refused("k and sigma2_scale", ctl.image_filter(NLM, k=bad))
            refused("k and sigma2_scale", ctl.image_filter(NLM, sigma2_scale=bad))
        refused("must not be NULL", ctl.image_filter(BOX), fbp=None)
        refused("must not be NULL", None, outp=None)
        refused("too large", ctl.image_filter(BOX), ww=70000, hh=70000)
        refused("unknown flag bit", ctl.image_filter(NLM, flags=2))
        refused("unknown flag bit", ctl.image_filter(BOX, flags=1 << 31))
        # an empty image is fine and writes nothing
        t.image_pipeline(None, 0, 16, None, filter=ctl.image_filter(BOX))
        t.image_pipeline(None, 16, 0, None)
        # and the context still works
        got = run(t, dev, fb, w, h, filt=ctl.image_filter(NLM, update_periodicity=1), var=var, splat=0.25)[1]
        wts = ref_weights(("A", w, h), fb, var, w, h, 0.25)
        assert np.array_equal(got, ref.nlm_apply(fb, wts, w, h, 0.25)[0])
    finally:
        t.close()
