"""The tail hand-over of the one-instance persistent path kernels (persistent_loop.h,
CTL_TAIL_LANES): a wave leaves its trace loop before its slowest rays end and those
lanes resume in the next iteration.  A hand-over only delays a lane's next round, so
every framebuffer and ray count here is the oracle's, bit for bit; the hand-over count
(ctl_tail_handovers) shows that the path ran."""
import numpy as np
import pytest

import deep_stack_cases as dc
from helpers import oracle_render

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

torch = pytest.importorskip("torch")

PASSES = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tracer(ctl, dev):
    t = ctl.PathTracer(0)
    yield t
    t.close()


_SCENES, _WANT = {}, {}


def generated(ctl, config, scale, w, h):
    key = (config, scale, w, h)
    if key not in _SCENES:
        s = ctl.HostScene().generate(config, scale, w, h)
        _SCENES[key] = (s, s.compile())
    return _SCENES[key][1]


def params(ctl):
    return ctl.PTParams(1, 50, 5, 1, 64, 1, 0, 0)   # the persistent schedule, any-hit shadow rays


def want_of(ctl, orc, key, d):
    """PASSES oracle passes of desc d, computed once per scene and shared read-only."""
    if key not in _WANT:
        fb, rays = oracle_render(orc, d, params(ctl), PASSES, d.camera.width, d.camera.height)
        fb.setflags(write=False)
        _WANT[key] = (fb, rays)
    return _WANT[key]


def render(ctl, tracer, d, dev, one_launch):
    """PASSES passes in one ctl_render_passes launch, or one ctl_render_pass launch each; ctl_sync raises
    on a stack overflow.  Returns (framebuffer, rays, (lanes handed over, trace loops left early))."""
    tracer.upload_scene(d)
    tracer.params = params(ctl)
    fb = torch.zeros((d.camera.width * d.camera.height, 7), dtype=torch.float32, device=dev)
    tracer.reset_rays()
    if one_launch:
        tracer.render_passes(fb.data_ptr(), 0, PASSES)
    else:
        for p in range(PASSES):
            tracer.do_pass(fb.data_ptr(), p)
    tracer.sync()
    return fb.cpu().numpy(), tracer.rays_traced(), tracer.tail_handovers()


def assert_oracle(got, grays, want, wrays):
    assert grays == wrays
    bad = np.nonzero((want.view(np.uint32) != got.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], want[bad[:3]], got[bad[:3]])


@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "launch_per_pass"])
@pytest.mark.parametrize("config,scale", [(2, 0.25), (3, 0.004), (5, 0.003)])
def test_parity_scenes(ctl, orc, tracer, dev, config, scale, one_launch):
    """The one-instance scenes of test_gpu_parity.py (lean shading; C5: the full shading kernel)."""
    d = generated(ctl, config, scale, 96, 64)
    want, wrays = want_of(ctl, orc, (config, scale, 96, 64), d)
    assert want[:, 6].min() == PASSES
    got, grays, (lanes, breaks) = render(ctl, tracer, d, dev, one_launch)
    print(f"C{config}: {grays} rays, {lanes} lanes handed over at {breaks} breaks")
    assert_oracle(got, grays, want, wrays)
    assert lanes > 0 and 0 < breaks <= lanes


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (13, 5)])
def test_small_images(ctl, orc, tracer, dev, w, h):
    """One lane; exactly one wave; 65 paths, i.e. a second wave holding a single lane: the shapes at which
    a break rule without its progress condition would cut a wave after every ray, or never end."""
    d = generated(ctl, 2, 0.25, w, h)
    want, wrays = want_of(ctl, orc, (2, 0.25, w, h), d)
    assert wrays >= PASSES * w * h
    for one_launch in (True, False):
        got, grays, _ = render(ctl, tracer, d, dev, one_launch)
        assert_oracle(got, grays, want, wrays)


def sparse_comb(ctl, n):
    """comb(n, render=True) seen through a camera three times as wide: the middle pixels' rays walk the
    whole chain (stack depth n), the others miss the comb and end at once, so waves hand over lanes whose
    stack top lies in LDS (n = 16), in the private array (17) and at the 128-entry limit."""
    def make():
        case = dc.comb(ctl, n, render=True)
        nt = float(case.n_tris)
        dist = 6.0 * nt
        fov = float(np.degrees(2.0 * np.arctan(1.5 * nt / dist)))
        cam = ((-dist, nt / 2.0, 0.0), (0.0, nt / 2.0, 0.0), (0.0, 0.0, 1.0), fov, 24, 24)
        hs, dcam = dc._host_scene(ctl, *dc.comb_triangles(2), (), cam)
        d = type(case.desc).from_buffer_copy(case.desc)
        d.camera = dcam.camera
        return case, d, (hs, dcam)
    return dc._cached(("tail_sparse_comb", n), make)


@pytest.mark.parametrize("n", [16, 17, 128])
def test_deep_stack_hand_over(ctl, orc, tracer, dev, n):
    case, d, _ = sparse_comb(ctl, n)
    orc.oracle_depth_peak_reset()
    want, wrays = want_of(ctl, orc, ("comb", n), d)
    if ("comb", n, "peak") not in _WANT:
        _WANT[("comb", n, "peak")] = orc.oracle_depth_peak()
    assert _WANT[("comb", n, "peak")] == case.reach("wide") == n      # the paths' own rays go that deep
    hit = want[:, :3].max(axis=1) > 0.0
    assert 0 < hit.sum() < hit.size                                   # some pixels see the comb, others miss
    got, grays, (lanes, breaks) = render(ctl, tracer, d, dev, True)   # sync inside: no overflow
    print(f"comb {n}: {grays} rays, {lanes} lanes handed over at {breaks} breaks")
    assert_oracle(got, grays, want, wrays)
    assert lanes > 0 and tracer.stack_bound() == case.bound


def test_two_level_scene_is_not_handed_over(ctl, orc, tracer, dev):
    """A scene with instances runs the two-level kernels, which the hand-over leaves as they were."""
    case = dc.two_level_render(ctl, 39, 87)
    want, wrays = want_of(ctl, orc, ("two_level", 39, 87), case.desc)
    got, grays, counts = render(ctl, tracer, case.desc, dev, True)
    assert_oracle(got, grays, want, wrays)
    assert counts == (0, 0)
