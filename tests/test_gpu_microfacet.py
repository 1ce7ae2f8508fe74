"""The rough dielectric and the rough conductor on the GPU: the HIP batch entry ctl_bsdf_eval on the
query sets of tests/microfacet_cases.py.  Every set is asserted twice: bit-equal to the host entry
ctl_host_bsdf_eval (the rough-dielectric GPU / host comparison), and against the float64 reference
of tests/microfacet_ref.py on the GPU's own results (the checks take an `evaluate` callable and
never see the host entry's).  One Tracer and one upload for the module.

The device transcendentals go through the device's fp64 library and the host's through libm; the
project assumes they round to the same fp32.  A bit difference is reported with its query."""
import numpy as np
import pytest
import torch

import microfacet_cases as MC
from bsdf_cases import same_bits


@pytest.fixture(scope="module")
def gpu(ctl):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    t = ctl.Tracer(0)
    t.upload_scene(MC.scene()[1])
    log = []

    def evaluate(q):
        q = np.ascontiguousarray(q, dtype=ctl.BSDF_QUERY_DTYPE)
        dq = torch.from_numpy(np.frombuffer(q.tobytes(), np.uint8).copy()).to(dev)
        dr = torch.zeros(len(q) * ctl.BSDF_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        t.bsdf_eval(len(q), dq.data_ptr(), dr.data_ptr())
        torch.cuda.synchronize()
        r = np.frombuffer(dr.cpu().numpy().tobytes(), dtype=ctl.BSDF_RESULT_DTYPE)
        log.append((q, r))
        return r

    evaluate.log = log
    yield evaluate
    t.close()


def _host_twin(evaluate):
    """Every batch the checks sent to the GPU since the last call, against the host entry, bit for bit."""
    n = 0
    for q, got in evaluate.log:
        want = MC.host_evaluate(q)
        bad = same_bits(got, want)
        assert bad.size == 0, (f"{len(bad)} of {len(q)} results differ between ctl_bsdf_eval and ctl_host_bsdf_eval; first:",
                               q[bad[0]], got[bad[0]], want[bad[0]])
        n += len(q)
    del evaluate.log[:]
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("mi", range(MC.N_MAT))
def test_f_and_pdf_on_the_gpu(gpu, mi):
    MC.check_closed_forms(gpu, mi)
    assert _host_twin(gpu) >= 4 * MC.N_PAIRS


@pytest.mark.gpu
@pytest.mark.parametrize("mi", range(MC.N_MAT))
def test_sampled_density_on_the_gpu(gpu, mi):
    cases = [c for c in MC.density_cases() if c[0] == mi]
    for c in cases:
        MC.check_density(gpu, *c)
    assert _host_twin(gpu) >= len(cases) * 1000


@pytest.mark.gpu
@pytest.mark.parametrize("mi", range(MC.N_MAT))
def test_sample_agrees_with_f_and_pdf_on_the_gpu(gpu, mi):
    MC.check_sample_identities(gpu, mi)
    assert _host_twin(gpu) >= MC.N_IDENT


@pytest.mark.gpu
def test_edge_inputs_on_the_gpu(gpu):
    MC.check_edges(gpu)
    MC.check_two_sided_mirror(gpu)
    assert _host_twin(gpu) >= len(MC.edge_queries())


@pytest.mark.gpu
def test_the_two_deviations_on_the_gpu(gpu):
    """The quantised two-lobe choice and the transmission pdf without its side check
    (tests/test_microfacet_host.py, (d)), on one rough dielectric."""
    MC.check_lobe_share_is_a_step(gpu, 0, 0.9)
    MC.check_pdf_without_side_check(gpu, 0, -0.8)
    _host_twin(gpu)
