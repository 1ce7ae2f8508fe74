"""The rough dielectric and the rough conductor on the CPU (ctl_host_bsdf_eval) against a float64
microfacet reference written from the papers (tests/microfacet_ref.py), not against the oracle's
restatement: closed forms, the density of the samples, sample against f and pdf, the reference's two
deviations from the textbook pinned as such, and edge inputs.  The checks themselves are in
tests/microfacet_cases.py, which tests/test_gpu_microfacet.py applies to the HIP entry.  No GPU."""
import numpy as np
import pytest

import microfacet_cases as MC
import microfacet_ref as M

U = MC.U


# ---------------------------------------------------------------------------------------------
# the reference checked against itself: no product code below this line until the next rule
_DISTS = [(M.GGX, 0.3, 0.3), (M.BECKMANN, 0.25, 0.25), (M.GGX, 0.15, 0.4), (M.BECKMANN, 0.35, 0.12)]


@pytest.mark.parametrize("dist,au,av", _DISTS)
def test_reference_D_is_normalised(dist, au, av):
    """int D(m) (m.n) dm = 1.  Midpoint rule on 1024 x 1024 cells of (theta, phi); the quadrature
    error, a third of what halving the grid moves (second order), is asserted below 1e-5 and the
    integral within twice that of 1."""
    fn = lambda m: M.D(dist, au, av, m) * m[..., 2]   # noqa: E731
    a, b = M.hemisphere_integral(fn, 1024), M.hemisphere_integral(fn, 512)
    err = abs(a - b) / 3
    print(f"{dist} ({au}, {av}): integral {a:.9f}, quadrature error {err:.2g}")
    assert err < 1e-5 and abs(a - 1.0) < 2 * err + 1e-9


@pytest.mark.parametrize("wiz", [0.8, 0.3, 0.05])
@pytest.mark.parametrize("dist,au,av", _DISTS)
def test_reference_visible_normals_are_normalised(dist, au, av, wiz):
    """int D_wi(m) dm = 1 for GGX and for Beckmann with the exact Smith G1 (1024 x 1024 midpoints;
    the integrand has a kink where wi.m changes sign, the rule stays second order: error = a third
    of the halving difference, asserted below 2e-5).  Beckmann with Walter's fit: its deviation from
    1 is printed and asserted below 1 %; it is what the fit may cost the sampled-density tests."""
    wi = M.sphere_dirs(np.array(wiz), np.array(MC.AZIMUTH))
    for g in ("exact", "fit"):
        fn = lambda m: M.D_visible(dist, au, av, wi, m, beckmann=g)   # noqa: E731
        a, b = M.hemisphere_integral(fn, 1024), M.hemisphere_integral(fn, 512)
        err = abs(a - b) / 3
        print(f"{dist} ({au}, {av}) wi.z {wiz} G1 {g}: integral {a:.7f} (deviation {a - 1:+.2e}), quadrature error {err:.2g}")
        assert err < 2e-5
        if dist == M.GGX or g == "exact":
            assert abs(a - 1.0) < 2e-5 + err
        else:
            assert abs(a - 1.0) < 1e-2


def test_reference_refraction_jacobian_against_central_differences():
    """Walter eq. 17 against the area ratio of wo -> h_t(wo) by float64 central differences, step
    1e-5 (second order: its error is a third of what halving it from 2e-5 moves).  Asserted: halving
    moves the quotient by less than 1e-5 relative on every pair with |n_i wi + n_o wo| > 0.2 (the
    map's curvature grows with 1 / |.|), and the closed form agrees within what halving moved."""
    rng = np.random.RandomState(2)
    n = 2000
    wi = MC._dirs(rng, n, np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0))
    wo = MC._dirs(rng, n, -np.sign(wi[:, 2]))
    for eta in (1.5, 1.33, 1 / 1.5):
        n_i, n_o = np.where(wi[:, 2] > 0, 1.0, eta), np.where(wi[:, 2] > 0, eta, 1.0)
        v = n_i[:, None] * wi + n_o[:, None] * wo
        keep = np.sqrt((v * v).sum(axis=1)) > 0.2
        h = M.normalize(-v)
        closed = M.jacobian_refract(wi, wo, h, n_i, n_o)[keep]
        a = M.refraction_jacobian_numeric(wi, wo, n_i, n_o, 2e-5)[keep]
        b = M.refraction_jacobian_numeric(wi, wo, n_i, n_o, 1e-5)[keep]
        step_err, err = np.abs(a / b - 1).max(), np.abs(b / closed - 1).max()
        print(f"eta {eta:.4f}: closed form against central differences {err:.2g}, halving the step moves {step_err:.2g}")
        assert step_err < 1e-5 and err <= step_err + 1e-9


def test_reference_fresnel_forms_agree():
    """The complex-arithmetic conductor Fresnel with k = 0 is the dielectric one, and at normal
    incidence both are ((n - 1)^2 + k^2) / ((n + 1)^2 + k^2)."""
    c = np.linspace(0.01, 1.0, 200)
    assert np.abs(M.fresnel_conductor(c, [1.5], [0.0])[:, 0] - M.fresnel_dielectric(c, 1.5)).max() < 1e-14
    n, k = np.array(MC.GOLD_ETA), np.array(MC.GOLD_K)
    assert np.abs(M.fresnel_conductor(np.array([1.0]), n, k)[0] - ((n - 1) ** 2 + k * k) / ((n + 1) ** 2 + k * k)).max() < 1e-14


# ---------------------------------------------------------------------------------------------
# (a) closed forms
@pytest.mark.parametrize("mi", range(MC.N_MAT))
def test_f_and_pdf_against_the_float64_reference(mi):
    """See microfacet_cases.check_closed_forms and the derivation above microfacet_cases.conditioning:
    within 1e-4 relative on the pairs the reference declares well conditioned (>= 25 % per lobe)."""
    MC.check_closed_forms(MC.host_evaluate, mi)


# ---------------------------------------------------------------------------------------------
# (b) the density of the samples
@pytest.mark.parametrize("mi,z,mask", MC.density_cases())
def test_sampled_density_against_the_reference_pdf(mi, z, mask):
    """200,000 samples (fixed seed) histogrammed over 16 x 16 bins of (cos theta, phi) against the
    reference pdf times [G1(wo, H) > 0] integrated per bin: tensor Gauss-Legendre, 24 x 24 nodes per
    bin, a bin split where the GGX transmission pdf jumps (h.z = 0), and the nodes of a bin doubled
    (up to 192 x 192) until doubling moves it by less than 0.05 %; asserted: the last doubling moved no
    category by more than 0.1 %.

    Categories.  The bins expecting >= 100 samples hold >= 99 % of the reference's mass in 21 of the
    36 cases only: GGX tails are heavy, and the 15 others hold 95.5 % (GGX 0.25, eta 1 / 1.5, wi.z 0.3,
    transmission) to 98.98 %.  So the smaller bins are not dropped and not pooled into one: runs of
    neighbouring smaller bins (ring by ring of cos theta, ascending phi) are closed into a category as
    soon as they expect >= 100 (microfacet_cases._categories).  Every category expects >= 100,
    together they hold >= 99.9 % of the mass (>= 99 % is asserted, on the categories alone), and
    chi-square runs over all of them, below the p = 1e-6 quantile for their number.  The threshold
    is derived, not tuned.

    Beckmann: pdf() uses Walter's fit of G1 while the visible-normal sampling inverts the exact one,
    so reference pdf and sample density differ by the fit's error; where the bias this predicts
    (microfacet_cases.density_plan, from the reference alone) reaches half the quantile, n is lowered
    to the largest power of ten where it does not (no case needs it today).  The quantile is never
    loosened.  For the same reason the accepted share is held to the integral under the exact G1
    (microfacet_cases.check_density); the fit's integral is printed beside it."""
    MC.check_density(MC.host_evaluate, mi, z, mask)


# ---------------------------------------------------------------------------------------------
# (c) sample against f and pdf
@pytest.mark.parametrize("mi", range(MC.N_MAT))
def test_sample_agrees_with_f_and_pdf(mi):
    """See microfacet_cases.check_sample_identities (with the count of roundings)."""
    MC.check_sample_identities(MC.host_evaluate, mi)


# ---------------------------------------------------------------------------------------------
# (e) edge inputs
def test_edge_inputs_give_finite_results():
    MC.check_edges(MC.host_evaluate)


def test_two_sided_conductor_mirrors_its_sample():
    MC.check_two_sided_mirror(MC.host_evaluate)


# ---------------------------------------------------------------------------------------------
# (d) the reference's two deviations from the textbook
@pytest.mark.parametrize("mi", MC.DIELECTRICS)
@pytest.mark.parametrize("z", [0.3, -0.8])
def test_two_lobe_choice_is_quantised_and_tied_to_the_normal(mi, z):
    """roughdielectric::sample, SceneTypes/BSDF_Simple.cu:548-556 with Math/MonteCarlo.cu:16-20: see
    microfacet_cases.check_lobe_choice."""
    MC.check_lobe_choice(MC.host_evaluate, mi, z)


@pytest.mark.parametrize("mi", [0, 1, 2])
def test_two_lobe_reflection_share_is_a_step_not_F(mi):
    """Near normal incidence on eta = 1.5, F is about 0.04-0.05 for nearly every sampled normal: the
    reflection lobe is taken with probability 0.1, not F (microfacet_cases.check_lobe_share_is_a_step)."""
    MC.check_lobe_share_is_a_step(MC.host_evaluate, mi, 0.9)


@pytest.mark.parametrize("mi,z", [(0, -0.8), (0, 0.3)])
def test_pdf_of_the_transmission_lobe_has_no_side_check(mi, z):
    """roughdielectric::pdf, SceneTypes/BSDF_Simple.cu:373-435: see
    microfacet_cases.check_pdf_without_side_check."""
    MC.check_pdf_without_side_check(MC.host_evaluate, mi, z)
