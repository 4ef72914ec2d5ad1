"""The small f64 linear algebra under every geometric solver (csrc/pnp_wave.h, em_wave.h, h_wave.h) against mpmath at
60 digits, on the HOST build of tests/probe/wave_probe.hip (explicit lane loops, as tests/sim/pnp_wave_sim.cpp).
tests/test_gpu_wave_linalg.py runs the same tables through the device build.  Case tables, assertions and the
derivation of every bound live in tests/wave_linalg_cases.py; the reference in tests/wave_linalg_reference.py shares
nothing with oracle/linalg_oracle.h, which is the library's own algorithm restated.

Figures measured on this build (what each check returns, `pytest -s` prints them), next to their bounds:
  Jacobi family, bound 64 N eps = 4.3e-14 (N = 3) .. 1.7e-13 (N = 12):
    svd3 / svd_small<3,3> with ls   reconstruction 4.2e-16, orthogonality 1.5e-15, sigma 1.7e-16
    svd_small<4,4>                  reconstruction 6.6e-16, orthogonality 1.1e-15, sigma 5.8e-16
    jacobi_rr<12,12,192> and <..64> reconstruction 9.8e-16, orthogonality 2.8e-15, sigma 8.3e-16 (identical figures)
    jacobi_rr<6,6> <6,9> <10,10>    reconstruction 9.3e-16, orthogonality 2.7e-15, sigma 9.7e-16
    h_eig8                          reconstruction 2.0e-15, orthogonality 2.0e-15, eigenvalues 7.2e-16
    eigenspaces (projectors)        at most 0.008 of 64 N eps ||A|| / gap
  solves: at most 0.0074 of 64 N eps kappa |x|; nearest_rotation_uvt 8.7e-16 (orthogonality), 7.7e-16 (polar factor)
  decompose_essential, bound 64 * 3 eps = 4.3e-14: 1.8e-15
  rodrigues_fwd, bound 16 eps max(1, theta): R 0.04 of it, dR/dr 0.036 of it (dR/dr was off by 3.8e-9 at theta = 1e-8
    and 2e-13 at 1e-4 before (1 - cos theta) / theta took the half-angle form)
  rodrigues_inv: 0 below sin(theta) = 1e-5 (off by theta itself, 7.9e-6 on this table), 3.9e-9 at pi - 1e-8, normal
    branch and round trip 0.0042 of their bound
  real_roots_deg10: every root within 0.33 of 4 ulp max(1, kappa) up to 6 decades; 2 of 60 roots lost at 8 decades,
    21 of 60 at 12, 8 of 10 on the twelve-decade polynomial TWELVE_DECADES; five-point polynomials span 3.0 decades
The sweep count is not reported: jacobi_rr and svd_small keep it in a local, and the probe does not change them."""
import pytest

import wave_linalg_cases as W


@pytest.fixture(scope="module")
def P():
    return W.load_probe("host")


@pytest.fixture(scope="module")
def S():
    from conftest import graft
    return graft.load_package().synth


def _report(what, figures):
    print("\n%s: %s" % (what, figures))


@pytest.mark.parametrize("entry", sorted(W.ROW_ENTRIES))
def test_jacobi_rows_against_mpmath(P, entry):
    """svd_small and jacobi_rr, every instantiation the product uses: reconstruction, orthogonality of the rotations
    and of the rotated rows, singular values, descending order with ties in input order, eigenspaces of symmetric
    inputs as subspaces."""
    _report(entry, W.check_rows(P, entry))


def test_svd3_against_mpmath(P):
    _report("svd3", W.check_svd3(P))


def test_h_eig8_against_mpmath(P):
    _report("h_eig8", W.check_eig8(P))


@pytest.mark.parametrize("nc", [3, 4, 5])
def test_svd_solve_6xn_against_mpmath(P, nc):
    _report("svd_solve_small<6,%d,1>" % nc, W.check_solve6(P, nc))


def test_svd_solve_3x3_against_mpmath(P):
    _report("svd_solve_small<3,3,3>", W.check_solve3(P))


def test_qr_solve_6x4_against_mpmath(P):
    _report("qr_solve_6x4", W.check_qr(P))


def test_nearest_rotation_against_mpmath(P):
    _report("nearest_rotation_uvt", W.check_nearest_rot(P))


def test_rodrigues_fwd_against_mpmath(P):
    _report("rodrigues_fwd", W.check_rodrigues_fwd(P))


def test_rodrigues_inv_branches_and_round_trip(P):
    _report("rodrigues_inv", W.check_rodrigues_inv(P))


def test_decompose_essential_against_mpmath(P):
    _report("decompose_essential", W.check_decompose_essential(P))


@pytest.mark.parametrize("group", W.ROOT_GROUPS)
def test_real_roots_against_mpmath(P, group):
    _report("real_roots_deg10 " + group, W.check_roots_table(P, group))


def test_real_roots_span_limit_is_pinned(P):
    _report("real_roots_deg10 span", W.check_roots_span_limit(P))


def test_real_roots_multiple_roots_are_pinned(P):
    _report("real_roots_deg10 multiple roots", W.check_roots_double(P))


def test_svd3_overflow_scales_are_pinned(P):
    _report("svd3 scales", W.check_scales(P))


def test_five_point_polynomials_stay_inside_the_span(P, S):
    _report("five-point polynomials", W.check_five_point_span(P, S))


def test_probe_refuses_bad_arguments(P):
    W.check_bad_arguments(P)
