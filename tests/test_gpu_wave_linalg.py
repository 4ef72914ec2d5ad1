"""tests/test_wave_linalg.py again, on the MI355X: the device build of tests/probe/wave_probe.hip (one workgroup per
case, the product's lane count, the LDS struct in __shared__ filled with 0xff) against mpmath, and against the host
build of the same source bit for bit -- the product claims bit reproducibility for everything but the trigonometric
functions, and a missing or misplaced PW_SYNC in jacobi_rr, above all in the three-wave <12, 12, 192> whose dots go
through js.dots, can only show here: the host build runs the lanes one after another.

Figures measured on the device: identical to the host build's (tests/test_wave_linalg.py lists them) wherever the
comparison is bit for bit; rodrigues_fwd and rodrigues_inv came out 0 ulp from the host build on this table (4 allowed).
Sensitivity: with the PW_SYNC after the rotation parameters of jacobi_rr removed, 25 of the 33 <12, 12, 192> cases differ
from the host build; without the one after the js.dots fill nothing changes on this hardware, because the lanes that
write js.dots and the lanes that read it all sit in wave 0."""
import pytest

import wave_linalg_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return W.load_probe("device")


@pytest.fixture(scope="module")
def H():
    return W.load_probe("host")


@pytest.fixture(scope="module")
def S():
    from conftest import graft
    return graft.load_package().synth


@pytest.fixture(scope="module")
def inputs(S):
    return W.bit_inputs(S)


def _report(what, figures):
    print("\n%s: %s" % (what, figures))


@pytest.mark.parametrize("entry", sorted(W.SIZES))
def test_device_matches_the_host_build(P, H, inputs, entry):
    """Every case of every table: bit equality, 4 ulp for the entries that call sin / cos / acos."""
    dev, host = P.run(entry, inputs[entry]), H.run(entry, inputs[entry])
    if entry in W.TRIG_ENTRIES:
        d = W.ulp_distance(dev, host)
        _report(entry, "device against host build: %.1f ulp" % d)
        assert d <= 4, "%s: device and host build differ by %.1f ulp" % (entry, d)
        return
    bad = [i for i in range(len(dev)) if dev[i].tobytes() != host[i].tobytes()]
    assert not bad, "%s: device differs from the host build on cases %r (first: %d of %d values, %.1f ulp)" % (
        entry, bad[:10], int((dev[bad[0]] != host[bad[0]]).sum()), dev.shape[1], W.ulp_distance(dev[bad[0]], host[bad[0]]))


@pytest.mark.parametrize("entry", sorted(W.ROW_ENTRIES))
def test_jacobi_rows_against_mpmath(P, entry):
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
