"""The cases of tests/test_ba_row_parking.py on the device: the register-row flavours of the BA window kernel on more than 512
edges per range (SLOTS = 2), at most 512 (SLOTS = 1) and on the window whose solve fails and is retried, fails and has its
stale step accepted, and succeeds -- through the launch path -- and the 2-workgroup window once through the resident
service (k_ba_service); bit for bit against the blocked oracle, every trial of the trace included."""
import pytest

import test_ba_row_parking as cases

pytestmark = pytest.mark.gpu


@pytest.fixture()
def knob(mvo):
    return mvo.debug_set


def test_slots2_more_than_512_edges_per_range(mvo, O, ctx, knob):
    cases.case_slots2(mvo, O, ctx, knob)


def test_slots1_at_most_512_edges_per_range(mvo, O, ctx, knob):
    cases.case_slots1(mvo, O, ctx, knob)


def test_failed_retried_stale_and_successful_solves(mvo, O, ctx, knob):
    st = cases.case_failed_and_stale(mvo, O, ctx, knob)
    assert st["failed_solves"] > 0 and st["stale_steps"] > 0


def test_resident_service_on_the_two_workgroup_window(mvo, O, knob):
    cases.case_resident_service(mvo, O, lambda: mvo.Context(0), knob)
