"""The kernel flavours that keep an edge's Jacobian rows in registers (SLOTS = 1 / 2 of ba_window, csrc/ba_kernels.hip) on the
smallest windows that take each of their paths, run on the emulated kernel (tests/sim) and held BIT FOR BIT to the blocked
oracle with the solve's plan and to the trace (lambda, chi2, rho, accepted per trial).

The cases were drawn up for parking those rows in the idle U area across the reduced solve -- every place where the rows
are handed from one phase of an LM trial to the next: more than 512 edges per range, at most 512, a failed solve that is
retried / whose stale step is accepted / a successful one, the reduced system aliased into the U area, a U area too small
to park in, the resident service.  The parking lost its A/B (profiles/r07_ab_runs.txt) and is not in the kernel; the cases
stay: they are as much the paths on which ba_window takes the thread index afresh at the head of every phase
(BA_PHASE_HEAD), and the smallest windows on which anything that touches the rows between the phases can go wrong."""
import ctypes as C

import numpy as np
import pytest

from test_ba_kernel_sim import simctx, simlib  # noqa: F401  (fixtures)
from test_gpu_ba import _args, _bitwise

SMALL = (5, 300, 7)          # 5 poses / 300 landmarks / ~1400 edges
STALE = (5, 300, 252)        # the same shape; on 2 workgroups its solve meets all three outcomes of the reduced solve
TINY = (3, 40, 5)            # 3 poses / 40 landmarks: one workgroup


def edges_per_range(pb, plan):
    """Largest number of edges of a landmark range of the plan."""
    cuts = np.asarray(plan["wg_pt_start"])
    owner = np.searchsorted(cuts, np.asarray(pb["edge_point"]), side="right") - 1
    return int(np.bincount(owner, minlength=len(cuts) - 1).max())


def solve_with_rows_in_registers(mvo, O, ctx, set_knob, pb, wgs, trace_out=None, **kw):
    """_bitwise on `wgs` workgroups with the rows of the first 512 edges of a range forced into registers (the planner
    would keep the rows of so small a window in LDS: SLOTS = 0)."""
    set_knob("ba_edge_rows", 1)
    set_knob("ba_wgs", wgs)
    try:
        return _bitwise(mvo, O, ctx, pb, trace_out=trace_out, fix_points=False, **kw)
    finally:
        set_knob("ba_edge_rows", -1)
        set_knob("ba_wgs", 0)


def case_slots2(mvo, O, ctx, set_knob):
    pb = mvo.synth.ba_problem(*SMALL)
    st, plan = solve_with_rows_in_registers(mvo, O, ctx, set_knob, pb, 2)
    assert plan["wgs"] == 2 and 512 < edges_per_range(pb, plan) <= 1024, plan   # the second edge of a thread: rows in LDS
    return st


def case_slots1(mvo, O, ctx, set_knob):
    pb = mvo.synth.ba_problem(*SMALL)
    st, plan = solve_with_rows_in_registers(mvo, O, ctx, set_knob, pb, 4)
    assert plan["wgs"] == 4 and edges_per_range(pb, plan) <= 512, plan
    return st


def case_failed_and_stale(mvo, O, ctx, set_knob):
    """A failed solve that is retried, a failed solve whose stale step is accepted and successful solves in one window.
    (The stale-step window of tests/test_gpu_ba.py -- 2000 landmarks -- cannot be cut into 2 workgroups: a range holds at
    most 1024 edges.  This one has the same three outcomes on 2 workgroups; found by running seeds through the emulator.)"""
    pb = mvo.synth.ba_problem(*STALE)
    out = []
    st, plan = solve_with_rows_in_registers(mvo, O, ctx, set_knob, pb, 2, trace_out=out)
    tr = out[0]
    failed = tr[:, 1] > 1e300
    assert plan["wgs"] == 2 and edges_per_range(pb, plan) > 512
    assert st["failed_solves"] > 0 and st["stale_steps"] > 0, st
    assert st["failed_solves"] == failed.sum() and st["stale_steps"] == (failed & (tr[:, 3] > 0)).sum(), st
    assert (failed & (tr[:, 3] == 0)).sum() > 0 and (~failed).sum() > 0   # ... retried, and solved
    return st


def case_alias_sl(mvo, O, ctx, set_knob):
    """The same plan with the reduced system in the U area (alias_sl = 1) and with LDS of its own (ba_alias_sl = 0): identical
    results, both the oracle's.  (The caller sets MVO_BA_NSPLIT=1: one column piece per chunk is what lets the planner alias;
    on 4 workgroups the one chunk of a range -- 75 landmarks, 228 columns -- fits the LDS, on 2 it would not.)"""
    pb = mvo.synth.ba_problem(*SMALL)
    res = []
    try:
        for alias in (1, 0):
            set_knob("ba_alias_sl", alias)
            out = []
            st, plan = solve_with_rows_in_registers(mvo, O, ctx, set_knob, pb, 4, trace_out=out, max_iterations=12)
            assert plan["wgs"] == 4 and plan["nsplit"] == 1, plan
            set_knob("ba_edge_rows", 1)
            set_knob("ba_wgs", 4)
            P, X, st2 = ctx.bundle_adjustment(*_args(pb), fix_points=False, max_iterations=12)
            assert st2 == st
            res.append((P, X, st, out[0]))
    finally:
        set_knob("ba_alias_sl", 1)
        set_knob("ba_edge_rows", -1)
        set_knob("ba_wgs", 0)
    (P1, X1, st1, tr1), (P0, X0, st0, tr0) = res
    assert np.array_equal(P1, P0) and np.array_equal(X1, X0) and st1 == st0 and tr1.tobytes() == tr0.tobytes()


def case_small_u_area(mvo, O, ctx, set_knob):
    """3 poses / 40 landmarks on one workgroup with its rows in registers: 30 MFMA steps in two pieces = 120 columns of
    33 doubles = 3960 doubles of U area, fewer than 12 per thread."""
    pb = mvo.synth.ba_problem(*TINY)
    st, plan = solve_with_rows_in_registers(mvo, O, ctx, set_knob, pb, 1)
    assert plan["wgs"] == 1 and edges_per_range(pb, plan) <= 512


def case_resident_service(mvo, O, make_ctx, set_knob):
    """The 2-workgroup window through k_ba_service (throughput mode, the grid forced up): the oracle's bits, and the same
    as on the launch path."""
    pb = mvo.synth.ba_problem(*SMALL)
    lat, c = make_ctx(), make_ctx()
    try:
        st_l, plan_l = solve_with_rows_in_registers(mvo, O, lat, set_knob, pb, 2, max_iterations=12)
        c.ba_set_mode("throughput")
        set_knob("ba_service", 2)          # (the default policy brings the grid up under load only)
        c.ba_launch_stats(reset=True)
        st, plan = solve_with_rows_in_registers(mvo, O, c, set_knob, pb, 2, max_iterations=12)
        assert c.ba_launch_stats()["resident_windows"] >= 1, c.ba_launch_stats()
        assert plan["wgs"] == 2 and st == st_l
    finally:
        set_knob("ba_service", 1)
        c.close()
        lat.close()


@pytest.fixture()
def sim_knob(simlib):
    def set_knob(key, value):
        assert simlib.mvo_debug_set(key.encode(), value) == 0, key
    return set_knob


def test_slots2_more_than_512_edges_per_range(mvo, O, simctx, sim_knob):
    case_slots2(mvo, O, simctx, sim_knob)


def test_slots1_at_most_512_edges_per_range(mvo, O, simctx, sim_knob):
    case_slots1(mvo, O, simctx, sim_knob)


def test_failed_retried_stale_and_successful_solves(mvo, O, simctx, sim_knob):
    case_failed_and_stale(mvo, O, simctx, sim_knob)


def test_reduced_system_aliased_into_the_u_area(mvo, O, simctx, sim_knob, monkeypatch):
    monkeypatch.setenv("MVO_BA_NSPLIT", "1")
    case_alias_sl(mvo, O, simctx, sim_knob)


def test_small_u_area(mvo, O, simctx, sim_knob):
    case_small_u_area(mvo, O, simctx, sim_knob)


def test_resident_service_on_the_two_workgroup_window(mvo, O, simlib, sim_knob):
    class Ctx(mvo.Context):  # (as in test_ba_kernel_sim.py: the C-ABI mirror bound to the emulated build)
        def __init__(self):
            self.lib = simlib
            h = C.c_void_p()
            assert simlib.mvo_create(C.byref(h), 0) == 0
            self.h, self.device, self.params = h, 0, {}

    case_resident_service(mvo, O, Ctx, sim_knob)
