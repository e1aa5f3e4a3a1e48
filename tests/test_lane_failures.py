"""Per-lane failure status and the isolation of failed lanes ("Lane status contract").

The parity tests compare the lanes the oracle leaves clean and mask the status bits out.  Here the batches are DESIGNED:
lane i is made to carry a known `JM_LANE_*` pattern, and every scenario asserts
  (a) that the oracle's status IS the designed pattern (no scenario passes vacuously),
  (b) that the status under test equals the oracle's on every lane, without a mask,
  (c) that the lanes designed clean match the oracle at the bars of `test_start_and_steps_match_oracle_fp64`
      (1e-11 after `start`, 1e-8 after steps),
and the isolation scenarios run a batch twice -- with poisoned robots and with those robots healthy (the twin) -- and ask
for bit-identical neighbours: 16 robots share a wave, the staged limb table, the `wave_any` loop exits, the attempt bound of
the persistent adaptive kernel, the sweep loops of the solvers and the compacted list of the per-stage adaptive stepper.

Every scenario exists twice: on the kernel code compiled for the host (unmarked; one robot after the other, so it pins the
logic and the designs) and on the device (`gpu`), where the cross-lane OR of the quad, the staging and the compaction live.

Poisoned inputs are data: no address and no loop bound of a kernel follows from the state (the height-map lookup clamps
its cell index as an integer, the solver and stepper loops end at their caps).

Known exception, history-driven forms (`Traits::lane_history()`, ANYmal's split constraint step): the sweep counters of
step n choose the form of step n + 2 for the whole batch, so a poisoned robot may change the form its neighbours step in.
Bit-identity is asserted over the first two steps (same form in both runs by construction) and over all steps of the single
kernel (JIMINY_AMD_QCON_SPLIT=0); beyond, the bar the project accepts between the two forms at B <= 128 applies
(`test_gpu_split_stepping_with_the_one_lane_per_robot_solve`: rel_err < 1e-8, equal `con_flags` and `status`).

FORCE_OVERFLOW is a bit of `start` / `reset_lanes` alone: the next step overwrites the status, in the oracle and in both
kernel families.  The bit is pinned as it is today."""
import dataclasses

import numpy as np
import pytest

from tests import lane_failures as lf
from tests.lane_failures import NAN, OOB, OVERFLOW, SOLVER, STEPPER

DT = {"anymal": 1e-3, "atlas": 2.5e-4}


def _host(setup, model):
    return lf.Host(setup, model)


# ------------------------------------------------------------------ 1. designed status batches
def scenario_nan_and_bounds(make, name, family, B):
    model = lf.model_of(name)
    s = lf.Setup(name, B, family=family, dt=DT[name])
    st, expect, names = lf.designed_status_batch(model, B, overflow=False)
    o, x = lf.Oracle(s, model), make(s, model)
    for e in (o, x):
        e.start(st["q"], st["v"], st["command"])
    assert np.array_equal(o.get("status"), expect), list(zip(names, o.get("status"), expect))          # (a)
    for k in range(4):
        assert any(n == f"v_nan limb {k}" for n in names) and any(n == f"above upper limb {k}" for n in names)
    assert np.array_equal(x.get("status"), o.get("status")), list(zip(names, x.get("status"), o.get("status")))   # (b)
    clean = expect == 0
    lf.assert_matches_oracle(lf.snapshot(x, s), lf.snapshot(o, s), clean, 1e-11, s, "start")            # (c)
    # a NaN acceleration (a step reads it as the first stage derivative) on a lane that started clean
    untouched = np.array([n == "clean" for n in names])
    a_lane = int(np.flatnonzero(untouched)[1])
    for e in (o, x):
        e.poke("a", 7, a_lane, np.nan)
    untouched[a_lane] = False
    nan_lanes = (expect & NAN) != 0
    nan_lanes[a_lane] = True
    for i in range(3):
        for e in (o, x):
            e.step()
        so, sx = o.get("status"), x.get("status")
        assert ((so[nan_lanes] & NAN) != 0).all(), (i, so)          # (a) the bit persists while the state is NaN
        assert (so[untouched] == 0).all(), (i, so)                  # (a)
        assert np.array_equal(sx, so), (i, list(zip(names, sx, so)))   # (b)
    lf.assert_matches_oracle(lf.snapshot(x, s), lf.snapshot(o, s), untouched, 1e-8, s, "steps")         # (c)


def scenario_bounds_under_the_constraint_model(make, name, family, B):
    """Joints at and beyond their bounds are rows of the solver there, not a failure: no bit."""
    model = lf.model_of(name)
    s = lf.Setup(name, B, family=family, contact="constraint", solver="euler_explicit", dt=5e-4)
    st, expect, names = lf.designed_status_batch(model, B, nan=False, overflow=False)
    assert (expect == OOB).sum() >= 8
    o, x = lf.Oracle(s, model), make(s, model)
    for e in (o, x):
        e.start(st["q"], st["v"], st["command"])
    # (a robot whose solve sits at the iteration cap with the tight tolerances of the parity tests carries SOLVER_FAILURE)
    assert ((o.get("status") & ~SOLVER) == 0).all(), o.get("status")
    assert np.array_equal(x.get("status"), o.get("status"))
    lf.assert_matches_oracle(lf.snapshot(x, s), lf.snapshot(o, s), slice(None), 1e-7, s, "start")   # (bar of test_gpu_constraint_model_matches_oracle)


def scenario_force_overflow(make, name, family, B):
    model = lf.model_of(name)
    s = lf.Setup(name, B, family=family, dt=DT[name])
    st, expect, names = lf.designed_status_batch(model, B, nan=False, overflow=True)
    o, x = lf.Oracle(s, model), make(s, model)
    for e in (o, x):
        e.start(st["q"], st["v"], st["command"])
    deep = int(np.flatnonzero(expect == OVERFLOW)[0])
    assert np.array_equal(o.get("status"), expect)                  # (a): raised at `start`
    assert np.array_equal(x.get("status"), o.get("status"))         # (b)
    # ... and at `reset_lanes`: two clean lanes are re-initialised at the state of the deep one
    clean = np.flatnonzero(np.array([n == "clean" for n in names]))[:2]
    mask = np.zeros(B, dtype=np.uint8)
    mask[clean] = 1
    q2, v2 = st["q"].copy(), st["v"].copy()
    q2[:, clean], v2[:, clean] = st["q"][:, [deep]], st["v"][:, [deep]]
    expect2 = expect.copy()
    expect2[clean] = OVERFLOW
    for e in (o, x):
        e.reset(mask, q2, v2)
    assert np.array_equal(o.get("status"), expect2)
    assert np.array_equal(x.get("status"), o.get("status"))
    # the next step overwrites the status: the bit is gone (today's behaviour of all three implementations)
    for e in (o, x):
        e.step()
    assert ((o.get("status") & OVERFLOW) == 0).all() and ((x.get("status") & OVERFLOW) == 0).all()
    assert np.array_equal(x.get("status"), o.get("status"))


def scenario_solver_failure(make, name, family, split, B):
    """Tolerances below round-off: the robots pressed 1 cm into the ground on all their contact points cannot meet them within
    the iteration cap (their sweeps still move the multipliers after 100 of them), the robots in free flight converge at once."""
    from jiminy_amd.synthetic import lowest_contact_height
    model = lf.model_of(name)
    s = lf.Setup(name, B, family=family, split=split, contact="constraint", solver="euler_explicit", dt=5e-4, copt=lf.UNMEETABLE)
    rng = np.random.default_rng(1)
    st = lf.healthy_states(model, B, seed=7, standing=True)
    q = np.repeat(model.neutral()[:, None], B, axis=1)
    q[0:2] = st["q"][0:2]
    q[7:] += rng.uniform(-0.02, 0.02, q[7:].shape)
    q[2] += -1e-2 - lowest_contact_height(model, q)
    v = rng.normal(0, 0.02, st["v"].shape)
    free = (np.arange(B) % 2) == 1
    q[2, free] += 1.0
    expect = np.where(free, 0, SOLVER).astype(np.int32)
    o, x = lf.Oracle(s, model), make(s, model)
    for e in (o, x):
        e.start(q, v, st["command"])
    for i in range(3):
        assert np.array_equal(o.get("status"), expect), (i, o.get("status"))       # (a)
        assert np.array_equal(x.get("status"), o.get("status")), (i, x.get("status"))   # (b)
        lf.assert_matches_oracle(lf.snapshot(x, s), lf.snapshot(o, s), free, 1e-8, s, f"evaluation {i}")   # (c)
        if i < 2:
            for e in (o, x):
                e.step()
    # the status is the one of the LAST evaluation: lifted off the ground, the robots converge and the bit clears
    mask = (~free).astype(np.uint8)
    q2 = q.copy()
    q2[2, ~free] += 1.0
    for e in (o, x):
        e.reset(mask, q2, v)
    assert (o.get("status") == 0).all()
    assert np.array_equal(x.get("status"), o.get("status"))
    for e in (o, x):
        e.step()
    assert (o.get("status") == 0).all()
    assert np.array_equal(x.get("status"), o.get("status"))


ADAPTIVE_UNMEETABLE = dict(tol_rel=1e-30, tol_abs=1e-30, dt_max=1e-3, successive_iter_failed_max=5)


def scenario_stepper_failure(make, name, family, B):
    """No gravity, every robot at rest in free flight.  Two lanes out of three carry a command: their error estimate is
    far above 1e-30 at any step size, six attempts fail in a row (successiveIterFailedMax = 5) -> STEPPER_FAILURE, `t` stays.
    Every third lane has no command: its derivative is exactly zero, so is its error estimate, it steps to `t_next`.
    The base is level (identity quaternion): the orientation part of the estimate, log(R1^T R2) of two equal rotations, is an
    exact zero only when the products have exact operands -- with a general quaternion a fused multiply-add leaves 1e-17 there,
    which is a legitimate failure at 1e-30 and would make the design depend on the contraction of the build."""
    model = lf.model_of(name)
    s = lf.Setup(name, B, family=family, adaptive=ADAPTIVE_UNMEETABLE, gravity=(0.0,) * 6, dt=1e-3)
    st = lf.healthy_states(model, B)
    st["q"][2] += 1.0
    st["q"][3:7] = np.array([0.0, 0.0, 0.0, 1.0])[:, None]
    rest = (np.arange(B) % 3) == 0
    st["v"][:] = 0.0
    st["command"][:, rest] = 0.0
    expect = np.where(rest, 0, STEPPER).astype(np.int32)
    o, x = lf.Oracle(s, model), make(s, model)
    for e in (o, x):
        e.start(st["q"], st["v"], st["command"])
    for i in range(2):
        for e in (o, x):
            e.step()
        assert np.array_equal(o.get("status"), expect), (i, o.get("status"))            # (a)
        assert np.array_equal(x.get("status"), o.get("status")), (i, x.get("status"))   # (b)
        for e in (o, x):        # flagged lanes stop advancing, the others reach t_next
            t = e.lane_time()
            assert np.allclose(t[rest], (i + 1) * s.dt, rtol=0, atol=1e-12) and (t[~rest] < 1e-9).all(), (i, t)
    lf.assert_matches_oracle(lf.snapshot(x, s), lf.snapshot(o, s), rest, 1e-8, s, "steps")              # (c)
    # recovery: the command is withdrawn and the failed lanes are reset -- fresh stepper state, they advance again
    before = lf.snapshot(x, s)
    for e in (o, x):
        e.set_command(np.zeros_like(st["command"]))
        e.reset((~rest).astype(np.uint8), st["q"], st["v"])
    after = lf.snapshot(x, s)
    assert (after["status"] == 0).all()
    lf.assert_lanes_identical(after, before, rest, "lanes outside the mask")
    for e in (o, x):
        e.step()
        assert (e.get("status") == 0).all(), e.get("status")
        assert np.allclose(e.lane_time(), 3 * s.dt, rtol=0, atol=1e-12), e.lane_time()


# ------------------------------------------------------------------ 2. isolation, 3. recovery
def _poison(model, lanes):
    """One poke per poisoned robot: a NaN on a joint of limb k (k follows the position in the list, so every lane of a quad
    is the source once), then a NaN base height, an inf base velocity and a NaN trunk / limb position."""
    rows = lf.limb_rows(model)
    pokes = []
    for i, lane in enumerate(lanes):
        iq, iv = rows["limb"][i % 4]
        pokes.append(("v", iv, lane, np.nan))
    extra = [("q", 2, np.nan), ("v", 1, np.inf), ("q", (rows["trunk"] or rows["limb"])[0][0], np.nan), ("q", 0, np.inf)]
    for (field, row, value), lane in zip(extra, lanes):
        pokes.append((field, row, lane, value))
    return pokes


def scenario_isolation(make, s, lanes, at_start=False, steps=3, exact_steps=None, with_oracle=True, oracle_sample=None, recover=True):
    """`exact_steps`: steps over which the form is the same in both runs by construction (None: all of them)."""
    model = lf.model_of(s.name)
    B = s.B
    st = lf.healthy_states(model, B, standing=s.constrained)
    lanes = np.asarray(lanes)
    others = np.ones(B, dtype=bool)
    others[lanes] = False
    pokes = _poison(model, lanes)
    a, twin = make(s, model), make(s, model)
    sample = np.arange(B) if oracle_sample is None else np.asarray(oracle_sample)
    so = dataclasses.replace(s, B=len(sample))
    o = lf.Oracle(so, model) if with_oracle else None
    if at_start:
        bad = {k: v.copy() for k, v in st.items()}
        for field, row, lane, value in pokes:
            bad[field][row, lane] = value
        a.start(bad["q"], bad["v"], bad["command"])
    else:
        a.start(st["q"], st["v"], st["command"])
        for p in pokes:
            a.poke(*p)
    twin.start(st["q"], st["v"], st["command"])
    # the oracle gets the same poison (its lanes are independent by construction): the designed bit is NAN
    at = {int(lane): i for i, lane in enumerate(sample)}
    in_sample = np.array([at[int(lane)] for lane in lanes if int(lane) in at], dtype=int)
    assert o is None or len(in_sample) >= 2
    if o is not None:
        src = bad if at_start else st
        o.start(src["q"][:, sample], src["v"][:, sample], src["command"][:, sample])
        if not at_start:
            for field, row, lane, value in pokes:
                if int(lane) in at:
                    o.poke(field, row, at[int(lane)], value)
    if at_start:
        assert o is None or (o.get("status")[in_sample] & NAN).all(), o.get("status")[in_sample]
        assert (a.get("status")[lanes] & NAN).all(), a.get("status")[lanes]
        lf.assert_lanes_identical(lf.snapshot(a, s), lf.snapshot(twin, s), others, "start")
    for i in range(steps):
        for e in (a, twin, o):
            if e is not None:
                e.step()
        sa, stw = lf.snapshot(a, s), lf.snapshot(twin, s)
        assert o is None or (o.get("status")[in_sample] & NAN).all(), (i, o.get("status")[in_sample])
        assert (sa["status"][lanes] & NAN).all(), (i, sa["status"][lanes])     # the poisoned robots carry the designed bit ...
        if exact_steps is None or i < exact_steps:
            lf.assert_lanes_identical(sa, stw, others, f"step {i}")            # ... and their neighbours do not notice
        else:
            assert np.array_equal(sa["con_flags"][:, others], stw["con_flags"][:, others]), i
            assert np.array_equal(sa["status"][others], stw["status"][others]), i
            lf.assert_matches_oracle(sa, stw, others, 1e-8, s, f"step {i} (another form)")
    if o is not None:
        # (ANYmal's solves sit at the iteration cap with the tight tolerances of the parity tests: that bit is no failure of the lane)
        ok = others[sample] & ((o.get("status") & ~SOLVER) == 0)
        assert ok.sum() >= len(sample) // 2
        got = {k: v[..., sample] for k, v in lf.snapshot(a, s).items()}
        # (constraint model: the bar of the parity tests of that model after steps, test_gpu_split_stepping_...: 1e-6)
        lf.assert_matches_oracle(got, lf.snapshot(o, so), ok, 1e-6 if s.constrained else 1e-8, s, "oracle")
    if not recover:
        return
    # ---- recovery: `reset_lanes` on the poisoned lanes only
    fresh = lf.healthy_states(model, B, seed=4, standing=s.constrained)
    if s.constrained:
        fresh["q"][2] += 1.0      # (free flight: no active row, so the solver status of the fresh lanes is 0 by design)
    mask = (~others).astype(np.uint8)
    before = lf.snapshot(a, s)
    for e in (a, twin):
        e.reset(mask, fresh["q"], fresh["v"])
    sa, stw = lf.snapshot(a, s), lf.snapshot(twin, s)
    assert (sa["status"][lanes] == 0).all(), sa["status"][lanes]
    lf.assert_lanes_identical(sa, stw, lanes, "reset lanes against the twin")
    lf.assert_lanes_identical(sa, before, others, "lanes outside the mask")
    for e in (a, twin):
        e.step()
    sa, stw = lf.snapshot(a, s), lf.snapshot(twin, s)
    assert (sa["status"][lanes] == 0).all()
    if s.adaptive:
        assert np.allclose(a.lane_time()[lanes], (steps + 1) * s.dt, rtol=0, atol=1e-12), a.lane_time()[lanes]
    if exact_steps is None:
        lf.assert_lanes_identical(sa, stw, slice(None), "step after the reset")
    else:
        assert np.array_equal(sa["con_flags"], stw["con_flags"]) and np.array_equal(sa["status"], stw["status"])
        lf.assert_matches_oracle(sa, stw, slice(None), 1e-8, s, "step after the reset")


ADAPTIVE = dict(tol_rel=1e-6, tol_abs=1e-7, dt_max=1e-3, successive_iter_failed_max=1000)


def _isolation_cases(device: bool):
    """name -> (setup, poisoned lanes, keyword arguments, environment of the device run).  The forms are those of
    jm_dispatch.h; the host emulation has one code path per family and contact model (and the split step)."""
    con = dict(contact="constraint", solver="euler_explicit", dt=5e-4)
    Bq, Pq = 48, (0, 15, 16, 47)             # three waves of 16 robots
    Bl, Pl = (130, (0, 63, 64, 129)) if device else (34, (0, 15, 16, 33))     # ragged third block of the lane kernels
    Ba, Pa = (48, Pq) if device else (16, (0, 7, 8, 15))
    return {
        "QUAD_ONE_WAVE": (lf.Setup("anymal", Bq), Pq, {}, {}),
        "QUAD_GEN": (lf.Setup("anymal", Bq, ground=lf.bumpy_ground()), Pq, dict(at_start=True), {}),
        "QCON": (lf.Setup("anymal", Bq, **con), Pq, {}, {"JIMINY_AMD_QCON_SPLIT": "0"}),
        "SPLIT_STEP_LANE": (lf.Setup("anymal", Bq, split=True, **con), Pq, dict(steps=4, exact_steps=2 if device else None),
                            {"JIMINY_AMD_QCON_SPLIT": "1"}),
        "SPLIT_STEP": (lf.Setup("atlas", Ba, split=True, **dict(con, dt=2.5e-4)), Pa, {}, {"JIMINY_AMD_QCON_SPLIT": "1"}),
        # poisoned at `start`: the NaN and inf robots go through the initialisation kernels next to the healthy ones (first
        # pass, exact solve, three Gauss-Seidel passes and the closing evaluation of the split start; k_quad_con<INIT>)
        "QCON_INIT": (lf.Setup("anymal", Bq, **con), Pq, dict(at_start=True), {"JIMINY_AMD_QCON_SPLIT": "0"}),
        "SPLIT_START": (lf.Setup("atlas", Ba, split=True, **dict(con, dt=2.5e-4)), Pa, dict(at_start=True), {"JIMINY_AMD_QCON_SPLIT": "1"}),
        "SPLIT_START_LANE": (lf.Setup("anymal", Bq, split=True, **con), Pq, dict(at_start=True, steps=4, exact_steps=2 if device else None),
                             {"JIMINY_AMD_QCON_SPLIT": "1"}),
        "LANE_BATCH": (lf.Setup("anymal", Bl, family="lane"), Pl, {}, {"JM_KERNEL_VARIANT": "lane"}),
        "LANE_CON": (lf.Setup("anymal", Bl, family="lane", **con), Pl, {}, {"JM_KERNEL_VARIANT": "lane"}),
        "DOPRI": (lf.Setup("anymal", Bq, adaptive=ADAPTIVE), Pq, {}, {"JIMINY_AMD_ADAPTIVE_FORM": "0"}),
        "DOPRI_STAGES": (lf.Setup("anymal", Bq, adaptive=ADAPTIVE), Pq, {}, {"JIMINY_AMD_ADAPTIVE_FORM": "1"}),
    }


# (no host twin: the block-wave `QUAD` and `DOPRI_STAGES` are launch forms, the host has one code path for each kernel body)
HOST_ISOLATION = ("QUAD_ONE_WAVE", "QUAD_GEN", "QCON", "SPLIT_STEP_LANE", "SPLIT_STEP", "QCON_INIT", "SPLIT_START", "SPLIT_START_LANE",
                  "LANE_BATCH", "LANE_CON", "DOPRI")

# what `select_form` must answer for the launches of a device case: (facts of the launch, form) -- checked before the case runs,
# so that a change of the policy or of the block sizes cannot move a case to another form unnoticed
_Q, _L = dict(family=1), dict(family=0)
_CON = dict(constraint=1)
DEVICE_FORMS = {
    "QUAD_ONE_WAVE": [(dict(_Q, mode="start"), "QUAD_ONE_WAVE"), (dict(_Q, mode="step"), "QUAD_ONE_WAVE")],
    "QUAD_GEN": [(dict(_Q, mode="start", ground=1), "QUAD_GEN"), (dict(_Q, mode="step", ground=1), "QUAD_GEN")],
    "QCON": [(dict(_Q, **_CON, mode="step", split=0), "QCON"), (dict(_Q, **_CON, mode="reset", split=0), "QCON_INIT")],
    "QCON_INIT": [(dict(_Q, **_CON, mode="start", split=0), "QCON_INIT"), (dict(_Q, **_CON, mode="step", split=0), "QCON")],
    "SPLIT_STEP_LANE": [(dict(_Q, **_CON, mode="step"), "SPLIT_STEP_LANE"), (dict(_Q, **_CON, mode="step", cooling=1), "QCON")],
    "SPLIT_START_LANE": [(dict(_Q, **_CON, mode="start"), "SPLIT_START"), (dict(_Q, **_CON, mode="step"), "SPLIT_STEP_LANE")],
    "SPLIT_STEP": [(dict(_Q, **_CON, mode="step"), "SPLIT_STEP"), (dict(_Q, **_CON, mode="reset"), "SPLIT_START")],
    "SPLIT_START": [(dict(_Q, **_CON, mode="start"), "SPLIT_START"), (dict(_Q, **_CON, mode="step"), "SPLIT_STEP")],
    "LANE_BATCH": [(dict(_L, mode="start"), "LANE_BATCH"), (dict(_L, mode="step"), "LANE_BATCH")],
    "LANE_CON": [(dict(_L, **_CON, mode="start"), "LANE_CON"), (dict(_L, **_CON, mode="step"), "LANE_CON")],
    "DOPRI": [(dict(_Q, per_stage=0), "DOPRI")],
    "DOPRI_STAGES": [(dict(_Q, per_stage=1), "DOPRI_STAGES")],
}


def _assert_forms(gpu_device, name, B, checks):
    import torch
    n_cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    for facts, form in checks:
        assert lf.expected_form(name, n_cus=n_cus, B=B, **facts) == form, (facts, form)


# ------------------------------------------------------------------ host emulation
@pytest.mark.parametrize("name,family,B", [("anymal", "quad", 32), ("anymal", "lane", 32), ("atlas", "quad", 40)])
def test_host_nan_and_bounds_status(name, family, B):
    scenario_nan_and_bounds(_host, name, family, B)


@pytest.mark.parametrize("name,family", [("anymal", "quad"), ("anymal", "lane"), ("atlas", "quad")])
def test_host_bounds_raise_no_bit_under_the_constraint_model(name, family):
    scenario_bounds_under_the_constraint_model(_host, name, family, 32)


@pytest.mark.parametrize("family", ["quad", "lane"])
def test_host_force_overflow_at_start_and_reset_is_gone_after_a_step(family):
    scenario_force_overflow(_host, "anymal", family, 32)


@pytest.mark.parametrize("name,family,split,B", [("anymal", "quad", False, 16), ("anymal", "quad", True, 16), ("atlas", "quad", True, 8),
                                                 ("anymal", "lane", False, 16)])
def test_host_solver_failure_status(name, family, split, B):
    scenario_solver_failure(_host, name, family, split, B)


def test_host_stepper_failure_status_and_recovery():
    scenario_stepper_failure(_host, "anymal", "quad", 32)


def scenario_carry_over_and_freeze(make, family, B):
    """Later intervals of an `Engine::step` (`new_step` = 0): the status is carried over and a lane that arrives with NAN or
    STEPPER_FAILURE is frozen -- state, stepper state and `t` stay -- while its neighbours run on; the first interval of the
    next `Engine::step` zeroes the status and the lane moves again.  Through the engine a flagged lane would be flagged again
    at once even if it were not frozen (its step size is below the minimum, its failure count is kept), so the freeze is
    only visible on healthy robots whose bits are written by hand between two intervals: robots in free fall, STEPPER_FAILURE
    on one lane of each of two waves, NAN on another."""
    model = lf.model_of("anymal")
    s = lf.Setup("anymal", B, family=family, adaptive=dict(ADAPTIVE))
    st = lf.healthy_states(model, B)
    st["q"][2] += 1.0
    bits = {2: STEPPER, 5: NAN, B - 1: STEPPER, B - 14: NAN}
    frozen = np.zeros(B, dtype=bool)
    frozen[list(bits)] = True
    expect = np.zeros(B, dtype=np.int32)
    for lane, b in bits.items():
        expect[lane] = b
    o, x = lf.Oracle(s, model), make(s, model)
    before = {}
    for e in (o, x):
        e.start(st["q"], st["v"], st["command"])
        e.interval(1e-3, True)
        assert (e.get("status") == 0).all(), e.get("status")
        for lane, b in bits.items():
            e.poke_status(lane, b)
        before[e] = lf.snapshot(e, s)
        e.interval(2e-3, False)
        assert np.array_equal(e.get("status"), expect), e.get("status")
        t = e.lane_time()
        assert np.allclose(t[~frozen], 2e-3, rtol=0, atol=1e-12) and np.allclose(t[frozen], 1e-3, rtol=0, atol=1e-12), t
        for k in ("q", "v", "a"):
            assert np.array_equal(e.get(k)[:, frozen], before[e][k][:, frozen]), k
    lf.assert_matches_oracle(lf.snapshot(x, s), lf.snapshot(o, s), ~frozen, 1e-8, s, "lanes that ran on")
    for e in (o, x):
        e.interval(3e-3, True)
        assert (e.get("status") == 0).all() and np.allclose(e.lane_time(), 3e-3, rtol=0, atol=1e-12), (e.get("status"), e.lane_time())


def test_host_adaptive_entry_points_carry_the_status_over_and_freeze_failed_lanes():
    scenario_carry_over_and_freeze(_host, "quad", 32)


@pytest.mark.parametrize("form", HOST_ISOLATION)
def test_host_isolation_and_recovery(form):
    s, lanes, kw, _ = _isolation_cases(device=False)[form]
    scenario_isolation(_host, s, lanes, **kw)


# ------------------------------------------------------------------ device
def _device(gpu_device):
    return lambda setup, model: lf.Device(setup, model, gpu_device)


def _family_env(monkeypatch, family):
    if family == "lane":
        monkeypatch.setenv("JM_KERNEL_VARIANT", "lane")


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,B", [("anymal", "quad", 48), ("anymal", "lane", 70), ("atlas", "quad", 48)])
def test_gpu_nan_and_bounds_status(gpu_device, monkeypatch, name, family, B):
    """The bounds check has four sites in the quad code (limb joints of lane k, trunk joints), the cross-lane OR brings
    them to the lead lane's store: every limb lane and a trunk joint are the only source of a bit once."""
    _family_env(monkeypatch, family)
    scenario_nan_and_bounds(_device(gpu_device), name, family, B)


@pytest.mark.gpu
@pytest.mark.parametrize("name,family", [("anymal", "quad"), ("anymal", "lane"), ("atlas", "quad")])
def test_gpu_bounds_raise_no_bit_under_the_constraint_model(gpu_device, monkeypatch, name, family):
    _family_env(monkeypatch, family)
    scenario_bounds_under_the_constraint_model(_device(gpu_device), name, family, 48)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["quad", "lane"])
def test_gpu_force_overflow_at_start_and_reset_is_gone_after_a_step(gpu_device, monkeypatch, family):
    _family_env(monkeypatch, family)
    scenario_force_overflow(_device(gpu_device), "anymal", family, 48)


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,split,B", [("anymal", "quad", "0", 48), ("anymal", "quad", "1", 48), ("atlas", "quad", "1", 48),
                                                 ("anymal", "lane", "0", 70)])
def test_gpu_solver_failure_status(gpu_device, monkeypatch, name, family, split, B):
    """Quad single kernel (k_quad_con), SPLIT_STEP_LANE (ANYmal, B a multiple of 16), SPLIT_STEP (Atlas), k_constrained."""
    _family_env(monkeypatch, family)
    monkeypatch.setenv("JIMINY_AMD_QCON_SPLIT", split)
    scenario_solver_failure(_device(gpu_device), name, family, split == "1", B)


@pytest.mark.gpu
@pytest.mark.parametrize("form,family", [("0", "quad"), ("1", "quad"), ("1", "lane")])
def test_gpu_stepper_failure_status_and_recovery(gpu_device, monkeypatch, form, family):
    """Persistent form (k_quad_dopri), per-stage form over compacted lanes, and the per-stage form of the lane family."""
    _family_env(monkeypatch, family)
    monkeypatch.setenv("JIMINY_AMD_ADAPTIVE_FORM", form)
    scenario_stepper_failure(_device(gpu_device), "anymal", family, 48 if family == "quad" else 70)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(_isolation_cases(device=True)))
def test_gpu_isolation_and_recovery(gpu_device, monkeypatch, form):
    s, lanes, kw, env = _isolation_cases(device=True)[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _assert_forms(gpu_device, s.name, s.B, DEVICE_FORMS[form])
    scenario_isolation(_device(gpu_device), s, lanes, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("form,family", [("0", "quad"), ("1", "quad"), ("1", "lane")])
def test_gpu_adaptive_intervals_carry_the_status_over_and_freeze_failed_lanes(gpu_device, monkeypatch, form, family):
    """`jm_qdopri.h` (persistent form) and `k_dopri_prepare` (per-stage form, both families): two `jm_batch_step_adaptive` calls,
    the second with `new_step` = 0, as `BatchedEngine.step` makes them for two controller periods."""
    _family_env(monkeypatch, family)
    monkeypatch.setenv("JIMINY_AMD_ADAPTIVE_FORM", form)
    scenario_carry_over_and_freeze(_device(gpu_device), family, 48)


@pytest.mark.gpu
def test_gpu_isolation_in_the_block_wave_form(gpu_device):
    """QUAD with the topology's block waves: `select_form` sends a batch there from `grid >= 2 * n_cus` blocks on.  ANYmal's
    blocks hold 4 waves of 16 robots, so the smallest such batch is 64 (2 n_cus - 1) + 1 robots (one robot less runs one wave
    per block: asserted).  Robots on both sides of a block boundary (63 | 64), the first robot and the last, which is alone in
    its block; twin on every lane, oracle on a 64-lane sample.  `start` plus three steps."""
    import torch
    B = 64 * (2 * torch.cuda.get_device_properties(gpu_device).multi_processor_count - 1) + 1
    _assert_forms(gpu_device, "anymal", B, [(dict(_Q, mode="start"), "QUAD"), (dict(_Q, mode="step"), "QUAD")])
    _assert_forms(gpu_device, "anymal", B - 1, [(dict(_Q, mode="step"), "QUAD_ONE_WAVE")])
    sample = np.concatenate([np.arange(48, 80), np.arange(B - 32, B)])
    scenario_isolation(_device(gpu_device), lf.Setup("anymal", B), (0, 63, 64, B - 1), steps=3, oracle_sample=sample, recover=False)
