"""Tracking windows on the device (csrc/jm_tracking.h behind `jm_block_tracking`, `blocks.TrackingWindows`, the
`trajectory_tracking` keyword of `WalkerVecEnv`): the drift of the odometry pose and the shift of the relative foot poses and of
the motor positions against a reference motion, over sliding windows of environment steps.

The expected values are the reference's own (`tests/golden/ref_tracking.npz`, written by tools/make_ref_tracking_fixtures.py
from the reference's `angle_difference`, `angle_distance`, `min_norm`, `compute_drift_error`, `l2_norm`, `quat_to_yaw` and
`radial_basis_function`, with its stacks restated); tests/tracking_numpy.py is a second statement, vectorised over the lanes,
and the home of the error bounds, which are derived from eps, the operation counts, the magnitudes and the window lengths and
not from what the kernel gives.  The kernel body runs on the host (tests/hostemu/tracking.cpp) and on the device, in float64
and float32.  Integer state, copied state, the slots a launch does not write and the designed exact lanes are compared bit
for bit, NaN as a pattern, everything else against its bound."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, codegen, load_builtin, tracking
from tests import tracking_numpy as tn
from tests.hostemu import tracking as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_tracking.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_tracking_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
NEW_SYMBOLS = ("jm_tracking_plan_create", "jm_tracking_plan_destroy", "jm_block_tracking")
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["cases"]]
WRAP_UP, WRAP_DOWN, EQUAL, NAN_LANE = range(4)
EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}
EXACT = ("count", "odom_ring", "yaw_prev")


def case(name: str):
    return tn.load_case(FX, name)


def present_rows(plan) -> list:
    return [r for f in tn.families(plan) for r in tn.FAMILY_ROWS[f]]


def check_sequence(name: str, got: dict, dtype, label: str) -> float:
    """`got` (`[E]`-stacked like the fixture's `expected`) against the reference's values of case `name`."""
    plan, inputs, modes, masks, expected = case(name)
    bounds = tn.bounds(plan, inputs, modes, masks, expected, EPS[dtype])
    rows = present_rows(plan)
    worst = 0.0
    for k, want in expected.items():
        g = got[k]
        assert g.shape == want.shape and g.dtype == tn.dtype_of(k, dtype), (k, g.shape, g.dtype)
        if k == "scalars":
            absent = [r for r in range(6) if r not in rows]
            assert np.isnan(g[:, absent]).all(), "a row of an absent family was written"
            g, want, bound = g[:, rows], want[:, rows], bounds[k][:, rows]
        elif k in ("delta_odom", "delta_odom_reference") and "odom" not in tn.families(plan):
            assert np.isnan(g).all(), "an output of the absent odometry family was written"
            continue
        else:
            bound = None if k in EXACT else bounds[k]
        assert np.array_equal(np.isnan(g), np.isnan(want)), (label, name, k, "the NaN pattern differs")
        if bound is None:
            assert np.array_equal(g, want.astype(g.dtype), equal_nan=True), (label, name, k, "not bit for bit")
            continue
        err = np.nan_to_num(np.abs(g.astype(np.float64) - want))
        over = err > bound
        assert not over.any(), (label, name, k, np.argwhere(over)[:4], float(err[over].max()), float(bound[over].min()))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    if "odom" in tn.families(plan):
        sc = got["scalars"]
        assert (sc[:, [tn.DRIFT_POSITION, tn.DRIFT_ORIENTATION], EQUAL] == 0).all() and (sc[:, tn.REWARD_ODOM_POSE, EQUAL] == 1).all()
    print(f"{label}, {name}, {np.dtype(dtype).name}: worst error / bound {worst:.3f}")
    return worst


# ------------------------------------------------------------------------------------------------------------ fixture
def test_fixture_regenerates_from_the_reference_tree():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_ref_tracking_fixtures as tool
    finally:
        sys.path.pop(0)
    if not os.path.isdir(tool.COMMON):
        pytest.skip("the reference tree is not available")
    done = subprocess.run([sys.executable, TOOL, "--check"], capture_output=True, text=True, cwd=ROOT)
    assert done.returncode == 0, done.stdout + done.stderr


def test_fixture_holds_the_designed_cases():
    assert os.path.getsize(FIXTURE) < 500e3 and set(CASES) == {"regular", "feet", "long", "staggered"}
    plans = {n: case(n)[0] for n in CASES}
    stacks = {int(p[f"max_stack_{f}"]) for p in plans.values() for f in ("odom", "foot", "motor")}
    assert {0, 2, 3, 5} <= stacks
    p = plans["regular"]
    assert len({p["max_stack_odom"], p["max_stack_foot"]}) == 2, "different horizons in one case"
    assert {p["n_rel"] for p in plans.values()} >= {1, 3} and {p["n_motors"] for p in plans.values()} >= {2, 12}
    assert plans["feet"]["max_stack_motor"] == 0 and plans["staggered"]["max_stack_foot"] == 0
    for name in CASES:
        plan, inputs, modes, masks, expected = case(name)
        assert masks.shape[1] == 64 and modes[0] == tn.RESTART and masks[0].all()
        assert set(expected) == set(tn.OUTPUTS + tn.state_names(plan))
        E = len(modes)
        for f in tn.families(plan):
            S = int(plan[f"max_stack_{f}"])
            if name == "long":
                assert S == E + 1, "the window never fills"
            elif name != "staggered":
                assert expected["count"][-1].max() >= 2 * S, "the ring wraps at least twice"
        for v in inputs.values():
            ok = np.isfinite(v)
            assert np.array_equal(v[ok], v[ok].astype(np.float32).astype(np.float64)), "the inputs are exact in float32"
    # lanes restarted while the others are mid-window
    plan, inputs, modes, masks, expected = case("staggered")
    partial = [e for e in range(len(modes)) if modes[e] == tn.RESTART and not masks[e].all()]
    assert len(partial) >= 3 and all((expected["count"][e][~masks[e]] > 0).all() for e in partial[1:])
    # the yaw walks through +-pi in both directions and turns more than once inside a window
    plan, inputs, modes, masks, expected = case("long")
    yaw = inputs["odom_pose"][:, 2]
    assert (np.diff(yaw[:, WRAP_UP]) < -np.pi).any() and (np.diff(yaw[:, WRAP_DOWN]) > np.pi).any()
    assert expected["delta_odom"][-1, 2, WRAP_UP] > 2 * np.pi and expected["delta_odom"][-1, 2, WRAP_DOWN] < -2 * np.pi
    # the NaN enters at event 1 and has left every window at the end
    plan, inputs, modes, masks, expected = case("regular")
    sc = expected["scalars"]
    assert np.isnan(inputs["odom_pose"][1, :, NAN_LANE]).all() and np.isnan(sc[1][:, NAN_LANE]).all()
    assert np.isfinite(sc[-1]).all() and np.isfinite(np.delete(sc, NAN_LANE, -1)).all()
    assert np.isnan(sc[2:, tn.SHIFT_MOTOR_POSITIONS, NAN_LANE]).sum() == 2, "inside the window of 3 for two more events"
    # the exact lane
    for name in CASES:
        plan, _, _, _, expected = case(name)
        sc = expected["scalars"]
        rows = [r for r in present_rows(plan) if r != tn.REWARD_ODOM_POSE]
        assert (sc[:, rows, EQUAL] == 0).all()
        if plan["max_stack_odom"]:
            assert (sc[:, tn.REWARD_ODOM_POSE, EQUAL] == 1).all()
            assert (-np.log(sc[:, tn.REWARD_ODOM_POSE][np.isfinite(sc[:, tn.REWARD_ODOM_POSE])]) / np.log(100.0) <= 4.0 + 1e-9).all()


def _fill(got: dict, plan) -> dict:
    """The outputs of `tn.quantities` with NaN where the kernel writes nothing (rows and outputs of absent families)."""
    got = {k: v.copy() for k, v in got.items()}
    rows = present_rows(plan)
    got["scalars"][[r for r in range(6) if r not in rows]] = np.nan
    if "odom" not in tn.families(plan):
        got["delta_odom"][:], got["delta_odom_reference"][:] = np.nan, np.nan
    return got


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    plan, inputs, modes, masks = case(name)[:4]
    for dtype in (np.float64, np.float32):
        step = lambda inp, st, mode, mask: _fill(tn.quantities(plan, inp, st, mode, mask, dtype), plan)      # noqa: E731, B023
        check_sequence(name, tn.replay(plan, inputs, modes, masks, dtype, step=step), dtype, "numpy")


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name):
    plan, inputs, modes, masks = case(name)[:4]
    for dtype in (np.float64, np.float32):
        step = lambda inp, st, mode, mask: emu.run(plan, inp, st, mode, mask, dtype)      # noqa: E731, B023
        check_sequence(name, tn.replay(plan, inputs, modes, masks, dtype, step=step), dtype, "host emulation")


# --------------------------------------------------------------------------------------- null pointers and the lane mask
POISON = 7.0


def check_nulls_and_mask(run) -> None:
    """`run(plan, inputs, state, mode, mask=None, outputs=tn.OUTPUTS, odometry_cutoff=None)` like `emu.run`: a name missing
    from `inputs` / `state` / `outputs` is a null pointer; unrequested outputs are not returned.  Held to: a family with a
    null input or state array writes nothing (outputs and its state stay), the other families and the counter are not
    affected; null outputs do not stop the state; without the counter nothing runs; a non-positive cutoff leaves the reward
    row; the lanes a mask leaves out keep every bit, state included."""
    plan, inputs, modes, masks, _ = case("regular")
    B = 64
    first, second = tn.event_inputs(inputs, 0), tn.event_inputs(inputs, 2)

    def poisoned():
        st = {k: np.full(tn.shape(k, plan, B), POISON, dtype=tn.dtype_of(k, np.float64)) for k in tn.state_names(plan)}
        return st
    full_state = poisoned()
    full = run(plan, first, full_state, tn.RESTART)
    assert (full_state["count"] == 0).all() and np.isfinite(full["scalars"]).all()
    for family in ("odom", "foot", "motor"):
        for missing in tn.FAMILY_INPUTS[family] + tn.FAMILY_STATE[family]:
            state = poisoned()
            if missing in state:
                del state[missing]
            got = run(plan, {k: v for k, v in first.items() if k != missing}, state, tn.RESTART)
            assert (state["count"] == 0).all(), missing
            assert np.isnan(got["scalars"][list(tn.FAMILY_ROWS[family])]).all(), (missing, "the family wrote a row")
            others = [r for r in range(6) if r not in tn.FAMILY_ROWS[family]]
            assert np.array_equal(got["scalars"][others], full["scalars"][others]), missing
            if family == "odom":
                assert np.isnan(got["delta_odom"]).all() and np.isnan(got["delta_odom_reference"]).all()
            for k, v in state.items():
                if k in tn.FAMILY_STATE[family]:
                    assert (v == POISON).all(), (missing, k, "the skipped family wrote its state")
                else:
                    assert np.array_equal(v, full_state[k]), (missing, k)
    # null outputs: the state runs on
    for outputs in ((), ("scalars",), ("delta_odom",), ("delta_odom_reference", "scalars")):
        state = poisoned()
        got = run(plan, first, state, tn.RESTART, outputs=outputs)
        assert sorted(got) == sorted(outputs) and all(np.array_equal(got[k], full[k]) for k in outputs)
        assert all(np.array_equal(state[k], full_state[k]) for k in state), outputs
    # without the counter nothing runs
    state = poisoned()
    del state["count"]
    got = run(plan, first, state, tn.RESTART)
    assert all(np.isnan(v).all() for v in got.values()) and all((v == POISON).all() for v in state.values())
    # a non-positive cutoff leaves the reward row
    for cutoff in (0.0, -1.0):
        got = run(plan, first, poisoned(), tn.RESTART, odometry_cutoff=cutoff)
        rows = [r for r in range(6) if r != tn.REWARD_ODOM_POSE]
        assert np.isnan(got["scalars"][tn.REWARD_ODOM_POSE]).all() and np.array_equal(got["scalars"][rows], full["scalars"][rows])
    # the lane mask: a push of every other lane (and of no lane) after the restart of all
    whole_state = {k: v.copy() for k, v in full_state.items()}
    whole = run(plan, second, whole_state, tn.PUSH)
    for mask in (np.arange(B) % 2 == 0, np.zeros(B, dtype=bool), np.arange(B) >= 63):
        state = {k: v.copy() for k, v in full_state.items()}
        into = {k: v.copy() for k, v in full.items()}
        got = run(plan, second, state, tn.PUSH, mask=mask, into=into)
        for k in tn.OUTPUTS:
            assert np.array_equal(got[k][..., ~mask], full[k][..., ~mask]) and np.array_equal(got[k][..., mask], whole[k][..., mask]), k
        for k in state:
            assert np.array_equal(state[k][..., ~mask], full_state[k][..., ~mask]), (k, "a masked-out lane changed state")
            assert np.array_equal(state[k][..., mask], whole_state[k][..., mask]), k
    # the slot stays inside the ring whatever the counter holds
    state = {k: v.copy() for k, v in full_state.items()}
    state["count"][:] = np.int32(-5)
    run(plan, second, state, tn.PUSH)
    assert (state["count"] == -4).all()


def test_emulated_null_pointers_skipped_families_and_lane_mask():
    check_nulls_and_mask(emu.run)


# ------------------------------------------------------------------------------------------------------ plan validation
def _good() -> dict:
    return dict(max_stack_odom=3, max_stack_foot=2, max_stack_motor=26, n_rel=3, n_motors=12)


def _rejections() -> list:
    out = []
    for f in ("odom", "foot", "motor"):
        for bad in (1, -2, 1025):
            out.append(({f"max_stack_{f}": bad}, f"max_stack_{f} {bad} out of range \\[2, 1024\\]"))
    out += [(dict(max_stack_odom=0, max_stack_foot=0, max_stack_motor=0, n_rel=0, n_motors=0), "no family"),
            (dict(n_rel=0), "1 <= n_rel <= 63"), (dict(n_rel=64), "1 <= n_rel <= 63"),
            (dict(n_motors=0), "1 <= n_motors <= 256"), (dict(n_motors=257), "1 <= n_motors <= 256"),
            (dict(max_stack_foot=0), "sizes of an absent family must be 0"), (dict(max_stack_motor=0), "sizes of an absent family must be 0")]
    return out


def test_plan_validation_rejects_every_malformed_description():
    emu.pack(tracking.make_desc(**_good())[0])
    for edge in (dict(max_stack_odom=2, max_stack_foot=1024, n_rel=63, n_motors=256), dict(max_stack_odom=0), dict(max_stack_foot=0, n_rel=0),
                 dict(max_stack_odom=0, max_stack_foot=0, n_rel=0)):
        emu.pack(tracking.make_desc(**{**_good(), **edge})[0])
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    for change, message in _rejections():
        with pytest.raises(ValueError, match=message):
            emu.pack(tracking.make_desc(**{**_good(), **change})[0])
    assert (tracking.MAX_STACK, tracking.MAX_REL, tracking.MAX_MOTORS) == (1024, 63, 256)


def _prebuilt(model):
    path = codegen.lib_path(model)
    if not os.path.exists(path):
        pytest.skip(f"{os.path.basename(path)} not built (run __graft_entry__.build())")
    return _lib.load_for(model, allow_build=False)


def _last_error(lib) -> str:
    buf = C.create_string_buffer(1024)
    lib.L.jm_last_error(buf, 1024)
    return buf.value.decode()


def test_plan_create_validates_before_touching_the_device():
    """The same rejections through the C ABI of a built library, on a machine without a device: JM_EINVAL and a message."""
    lib = _prebuilt(load_builtin("cartpole"))
    h = C.c_void_p()
    assert lib.L.jm_tracking_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, _ = tracking.make_desc(**_good())
    assert lib.L.jm_tracking_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    for change, message in _rejections():
        d, _ = tracking.make_desc(**{**_good(), **change})
        rc = lib.L.jm_tracking_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and re.search(message, _last_error(lib)), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    io = _abi.TrackingIO()
    assert lib.L.jm_block_tracking(None, _abi.JM_F64, 64, C.byref(io), 0, 0.0, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    # the order of the fields in the header is the order of the ctypes mirrors
    body = header.split("typedef struct jm_tracking_desc")[1].split("} jm_tracking_desc;")[0]
    order = [line.split(";")[0].split()[-1] for line in body.splitlines() if ";" in line]
    assert order == [f[0] for f in _abi.TrackingDesc._fields_] == list(tn.PLAN_KEYS)
    body = header.split("typedef struct jm_tracking_io")[1].split("} jm_tracking_io;")[0]
    order = [line.split("*")[1].strip(" ;") for line in body.splitlines() if "*" in line]
    assert order == list(_abi.TRACKING_IO_FIELDS) and set(order) == set(tn.INPUTS + tn.STATE + tn.OUTPUTS + ("lane_mask",))
    assert os.path.join(codegen.CSRC, "jm_tracking.h") in codegen._sources()
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


@pytest.mark.parametrize("name, n_feet, n_motors", [("anymal", 4, 12), ("atlas", 2, 30)])
def test_host_plan_of_the_builtin_robots(name, n_feet, n_motors):
    from jiminy_amd.locomotion import sanitize_foot_frame_names
    model = load_builtin(name)
    feet = sanitize_foot_frame_names(model, "auto")
    assert len(feet) == n_feet and model.nmotors == n_motors
    plan = tracking.build_plan(step_dt=0.04, odometry_horizon=1.0, foot_horizon=0.04, motor_horizon=0.07, n_feet=len(feet),
                               n_motors=model.nmotors)
    assert (plan.max_stack_odom, plan.max_stack_foot, plan.max_stack_motor, plan.n_rel, plan.n_motors) == (26, 2, 3, n_feet - 1, n_motors)
    emu.pack(plan.desc()[0])
    only = tracking.build_plan(step_dt=0.04, motor_horizon=0.3, n_motors=model.nmotors)
    assert (only.max_stack_odom, only.max_stack_foot, only.max_stack_motor, only.n_rel, only.n_motors) == (0, 0, 9, 0, n_motors)
    emu.pack(only.desc()[0])
    assert [tracking.stack_length(h, d) for h, d in ((1.0, 0.04), (0.04, 0.04), (0.07, 0.04), (0.3, 0.1))] == [26, 2, 3, 4]


def test_python_surface_refusals_on_the_host(monkeypatch):
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.envs import VecJiminyEnv, WalkerVecEnv
    model = load_builtin("anymal")
    eng = SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _lib=SimpleNamespace(L=None, check=None))
    other = SimpleNamespace(model=model)
    loco, feet = SimpleNamespace(_eng=eng), SimpleNamespace(_eng=eng, plan=SimpleNamespace(n_feet=4))
    act = SimpleNamespace(_eng=eng, motor_side=False, plan=SimpleNamespace(n_motors=12))
    make = blocks.TrackingWindows
    with pytest.raises(TypeError):
        make(eng, odometry_horizon=1.0, locomotion=loco)           # (step_dt is required)
    for keyword, horizon in (("locomotion", "odometry_horizon"), ("foot_poses", "foot_horizon"), ("actuation", "motor_horizon")):
        with pytest.raises(ValueError, match=f"{horizon} reads the {keyword} block"):
            make(eng, step_dt=0.04, **{horizon: 0.2})
        with pytest.raises(ValueError, match=f"the {keyword} block belongs to another engine"):
            make(eng, step_dt=0.04, **{horizon: 0.2, keyword: SimpleNamespace(_eng=other)})
        with pytest.raises(ValueError, match=f"{horizon} must not be below step_dt"):
            make(eng, step_dt=0.04, locomotion=loco, foot_poses=feet, actuation=act, **{horizon: 0.039})
        with pytest.raises(ValueError, match="at most 1024"):
            make(eng, step_dt=0.04, locomotion=loco, foot_poses=feet, actuation=act, **{horizon: 50.0})
    with pytest.raises(ValueError, match="at least one of odometry_horizon"):
        make(eng, step_dt=0.04, locomotion=loco)
    for cutoff in (0.0, -1.0):
        with pytest.raises(ValueError, match="cutoff must be positive"):
            make(eng, step_dt=0.04, locomotion=loco, odometry_horizon=0.2, odometry_cutoff=cutoff)
    with pytest.raises(ValueError, match="give odometry_horizon as well"):
        make(eng, step_dt=0.04, actuation=act, motor_horizon=0.2, odometry_cutoff=0.5)
    with pytest.raises(ValueError, match="motor_side=True"):
        make(eng, step_dt=0.04, actuation=SimpleNamespace(_eng=eng, motor_side=True, plan=act.plan), motor_horizon=0.2)
    with pytest.raises(ValueError, match="two feet or more"):
        make(eng, step_dt=0.04, foot_poses=SimpleNamespace(_eng=eng, plan=SimpleNamespace(n_feet=1)), foot_horizon=0.2)
    with pytest.raises(ValueError, match="step_dt must be positive"):
        make(eng, step_dt=0.0, locomotion=loco, odometry_horizon=0.2)
    names = blocks.tracking_fieldnames(["a", "b"], ["m"])
    assert names["scalars"] == list(tracking.SCALARS) == ["drift_odom_position", "drift_odom_orientation", "reward_odom_pose",
                                                           "shift_foot_positions", "shift_foot_orientations", "shift_motor_positions"]
    assert names["reference_position"] == ["m.ReferencePosition"] and names["delta_odom"] == ["DeltaOdom.X", "DeltaOdom.Y", "DeltaOdom.Yaw"]
    assert names["reference_relative_pose"][0] == ["a.ReferenceRelativeX"]

    # the keywords of the environment, refused before any block is built (the base class is not run: it needs a device)
    def bare_init(self, *args, **kw):
        self.model, self.num_envs, self.step_dt, self.dtype, self.device, self.engine = model, 4, 0.04, torch.float64, torch.device("cpu"), None
    monkeypatch.setattr(VecJiminyEnv, "__init__", bare_init)
    for term in ("drift_odom_position", "drift_odom_orientation", "shift_foot_positions", "shift_foot_orientations", "shift_motor_positions"):
        with pytest.raises(ValueError, match="read the tracking windows block: give trajectory_tracking as well"):
            WalkerVecEnv(terminations={term: (0.1, 0.0)})
    with pytest.raises(ValueError, match=r"drift_odom_position termination needs trajectory_tracking\['odometry_horizon'\]"):
        WalkerVecEnv(terminations=dict(drift_odom_position=(0.1, 0.0)), trajectory_tracking=dict(motor_horizon=0.2), actuated_joints={})
    with pytest.raises(ValueError, match=r"shift_foot_orientations termination needs trajectory_tracking\['foot_horizon'\]"):
        WalkerVecEnv(terminations=dict(shift_foot_orientations=(0.1, 0.0)), trajectory_tracking=dict(motor_horizon=0.2), actuated_joints={})
    with pytest.raises(ValueError, match=r"shift_motor_positions termination needs trajectory_tracking\['motor_horizon'\]"):
        WalkerVecEnv(terminations=dict(shift_motor_positions=(0.1, 0.0)), trajectory_tracking=dict(foot_horizon=0.2), foot_poses={})
    with pytest.raises(ValueError, match="odom_pose reward term reads the tracking windows block"):
        WalkerVecEnv(reward_mixture={"odom_pose": 1.0})
    with pytest.raises(ValueError, match=r"reward_mixture\['odom_pose'\] needs trajectory_tracking\['odometry_cutoff'\]"):
        WalkerVecEnv(reward_mixture={"odom_pose": 1.0}, trajectory_tracking=dict(odometry_horizon=0.2), locomotion_quantities={})
    for horizon, keyword in (("odometry_horizon", "locomotion_quantities"), ("foot_horizon", "foot_poses"), ("motor_horizon", "actuated_joints")):
        with pytest.raises(ValueError, match=f"give {keyword} as well"):
            WalkerVecEnv(trajectory_tracking={horizon: 0.2})
    with pytest.raises(ValueError, match="takes no 'actuation'"):
        WalkerVecEnv(trajectory_tracking=dict(motor_horizon=0.2, actuation=act), actuated_joints={})
    with pytest.raises(ValueError, match="shift_motor_positions"):
        WalkerVecEnv(terminations=dict(overheating=(1.0, 0.0)))
    # the terminations that read the frame kinematics block still ask for it, the new ones do not
    with pytest.raises(ValueError, match="the terminations read the frame kinematics block"):
        WalkerVecEnv(terminations=dict(min_base_height=(0.2, 0.0), shift_motor_positions=(0.1, 0.0)), trajectory_tracking=dict(motor_horizon=0.2),
                     actuated_joints={})


# ------------------------------------------------------------------------------------------------------------ device
class DeviceTracking:
    """Plans on the device and the launch on numpy arrays (copied in and out), with the signature of `emu.run`."""

    def __init__(self, lib, device):
        import torch
        self.torch, self.lib, self.device, self.plans = torch, lib, device, {}

    def handle(self, plan: dict):
        key = tuple(int(plan[k]) for k in tn.PLAN_KEYS)
        if key not in self.plans:
            desc, _ = emu.plan_desc(plan)
            h = C.c_void_p()
            with self.torch.cuda.device(self.device):
                self.lib.check(self.lib.L.jm_tracking_plan_create(C.byref(desc), C.byref(h)))
            self.plans[key] = h
        return self.plans[key]

    def close(self):
        for h in self.plans.values():
            self.lib.L.jm_tracking_plan_destroy(h)

    def run(self, plan, inputs, state, mode, mask=None, dtype=np.float64, outputs=tn.OUTPUTS, into=None, odometry_cutoff=None, B=None):
        torch = self.torch
        B = int(B if B is not None else next(iter(state.values())).shape[-1])
        io, held, dev_state, out = _abi.TrackingIO(), [], {}, {}
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=self.device)      # noqa: E731
        for name in tn.INPUTS:
            if name in inputs:
                assert inputs[name].shape == tn.shape(name, plan, B)
                held.append(up(np.asarray(inputs[name], dtype=dtype)))
                setattr(io, name, held[-1].data_ptr())
        if mask is not None:
            held.append(up(np.asarray(mask, dtype=np.uint8)))
            io.lane_mask = held[-1].data_ptr()
        for name in tn.state_names(plan):
            if name in state:
                assert state[name].shape == tn.shape(name, plan, B) and state[name].dtype == tn.dtype_of(name, dtype)
                dev_state[name] = up(state[name])
                setattr(io, name, dev_state[name].data_ptr())
        for name in outputs:
            a = into[name] if into is not None and name in into else np.full(tn.shape(name, plan, B), np.nan, dtype=dtype)
            assert a.shape == tn.shape(name, plan, B) and a.dtype == np.dtype(dtype)
            out[name] = up(a)
            setattr(io, name, out[name].data_ptr())
        cutoff = float(plan["odometry_cutoff"] if odometry_cutoff is None else odometry_cutoff)
        self.lib.check(self.lib.L.jm_block_tracking(self.handle(plan), _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B,
                                                    C.byref(io), int(mode), cutoff,
                                                    C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        for name, t in dev_state.items():
            state[name][...] = t.cpu().numpy()
        del held
        return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.fixture
def device_tracking(gpu_device):
    dev = DeviceTracking(_prebuilt(load_builtin("cartpole")), gpu_device)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, device_tracking):
    """Every fixture case through the C ABI at B = 64, both dtypes."""
    plan, inputs, modes, masks = case(name)[:4]
    for dtype in (np.float64, np.float32):
        step = lambda inp, st, mode, mask: device_tracking.run(plan, inp, st, mode, mask, dtype)        # noqa: E731, B023
        check_sequence(name, tn.replay(plan, inputs, modes, masks, dtype, step=step), dtype, "device")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["regular", "staggered"])
def test_device_lanes_equal_the_lane_alone(name, device_tracking):
    """A case tiled to B = 300 (one full block of 256 and a partial one), the lanes rotated by 29: after every event, lane b of
    the tiled batch holds the bits lane (b + 29) % 64 holds when it is computed alone at B = 1, in both dtypes."""
    plan, inputs, modes, masks = case(name)[:4]
    lanes = (np.arange(300) + 29) % 64
    tile = lambda d: {k: np.ascontiguousarray(v[..., lanes]) for k, v in d.items()}      # noqa: E731
    for dtype in (np.float64, np.float32):
        step = lambda inp, st, mode, mask: device_tracking.run(plan, inp, st, mode, mask, dtype)      # noqa: E731, B023
        big = tn.replay(plan, tile(inputs), modes, masks[:, lanes], dtype, step=step)
        alone = []
        for b in range(64):
            # (an event that leaves the lane out is not launched for it: `replay` carries its tensors over)
            keep = np.flatnonzero(masks[:, b])
            got = tn.replay(plan, {k: np.ascontiguousarray(v[keep][..., b:b + 1]) for k, v in inputs.items()},
                            np.asarray(modes)[keep], masks[keep][:, b:b + 1], dtype, step=step)
            at = np.searchsorted(keep, np.arange(len(modes)), side="right") - 1
            alone.append({k: v[at] for k, v in got.items()})
        for k in big:
            want = np.concatenate([a[k] for a in alone], -1)[..., lanes]
            assert big[k].shape[-1] == 300 and np.array_equal(big[k], want, equal_nan=True), (k, dtype)


@pytest.mark.gpu
def test_device_null_pointers_skipped_families_and_lane_mask(device_tracking):
    """What the emulation is held to, on the device at B = 300 (a block boundary and a partial last block)."""
    lanes = np.arange(300) % 64

    def run(plan, inputs, state, mode, mask=None, outputs=tn.OUTPUTS, into=None, odometry_cutoff=None):
        tile = lambda d: {k: np.ascontiguousarray(v[..., lanes]) for k, v in d.items()}      # noqa: E731
        big = tile(state)
        got = device_tracking.run(plan, tile(inputs), big, mode, None if mask is None else mask[lanes], outputs=outputs,
                                  into=None if into is None else tile(into), odometry_cutoff=odometry_cutoff, B=300)
        for k in state:
            assert np.array_equal(big[k], big[k][..., :64][..., lanes], equal_nan=True)     # (the tiles agree with each other)
            state[k][...] = big[k][..., :64]
        assert all(np.array_equal(v, v[..., :64][..., lanes], equal_nan=True) for v in got.values())
        return {k: v[..., :64] for k, v in got.items()}
    check_nulls_and_mask(run)


def _sources(env) -> dict:
    """The tensors the tracking block of an environment reads, as numpy arrays in the layout of the kernel's inputs."""
    t = env.tracking
    return dict(odom_pose=env.locomotion.odom_pose, reference_odom_pose=t.reference_odom_pose, relative_pose=env.foot_poses.relative_pose,
                reference_relative_pose=env.foot_poses.reference_relative_pose, position=env.actuation.position,
                reference_position=t.reference_position)


def _numpy(d: dict) -> dict:
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def _plan_of(block) -> dict:
    p = block.plan
    return dict(max_stack_odom=p.max_stack_odom, max_stack_foot=p.max_stack_foot, max_stack_motor=p.max_stack_motor, n_rel=p.n_rel,
                n_motors=p.n_motors, odometry_cutoff=block.odometry_cutoff or 0.0)


def _compare_run(plan, events, modes, masks, got, label):
    """`got [E]` (the block's outputs and state after every event) against the numpy restatement on the recorded inputs."""
    inputs = {k: np.stack([e[k] for e in events]) for k in events[0]}
    want = tn.replay(plan, inputs, modes, masks)
    bounds = tn.bounds(plan, inputs, modes, masks, want, EPS[np.float64])
    worst = 0.0
    for k in got[0]:
        g = np.stack([r[k] for r in got])
        if k in EXACT:
            assert np.array_equal(g, want[k]), (label, k)
            continue
        err = np.abs(g - want[k])
        assert (err <= bounds[k]).all(), (label, k, float(err.max()), np.argwhere(err > bounds[k])[:4])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bounds[k] > 0, err / bounds[k], 0.0))))
    print(f"{label}: worst error / bound {worst:.3f}")
    return want, bounds


TRACKED = dict(locomotion_quantities=dict(forces=False, momentum=False), foot_poses={}, actuated_joints={})


@pytest.mark.gpu
def test_block_on_an_engine(gpu_device):
    """`blocks.TrackingWindows` on the engine of an ANYmal environment with constraint contacts, B = 64, next to the
    environment's own source blocks: more refreshes than the longest window against tests/tracking_numpy.py fed the source
    tensors read back at every step; a masked reset mid-run leaves the other lanes' rings and counters bit for bit."""
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.envs import make_anymal_env
    B = 64
    env = make_anymal_env(B, device=gpu_device, contact_model="constraint", auto_reset=False, **TRACKED)
    env.reset(seed=5)
    blk = blocks.TrackingWindows(env.engine, locomotion=env.locomotion, foot_poses=env.foot_poses, actuation=env.actuation,
                                 odometry_horizon=0.12, foot_horizon=0.04, motor_horizon=0.08, odometry_cutoff=0.5, step_dt=env.step_dt)
    plan = _plan_of(blk)
    assert (plan["max_stack_odom"], plan["max_stack_foot"], plan["max_stack_motor"], plan["n_rel"], plan["n_motors"]) == (4, 2, 3, 3, 12)
    assert blk.reference_relative_pose is env.foot_poses.reference_relative_pose and blk.fieldnames["scalars"] == list(tracking.SCALARS)
    assert blk.odom_ring.shape == (4, 4, B) and blk.yaw_ring.shape == (3, 2, B) and blk.foot_ring.shape == (2, 2, B)
    names = tn.OUTPUTS + tn.state_names(plan)
    tensors = {k: getattr(blk, k) for k in names}
    address = {k: t.data_ptr() for k, t in tensors.items()}
    read = lambda: _numpy(dict(odom_pose=env.locomotion.odom_pose, reference_odom_pose=blk.reference_odom_pose,      # noqa: E731
                               relative_pose=env.foot_poses.relative_pose, reference_relative_pose=blk.reference_relative_pose,
                               position=env.actuation.position, reference_position=blk.reference_position))
    events, modes, masks, got = [], [], [], []

    def record(mode, mask=None):
        torch.cuda.synchronize(gpu_device)
        events.append(read()); modes.append(mode); masks.append(np.ones(B, bool) if mask is None else mask)
        got.append(_numpy(tensors))
    # the reference: the pose of the start on every other lane, zero (the initial tensors) on the others
    lane = torch.arange(B, device=gpu_device)
    blk.set_reference_from_current(lane % 2 == 0)
    assert torch.equal(blk.reference_position[:, 0::2], env.actuation.position[:, 0::2]) and (blk.reference_position[:, 1::2] == 0).all()
    blk.reset()
    record(tn.RESTART)
    assert (blk.scalars[[0, 1, 3, 4, 5]][:, 0::2] == 0).all() and (blk.reward_odom_pose[0::2] == 1).all()
    gen = torch.Generator(device="cpu").manual_seed(7)
    step = lambda: env.step((0.5 * (2.0 * torch.rand(B, env.model.nmotors, generator=gen, dtype=torch.float64) - 1.0)).to(gpu_device))      # noqa: E731
    for _ in range(6):
        step()
        blk.refresh()
        record(tn.PUSH)
    assert (blk.count == 6).all()
    before = _numpy(tensors)
    mask = lane % 3 == 0
    blk.reset(mask)
    record(tn.RESTART, mask.cpu().numpy())
    keep = ~mask.cpu().numpy()
    for k, t in tensors.items():
        assert t is getattr(blk, k) and t.data_ptr() == address[k], k
        assert np.array_equal(got[-1][k][..., keep], before[k][..., keep]), (k, "a lane outside the mask changed")
    assert (blk.count[mask] == 0).all() and (blk.count[~mask] == 6).all()
    for _ in range(3):
        step()
        blk.refresh()
        record(tn.PUSH)
    want, _ = _compare_run(plan, events, modes, np.stack(masks), got, "block on the ANYmal engine")
    assert (want["scalars"][-1][[0, 1, 3, 4, 5]] > 0).all(), "the robot has left its references"
    with pytest.raises(ValueError, match="lane_mask must have shape"):
        blk.reset(mask[:5])
    only = blocks.TrackingWindows(env.engine, actuation=env.actuation, motor_horizon=0.08, step_dt=env.step_dt)
    only.reset()
    torch.cuda.synchronize(gpu_device)
    assert only.odom_ring is None and only.foot_ring is None and (only.scalars[:5] == 0).all() and (only.shift_motor_positions > 0).all()
    for name in ("drift_odom_position", "drift_odom_orientation", "reward_odom_pose", "shift_foot_positions", "shift_foot_orientations",
                 "reference_relative_pose"):
        with pytest.raises(ValueError, match="build it with"):
            getattr(only, name)
    env.close()


@pytest.mark.gpu
def test_environment_records_replays_and_terminates(gpu_device):
    """`make_anymal_env(64, contact_model="constraint", trajectory_tracking=...)`, `auto_reset=False`, seeded actions, a reset
    of every third lane after step 4.  Stage 1 records the three true tensors at every call of `_update_tracking_reference`
    (a subclass's).  Stage 2 replays them as the references under the same actions: the five values are exactly 0, the
    reward exactly its weight, no tracking termination fires.  Stage 3 replays them under other actions, the motor reference
    0.05 rad off from the first call on (so that a shift is above its threshold inside its horizon too): the values become
    positive, and the terminated mask is that of the same run without the terminations or-ed with the numpy evaluation of the
    recorded tensors -- `(t >= grace) & (value > threshold)`, the shift terms with max(grace, horizon) -- on every lane (no value
    sits within its bound of its threshold).  The thresholds of four terms are the medians over the lanes of what the run
    without terminations ends with, so that each fires on some lanes and not on others; the motor threshold lies below what the
    offset alone gives."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    B, steps, reset_after = 64, 8, 4
    cfg = dict(odometry_horizon=0.08, foot_horizon=0.12, motor_horizon=0.08, odometry_cutoff=0.5)
    graces = dict(drift_odom_position=0.08, drift_odom_orientation=0.0, shift_foot_positions=0.0, shift_foot_orientations=0.2,
                  shift_motor_positions=0.0)
    thresholds = {k: (1.0e3, g) for k, g in graces.items()}         # (stage 2: nothing fires whatever the threshold)
    common = dict(device=gpu_device, contact_model="constraint", auto_reset=False, **TRACKED)
    lane = torch.arange(B, device=gpu_device)

    def make(hook, terminations=None, reward=None):
        env = make_anymal_env(B, trajectory_tracking=cfg, terminations=terminations, reward_mixture=reward or {"survival": 1.0}, **common)
        env.__class__ = type("Tracked", (type(env),), {"_update_tracking_reference": hook})
        return env

    def actions(seed):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        return [(0.5 * (2.0 * torch.rand(B, 12, generator=gen, dtype=torch.float64) - 1.0)).to(gpu_device) for _ in range(steps)]

    def drive(env, acts, after=None):
        outs = []
        env.reset(seed=11)
        for i, a in enumerate(acts):
            if i == reset_after:
                env.reset_lanes(lane % 3 == 0)
            outs.append(env.step(a))
            if after is not None:
                after(env, outs[-1])
        return outs
    # stage 1: record
    trajectory, calls = [], []

    def recording(self, lane_mask):
        calls.append(None if lane_mask is None else lane_mask.clone())
        trajectory.append({k: v.clone() for k, v in _sources(self).items() if not k.startswith("reference_")})
    first = make(recording)
    assert first.tracking is not None and first.tracking.plan.max_stack_foot == 4
    drive(first, actions(3))
    assert len(trajectory) == steps + 2 and calls[0] is None and torch.equal(calls[reset_after + 1], lane % 3 == 0)
    assert sum(c is not None for c in calls) == 1

    def replaying(offset):
        index = [0]

        def hook(self, lane_mask):
            frame = trajectory[index[0]]
            index[0] += 1
            self.tracking.reference_odom_pose.copy_(frame["odom_pose"])
            self.foot_poses.reference_relative_pose.copy_(frame["relative_pose"])
            self.tracking.reference_position.copy_(frame["position"] + offset)
        return hook
    # stage 2: the same actions
    second = make(replaying(0.0), terminations=thresholds, reward={"survival": 1.0, "odom_pose": 0.25})
    plain = make_anymal_env(B, device=gpu_device, contact_model="constraint", auto_reset=False)
    outs, base = drive(second, actions(3)), drive(plain, actions(3))
    assert second.tracking.count.tolist() == [steps - reset_after if b % 3 == 0 else steps for b in range(B)]
    for o, p in zip(outs, base):
        assert torch.equal(o[2], p[2]) and torch.equal(o[1], p[1] + 0.25), "no tracking termination fires, the reward is its weight"
    t = second.tracking
    assert (t.scalars[[0, 1, 3, 4, 5]] == 0).all() and (t.reward_odom_pose == 1).all()
    assert (t.delta_odom == t.delta_odom_reference).all() and (t.delta_odom[:2].abs().max() > 0)
    # stage 3: other actions
    loose = make(replaying(0.05))
    base3 = drive(loose, actions(4))
    torch.cuda.synchronize(gpu_device)
    final = loose.tracking.scalars.cpu().numpy()
    thresholds = {k: (float(np.median(final[tracking.SCALARS.index(k)])), g) for k, g in graces.items()}
    thresholds["shift_motor_positions"] = (0.06, 0.0)          # (twelve motors 0.05 rad off: 0.17 at the least)
    print(f"environment: thresholds {thresholds}")
    third = make(replaying(0.05), terminations=thresholds, reward={"survival": 1.0, "odom_pose": 0.25})
    plan = _plan_of(third.tracking)
    events, modes, masks, got, flags, times = [], [], [], [], [], []

    def after(env, out):
        torch.cuda.synchronize(gpu_device)
        events.append(_numpy(_sources(env))); modes.append(tn.PUSH); masks.append(np.ones(B, bool))
        got.append(_numpy({k: getattr(env.tracking, k) for k in tn.OUTPUTS + tn.state_names(plan)}))
        flags.append(out[2].cpu().numpy()); times.append(env._lane_time().cpu().numpy().copy())
    # (the restarts are launches too: the events of `reset` and `reset_lanes` are read after the fact from the recording hook)
    restarts = []
    hook3 = third._update_tracking_reference.__func__

    def watching(self, lane_mask):
        hook3(self, lane_mask)
        if lane_mask is not None or not events and not restarts:
            restarts.append((len(events), _numpy(_sources(self)), np.ones(B, bool) if lane_mask is None else lane_mask.cpu().numpy()))
    third.__class__ = type("Watched", (type(third),), {"_update_tracking_reference": watching})
    outs3 = drive(third, actions(4), after)
    for at, ev, mask in reversed(restarts):
        events.insert(at, ev); modes.insert(at, tn.RESTART); masks.insert(at, mask)
    assert modes == [0] + [1] * reset_after + [0] + [1] * (steps - reset_after)
    pushes = [i for i, m in enumerate(modes) if m == tn.PUSH]
    inputs = {k: np.stack([e[k] for e in events]) for k in events[0]}
    want = tn.replay(plan, inputs, modes, np.stack(masks))
    bounds = tn.bounds(plan, inputs, modes, np.stack(masks), want, EPS[np.float64])
    fired = {k: 0 for k in thresholds}
    inside_horizon = 0
    horizon = dict(shift_foot_positions=cfg["foot_horizon"], shift_foot_orientations=cfg["foot_horizon"], shift_motor_positions=cfg["motor_horizon"])
    for i, e in enumerate(pushes):
        for k in got[i]:
            if k in EXACT:
                assert np.array_equal(got[i][k], want[k][e]), (k, i)
            else:
                assert (np.abs(got[i][k] - want[k][e]) <= bounds[k][e]).all(), (k, i)
        expected_flags, sure = base3[i][2].cpu().numpy().copy(), np.ones(B, bool)
        for k, (threshold, grace) in thresholds.items():
            row = tracking.SCALARS.index(k)
            value, bound = want["scalars"][e][row], bounds["scalars"][e][row]
            sure &= np.abs(value - threshold) > bound
            over = value > threshold
            late = times[i] >= max(grace, horizon.get(k, 0.0))
            if k == "shift_motor_positions":
                inside_horizon += int((over & ~late).sum())
            fired[k] += int((over & late).sum())
            expected_flags |= over & late
        assert sure.all(), "a value sits within its bound of its threshold"
        assert np.array_equal(flags[i], expected_flags), i
        reward = base3[i][1].cpu().numpy() + 0.25 * want["scalars"][e][tn.REWARD_ODOM_POSE]
        assert (np.abs(outs3[i][1].cpu().numpy() - reward) <= 0.25 * bounds["scalars"][e][tn.REWARD_ODOM_POSE] + 4 * EPS[np.float64]).all(), i
    print(f"environment: fired {fired}; {inside_horizon} lane-steps over the motor threshold inside its horizon")
    assert (want["scalars"][-1][[0, 1, 3, 4, 5]] > 0).all() and (want["scalars"][-1][tn.REWARD_ODOM_POSE] < 1).all()
    assert all(n > 0 for n in fired.values()) and inside_horizon > 0
    assert any(f.sum() < B for f in flags), "not every lane terminates"
    # whole-step graphs refuse the block, with the wording of the actuation block
    with pytest.raises(NotImplementedError, match="whole-step graphs"):
        third.enable_graph(True, whole_step=True)
    for env in (first, second, third, loose, plain):
        env.close()
