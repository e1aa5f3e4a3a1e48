"""Actuated-joint quantities on the device (csrc/jm_actuation.h behind `jm_block_actuation`, `blocks.ActuatedJointQuantities`, the
`mechanical_safety` / `power_consumption` terminations and the `power` reward term of `WalkerVecEnv`).

Specification: the reference's own output, tests/golden/ref_actuation.npz (tools/make_ref_actuation_fixtures.py executes the
reference's `compute_power`, `mean` and `radial_basis_function`; eight cases of 64 lanes, each a sequence of launches).

Bounds, derived and not measured (`eps` the machine epsilon of the kernel's type; tests/actuation_numpy.py holds them):
  position, velocity, acceleration, bound_low, bound_high: one copy, one product or one difference each: bit-exact -- float64
    against the fixture, float32 against numpy float32 arithmetic on the float32-rounded inputs;
  safety and the counters: exact;
  POWER: |got - want| <= 4 (M + 2) eps sum_m |v_m r_m e_m|;
  POWER_AVERAGE over n entries: the mean of the n per-entry power bounds + 2 n eps mean_k |p_k|;
  REWARD_POWER: r ln(100) 2 |avg| bound_avg / cutoff^2 + 8 eps, in float64 capped by 1e-13 (the draw keeps it below 2.5e-14).
For float32 the expected scalars are the float64 restatement of tests/actuation_numpy.py on the float32-rounded inputs, and that
restatement is itself pinned to the fixture in float64.

Measured on the host (largest error over bound, all cases, lanes and events): float64 emulation 0.068 (POWER_AVERAGE,
`staggered`), numpy restatement 0.068; float32 emulation 0.086 (POWER, `one_motor`).

Measured on the device (MI355X; the same eight cases through the C ABI, largest error over bound | largest error):
  float64  POWER 0.032 | 3.6e-12 W (`regular`)   POWER_AVERAGE 0.068 | 4.5e-13 W (`staggered`)   REWARD_POWER 0.094 | 5.6e-16
  float32  POWER 0.086 | 4.9e-4 W   POWER_AVERAGE 0.083 | 5.0e-4 W   REWARD_POWER 0.101 | 2.2e-7 (all `one_motor`)
  kinematics, bound distances, safety counts, counters: exact in both dtypes, as derived.
  Environment (ANYmal, 32 lanes, 12 steps of random actions, LOST_EACH): the average power runs from 70 to 830 W, which is
  where the thresholds of that test come from (250 W for the termination, a cutoff of 500 W); reward against the numpy
  restatement 2.2e-16.
"""
from __future__ import annotations

import copy
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, actuation, codegen, load_builtin
from tests import actuation_numpy as an
from tests.hostemu import actuation as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_actuation.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_actuation_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
TOL64 = 1e-13
NEW_SYMBOLS = ("jm_actuation_plan_create", "jm_actuation_plan_destroy", "jm_block_actuation")
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["cases"]]
_CASES: dict = {}


def rounded(inputs: dict) -> dict:
    """The inputs as the float32 kernel sees them, in float64."""
    return {k: v.astype(np.float32).astype(np.float64) for k, v in inputs.items()}


def case(name: str):
    """plan, inputs, modes, masks, expected of a case and, computed once: the float64 restatement, the float32 one, the
    float64 one of the float32-rounded inputs, and the scalar bounds of both dtypes."""
    if name not in _CASES:
        plan, inputs, modes, masks, expected = an.load_case(FX, name)
        n64 = an.replay(plan, inputs, modes, masks, np.float64)
        n32 = an.replay(plan, inputs, modes, masks, np.float32)
        w32 = an.replay(plan, rounded(inputs), modes, masks, np.float64)
        b64 = an.scalar_bounds(plan, inputs, modes, masks, expected["scalars"], float(np.finfo(np.float64).eps))
        b64[:, an.REWARD_POWER] = np.minimum(b64[:, an.REWARD_POWER], TOL64)
        b32 = an.scalar_bounds(plan, rounded(inputs), modes, masks, w32["scalars"], float(np.finfo(np.float32).eps))
        _CASES[name] = (plan, inputs, modes, masks, expected, n64, n32, w32, b64, b32)
    return _CASES[name]


def check_sequence(name: str, got: dict, dtype, label: str) -> None:
    """`[E]`-stacked tensors of a replay (`an.replay`) against the fixture (float64) or the numpy restatements (float32)."""
    plan, inputs, modes, masks, expected, n64, n32, w32, b64, b32 = case(name)
    if np.dtype(dtype) == np.float64:
        for k in an.CONSTANT_OUTPUTS:
            assert all(np.array_equal(row, expected[k]) for row in got[k]), (name, k)
        assert np.array_equal(got["velocity"], expected["velocity"]), name
        want, bounds = expected["scalars"], b64
    else:
        for k in an.KINEMATICS:
            assert got[k].dtype == np.float32 and np.array_equal(got[k], n32[k]), (name, k)
        want, bounds = w32["scalars"], b32
    assert np.array_equal(got["safety"], expected["safety"]) and np.array_equal(got["power_count"], expected["power_count"]), name
    err = np.abs(got["scalars"].astype(np.float64) - want)
    assert np.isfinite(got["scalars"]).all()
    for row, row_name in enumerate(("POWER", "POWER_AVERAGE", "REWARD_POWER")):
        print(f"{label} {name} {np.dtype(dtype).name} {row_name}: error {err[:, row].max():.2e}, "
              f"largest error / bound {(err[:, row] / bounds[:, row]).max():.3f}")
    assert (err <= bounds).all(), (name, float((err / bounds).max()))
    # the ring holds the powers that were pushed, bit for bit
    S = int(plan["max_stack"])
    used = np.arange(S)[None, :, None] < np.minimum(got["power_count"] + 1, S)[:, None, :]
    ring_err = np.abs(got["power_ring"].astype(np.float64) - (expected if np.dtype(dtype) == np.float64 else w32)["power_ring"])
    assert (ring_err[used] <= np.broadcast_to(bounds[:, an.POWER].max(0), ring_err.shape)[used]).all(), name


# ------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_from_the_reference_tree():
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        pytest.skip("the reference tree is not here: the committed fixture stands")
    subprocess.check_call([sys.executable, TOOL, "--check"], stdout=subprocess.DEVNULL)


def test_fixture_holds_the_designed_cases():
    assert CASES == ["regular", "one_motor", "charge", "lost_each", "lost_global", "penalize", "staggered", "thresholds"]
    assert os.path.getsize(FIXTURE) <= 500_000
    eps = float(np.finfo(np.float64).eps)
    for name in CASES:
        plan, inputs, modes, masks, expected = case(name)[:5]
        assert inputs["q"].shape[-1] == 64 and masks.shape == (len(modes), 64) and modes[0] == an.RESTART and masks[0].all()
        assert all(np.isfinite(v).all() for v in expected.values())
        avg = expected["scalars"][:, an.POWER_AVERAGE]
        assert ((avg / plan["power_cutoff"]) ** 2 <= 4.0).all()
        bounds = an.scalar_bounds(plan, inputs, modes, masks, expected["scalars"], eps)
        assert bounds[:, an.REWARD_POWER].max() <= 2.5e-14
        if name != "thresholds":
            # every pair the safety test compares is at least 1e-3 apart
            v = inputs["v"][:, plan["idx_v"].astype(int)]
            pairs = [expected["bound_low"] - plan["position_margin"], expected["bound_high"] - plan["position_margin"],
                     v + plan["velocity_max"], v - plan["velocity_max"]]
            assert min(np.abs(p).min() for p in pairs) >= 1e-3
    plan, inputs, modes, masks, expected = case("regular")[:5]
    assert len(plan["idx_q"]) == 12 and plan["max_stack"] == 3 and list(modes) == [0] + [1] * 8 and plan["motor_side"]
    assert not np.array_equal(plan["idx_q"], np.sort(plan["idx_q"])) and (np.abs(plan["reduction"] - 1.0) > 1.0).all()
    assert (expected["power_count"][-1] == 8).all() and (expected["safety"] > 0).any() and (expected["safety"] == 0).any()
    plan = case("one_motor")[0]
    assert len(plan["idx_q"]) == 1 and plan["max_stack"] == 2
    # one case per generator mode on the same draws, negative per-motor powers, negative totals under LOST_GLOBAL
    assert [case(n)[0]["generator_mode"] for n in ("charge", "lost_each", "lost_global", "penalize")] == [0, 1, 2, 3]
    for n in ("lost_each", "lost_global", "penalize"):
        assert all(np.array_equal(case(n)[1][k], case("charge")[1][k]) for k in an.INPUTS)
    plan, inputs = case("charge")[:2]
    assert (an.motor_powers(plan, an.event_inputs(inputs, 0)) < 0).any()
    total = case("charge")[4]["scalars"][:, an.POWER]
    assert (total < 0).any() and (case("lost_global")[4]["scalars"][:, an.POWER][total < 0] == 0).all()
    # staggered: the counters differ within a wave
    plan, inputs, modes, masks, expected = case("staggered")[:5]
    assert list(modes) == [0] + [0, 1] * 6 and all(0 < m.sum() < 64 for m in masks[1::2]) and masks[2::2].all()
    assert len(np.unique(expected["power_count"][-1])) >= 4
    # thresholds: exact in float32; half of the designed lanes on a threshold (not counted), half one step inside (counted)
    plan, inputs, modes, masks, expected = case("thresholds")[:5]
    on = FX["thresholds.designed_on"]
    assert on.sum() == 32 and all(np.array_equal(v, rounded({"x": v})["x"]) for v in inputs.values())
    low, high, v0 = expected["bound_low"][0], expected["bound_high"][0], inputs["v"][0][plan["idx_v"][0]]
    margin, vmax = plan["position_margin"], plan["velocity_max"]
    assert (((low == margin) | (high == margin) | (v0 == -vmax) | (v0 == vmax)) == on).all()
    extra = (np.arange(64) % 16 >= 8).astype(np.int32)
    assert np.array_equal(expected["safety"][0], (~on).astype(np.int32) + extra)


# ------------------------------------------------------------------------------------------------------ the host side
@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    plan, inputs, modes, masks, expected, n64 = case(name)[:6]
    check_sequence(name, n64, np.float64, "numpy")


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name):
    plan, inputs, modes, masks = case(name)[:4]
    for dtype in (np.float64, np.float32):
        got = an.replay(plan, inputs, modes, masks, dtype,
                        step=lambda inp, st, mode, mask: emu.run(plan, inp, st, mode, mask, dtype))        # noqa: B023
        check_sequence(name, got, dtype, "emulation")


def _poisoned_state(plan, B=64, dtype=np.float64):
    return {"power_ring": np.full((int(plan["max_stack"]), B), 7.25, dtype=dtype), "power_count": np.full(B, 5, dtype=np.int32)}


def check_nulls_mask_and_skipped_rows(run) -> None:
    """`run(inputs, state, mode, mask=None, outputs=..., fill=..., **scalars) -> outputs`: what null pointers, the lane mask
    and the skipped rows leave untouched, for the emulation and for the device alike."""
    plan, inputs = case("regular")[:2]
    inp = an.event_inputs(inputs, 1)
    B = inp["q"].shape[-1]
    state = an.new_state(plan, B)
    full = run(inp, state, an.RESTART)
    assert (full["scalars"][an.POWER_AVERAGE] == full["scalars"][an.POWER]).all() and (state["power_count"] == 0).all()
    # an output that is not asked for is not written; the others do not change
    some = run(inp, an.new_state(plan, B), an.RESTART, outputs=("bound_low", "scalars"), fill=7.25)
    for k, v in some.items():
        assert np.array_equal(v, full[k]) if k in ("bound_low", "scalars") else (v == (7 if k == "safety" else 7.25)).all(), k
    # without the inputs of a part, its outputs keep the poison
    got = run({k: v for k, v in inp.items() if k != "command"}, _poisoned_state(plan, B), an.PUSH, fill=7.25)
    assert (got["scalars"] == 7.25).all() and np.array_equal(got["safety"], full["safety"]) and np.array_equal(got["velocity"], full["velocity"])
    got = run({k: v for k, v in inp.items() if k not in ("q", "a")}, an.new_state(plan, B), an.RESTART, fill=7.25)
    assert all((got[k] == 7.25).all() for k in ("position", "acceleration", "bound_low", "bound_high")) and (got["safety"] == 7).all()
    assert np.array_equal(got["scalars"], full["scalars"]) and np.array_equal(got["velocity"], full["velocity"])
    got = run({k: v for k, v in inp.items() if k != "v"}, _poisoned_state(plan, B), an.PUSH, fill=7.25)
    assert (got["velocity"] == 7.25).all() and (got["scalars"] == 7.25).all() and (got["safety"] == 7).all()
    assert np.array_equal(got["position"], full["position"]) and np.array_equal(got["bound_high"], full["bound_high"])
    # without the window: the power alone; the ring and the counter are not needed
    got = run(inp, None, an.PUSH, fill=7.25)
    assert np.array_equal(got["scalars"][an.POWER], full["scalars"][an.POWER]) and (got["scalars"][1:] == 7.25).all()
    # a negative velocity_max: no safety row; a non-positive cutoff: no reward row
    st = _poisoned_state(plan, B)
    got = run(inp, st, an.RESTART, fill=7.25, velocity_max=-1.0, power_cutoff=0.0)
    assert (got["safety"] == 7).all() and (got["scalars"][an.REWARD_POWER] == 7.25).all()
    assert np.array_equal(got["scalars"][:2], full["scalars"][:2]) and (st["power_count"] == 0).all()
    assert (st["power_ring"][1:] == 7.25).all() and np.array_equal(st["power_ring"][0], full["scalars"][an.POWER])
    # masked lanes only: the others keep outputs, ring and counter bit for bit
    mask = np.arange(B) % 3 == 0
    st = _poisoned_state(plan, B)
    got = run(inp, st, an.PUSH, mask=mask, fill=7.25)
    for k, v in got.items():
        assert (v[..., ~mask] == (7 if k == "safety" else 7.25)).all(), k
    for k in an.KINEMATICS + ("safety",):
        assert np.array_equal(got[k][..., mask], full[k][..., mask]), k
    assert (st["power_count"][mask] == 6).all() and (st["power_count"][~mask] == 5).all()          # slot 6 % 3 = 0
    assert (st["power_ring"][:, ~mask] == 7.25).all() and (st["power_ring"][1:, mask] == 7.25).all()
    assert np.array_equal(st["power_ring"][0, mask], full["scalars"][an.POWER][mask])
    assert np.array_equal(got["scalars"][an.POWER][mask], full["scalars"][an.POWER][mask])
    want = (full["scalars"][an.POWER] + 7.25 + 7.25) / 3.0
    assert np.abs(got["scalars"][an.POWER_AVERAGE] - want)[mask].max() <= 1e-12 * np.abs(want).max()


def test_emulated_null_pointers_lane_mask_and_skipped_rows():
    plan = case("regular")[0]

    def run(inputs, state, mode, mask=None, outputs=an.OUTPUTS, fill=np.nan, **scalars):
        B = next(iter(inputs.values())).shape[-1]
        into = {k: np.full(an.output_shape(k, plan, B), 7 if k == "safety" else fill, dtype=an.output_dtype(k, np.float64)) for k in an.OUTPUTS}
        emu.run(plan, inputs, state, mode, mask, outputs=outputs, into=into, **scalars)
        return into
    check_nulls_mask_and_skipped_rows(run)


def _good() -> dict:
    plan = case("regular")[0]
    return {k: np.array(plan[k]) for k in an.PLAN_KEYS}


def _set_at(index, value):
    def f(a):
        a = a.copy()
        a.reshape(-1)[index] = value
        return a
    return f


def _rejections() -> list:
    """(changes of the description, what the message must say) for every rejection of `jm_actuation_plan_create`."""
    value = lambda v: (lambda a: v)      # noqa: E731
    grow = lambda n, dtype: (lambda a: np.zeros(n, dtype))      # noqa: E731
    many = {k: grow(257, int if k.startswith("idx") else float) for k in ("idx_q", "idx_v", "reduction", "position_low", "position_high")}
    none = {k: grow(0, int if k.startswith("idx") else float) for k in many}
    return [
        (none, "bad sizes"),
        (many, "bad sizes"),
        (dict(nq=value(0)), "bad sizes"),
        (dict(nv=value(0)), "bad sizes"),
        (dict(idx_q=_set_at(3, 14)), r"idx_q\[3\]"),
        (dict(idx_q=_set_at(0, -1)), r"idx_q\[0\]"),
        (dict(idx_v=_set_at(11, 13)), r"idx_v\[11\]"),
        (dict(idx_v=_set_at(2, -1)), r"idx_v\[2\]"),
        (dict(reduction=_set_at(4, np.nan)), r"reduction\[4\] is not finite"),
        (dict(reduction=_set_at(4, np.inf)), r"reduction\[4\] is not finite"),
        (dict(position_low=_set_at(1, -np.inf)), "bounds of motor 1 are not finite"),
        (dict(position_high=_set_at(5, np.nan)), "bounds of motor 5 are not finite"),
        (dict(position_low=_set_at(7, 3.0)), r"position_low\[7\] > position_high\[7\]"),
        (dict(generator_mode=value(4)), "generator_mode"),
        (dict(generator_mode=value(-1)), "generator_mode"),
        (dict(max_stack=value(1)), "max_stack 1 out of range"),
        (dict(max_stack=value(1025)), "max_stack 1025 out of range"),
    ]


def _broken(change: dict):
    arrays = _good()
    for k, f in change.items():
        arrays[k] = f(arrays[k])
    desc, keep = actuation.make_desc(**arrays)
    return desc, keep


def test_plan_validation_rejects_every_malformed_description():
    desc, keep = actuation.make_desc(**_good())
    emu.pack(desc)
    for ok in (dict(max_stack=lambda a: 2), dict(max_stack=lambda a: 1024), dict(position_low=lambda a: case("regular")[0]["position_high"])):
        emu.pack(_broken(ok)[0])
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    for field in ("idx_q", "idx_v", "reduction", "position_low", "position_high"):
        d, keep_ = actuation.make_desc(**_good())
        setattr(d, field, None)
        with pytest.raises(ValueError, match="null array"):
            emu.pack(d)
    for change, message in _rejections():
        d, keep_ = _broken(change)
        with pytest.raises(ValueError, match=message):
            emu.pack(d)
    assert actuation.MAX_MOTORS == 256 >= 64 and actuation.MAX_STACK == 1024


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
    import re
    lib = _prebuilt(load_builtin("cartpole"))
    h = C.c_void_p()
    assert lib.L.jm_actuation_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = actuation.make_desc(**_good())
    assert lib.L.jm_actuation_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.reduction = None
    assert lib.L.jm_actuation_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)
    for change, message in _rejections():
        d, keep_ = _broken(change)
        rc = lib.L.jm_actuation_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and re.search(message, _last_error(lib)), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    io = _abi.ActuationIO()
    assert lib.L.jm_block_actuation(None, _abi.JM_F64, 64, C.byref(io), 0, 0, 0.0, 0.0, 0.0, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    # the order of the fields in the header is the order of the ctypes mirrors
    body = header.split("typedef struct jm_actuation_desc")[1].split("} jm_actuation_desc;")[0]
    order = [line.split(";")[0].split()[-1].strip("*") for line in body.splitlines() if ";" in line]
    assert order == [f[0] for f in _abi.ActuationDesc._fields_]
    assert order == ["n_motors", "nq", "nv", "idx_q", "idx_v", "reduction", "position_low", "position_high", "generator_mode", "max_stack"]
    body = header.split("typedef struct jm_actuation_io")[1].split("} jm_actuation_io;")[0]
    order = [line.split("*")[1].strip(" ;") for line in body.splitlines() if "*" in line]
    assert order == list(_abi.ACTUATION_IO_FIELDS)
    assert os.path.join(codegen.CSRC, "jm_actuation.h") in codegen._sources()
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


@pytest.mark.parametrize("name, n_motors", [("anymal", 12), ("atlas", 30), ("arm7", 7)])
def test_host_plan_of_the_builtin_robots(name, n_motors):
    model = load_builtin(name)
    plan = actuation.build_plan(model, generator_mode="LOST_EACH", power_horizon=0.2, step_dt=0.01)
    a = plan.arrays
    assert plan.n_motors == n_motors == len(a["idx_q"]) and plan.motor_names == [m.name for m in model.motors]
    assert plan.max_stack == 21 and plan.has_horizon and plan.generator_mode == 1 and (a["nq"], a["nv"]) == (model.nq, model.nv)
    for k, m in enumerate(model.motors):
        assert (a["idx_q"][k], a["idx_v"][k], a["reduction"][k]) == (m.idx_q, m.idx_v, m.reduction)
        assert a["position_low"][k] == model.position_lower[m.idx_q] and a["position_high"][k] == model.position_upper[m.idx_q]
        assert a["idx_q"][k] == model.idx_q[m.joint] and a["idx_v"][k] == model.idx_v[m.joint]
    assert (a["position_low"] < a["position_high"]).all() and np.isfinite(a["position_low"]).all()
    emu.pack(plan.desc()[0])
    other = actuation.build_plan(model)
    assert other.max_stack == 2 and not other.has_horizon and other.generator_mode == 0


def _unbounded(model):
    from jiminy_amd.model import JT_RUBX
    model = copy.deepcopy(model)
    model.jtypes = model.jtypes.copy()
    model.jtypes[model.motors[0].joint] = JT_RUBX
    return model


def test_host_plan_refusals_and_the_stack_length():
    model = load_builtin("arm7")
    pairs = {(0.2, 0.01): 21, (0.07, 0.01): 9, (0.3, 0.1): 4, (0.005, 0.01): 2}
    assert 0.07 / 0.01 > 7.0       # (7.000000000000001: the reference's ceil gives 8)
    for (horizon, step_dt), want in pairs.items():
        assert actuation.stack_length(horizon, step_dt) == want
        assert actuation.build_plan(model, power_horizon=horizon, step_dt=step_dt).max_stack == want
    with pytest.raises(ValueError, match="Revolute unbounded joints are not supported for now."):
        actuation.build_plan(_unbounded(model))
    bare = copy.deepcopy(model)
    bare.motors = []
    with pytest.raises(ValueError, match="need a model with motors"):
        actuation.build_plan(bare)
    with pytest.raises(ValueError, match="generator_mode must be one of CHARGE, LOST_EACH, LOST_GLOBAL, PENALIZE"):
        actuation.build_plan(model, generator_mode="RECYCLE")
    with pytest.raises(ValueError, match="generator_mode"):
        actuation.build_plan(model, generator_mode=4)
    with pytest.raises(ValueError, match="give step_dt"):
        actuation.build_plan(model, power_horizon=0.2)
    with pytest.raises(ValueError, match="power_horizon must be positive"):
        actuation.build_plan(model, power_horizon=0.0, step_dt=0.01)
    with pytest.raises(ValueError, match="step_dt must be positive"):
        actuation.build_plan(model, power_horizon=0.2, step_dt=0.0)
    with pytest.raises(ValueError, match="at most 1024"):
        actuation.build_plan(model, power_horizon=20.0, step_dt=0.01)
    assert [actuation.energy_generation_mode(m) for m in ("charge", "LOST_EACH", 2, "PENALIZE")] == [0, 1, 2, 3]


def test_python_surface_refusals_on_the_host(monkeypatch):
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.envs import VecJiminyEnv, WalkerVecEnv
    model = load_builtin("anymal")

    def engine(model=model):
        return SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _lib=SimpleNamespace(L=None, check=None))
    make = blocks.ActuatedJointQuantities
    with pytest.raises(ValueError, match="cutoff must be positive"):
        make(engine(), power_horizon=0.2, step_dt=0.01, power_cutoff=0.0)
    with pytest.raises(ValueError, match="give power_horizon as well"):
        make(engine(), power_cutoff=10.0)
    with pytest.raises(ValueError, match="position_margin and velocity_max together"):
        make(engine(), position_margin=0.1)
    with pytest.raises(ValueError, match="must not be negative"):
        make(engine(), position_margin=0.1, velocity_max=-1.0)
    with pytest.raises(ValueError, match="give step_dt"):
        make(engine(), power_horizon=0.2)
    with pytest.raises(ValueError, match="generator_mode"):
        make(engine(), generator_mode="RECYCLE")
    with pytest.raises(ValueError, match="Revolute unbounded"):
        make(engine(_unbounded(model)))
    names = blocks.actuation_fieldnames(["LF_HAA", "LF_HFE"])
    assert names["scalars"] == ["power", "power_average", "reward_power"] == list(blocks.ACTUATION_SCALARS)
    assert names["bound_low"] == ["LF_HAA.BoundLow", "LF_HFE.BoundLow"] and sorted(names) == sorted(an.KINEMATICS + ("scalars",))

    # the keywords of the environment, refused before any block is built (the base class is not run: it needs a device)
    def bare_init(self, *args, **kw):
        self.model, self.num_envs, self.step_dt, self.dtype, self.device, self.engine = model, 4, 0.04, torch.float64, torch.device("cpu"), None
    monkeypatch.setattr(VecJiminyEnv, "__init__", bare_init)
    with pytest.raises(ValueError, match="mechanical_safety and power_consumption terminations read the actuated-joint quantities"):
        WalkerVecEnv(terminations=dict(mechanical_safety=(0.1, 1.0, 0.0)))
    with pytest.raises(ValueError, match="give actuated_joints as well"):
        WalkerVecEnv(terminations=dict(power_consumption=(100.0, 0.0)))
    with pytest.raises(ValueError, match="power reward term reads the actuated-joint quantities"):
        WalkerVecEnv(reward_mixture={"power": 1.0})
    with pytest.raises(ValueError, match=r"needs actuated_joints\['power_cutoff'\] and actuated_joints\['power_horizon'\]"):
        WalkerVecEnv(reward_mixture={"power": 1.0}, actuated_joints=dict(power_horizon=0.2))
    with pytest.raises(ValueError, match=r"needs actuated_joints\['power_cutoff'\]"):
        WalkerVecEnv(reward_mixture={"power": 1.0}, actuated_joints=dict(power_cutoff=50.0))
    with pytest.raises(ValueError, match="different position_margin"):
        WalkerVecEnv(terminations=dict(mechanical_safety=(0.1, 1.0, 0.0)), actuated_joints=dict(position_margin=0.2, velocity_max=1.0))
    with pytest.raises(ValueError, match="mechanical_safety, power_consumption"):
        WalkerVecEnv(terminations=dict(overheating=(1.0, 0.0)))
    # the four terminations that read the frame kinematics block still ask for it, the two new ones do not
    with pytest.raises(ValueError, match="the terminations read the frame kinematics block"):
        WalkerVecEnv(terminations=dict(min_base_height=(0.2, 0.0), mechanical_safety=(0.1, 1.0, 0.0)), actuated_joints={})
    with pytest.raises(ValueError, match="locomotion_quantities"):
        WalkerVecEnv(terminations=dict(flying=(1.0, 0.0)), actuated_joints={})


# ------------------------------------------------------------------------------------------------------------ device
class DeviceActuation:
    """A plan on the device and the launch on numpy arrays (copied in and out)."""

    def __init__(self, lib, plan: dict, device):
        import torch
        self.torch, self.lib, self.device, self.plan = torch, lib, device, plan
        desc, keep = emu.plan_desc(plan)
        self.h = C.c_void_p()
        with torch.cuda.device(device):
            lib.check(lib.L.jm_actuation_plan_create(C.byref(desc), C.byref(self.h)))

    def close(self):
        self.lib.L.jm_actuation_plan_destroy(self.h)

    def run(self, inputs: dict, state, mode: int, mask=None, dtype=np.float64, outputs=an.OUTPUTS, fill=np.nan, **scalars):
        """One launch; `state` (numpy ring and counter, or None) is updated in place."""
        torch = self.torch
        B = next(iter(inputs.values())).shape[-1]
        io, held, out = _abi.ActuationIO(), [], {}
        for name, a in inputs.items():
            held.append(torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=self.device))
            setattr(io, name, held[-1].data_ptr())
        if mask is not None:
            held.append(torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device=self.device))
            io.lane_mask = held[-1].data_ptr()
        dev_state = {}
        if state is not None:
            for name in an.STATE:
                a = state[name]
                assert a.shape == an.output_shape(name, self.plan, B) and a.dtype == an.output_dtype(name, dtype)
                dev_state[name] = torch.as_tensor(np.ascontiguousarray(a), device=self.device)
                setattr(io, name, dev_state[name].data_ptr())
        for name in an.OUTPUTS:
            shape, dt = an.output_shape(name, self.plan, B), an.output_dtype(name, dtype)
            out[name] = torch.as_tensor(np.full(shape, 7 if name == "safety" else fill, dtype=dt), device=self.device)
            if name in outputs:
                setattr(io, name, out[name].data_ptr())
        self.lib.check(self.lib.L.jm_block_actuation(self.h, _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B, C.byref(io),
                                                     int(mode), *emu.launch_scalars(self.plan, **scalars),
                                                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        for name, t in dev_state.items():
            state[name][...] = t.cpu().numpy()
        del held
        return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, gpu_device):
    """Every fixture case through the C ABI at B = 64, both dtypes."""
    plan, inputs, modes, masks = case(name)[:4]
    dev = DeviceActuation(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        for dtype in (np.float64, np.float32):
            got = an.replay(plan, inputs, modes, masks, dtype,
                            step=lambda inp, st, mode, mask: dev.run(inp, st, mode, mask, dtype))        # noqa: B023
            check_sequence(name, got, dtype, "device")
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_lanes_equal_the_lane_alone(gpu_device):
    """`staggered` tiled to B = 300 (one full block of 256 and a partial one), the lanes rotated by 29: after every event, lane
    b of the tiled batch holds the bits lane (b + 29) % 64 holds when it is computed alone at B = 1, in both dtypes."""
    plan, inputs, modes, masks = case("staggered")[:4]
    dev = DeviceActuation(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        lanes = (np.arange(300) + 29) % 64
        tile = lambda d: {k: np.ascontiguousarray(v[..., lanes]) for k, v in d.items()}      # noqa: E731
        for dtype in (np.float64, np.float32):
            step = lambda inp, st, mode, mask: dev.run(inp, st, mode, mask, dtype)      # noqa: E731, B023
            big = an.replay(plan, tile(inputs), modes, masks[:, lanes], dtype, step=step)
            alone = []
            for b in range(64):
                one = {k: np.ascontiguousarray(v[..., b:b + 1]) for k, v in inputs.items()}
                # (an event that leaves the lane out is not launched for it: `replay` carries its tensors over)
                keep = np.flatnonzero(masks[:, b])
                got = an.replay(plan, {k: (v[keep] if k in an.PER_EVENT_INPUTS else v) for k, v in one.items()},
                                np.asarray(modes)[keep], masks[keep][:, b:b + 1], dtype, step=step)
                at = np.searchsorted(keep, np.arange(len(modes)), side="right") - 1
                alone.append({k: v[at] for k, v in got.items()})
            for k in big:
                want = np.concatenate([a[k] for a in alone], -1)[..., lanes]
                assert big[k].shape[-1] == 300 and np.array_equal(big[k], want), (k, dtype)
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_null_pointers_lane_mask_and_skipped_rows(gpu_device):
    """What the emulation is held to, on the device at B = 300 (a partial last block): null pointers and skipped rows leave
    their targets, masked-out lanes keep outputs, ring and counter bit for bit."""
    plan = case("regular")[0]
    dev = DeviceActuation(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        lanes = np.arange(300) % 64

        def run(inputs, state, mode, mask=None, outputs=an.OUTPUTS, fill=np.nan, **scalars):
            tiled = {k: np.ascontiguousarray(v[..., lanes]) for k, v in inputs.items()}
            big = None if state is None else {k: np.ascontiguousarray(v[..., lanes]) for k, v in state.items()}
            got = dev.run(tiled, big, mode, None if mask is None else mask[lanes], outputs=outputs, fill=fill, **scalars)
            for k in (state or {}):
                assert np.array_equal(big[k], big[k][..., :64][..., lanes])     # (the tiles agree with each other)
                state[k][...] = big[k][..., :64]
            assert all(np.array_equal(v, v[..., :64][..., lanes]) for v in got.values())
            return {k: v[..., :64] for k, v in got.items()}
        check_nulls_mask_and_skipped_rows(run)
    finally:
        dev.close()


@pytest.mark.gpu
def test_block_on_the_cartpole(gpu_device):
    """`blocks.ActuatedJointQuantities` on the smallest built-in robot with a motor, B = 8: 2 x max_stack + 1 refreshes against
    tests/actuation_numpy.py fed the engine's own q / v / a / command read back at every step; then the reset of a lane
    subset restarts exactly those windows and keeps the other lanes and the addresses of the tensors."""
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.engine import BatchedEngine
    model = load_builtin("cartpole")
    B, dt = 8, 1e-2
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device)
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": 1e-3, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt}})
    rg = np.random.default_rng(5)
    q0 = np.tile(model.neutral()[:, None], (1, B))
    q0[model.motors[0].idx_q] = rg.uniform(-1.0, 1.0, B)
    eng.start(torch.from_numpy(q0), torch.from_numpy(rg.uniform(-1.0, 1.0, (model.nv, B))))
    blk = blocks.ActuatedJointQuantities(eng, generator_mode="LOST_EACH", power_horizon=0.025, power_cutoff=40.0, position_margin=9.5,
                                         velocity_max=0.25, motor_side=True, step_dt=dt)
    S = blk.plan.max_stack
    assert S == 4 and blk.fieldnames["position"] == [model.motors[0].name + ".Position"] and blk.power_ring.shape == (S, B)
    plan = dict(blk.plan.arrays, motor_side=True, position_margin=9.5, velocity_max=0.25, power_cutoff=40.0)
    read = lambda: {k: eng.field(k).cpu().numpy().copy() for k in an.INPUTS}      # noqa: E731
    eps = float(np.finfo(np.float64).eps)
    state = an.new_state(plan, B)
    frames, modes, masks, wants = [], [], [], []

    def compare(mode, mask=None):
        torch.cuda.synchronize(gpu_device)
        frames.append(read()); modes.append(mode); masks.append(np.ones(B, bool) if mask is None else mask)
        want = an.quantities(plan, frames[-1], state, mode, masks[-1])
        held = want if not wants else {k: np.where(masks[-1], v, wants[-1][k]) for k, v in want.items()}
        wants.append(held)
        for k in an.KINEMATICS + ("safety",):
            assert np.array_equal(getattr(blk, k).cpu().numpy(), held[k]), (k, len(frames))
        assert np.array_equal(blk.power_count.cpu().numpy(), state["power_count"])
        seq = {"q": frames[0]["q"], "a": frames[0]["a"], "v": np.stack([f["v"] for f in frames]), "command": np.stack([f["command"] for f in frames])}
        bounds = an.scalar_bounds(plan, seq, modes, np.stack(masks), np.stack([w["scalars"] for w in wants]), eps)[-1]
        err = np.abs(blk.scalars.cpu().numpy() - held["scalars"])
        assert (err <= np.maximum(bounds, 0.0)).all(), (len(frames), float((err / bounds).max()))
        return held
    blk.reset()
    compare(an.RESTART)
    assert torch.equal(blk.power_average, blk.power)
    counted = 0
    for i in range(2 * S + 1):
        eng.set_command(torch.from_numpy(rg.uniform(-20.0, 20.0, (model.nmotors, B))))
        eng.step(dt)
        blk.refresh()
        counted += int(compare(an.PUSH)["safety"].sum())
    assert (blk.power_count == 2 * S + 1).all() and counted > 0
    assert float(blk.reward_power.min()) > 0.0 and float(blk.reward_power.max()) <= 1.0
    # a partial reset
    tensors = {k: getattr(blk, k) for k in an.OUTPUTS + an.STATE}
    before = {k: t.clone() for k, t in tensors.items()}
    address = {k: t.data_ptr() for k, t in tensors.items()}
    mask = torch.arange(B, device=gpu_device) % 3 == 0
    blk.reset(mask)
    held = compare(an.RESTART, mask.cpu().numpy())
    for k, t in tensors.items():
        assert t is getattr(blk, k) and t.data_ptr() == address[k], k
        assert torch.equal(t[..., ~mask], before[k][..., ~mask]), k
    assert (blk.power_count[mask] == 0).all() and (blk.power_count[~mask] == 2 * S + 1).all()
    assert torch.equal(blk.power_average[mask], blk.power[mask]) and torch.equal(blk.power_ring[0][mask], blk.power[mask])
    with pytest.raises(ValueError, match="lane_mask must have shape"):
        blk.reset(mask[:5])
    # tensors of another dtype are refused before the launch
    good, blk.position = blk.position, blk.position.to(torch.float32)
    with pytest.raises(ValueError, match="engine-dtype tensors"):
        blk.refresh()
    blk.position = good
    assert (blk.power_count[~mask] == 2 * S + 1).all()
    # without a horizon the window is not exposed
    bare = blocks.ActuatedJointQuantities(eng)
    bare.reset()
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(bare.power, torch.as_tensor(an.power(dict(plan, generator_mode=0), read()), device=gpu_device))
    assert (bare.scalars[1:] == 0).all() and (bare.safety == 0).all()
    for name in ("power_average", "reward_power"):
        with pytest.raises(ValueError, match="build it with"):
            getattr(bare, name)
    eng.stop()


def _same(a, b) -> bool:
    """Two step results (nested tuples / dictionaries of tensors) hold the same bits."""
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return bool((a == b).all()) if hasattr(a, "shape") else a == b


@pytest.mark.gpu
def test_environment_terminations_and_reward(gpu_device):
    """`make_anymal_env(32, contact_model="constraint", actuated_joints=..., terminations=..., reward_mixture=...)`, 12 steps of
    random actions.  Both terminations and the reward term equal the numpy restatement evaluated on the environment's own
    q / v / a / command after every step (lanes whose value lies within its bound of the threshold are not compared: there are
    none); with a grace period of 10 s the flags are those of the plain environment; with a margin wider than every joint
    range and `velocity_max = 0` every moving joint counts, so some lane terminates; and an environment without the keyword
    gives the bits of one built as before, while the block does not touch the physics."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    B, steps = 32, 12
    common = dict(device=gpu_device, contact_model="constraint", auto_reset=False)
    cfg = dict(generator_mode="LOST_EACH", power_horizon=0.1, power_cutoff=500.0)
    safety, power_term = (0.3, 1.0, 0.0), (250.0, 0.0)
    env = make_anymal_env(B, actuated_joints=cfg, terminations=dict(mechanical_safety=safety, power_consumption=power_term),
                          reward_mixture={"survival": 1.0, "power": 0.5}, **common)
    graceful = make_anymal_env(B, actuated_joints=cfg, terminations=dict(mechanical_safety=(100.0, 0.0, 10.0), power_consumption=(0.0, 10.0)), **common)
    wide = make_anymal_env(B, actuated_joints={}, terminations=dict(mechanical_safety=(100.0, 0.0, 0.0)), **common)
    plain, plain2 = make_anymal_env(B, **common), make_anymal_env(B, actuated_joints=None, **common)
    assert plain.actuation is None and plain.frames is None and env.frames is None and env.actuation.plan.max_stack == 4
    assert (env.actuation.position_margin, env.actuation.velocity_max) == safety[:2] and not wide.actuation.plan.has_horizon
    envs = (env, graceful, wide, plain, plain2)
    for e in envs:
        e.reset(seed=11)
    act = env.actuation
    plan = dict(act.plan.arrays, motor_side=False, position_margin=safety[0], velocity_max=safety[1], power_cutoff=cfg["power_cutoff"])
    read = lambda: {k: env.engine.field(k).cpu().numpy().copy() for k in an.INPUTS}      # noqa: E731
    eps = float(np.finfo(np.float64).eps)
    state = an.new_state(plan, B)
    frames = [read()]
    wants = [an.quantities(plan, frames[0], state, an.RESTART)]
    assert np.array_equal(act.power_count.cpu().numpy(), np.zeros(B, np.int32))
    gen = torch.Generator().manual_seed(3)
    fired = {"safety": 0, "power": 0, "wide": 0}
    worst = 0.0
    for i in range(steps):
        action = (torch.rand(B, env.model.nmotors, generator=gen, dtype=torch.float64) * 2.0 - 1.0).to(gpu_device) * 3.0
        out = [e.step(action) for e in envs]
        torch.cuda.synchronize(gpu_device)
        frames.append(read())
        wants.append(an.quantities(plan, frames[-1], state, an.PUSH))
        want = wants[-1]
        seq = {"q": frames[0]["q"], "a": frames[0]["a"], "v": np.stack([f["v"] for f in frames]), "command": np.stack([f["command"] for f in frames])}
        bounds = an.scalar_bounds(plan, seq, [0] + [1] * (i + 1), np.ones((i + 2, B), bool), np.stack([w["scalars"] for w in wants]), eps)[-1]
        got = act.scalars.cpu().numpy()
        assert (np.abs(got - want["scalars"]) <= bounds).all(), i
        assert np.array_equal(act.safety.cpu().numpy(), want["safety"]) and np.array_equal(act.power_count.cpu().numpy(), state["power_count"])
        for k in an.KINEMATICS:
            assert np.array_equal(getattr(act, k).cpu().numpy(), want[k]), (k, i)
        average = want["scalars"][an.POWER_AVERAGE]
        assert (np.abs(average - power_term[0]) > bounds[an.POWER_AVERAGE]).all()
        base = out[3][2].cpu().numpy()
        unsafe, hungry = want["safety"] > 0, average > power_term[0]
        print(f"step {i}: average power {average.min():.1f} .. {average.max():.1f} W, {int(unsafe.sum())} unsafe lanes, {int(hungry.sum())} over the power")
        assert np.array_equal(out[0][2].cpu().numpy(), base | unsafe | hungry), i
        reward = 1.0 + 0.5 * want["scalars"][an.REWARD_POWER]
        worst = max(worst, float(np.abs(out[0][1].cpu().numpy() - reward).max()))
        # (the weight times the bound of the row, plus the roundings of one product and one sum of values below 1.5)
        assert (np.abs(out[0][1].cpu().numpy() - reward) <= 0.5 * bounds[an.REWARD_POWER] + 4 * eps).all(), i
        fired["safety"] += int(unsafe.sum()); fired["power"] += int(hungry.sum())
        # before the grace period nothing of the new terminations fires
        assert torch.equal(out[1][2], out[3][2]), i
        fired["wide"] += int((out[2][2] & ~out[3][2]).sum())
        # without the keyword: the same bits; and the block does not touch the physics
        assert _same(out[3], out[4]), i
        assert _same(out[0][0], out[3][0]) and torch.equal(env.engine.robot_state.q, plain.engine.robot_state.q), i
    print(f"environment: reward against the numpy restatement {worst:.2e}; fired {fired}")
    assert fired["wide"] > 0 and fired["power"] > 0 and fired["power"] < B * steps
    # a partial reset restarts the windows of the reset lanes and keeps the others
    mask = torch.arange(B, device=gpu_device) % 2 == 0
    kept = {k: getattr(act, k).clone() for k in an.OUTPUTS + an.STATE}
    env.reset_lanes(mask)
    for k, t in kept.items():
        assert torch.equal(getattr(act, k)[..., ~mask], t[..., ~mask]), k
    assert (act.power_count[mask] == 0).all() and (act.power_count[~mask] == steps).all()
    assert torch.equal(act.power_average[mask], act.power[mask])
    for e in envs:
        e.close()
