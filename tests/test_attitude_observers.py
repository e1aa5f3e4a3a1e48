"""The attitude observers: `MahonyFilter` with its options and `BodyObserver` -- kernel bodies (host emulation and device), plan
builder, C ABI, Python surface, environment.

The specification is the reference's own output (tests/golden/ref_attitude.npz, written by tools/make_ref_attitude_fixtures.py
from the reference's functions), every lane of it; the exact initialisation is checked against a rotation walk over the
compiled model coded in this file.

Tolerances.
* float64 against the fixture: 1e-13 relative to max(|want|, 1), the bar of every block pinned to reference Python.  The
  numpy float64 restatement of tests/attitude_numpy.py must keep it as well on the regular cases.
* `mahony.n3_singular` puts one IMU of every second lane upside down on its first tick (tilt within 5e-6 of -e_z, the
  singular branch of `swing_from_vector`); its bound is max(1e-13, 4 x the deviation the numpy float64 restatement shows
  on the same case).  That tick is authored at rest, so the filter's early return hands the stored quaternion to the twist
  removal bit for bit, and the tilt is evaluated without fused multiply-adds in the kernel (`quat_tilt<TILT_ROUNDED>`): the one
  quantity that the branch amplifies by 1e5 is then the same number in all three implementations.  Measured (quat | rpy):
  numpy restatement 0 | 0 (the same operations in the same order as the reference's), emulated kernel 7.8e-16 | 7.5e-15,
  MI355X 2.2e-15 | 9.1e-15; the bound is its floor, 1e-13.  Regular cases: emulated kernel 0 | 4.4e-16, MI355X 3.3e-16 |
  8.9e-16.
* float32 against the float64 fixture: measured, not chosen: 4 x the error of the numpy float32 restatement on the same case
  and quantity.  Measured largest over the regular cases (numpy float32 | emulated kernel): Mahony quat 2.4e-7 | 2.4e-7, rpy
  3.9e-7 | 4.5e-7, body quat 1.1e-7 | 1.1e-7, rpy 3.8e-7 | 3.0e-7, initialisation quat 1.6e-7, rpy 6.4e-6.  In float32 the tilt
  of an upside-down IMU is rounding noise (1 + v_z of 1e-11 .. 5e-6 next to an ulp of 6e-8): `n3_singular` quat 1.1e-3 | 1.1e-3,
  rpy 2.0 | 2.0 (a roll on the other side of the +-pi cut), which says what float32 is worth there, not how well the
  kernel is written.  The float32 tests of that case therefore assert the same rule once more on the (IMU, lane) pairs that stay
  upright (`_check_float32_on_upright_pairs`), where it means what it means elsewhere.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, attitude, codegen, load_builtin
from jiminy_amd.model import (JT_FREEFLYER, JT_PU, JT_PX, JT_RU, JT_RUBU, JT_RUBX, JT_RX, JT_RZ, JT_SPHERICAL, add_sensor)
from tests import attitude_numpy as an
from tests import deformation_numpy as dn
from tests import robots
from tests import robots_deformation as rd
from tests.hostemu import attitude as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_attitude.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_attitude_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
TOL = 1e-13
NEW_SYMBOLS = ("jm_attitude_plan_create", "jm_attitude_plan_destroy", "jm_block_attitude_init", "jm_block_mahony_observer",
               "jm_block_body_observer")
FX = np.load(FIXTURE)
MAHONY_CASES = [str(c) for c in FX["mahony_cases"]]
BODY_CASES = [str(c) for c in FX["body_cases"]]
INIT_KEYS = ("nq", "frame_seg_start", "seg_kind", "seg_q_index", "seg_rot", "seg_axis")


def _err(got: np.ndarray, want: np.ndarray) -> float:
    assert got.shape == want.shape and np.isfinite(got).all(), (got.shape, want.shape)
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)))


def _plain_arrays(n_imu: int, kp=None, ki=None, rel_quat=None) -> dict:
    """A description whose frames are the identity: what the cases that do not initialise need."""
    return dict(nq=0, kp=np.ones(n_imu) if kp is None else kp, ki=np.ones(n_imu) if ki is None else ki,
                rel_quat=np.tile([0.0, 0.0, 0.0, 1.0], (n_imu, 1)) if rel_quat is None else rel_quat,
                frame_seg_start=np.arange(n_imu + 1), seg_kind=np.zeros(n_imu, dtype=np.int32),
                seg_q_index=-np.ones(n_imu, dtype=np.int32), seg_rot=np.tile(np.eye(3), (n_imu, 1, 1)), seg_axis=np.zeros((n_imu, 3)))


# ------------------------------------------------------------------------------------------------ the cases, any driver
def _mahony_case(name: str) -> dict:
    return {k: FX[f"mahony.{name}.{k}"] for k in ("n_imu", "kp", "ki", "dt", "ignore_twist", "compute_rpy", "quat0", "bias0", "imu",
                                                   "quat", "bias", "omega", "cf", "lane_kind")} | \
        ({"rpy": FX[f"mahony.{name}.rpy"]} if int(FX[f"mahony.{name}.compute_rpy"]) else {})


def _tile(a: np.ndarray, lanes) -> np.ndarray:
    return a if lanes is None else np.ascontiguousarray(a[..., lanes])


def run_mahony(tick, c: dict, dtype, lanes=None) -> dict:
    """All ticks of a Mahony case through `tick(imu, quat, omega, cf, bias, rpy)` (in place).  Returns what the fixture holds."""
    n = int(c["n_imu"])
    quat, bias = _tile(c["quat0"], lanes).astype(dtype), _tile(c["bias0"], lanes).astype(dtype)
    Bn = quat.shape[-1]
    omega, cf = np.full((3, n, Bn), np.nan, dtype), np.full((3, n, Bn), np.nan, dtype)
    rpy = np.full((3, n, Bn), np.nan, dtype) if int(c["compute_rpy"]) else None
    out = {"quat": [], "rpy": []}
    for t in range(c["imu"].shape[0]):
        tick(_tile(c["imu"][t], lanes), quat, omega, cf, bias, rpy)
        out["quat"].append(quat.copy())
        if rpy is not None:
            out["rpy"].append(rpy.copy())
    got = {"quat": np.stack(out["quat"]), "bias": bias, "omega": omega, "cf": cf}
    if rpy is not None:
        got["rpy"] = np.stack(out["rpy"])
    return got


def emu_mahony_tick(c: dict):
    desc, keep = attitude.make_desc(**_plain_arrays(int(c["n_imu"]), c["kp"], c["ki"]))

    def tick(imu, quat, omega, cf, bias, rpy):
        emu.mahony(desc, imu, quat, omega, cf, bias, float(c["dt"]), bool(c["ignore_twist"]), rpy)
    tick.keep = keep
    return tick


def numpy_mahony_tick(c: dict, dtype):
    def tick(imu, quat, omega, cf, bias, rpy):
        q, b, o, f = an.mahony_tick(quat, bias, imu, c["kp"], c["ki"], float(c["dt"]), bool(c["ignore_twist"]), dtype)
        quat[:], bias[:], omega[:], cf[:] = q, b, o, f
        if rpy is not None:
            rpy[:] = an.rpy_of(quat)
    return tick


def _errors(got: dict, c: dict, lanes=None) -> dict:
    return {k: _err(v, _tile(c[k], lanes)) for k, v in got.items()}


def _mahony_bounds(name: str, c: dict, dtype) -> dict:
    errs = _errors(run_mahony(numpy_mahony_tick(c, dtype), c, dtype), c)
    if dtype == np.float32:
        return {k: 4 * e for k, e in errs.items()}, errs
    if name != "n3_singular":
        assert max(errs.values()) <= TOL, (name, errs)      # the restatement itself keeps the bar on the regular cases
        return {k: TOL for k in errs}, errs
    return {k: max(TOL, 4 * e) for k, e in errs.items()}, errs


def _upright_pairs(c: dict) -> np.ndarray:
    """`[n_imu][B]`: the (IMU, lane) pairs that never enter the singular branch (the ticks after the first are authored away from
    it).  An IMU's state is its own -- only the singular flag is shared by the lane -- so on these pairs float32 is worth what
    it is worth on a regular case, double normalisation of the singular lanes included."""
    return ~(an.tilt(c["quat0"])[2] < -1 + 1e-5)


def _check_float32_on_upright_pairs(tick, c: dict, label: str, lanes=None) -> None:
    """The float32 bound of `n3_singular` as a whole is that of its upside-down IMUs (see the module docstring).  Here the same
    rule -- 4 x the error of the numpy float32 restatement -- on the other pairs only: measured there, numpy float32 | emulated
    kernel | MI355X, quat 1.9e-7 | 1.9e-7 | 1.8e-7, cf 4.0e-7 | 4.0e-7 | 5.8e-7, rpy 4.0e-7 | 3.8e-7 | 4.8e-7."""
    pairs = _tile(_upright_pairs(c), lanes)
    assert 0 < (~pairs).sum() < pairs.size / 3
    want = {k: _tile(c[k], lanes)[..., pairs] for k in ("quat", "bias", "omega", "cf", "rpy")}
    ref = {k: _err(v[..., pairs], want[k]) for k, v in run_mahony(numpy_mahony_tick(c, np.float32), c, np.float32, lanes).items()}
    got = {k: _err(v[..., pairs], want[k]) for k, v in run_mahony(tick, c, np.float32, lanes).items()}
    print(f"n3_singular float32, pairs that stay upright: {label} {got} | numpy float32 {ref}")
    assert max(ref["quat"], ref["rpy"]) < 1e-5        # (the restriction does what it is for: float32 rounding, not 1e-3)
    assert all(got[k] <= 4 * ref[k] for k in got), (got, ref)


def _body_case(name: str) -> dict:
    keys = ["n_imu", "rel_quat", "dt", "twist_mode", "time_constant_inv", "compute_rpy", "imu_quat", "imu_omega", "quat", "omega"]
    c = {k: FX[f"body.{name}.{k}"] for k in keys}
    for k in ("twist", "rpy"):
        if f"body.{name}.{k}" in FX.files:
            c[k] = FX[f"body.{name}.{k}"]
    return c


def run_body(tick, c: dict, dtype, lanes=None) -> dict:
    n = int(c["n_imu"])
    Bn = _tile(c["imu_quat"][0], lanes).shape[-1]
    twist = np.zeros((n, Bn), dtype)
    quat, omega = np.full((4, n, Bn), np.nan, dtype), np.full((3, n, Bn), np.nan, dtype)
    rpy = np.full((3, n, Bn), np.nan, dtype) if int(c["compute_rpy"]) else None
    out = {k: [] for k in ("quat", "omega", "twist", "rpy")}
    for t in range(c["imu_quat"].shape[0]):
        tick(_tile(c["imu_quat"][t], lanes), _tile(c["imu_omega"][t], lanes), quat, omega, twist, rpy)
        for k, v in (("quat", quat), ("omega", omega), ("twist", twist), ("rpy", rpy)):
            if v is not None:
                out[k].append(v.copy())
    return {k: np.stack(v) for k, v in out.items() if v and k in c}


def emu_body_tick(c: dict):
    desc, keep = attitude.make_desc(**_plain_arrays(int(c["n_imu"]), rel_quat=c["rel_quat"]))

    def tick(iq, io, quat, omega, twist, rpy):
        emu.body(desc, iq, io, quat, omega, twist, int(c["twist_mode"]), float(c["time_constant_inv"]), float(c["dt"]), rpy)
    tick.keep = keep
    return tick


def numpy_body_tick(c: dict, dtype):
    def tick(iq, io, quat, omega, twist, rpy):
        q, o, tw = an.body_tick(iq, io, c["rel_quat"], twist, int(c["twist_mode"]), float(c["time_constant_inv"]), float(c["dt"]), dtype)
        quat[:], omega[:], twist[:] = q, o, tw
        if rpy is not None:
            rpy[:] = an.rpy_of(quat)
    return tick


def _body_bounds(c: dict, dtype):
    errs = _errors(run_body(numpy_body_tick(c, dtype), c, dtype), c)
    if dtype == np.float32:
        return {k: 4 * e for k, e in errs.items()}, errs
    assert max(errs.values()) <= TOL, errs
    return {k: TOL for k in errs}, errs


def _init_arrays() -> dict:
    a = {k: FX[f"init.joints.{k}"] for k in INIT_KEYS}
    n = int(FX["init.joints.n_imu"])
    return dict(a, nq=int(a["nq"]), kp=np.ones(n), ki=np.ones(n), rel_quat=np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))


def run_init(call, exact_init: bool, dtype, lanes=None, mask=None, prefill=None):
    """`call(q, imu, mask, exact_init, quat, omega, cf, bias, twist, rpy)` on the initialisation case."""
    n = int(FX["init.joints.n_imu"])
    q, imu = _tile(FX["init.joints.q"], lanes).astype(dtype), _tile(FX["init.joints.imu"], lanes).astype(dtype)
    Bn = q.shape[-1]
    fill = np.nan if prefill is None else prefill
    state = dict(quat=np.full((4, n, Bn), fill, dtype), omega=np.full((3, n, Bn), fill, dtype), cf=np.full((3, n, Bn), fill, dtype),
                 bias=np.full((3, n, Bn), fill, dtype), twist=np.full((n, Bn), fill, dtype), rpy=np.full((3, n, Bn), fill, dtype))
    call(q, imu, mask, exact_init, *state.values())
    return state


def _check_init(state: dict, exact_init: bool, bounds: dict, lanes=None, where=slice(None)) -> dict:
    tag = "exact" if exact_init else "acc"
    eq = _err(state["quat"][..., where], _tile(FX[f"init.joints.quat_{tag}"], lanes)[..., where])
    er = _err(state["rpy"][..., where], _tile(FX[f"init.joints.rpy_{tag}"], lanes)[..., where])
    assert eq <= bounds["quat"] and er <= bounds["rpy"], (tag, eq, er, bounds)
    for k in ("omega", "cf", "bias", "twist"):
        assert not state[k][..., where].any(), k
    return {"quat": eq, "rpy": er}


def _init_bounds(exact_init: bool, dtype) -> dict:
    tag = "exact" if exact_init else "acc"
    q, falling = an.init(_init_arrays(), FX["init.joints.q"], FX["init.joints.imu"], exact_init, dtype)
    errs = {"quat": _err(q, FX[f"init.joints.quat_{tag}"]), "rpy": _err(an.rpy_of(q), FX[f"init.joints.rpy_{tag}"])}
    if not exact_init:
        assert np.array_equal(falling, FX["init.joints.lane_kind"] == "fallback")
    if dtype == np.float32:
        return {k: 4 * e for k, e in errs.items()}
    assert max(errs.values()) <= TOL, errs
    return {k: TOL for k in errs}


def emu_init_call():
    desc, keep = attitude.make_desc(**_init_arrays())

    def call(q, imu, mask, exact_init, quat, omega, cf, bias, twist, rpy):
        emu.init(desc, q, imu, exact_init, quat, omega, cf, bias, twist, rpy, mask)
    call.keep = keep
    return call


# ------------------------------------------------------------------------------------------------------ fixture, bodies
def test_fixture_covers_what_it_claims():
    assert os.path.getsize(FIXTURE) < 1 << 20 and "restated" in str(FX["tier"]) and str(FX["tier"]).startswith("A")
    combos, rest, one, swing = set(), 0, 0, {}
    for name in MAHONY_CASES:
        c = _mahony_case(name)
        assert c["quat"].shape == (5, 4, int(c["n_imu"]), 64) and c["imu"].shape == (5, int(c["n_imu"]), 6, 64)
        combos.add((int(c["n_imu"]), int(c["ignore_twist"]), int(c["compute_rpy"])))
        hits = json.loads(str(FX[f"mahony.{name}.hits"]))
        assert hits["moving"] > 0
        kinds = [str(k) for k in c["lane_kind"]]
        rest += hits["rest"] if "rest" in kinds else 0
        one += kinds.count("one")
        for k, v in hits["swing"].items():
            swing[k] = swing.get(k, 0) + v
        assert len(set(c["kp"])) == len(c["kp"]) and len(set(c["ki"])) == len(c["ki"])      # unequal gains per IMU
    assert combos >= {(n, i, r) for n in (1, 3) for i in (0, 1) for r in (0, 1)}
    assert rest > 0 and one > 0
    assert set(swing) == {"regular", "xy", "ratio_x", "ratio_y", "general_x", "general_y"} and min(swing.values()) > 0
    s = _mahony_case("n3_singular")
    kinds = [str(k) for k in s["lane_kind"]]
    assert {k.split(":")[1] for k in kinds if ":" in k} == {"xy", "ratio_x", "ratio_y", "general_x", "general_y"}
    # on the singular lanes exactly one IMU of three is upside down at the first swing, the other two are regular
    vz = an.tilt(s["quat0"])[2]
    sing = np.array([":" in k for k in kinds])
    assert ((vz[:, sing] < -1 + 1e-5).sum(0) == 1).all() and not (vz[:, ~sing] < -1 + 1e-5).any()
    kinds = [str(k) for k in FX["init.joints.lane_kind"]]
    assert min(kinds.count(k) for k in ("regular", "fallback", "single")) >= 16
    assert set(int(k) for k in FX["init.joints.seg_kind"]) == set(range(7)) and (FX["init.joints.m2q_hits"] > 0).sum() >= 3
    low = 0.1 * 9.81
    acc = np.abs(FX["init.joints.imu"][:, 3:])
    for k, want in (("fallback", 0), ("single", 1)):
        assert ((acc[..., np.array(kinds) == k] >= low).sum((0, 1)) == want).all()
    modes, ratios, rpys = set(), set(), set()
    for name in BODY_CASES:
        c = _body_case(name)
        modes.add(int(c["twist_mode"]))
        rpys.add(int(c["compute_rpy"]))
        if int(c["twist_mode"]) == 2:
            ratios.add(float(c["dt"]) * float(c["time_constant_inv"]) > 1.0)
        assert np.abs(c["rel_quat"][:, 3]).max() < 0.9                                     # mounting rotations of more than 0.9 rad
    assert modes == {0, 1, 2} and ratios == {False, True} and rpys == {0, 1}


@pytest.mark.parametrize("name", MAHONY_CASES)
def test_emulated_mahony_float64_matches_the_reference(name):
    c = _mahony_case(name)
    bounds, ref_errs = _mahony_bounds(name, c, np.float64)
    errs = _errors(run_mahony(emu_mahony_tick(c), c, np.float64), c)
    print(f"{name}: kernel {errs} | numpy restatement {ref_errs}")
    assert all(errs[k] <= bounds[k] for k in errs), (name, errs, bounds)


@pytest.mark.parametrize("name", MAHONY_CASES)
def test_emulated_mahony_float32_within_the_measured_bound(name):
    c = _mahony_case(name)
    bounds, ref_errs = _mahony_bounds(name, c, np.float32)
    errs = _errors(run_mahony(emu_mahony_tick(c), c, np.float32), c)
    print(f"{name}: kernel float32 {errs} | numpy float32 {ref_errs}")
    assert all(errs[k] <= bounds[k] for k in errs), (name, errs, bounds)
    if name == "n3_singular":
        _check_float32_on_upright_pairs(emu_mahony_tick(c), c, "kernel")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", BODY_CASES)
def test_emulated_body_observer_matches_the_reference(name, dtype):
    c = _body_case(name)
    bounds, ref_errs = _body_bounds(c, dtype)
    errs = _errors(run_body(emu_body_tick(c), c, dtype), c)
    print(f"{name} {np.dtype(dtype).name}: kernel {errs} | numpy restatement {ref_errs}")
    assert all(errs[k] <= bounds[k] for k in errs), (name, errs, bounds)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("exact_init", [True, False])
def test_emulated_initialisation_matches_the_reference(exact_init, dtype):
    got = _check_init(run_init(emu_init_call(), exact_init, dtype), exact_init, _init_bounds(exact_init, dtype))
    print(f"init exact={exact_init} {np.dtype(dtype).name}: {got}")


def test_emulated_initialisation_leaves_unmasked_lanes_alone():
    mask = (np.arange(64) % 2).astype(np.uint8)
    state = run_init(emu_init_call(), False, np.float64, mask=mask, prefill=7.25)
    _check_init(state, False, _init_bounds(False, np.float64), where=mask.astype(bool))
    for k, v in state.items():
        assert (v[..., ~mask.astype(bool)] == 7.25).all(), k


# ------------------------------------------------------------------------------------ exact initialisation on real models
def world_rotations(model, q: np.ndarray) -> np.ndarray:
    """World rotation of every joint frame for the configurations q `[nq][B]`, coded here on the compiled model's own arrays
    (independent of the plan and of the kernel): `[njoints][B][3][3]`."""
    Bn = q.shape[1]
    out = [np.tile(np.eye(3), (Bn, 1, 1))]
    for j in range(1, model.njoints):
        t, iq = int(model.jtypes[j]), int(model.idx_q[j])
        R = out[int(model.parents[j])] @ np.asarray(model.placement_R[j], dtype=np.float64)
        a = np.asarray(model.axes[j], dtype=np.float64)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        if JT_RX <= t <= JT_RU or JT_RUBX <= t <= JT_RUBU:
            c, s = (np.cos(q[iq]), np.sin(q[iq])) if t <= JT_RU else (q[iq], q[iq + 1])
            R = R @ (c[:, None, None] * np.eye(3) + s[:, None, None] * K + (1 - c)[:, None, None] * np.outer(a, a))
        elif t in (JT_SPHERICAL, JT_FREEFLYER):
            x, y, z, w = q[iq + (3 if t == JT_FREEFLYER else 0):][:4]
            R = R @ np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                              [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                              [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
        else:
            assert JT_PX <= t <= JT_PU, t
        out.append(R)
    return np.array(out)


def imu_rotations(model, q: np.ndarray) -> np.ndarray:
    """`[n_imu][3][3][B]`"""
    Rj = world_rotations(model, q)
    return np.array([(Rj[int(model.frame(s["frame"]).parent_joint)] @ np.asarray(model.frame(s["frame"]).R)).transpose(1, 2, 0)
                     for s in model.sensors["ImuSensor"]])


def random_configurations(model, Bn: int, seed: int, max_tilt: float = 3.0) -> np.ndarray:
    rg = np.random.default_rng(seed)
    q = np.zeros((model.nq, Bn))
    for j in range(1, model.njoints):
        t, iq = int(model.jtypes[j]), int(model.idx_q[j])
        if t in (JT_SPHERICAL, JT_FREEFLYER):
            o = iq + (3 if t == JT_FREEFLYER else 0)
            axis = rg.normal(size=(3, Bn))
            axis /= np.linalg.norm(axis, axis=0)
            angle = rg.uniform(-0.5, 0.5, Bn) if t == JT_SPHERICAL else rg.uniform(-max_tilt, max_tilt, Bn)
            q[o:o + 3], q[o + 3] = axis * np.sin(angle / 2), np.cos(angle / 2)
            if t == JT_FREEFLYER:
                q[iq:iq + 3] = rg.normal(size=(3, Bn))
        elif JT_RUBX <= t <= JT_RUBU:
            a = rg.uniform(-np.pi, np.pi, Bn)
            q[iq], q[iq + 1] = np.cos(a), np.sin(a)
        else:
            q[iq] = rg.uniform(-1.0, 1.0, Bn)
    return q


def unbounded_tree():
    """A tree of tests/robots.py with an unbounded revolute joint and an IMU behind it; where none of them carries such a
    sensor, one is attached here to the first frame found behind the joint."""
    for make in (lambda: robots.tree_arm(False), lambda: robots.tree_arm(True), robots.crane_walker):
        model = make()
        unbounded = [j for j in range(1, model.njoints) if JT_RUBX <= int(model.jtypes[j]) <= JT_RUBU]
        if not unbounded:
            continue

        def behind(j: int) -> bool:
            while j != 0:
                if j in unbounded:
                    return True
                j = int(model.parents[j])
            return False
        if not any(behind(int(model.frame(s["frame"]).parent_joint)) for s in model.sensors.get("ImuSensor", [])):
            name = next(n for n, f in model.frames.items() if behind(int(f.parent_joint)))
            add_sensor(model, "ImuSensor", "imu_behind_unbounded", frame_name=name)
        return model
    return rd.flex_arm(False, continuous_elbow=True)        # (authored for the deformation tests: imu4, imu5 behind the elbow)


MODELS = {"flex_arm": lambda: rd.flex_arm(False), "flex_arm_ff": lambda: rd.flex_arm(True), "anymal": lambda: load_builtin("anymal"),
          "unbounded": unbounded_tree, "flex_arm_continuous": lambda: rd.flex_arm(False, continuous_elbow=True)}


def _emu_model_init(model, q, imu, exact_init):
    plan = attitude.build_plan(model)
    desc, keep = plan.desc()
    n, Bn = plan.n_imu, q.shape[1]
    st = [np.full((4, n, Bn), np.nan), *[np.full((3, n, Bn), np.nan) for _ in range(3)], np.full((n, Bn), np.nan), np.full((3, n, Bn), np.nan)]
    emu.init(desc, q, imu, exact_init, *st)
    return plan, st[0], st[5]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_exact_initialisation_is_the_forward_kinematics_of_the_model(name):
    """Quaternions of a product of up to nine rotations; `matrices_to_quat` divides by 2 sqrt(t) with t >= 1: 1e-14 is forty
    roundings.  Measured: 3.3e-16 at most."""
    model = MODELS[name]()
    if name in ("unbounded", "flex_arm_continuous"):
        assert any(JT_RUBX <= int(t) <= JT_RUBU for t in model.jtypes)
    q = random_configurations(model, 128, seed=5)
    n = len(model.sensors["ImuSensor"])
    plan, quat, rpy = _emu_model_init(model, q, np.zeros((n, 6, 128)), True)
    R = imu_rotations(model, q)
    want = np.stack([dn.rot_to_quat(R[s]) for s in range(n)], 1)
    err = float(np.minimum(np.abs(quat - want).max(0), np.abs(quat + want).max(0)).max())
    print(f"{name}: {n} IMUs, segment kinds {sorted(set(int(k) for k in plan.arrays['seg_kind']))}, error {err:.2e}")
    assert err <= 1e-14
    assert _err(rpy, an.rpy_of(quat)) <= TOL
    # the relative rotations are those of the sensor frames, by the reference's branch rule
    for s, sensor in enumerate(model.sensors["ImuSensor"]):
        Rf = np.asarray(model.frame(sensor["frame"]).R, dtype=np.float64)
        assert np.abs(dn.quat_to_rot(plan.rel_quat[s][:, None])[:, :, 0] - Rf).max() <= 1e-15


def test_accelerometer_initialisation_is_the_exact_one_without_twist():
    """A robot at rest reads `R^T (0, 0, 9.81)`: the swing of that vector is the exact quaternion with its twist removed, to
    1e-13 on every non-singular lane (every IMU with v_z >= -1 + 1e-5): all 256 of this draw, none left out.

    The two sides evaluate the same tilt v along two paths (`matrices_to_quat` of R, then `compute_tilt_from_quat`; the last
    row of R times 9.81, normalised), so the tilts differ by roundings.  The regular branch of `swing_from_vector`,
    (v_y, -v_x, 0, 1 + v_z) / sqrt(2 (1 + v_z)), turns a tilt error d into d (1 / (2 u) + 1 / sqrt(2 u)) on the quaternion,
    u = 1 + v_z.  The smallest u of the draw is 7.6e-4 (amplification 680): one ulp of v_z there (1.1e-16) moves the quaternion
    by 7.5e-14: the bar holds there only while the two tilts agree to the last bit or so, which they do on this
    seeded draw (1 + v_z adds no rounding of its own: the sum is exact for v_z in [-1, -0.5]).  Measured: worst lane 8.5e-15 (the one
    with u = 7.6e-4), 1.7e-15 at most on the 230 lanes with u >= 0.05."""
    model = rd.flex_arm(True)
    B = 256
    q = random_configurations(model, B, seed=9)
    n = len(model.sensors["ImuSensor"])
    R = imu_rotations(model, q)
    imu = np.zeros((n, 6, B))
    imu[:, 3:] = 9.81 * R[:, 2]                                       # R^T e_z: the last row of R
    _, exact, _ = _emu_model_init(model, q, imu, True)
    _, acc, _ = _emu_model_init(model, q, imu, False)
    u = (1.0 + R[:, 2, 2]).min(0)                                     # the smallest 1 + v_z of the lane
    assert (u >= 1e-5).all() and u.min() < 1e-3, "every lane of the draw is non-singular, and some are close to the branch"
    err = np.abs(acc - an.remove_twist(exact)).max((0, 1))
    worst = int(np.argmax(err))
    print(f"swing of the exact quaternion vs accelerometer initialisation, {B} of {B} lanes: worst error {err[worst]:.2e} (u = {u[worst]:.2e}), "
          f"smallest u {u.min():.2e}; {err[u >= 0.05].max():.2e} on the {int((u >= 0.05).sum())} lanes with u >= 0.05")
    assert np.isfinite(err).all() and err.max() <= TOL, (err[worst], u[worst])


def test_build_plan_gains_and_errors():
    model = rd.flex_arm(True)
    n = len(model.sensors["ImuSensor"])
    plan = attitude.build_plan(model, kp=2.0, ki=[0.1, 0.2, 0.3, 0.4, 0.5])
    assert plan.kp.tolist() == [2.0] * n and plan.ki.tolist() == [0.1, 0.2, 0.3, 0.4, 0.5]
    assert plan.imu_names == [s["name"] for s in model.sensors["ImuSensor"]]
    with pytest.raises(ValueError):
        attitude.build_plan(model, kp=[1.0, 2.0])
    with pytest.raises(ValueError):
        attitude.build_plan(load_builtin("cartpole"))


# --------------------------------------------------------------------------------------------------------- provenance
def test_fixture_generator_is_committed_and_names_the_reference_functions():
    text = open(TOOL).read()
    for name in ("mahony_filter", "update_twist", "compute_tilt_from_quat", "swing_from_vector", "remove_twist_from_quat",
                 "quat_to_rpy", "quat_multiply", "quat_apply", "matrices_to_quat", "blocks/mahony_filter.py",
                 "blocks/body_orientation_observer.py", "utils/math.py"):
        assert f'"{name}"' in text, name
    assert "def mahony_filter" not in text and "def swing_from_vector" not in text and "def update_twist" not in text
    assert "ast.parse" in text


def test_fixture_regenerates_from_the_reference_tree(tmp_path):
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        return      # (nothing to compare with where the reference tree is absent; the committed fixture stands)
    out = tmp_path / "ref_attitude.npz"
    subprocess.check_call([sys.executable, TOOL, str(out)], stdout=subprocess.DEVNULL)
    assert open(out, "rb").read() == open(FIXTURE, "rb").read()


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_version_and_new_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    assert "typedef struct jm_attitude_desc" in header


def _prebuilt(model):
    path = codegen.lib_path(model)
    if not os.path.exists(path):
        pytest.skip(f"{os.path.basename(path)} not built (run __graft_entry__.build())")
    return _lib.load_for(model, allow_build=False)


def _last_error(lib) -> str:
    buf = C.create_string_buffer(1024)
    lib.L.jm_last_error(buf, 1024)
    return buf.value.decode()


def test_plan_create_validates_the_description_before_touching_the_device():
    lib = _prebuilt(load_builtin("cartpole"))
    good = _init_arrays()
    h = C.c_void_p()
    assert lib.L.jm_attitude_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = attitude.make_desc(**good)
    assert lib.L.jm_attitude_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.seg_rot = None
    assert lib.L.jm_attitude_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)

    def broken(**change):
        arrays = {k: np.array(v) for k, v in good.items()}
        for k, f in change.items():
            arrays[k] = f(arrays[k])
        arrays["nq"] = int(arrays["nq"])
        d, keep_ = attitude.make_desc(**arrays)
        rc = lib.L.jm_attitude_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value
        with pytest.raises(ValueError):
            lib.check(rc)
        return _last_error(lib), d, keep_

    def set_at(index, value):
        def f(a):
            a = a.copy()
            a.reshape(-1)[index] = value
            return a
        return f
    kinds = good["seg_kind"]
    quat_seg, unb_seg, rev_seg = (int(np.flatnonzero(kinds == k)[0]) for k in (6, 5, 1))
    assert "unknown joint kind" in broken(seg_kind=set_at(0, 7))[0]
    assert "unknown joint kind" in broken(seg_kind=set_at(1, -1))[0]
    assert "reads q rows [14, 18) out of range [0, 17)" in broken(seg_q_index=set_at(quat_seg, 14))[0]
    assert "reads q rows [16, 18) out of range" in broken(seg_q_index=set_at(unb_seg, 16))[0]
    assert "reads q rows [-1, 0) out of range" in broken(seg_q_index=set_at(rev_seg, -1))[0]
    assert "out of range [0, 4)" in broken(nq=lambda a: np.array(4))[0]
    assert "frame_seg_start" in broken(frame_seg_start=set_at(-1, 3))[0]
    assert "bad segment count" in broken(frame_seg_start=set_at(1, 0))[0]
    assert "not a unit quaternion" in broken(rel_quat=set_at(3, 0.5))[0]
    assert "not finite" in broken(kp=set_at(1, np.nan))[0]
    assert "bad sizes" in broken(kp=lambda a: a[:0], ki=lambda a: a[:0], rel_quat=lambda a: a[:0])[0]
    assert lib.L.jm_attitude_plan_destroy(None) == _abi.JM_OK
    # the calls themselves check their arguments first as well
    assert lib.L.jm_block_attitude_init(None, _abi.JM_F64, 4, None, None, None, 1, None, None, None, None, None, None, None) == _abi.JM_EINVAL
    assert lib.L.jm_block_mahony_observer(None, _abi.JM_F64, 4, None, None, None, None, None, 0.005, 0, None, None) == _abi.JM_EINVAL
    assert lib.L.jm_block_body_observer(None, _abi.JM_F64, 4, None, None, None, None, None, 0, 0.0, 0.005, None, None) == _abi.JM_EINVAL
    # the host emulation runs the same check
    _, d, keep3 = broken(seg_q_index=set_at(quat_seg, 14))
    with pytest.raises(ValueError, match="out of range"):
        run_init(lambda q, imu, mask, exact, *st: emu.init(d, q, imu, exact, *st), True, np.float64)


# ================================================================================================================ GPU
class DevicePlan:
    """A plan on the device and the three calls on numpy arrays (copied in and out: the ticks of a case are few)."""

    def __init__(self, lib, arrays: dict, device):
        import torch
        self.torch, self.lib, self.device = torch, lib, device
        desc, keep = attitude.make_desc(**arrays)
        self.h = C.c_void_p()
        with torch.cuda.device(device):
            lib.check(lib.L.jm_attitude_plan_create(C.byref(desc), C.byref(self.h)))

    def close(self):
        self.lib.L.jm_attitude_plan_destroy(self.h)

    def _run(self, call, arrays, outputs):
        torch = self.torch
        ts = [None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=self.device).contiguous() for a in arrays]
        ptr = [None if t is None else C.c_void_p(t.data_ptr()) for t in ts]
        self.lib.check(call(ptr, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        for i in outputs:
            if arrays[i] is not None:
                arrays[i][...] = ts[i].cpu().numpy()

    @staticmethod
    def _code(a):
        return _abi.JM_F64 if a.dtype == np.float64 else _abi.JM_F32

    def mahony(self, imu, quat, omega, cf, bias, dt, ignore_twist, rpy):
        L, h, Bn = self.lib.L, self.h, quat.shape[-1]
        self._run(lambda p, s: L.jm_block_mahony_observer(h, self._code(quat), Bn, p[0], p[1], p[2], p[3], p[4], float(dt),
                                                          int(ignore_twist), p[5], s),
                  [imu.astype(quat.dtype), quat, omega, cf, bias, rpy], (1, 2, 3, 4, 5))

    def body(self, iq, io, quat, omega, twist, mode, tci, dt, rpy):
        L, h, Bn = self.lib.L, self.h, quat.shape[-1]
        self._run(lambda p, s: L.jm_block_body_observer(h, self._code(quat), Bn, p[0], p[1], p[2], p[3], p[4], int(mode), float(tci),
                                                        float(dt), p[5], s),
                  [iq.astype(quat.dtype), io.astype(quat.dtype), quat, omega, twist, rpy], (2, 3, 4, 5))

    def init(self, q, imu, mask, exact_init, quat, omega, cf, bias, twist, rpy):
        L, h, Bn = self.lib.L, self.h, quat.shape[-1]
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._run(lambda p, s: L.jm_block_attitude_init(h, self._code(quat), Bn, p[0], p[1], p[2], int(exact_init), p[3], p[4], p[5],
                                                        p[6], p[7], p[8], s),
                  [q, imu, m, quat, omega, cf, bias, twist, rpy], (3, 4, 5, 6, 7, 8))


def _device_mahony_tick(plan: DevicePlan, c: dict):
    def tick(imu, quat, omega, cf, bias, rpy):
        plan.mahony(imu, quat, omega, cf, bias, float(c["dt"]), bool(c["ignore_twist"]), rpy)
    return tick


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAHONY_CASES)
def test_device_mahony_observer_matches_the_reference(name, gpu_device):
    lib = _prebuilt(load_builtin("cartpole"))
    c = _mahony_case(name)
    plan = DevicePlan(lib, _plain_arrays(int(c["n_imu"]), c["kp"], c["ki"]), gpu_device)
    try:
        for dtype in (np.float64, np.float32):
            bounds, ref_errs = _mahony_bounds(name, c, dtype)
            errs = _errors(run_mahony(_device_mahony_tick(plan, c), c, dtype), c)
            print(f"{name} {np.dtype(dtype).name}: device {errs} | numpy restatement {ref_errs}")
            assert all(errs[k] <= bounds[k] for k in errs), (name, errs, bounds)
        if name == "n3_singular":
            _check_float32_on_upright_pairs(_device_mahony_tick(plan, c), c, "device")
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", BODY_CASES)
def test_device_body_observer_matches_the_reference(name, gpu_device):
    lib = _prebuilt(load_builtin("cartpole"))
    c = _body_case(name)
    plan = DevicePlan(lib, _plain_arrays(int(c["n_imu"]), rel_quat=c["rel_quat"]), gpu_device)

    def tick(iq, io, quat, omega, twist, rpy):
        plan.body(iq, io, quat, omega, twist, int(c["twist_mode"]), float(c["time_constant_inv"]), float(c["dt"]), rpy)
    try:
        for dtype in (np.float64, np.float32):
            bounds, ref_errs = _body_bounds(c, dtype)
            errs = _errors(run_body(tick, c, dtype), c)
            print(f"{name} {np.dtype(dtype).name}: device {errs} | numpy restatement {ref_errs}")
            assert all(errs[k] <= bounds[k] for k in errs), (name, errs, bounds)
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("exact_init", [True, False])
def test_device_initialisation_matches_the_reference(exact_init, gpu_device):
    lib = _prebuilt(load_builtin("cartpole"))
    plan = DevicePlan(lib, _init_arrays(), gpu_device)
    try:
        for dtype in (np.float64, np.float32):
            got = _check_init(run_init(plan.init, exact_init, dtype), exact_init, _init_bounds(exact_init, dtype))
            print(f"init exact={exact_init} {np.dtype(dtype).name}: device {got}")
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("Bn", [67, 257])
def test_device_partial_wave_and_second_block(Bn, gpu_device):
    """One case of each kernel replicated to a batch with a partial wave (67) and a second block (257): every lane compared."""
    lib = _prebuilt(load_builtin("cartpole"))
    lanes = np.arange(Bn) % 64
    c = _mahony_case("n3_singular")
    plan = DevicePlan(lib, _plain_arrays(int(c["n_imu"]), c["kp"], c["ki"]), gpu_device)
    try:
        bounds, _ = _mahony_bounds("n3_singular", c, np.float64)
        errs = _errors(run_mahony(_device_mahony_tick(plan, c), c, np.float64, lanes), c, lanes)
        assert all(errs[k] <= bounds[k] for k in errs), (errs, bounds)
    finally:
        plan.close()
    c = _body_case("leak_rpy")
    plan = DevicePlan(lib, _plain_arrays(int(c["n_imu"]), rel_quat=c["rel_quat"]), gpu_device)
    try:
        bounds, _ = _body_bounds(c, np.float64)
        errs = _errors(run_body(lambda iq, io, quat, omega, twist, rpy: plan.body(
            iq, io, quat, omega, twist, int(c["twist_mode"]), float(c["time_constant_inv"]), float(c["dt"]), rpy), c, np.float64, lanes), c, lanes)
        assert all(errs[k] <= bounds[k] for k in errs), (errs, bounds)
    finally:
        plan.close()
    plan = DevicePlan(lib, _init_arrays(), gpu_device)
    try:
        for exact_init in (True, False):
            _check_init(run_init(plan.init, exact_init, np.float64, lanes), exact_init, _init_bounds(exact_init, np.float64), lanes)
    finally:
        plan.close()


@pytest.mark.gpu
def test_device_initialisation_mask(gpu_device):
    """B = 130, every second lane masked: masked lanes equal the fixture, the others keep the bits of all six outputs."""
    lib = _prebuilt(load_builtin("cartpole"))
    lanes = np.arange(130) % 64
    mask = (np.arange(130) % 2 == 1)
    plan = DevicePlan(lib, _init_arrays(), gpu_device)
    try:
        for exact_init in (True, False):
            state = run_init(plan.init, exact_init, np.float64, lanes, mask=mask, prefill=-3.5)
            _check_init(state, exact_init, _init_bounds(exact_init, np.float64), lanes, where=mask)
            assert sorted(state) == ["bias", "cf", "omega", "quat", "rpy", "twist"]
            for k, v in state.items():
                assert (v[..., ~mask] == -3.5).all(), k
    finally:
        plan.close()


def _counting_library(monkeypatch, lib):
    """Count the calls of every entry point of a loaded library (the launches an environment step issues)."""
    counts = {}

    class Proxy:
        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            f = getattr(self._L, name)

            def call(*a):
                counts[name] = counts.get(name, 0) + 1
                return f(*a)
            return call
    monkeypatch.setattr(lib, "L", Proxy(lib.L))
    return counts


def _features(obs) -> dict:
    out = {}
    for block in ("mahony_filter", "body_observer"):
        for k, v in obs["features"][block].items():
            out[f"{block}.{k}"] = v.permute(1, 2, 0).cpu().numpy()      # back to [rows][n_imu][B]
    return out


@pytest.mark.gpu
def test_environment_with_both_blocks(gpu_device, monkeypatch):
    """ANYmal, 64 environments, `MahonyFilter(ignore_twist, compute_rpy, exact_init)` -> `BodyObserver(twist_time_constant=0.5)`.
    The features follow the numpy restatement driven by the engine's own IMU rows tick by tick (1e-12: 24 ticks of a filter
    whose every tick agrees to 1e-15; a wrong order, gain or frame shows at 1e-3); a partial reset re-initialises its lanes
    and leaves the others bit for bit; eager and graph replay agree bit for bit."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    B = 64
    cfg = dict(mahony_filter=dict(ignore_twist=True, compute_rpy=True, exact_init=True), body_observer=dict(twist_time_constant=0.5))
    model = load_builtin("anymal")
    counts = _counting_library(monkeypatch, _lib.load_for(model))
    eager = make_anymal_env(B, device=gpu_device, auto_reset=False, **cfg)
    graphed = make_anymal_env(B, device=gpu_device, auto_reset=False, **cfg)
    graphed.enable_graph()
    with pytest.raises(NotImplementedError):
        make_anymal_env(B, device=gpu_device, **cfg).enable_graph(whole_step=True)
    with pytest.raises(NotImplementedError, match="update_ratio"):
        make_anymal_env(B, device=gpu_device, mahony_filter=dict(update_ratio=2))
    plan = eager._mahony.plan
    assert plan.n_imu == 1 and eager._body.fieldnames["omega"][2] == [plan.imu_names[0] + ".Z"]
    imu_log = []
    refresh = eager._mahony.refresh

    def logged(dt):
        imu_log.append(eager.engine.field("imu").clone())
        refresh(dt)
    monkeypatch.setattr(eager._mahony, "refresh", logged)

    def numpy_init(lanes=slice(None)):
        q = eager.engine.robot_state.q.cpu().numpy()
        imu = eager.engine.field("imu").cpu().numpy().reshape(1, 6, B)
        quat, _ = an.init(plan.arrays, q[:, lanes], imu[..., lanes], True)
        bq, bo, _ = an.body_tick(quat, np.zeros((3, 1, quat.shape[-1])), plan.rel_quat, np.zeros((1, quat.shape[-1])), 1, 0.0, 0.0)
        return quat, bq, bo

    def compare(obs, st, lanes=slice(None), tol=1e-12):
        got = _features(obs)
        want = {"mahony_filter.quat": st["quat"], "mahony_filter.omega": st["omega"], "mahony_filter.rpy": an.rpy_of(st["quat"]),
                "body_observer.quat": st["bquat"], "body_observer.omega": st["bomega"], "body_observer.rpy": an.rpy_of(st["bquat"])}
        assert sorted(got) == sorted(want)
        errs = {k: _err(got[k][..., lanes], want[k][..., lanes]) for k in want}
        assert max(errs.values()) <= tol, errs
        return max(errs.values())

    obs_e, _ = eager.reset(seed=3)
    obs_g, _ = graphed.reset(seed=3)
    quat, bquat, bomega = numpy_init()
    st = dict(quat=quat, bias=np.zeros((3, 1, B)), omega=np.zeros((3, 1, B)), twist=np.zeros((1, B)), bquat=bquat, bomega=bomega)
    worst = compare(obs_e, st)
    assert sorted(obs_e["features"]["mahony_filter"]) == ["omega", "quat", "rpy"]
    assert tuple(obs_e["features"]["body_observer"]["quat"].shape) == (B, 4, 1)
    dt = eager.control_dt
    g = torch.Generator(device="cpu").manual_seed(1)

    def step_both(i):
        nonlocal worst
        action = (0.3 * torch.randn(B, model.nmotors, generator=g, dtype=torch.float64)).to(gpu_device)
        imu_log.clear()
        counts.clear()
        obs_e = eager.step(action)[0]
        n_eager = dict(counts)
        obs_g = graphed.step(action)[0]
        assert len(imu_log) == eager._n_ctrl
        for imu in imu_log:
            st["quat"], st["bias"], st["omega"], _ = an.mahony_tick(st["quat"], st["bias"], imu.cpu().numpy().reshape(1, 6, B),
                                                                    plan.kp, plan.ki, dt, True)
            st["bquat"], st["bomega"], st["twist"] = an.body_tick(st["quat"], st["omega"], plan.rel_quat, st["twist"], 2, 1.0 / 0.5, dt)
        worst = max(worst, compare(obs_e, st))
        fe, fg = _features(obs_e), _features(obs_g)
        for k in fe:
            assert np.array_equal(fe[k], fg[k]), (i, k)
        assert torch.equal(obs_e["states"]["agent"]["q"], obs_g["states"]["agent"]["q"])
        return n_eager
    for i in range(3):
        n_eager = step_both(i)
    assert n_eager["jm_block_mahony_observer"] == n_eager["jm_block_body_observer"] == eager._n_ctrl
    assert "jm_block_mahony_filter" not in n_eager and "jm_block_attitude_init" not in n_eager
    assert graphed._graph is not None
    assert float(np.abs(st["twist"]).max()) > 1e-6 and float(np.abs(st["bias"]).max()) > 0.0
    # partial reset of half the lanes
    mask = torch.zeros(B, dtype=torch.bool, device=gpu_device)
    mask[::2] = True
    before = _features(eager.observation())
    counts.clear()
    for e in (eager, graphed):
        e.reset_lanes(mask)
    assert counts["jm_block_attitude_init"] == 2
    after = _features(eager.observation())
    m = mask.cpu().numpy()
    for k in before:
        assert np.array_equal(after[k][..., ~m], before[k][..., ~m]), k
    quat, bquat, bomega = numpy_init(m)
    for k, fresh in (("quat", quat), ("bquat", bquat), ("bomega", bomega)):
        st[k] = st[k].copy()
        st[k][..., m] = fresh
    for k in ("bias", "omega", "twist"):
        st[k] = st[k].copy()
        st[k][..., m] = 0.0
    worst = max(worst, compare(eager.observation(), st))
    assert not bool(eager._body.twist[:, mask].any()) and not bool(eager._mahony.bias[:, :, mask].any())
    fe, fg = _features(eager.observation()), _features(graphed.observation())
    for k in fe:
        assert np.array_equal(fe[k], fg[k]), k
    step_both(3)
    print(f"environment features vs numpy restatement: {worst:.2e}")


@pytest.mark.gpu
def test_default_environment_is_unchanged(gpu_device, monkeypatch):
    """Without the new options: the launches and the observation keys of before, episodes start from the unit quaternion,
    none of the new exports is called -- and the blocks only observe: with them the other keys hold the same bits."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    B = 64
    model = load_builtin("anymal")
    counts = _counting_library(monkeypatch, _lib.load_for(model))
    plain = make_anymal_env(B, device=gpu_device, auto_reset=False)
    assert not any(name in counts for name in NEW_SYMBOLS)
    full = make_anymal_env(B, device=gpu_device, auto_reset=False, mahony_filter=dict(ignore_twist=True, compute_rpy=True),
                           body_observer=dict(twist_time_constant=0.5))
    counts.clear()
    obs, _ = plain.reset(seed=3)
    full.reset(seed=3)
    feat = obs["features"]
    assert sorted(feat) == ["mahony_filter"] and torch.is_tensor(feat["mahony_filter"])
    assert tuple(feat["mahony_filter"].shape) == (B, 4, 1)
    assert torch.equal(feat["mahony_filter"][:, 3], torch.ones_like(feat["mahony_filter"][:, 3])) and not bool(feat["mahony_filter"][:, :3].any())
    g = torch.Generator(device="cpu").manual_seed(1)
    for i in range(2):
        action = (0.3 * torch.randn(B, model.nmotors, generator=g, dtype=torch.float64)).to(gpu_device)
        counts.clear()
        obs = plain.step(action)[0]
        n_plain = dict(counts)
        other = full.step(action)[0]
        assert sorted(obs) == ["actions", "features", "measurements", "states", "t"] and sorted(obs["features"]) == ["mahony_filter"]
        assert torch.equal(obs["features"]["mahony_filter"], plain.imu_quat.permute(2, 0, 1))
        for k in ("q", "v"):
            assert torch.equal(obs["states"]["agent"][k], other["states"]["agent"][k])
        for k in obs["measurements"]:
            assert torch.equal(obs["measurements"][k], other["measurements"][k]), k
        assert torch.equal(obs["actions"]["pd_controller"], other["actions"]["pd_controller"]) and torch.equal(obs["t"], other["t"])
    assert n_plain["jm_block_mahony_filter"] == plain._n_ctrl and n_plain["jm_block_pd_controller"] == plain._n_ctrl
    assert n_plain["jm_block_pd_adapter"] == 1 and not any(name in n_plain for name in NEW_SYMBOLS)
    mask = torch.zeros(B, dtype=torch.bool, device=gpu_device)
    mask[::3] = True
    counts.clear()
    plain.reset_lanes(mask)
    assert not any(name in counts for name in NEW_SYMBOLS)
    assert torch.equal(plain.imu_quat[3][:, mask], torch.ones_like(plain.imu_quat[3][:, mask])) and not bool(plain.imu_quat[:3][:, :, mask].any())
