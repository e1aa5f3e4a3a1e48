"""Frame kinematics on the device (csrc/jm_frames.h behind `jm_block_frame_kinematics` / `jm_block_frame_average`,
`blocks.FrameKinematics`, the two terminations of `WalkerVecEnv`).

Two specifications:
* the step average is pinned to the reference's own output, tests/golden/ref_frames.npz (tools/make_ref_frames_fixtures.py
  executes the reference's functions): float64 within 1e-13 relative to max(|want|, 1) on every lane; on the `small_angle`
  case the positions of the mean pose within 1e-13 + 8 * 2.2e-16 * |t| / theta per lane, t the translation handed to `exp6`
  and theta its angle -- the conditioning of the reference's own (1 - cos theta) / theta^2: one rounding of cos theta is
  1.1e-16 absolute, the quotient multiplies a product of size theta |t|.  float32: 4 x the error of the numpy float32
  restatement (tests/frames_numpy.py) on the same case and quantity.
* the kinematics follow an independent float64 forward kinematics (4x4 transforms, Jacobian columns; tests/frames_numpy.py)
  within 64 * depth * 2.2e-16 * max(|want|, 1), depth the segment count of the frame (every segment a bounded number of
  multiply-adds), and a central difference of that pose at eps = 1e-6 within 1e-8 (truncation O(eps^2), rounding 2.2e-16 / eps).
  The configurations are drawn so that the pitch of every frame keeps 0.1 rad from +-pi/2, where Euler angles lose
  1 / cos(pitch) digits; angles are compared modulo 2 pi and quaternions up to their sign.

Measured, step average (error relative to max(|want|, 1), largest over the steps and lanes; `small_angle` positions in units of
their own bound scaled to 1e-13):
  float64, host emulation | device (the numpy restatement gives the figures of the emulation bit for bit)
    regular      v_avg 6.5e-15 | 6.5e-15   pose_mean 2.2e-16 | 2.2e-16   quat_no_yaw 7.8e-16 | 7.8e-16
    rest         v_avg 2.3e-14 | 2.3e-14   pose_mean 2.2e-16 | 2.2e-16   quat_no_yaw 4.6e-15 | 4.6e-15
    small_angle  v_avg 2.7e-15 | 2.7e-15   pose_mean 1.1e-16 | 1.1e-16   quat_no_yaw 7.4e-16 | 7.4e-16
    K1           v_avg 3.1e-15 | 3.4e-15   pose_mean 1.9e-16 | 2.2e-16   quat_no_yaw 1.2e-15 | 1.2e-15
    (with the products of `remove_yaw_from_quat` fused into their sums the device gave v_avg 4.9e-14 on `regular` and
    1.6e-13 on `small_angle`, quat_no_yaw 2.4e-14: jm_frames.h rounds them one by one.)
  float32, numpy restatement | host emulation | device (the error is that of rounding the poses to float32)
    regular      v_avg 7.23e-5 | 7.24e-5 | 7.24e-5   pose_mean 5.9e-7 | 5.9e-7 | 6.1e-7   quat_no_yaw 3.6e-5 | 3.6e-5 | 3.6e-5
    rest         v_avg 1.91e-5 | 1.91e-5 | 1.91e-5   pose_mean 7.8e-7 | 7.8e-7 | 8.9e-7   quat_no_yaw 7.7e-5 | 7.7e-5 | 7.7e-5
    small_angle  v_avg 3.09e-5 | 3.09e-5 | 3.09e-5   pose_mean 8.9e-8 | 8.9e-8 | 8.9e-8   quat_no_yaw 6.6e-6 | 6.6e-6 | 6.6e-6
    K1           v_avg 4.55e-6 | 4.55e-6 | 4.61e-6   pose_mean 5.1e-7 | 5.1e-7 | 4.3e-7   quat_no_yaw 3.0e-5 | 3.0e-5 | 3.0e-5
Measured, kinematics (largest error in units of the bound): host emulation 0.032 (float64), device 0.11 (float64, the Euler
angles of ANYmal) and 0.073 (float32); velocity against the central difference 5.4e-10 at most; IMU gyroscope against the LOCAL
angular velocity of the block 7.2e-16; environment, step average against the restatement 6.7e-16.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, attitude, codegen, deformation, frames, load_builtin
from jiminy_amd.model import JT_FREEFLYER, JT_RUBU, JT_RUBX, JT_SPHERICAL
from tests import frames_numpy as fn
from tests import robots
from tests import robots_deformation as rd
from tests.hostemu import frames as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_frames.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_frames_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
TOL = 1e-13
EPS = 2.2e-16
NEW_SYMBOLS = ("jm_frames_plan_create", "jm_frames_plan_destroy", "jm_block_frame_kinematics", "jm_block_frame_average")
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["cases"]]
OUTPUTS = ("v_avg", "pose_mean", "quat_no_yaw")


def _rel(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    assert got.shape == want.shape and np.isfinite(got).all(), (got.shape, want.shape)
    return np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)


# ------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_from_the_reference_tree():
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        pytest.skip("the reference tree is not here: the committed fixture stands")
    subprocess.check_call([sys.executable, TOOL, "--check"], stdout=subprocess.DEVNULL)
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_attitude.npz"))
    assert all(FX[f"{c}.pose"].shape[-1] == 64 and FX[f"{c}.pose"].shape[0] == 4 for c in CASES)
    assert list(FX["regular.modes"]) == [0, 1, 2] and FX["K1.pose"].shape[2] == 1 and FX["rest.rest"][::2].all()


def _case(name: str) -> dict:
    return {k[len(name) + 1:]: FX[k] for k in FX.files if k.startswith(name + ".")}


def _plain_arrays(modes) -> dict:
    """A description whose frames are one constant segment each: what the average, which reads the modes alone, needs."""
    K = len(modes)
    return dict(nq=0, nv=0, njoints=1, frame_seg_start=np.arange(K + 1), frame_mode=np.asarray(modes), seg_kind=np.zeros(K, int),
                seg_joint=-np.ones(K, int), seg_q_index=-np.ones(K, int), seg_v_index=-np.ones(K, int),
                seg_rot=np.tile(np.eye(3).reshape(-1), (K, 1)), seg_trans=np.zeros((K, 3)), seg_axis=np.zeros((K, 3)))


def run_average(step, c: dict, dtype, lanes=slice(None)) -> dict:
    """The three steps of a case through `step(pose_prev, pose, inv_step_dt, v_avg, pose_mean, quat_no_yaw)`, the previous
    pose carried by the callee: `[3][rows][K][B]` per output."""
    pose = np.ascontiguousarray(c["pose"][..., lanes]).astype(dtype)
    prev = pose[0].copy()
    K, Bn = pose.shape[2:]
    out = {k: [] for k in OUTPUTS}
    for t in range(3):
        bufs = [np.full((rows, K, Bn), np.nan, dtype=dtype) for rows in (6, 7, 4)]
        step(prev, pose[t + 1].copy(), float(c["inv_step_dt"]), *bufs)
        assert np.array_equal(prev, pose[t + 1]), "the pose must become the previous pose"
        for k, b in zip(OUTPUTS, bufs):
            out[k].append(b)
    return {k: np.stack(v) for k, v in out.items()}


def numpy_step(modes):
    def step(prev, pose, inv_dt, v_avg, pose_mean, quat_no_yaw):
        got = fn.average_step(prev, pose, inv_dt, modes)
        v_avg[...], pose_mean[...], quat_no_yaw[...] = got["v_avg"], got["pose_mean"], got["quat_no_yaw"]
        prev[...] = pose
    return step


def emu_step(modes):
    desc, keep = frames.make_desc(**_plain_arrays(modes))

    def step(prev, pose, inv_dt, v_avg, pose_mean, quat_no_yaw):
        assert keep
        emu.average(desc, prev, pose, inv_dt, v_avg, pose_mean, quat_no_yaw)
    return step


def small_angle_bound(c: dict, lanes=slice(None)) -> np.ndarray:
    """`[3][1][K][B]`: 1e-13 + 8 * 2.2e-16 * |t| / theta of the `exp6` of every step, frame and lane, from the fixture's poses."""
    pose = c["pose"][..., lanes]
    out = []
    for t in range(3):
        diff = fn.average_step(pose[t], pose[t + 1], 1.0, [0] * pose.shape[2])["diff"]
        tn, th = 0.5 * np.linalg.norm(diff[:3], axis=0), 0.5 * np.linalg.norm(diff[3:], axis=0)
        out.append((TOL + 8 * EPS * tn / th)[None])
    return np.stack(out)


def average_errors(got: dict, c: dict, name: str, lanes=slice(None)) -> dict:
    """Largest error of every output relative to max(|want|, 1); on `small_angle` the positions of the mean pose are
    measured in units of their own bound, scaled to 1e-13."""
    errs = {}
    for k in OUTPUTS:
        e = _rel(got[k], c[k][..., lanes])
        if name == "small_angle" and k == "pose_mean":
            pos = np.abs(got[k][:, :3].astype(np.float64) - c[k][..., lanes][:, :3]) / small_angle_bound(c, lanes) * TOL
            e = np.concatenate([pos, e[:, 3:]], 1)
        errs[k] = float(e.max())
    return errs


def check_rest_lanes(got: dict, c: dict, dtype, lanes=slice(None)) -> None:
    """Two identical poses: a zero difference (so a zero velocity) exactly, an unchanged mean pose, a finite `quat_no_yaw`."""
    rest = c["rest"][lanes]
    assert rest.any()
    pose = c["pose"][..., lanes].astype(dtype)
    assert (got["v_avg"][..., rest] == 0.0).all()
    assert np.array_equal(got["pose_mean"][..., rest], pose[1:][..., rest])
    assert np.isfinite(got["quat_no_yaw"][..., rest]).all()


def average_bounds(name: str, c: dict, dtype):
    """float64: the fixture's 1e-13; float32: 4 x the error of the numpy float32 restatement on the same case and quantity."""
    if dtype == np.float64:
        return {k: TOL for k in OUTPUTS}, None
    ref = average_errors(run_average(numpy_step(c["modes"]), c, np.float32), c, name)
    return {k: 4.0 * v for k, v in ref.items()}, ref


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_of_the_average_matches_the_reference(name, dtype):
    c = _case(name)
    got = run_average(numpy_step(c["modes"]), c, dtype)
    errs = average_errors(got, c, name)
    print(f"{name} {np.dtype(dtype).name}: numpy restatement {errs}")
    if dtype == np.float64:
        assert all(v <= TOL for v in errs.values()), errs
    if name == "rest":
        check_rest_lanes(got, c, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CASES)
def test_emulated_average_matches_the_reference(name, dtype):
    c = _case(name)
    bounds, ref = average_bounds(name, c, dtype)
    got = run_average(emu_step(c["modes"]), c, dtype)
    errs = average_errors(got, c, name)
    print(f"{name} {np.dtype(dtype).name}: emulation {errs} | numpy restatement {ref}")
    assert all(errs[k] <= bounds[k] for k in errs), (errs, bounds)
    if name == "rest":
        check_rest_lanes(got, c, dtype)


def test_relative_height_of_the_reference():
    """`compute_height` as the environment states it (root z minus the lowest contact z) on the fixture's poses."""
    c = _case("regular")
    z = c["pose"][:, 2]        # [4][K][B]
    assert np.array_equal(z[:, 0] - z[:, 1:].min(1), c["height"])


# ------------------------------------------------------------------------------------------------------- kinematics
def unbounded_model():
    model = rd.flex_arm(False, continuous_elbow=True)
    assert any(JT_RUBX <= int(t) <= JT_RUBU for t in model.jtypes)
    return model


MODELS = {"arm7": lambda: load_builtin("arm7"), "cartpole": lambda: load_builtin("cartpole"), "flex_arm": lambda: rd.flex_arm(False),
          "unbounded": unbounded_model, "biped": robots.biped, "anymal": lambda: load_builtin("anymal"),
          # a branched tree: the segment walk to the head and to the tail leaves the waist's body on different branches,
          # the walk to a hand leaves the chest next to the neck
          "hydra": robots.hydra}


def model_frames(name: str, model) -> list:
    if name == "anymal":
        return ["root_joint"] + list(model.contacts) + [s["frame"] for s in model.sensors["ImuSensor"]]
    if name == "hydra":
        return ["head", "tail2", "l_palm", "r_toe"]
    return list(model.frames)[:12]


def random_state(model, names, Bn: int, seed: int):
    """`q` (unit quaternions, unit (cos, sin) pairs) and `v` for Bn lanes on which the pitch of every named frame keeps 0.1 rad
    from +-pi/2 (drawn four times over, the first Bn such lanes kept)."""
    rg = np.random.default_rng(seed)
    n = 4 * Bn
    q = np.zeros((model.nq, n))
    for j in range(1, model.njoints):
        t, iq = int(model.jtypes[j]), int(model.idx_q[j])
        if t in (JT_SPHERICAL, JT_FREEFLYER):
            o = iq + (3 if t == JT_FREEFLYER else 0)
            axis = rg.normal(size=(3, n))
            axis /= np.linalg.norm(axis, axis=0)
            angle = rg.uniform(-0.5, 0.5, n) if t == JT_SPHERICAL else rg.uniform(-3.0, 3.0, n)
            q[o:o + 3], q[o + 3] = axis * np.sin(angle / 2), np.cos(angle / 2)
            if t == JT_FREEFLYER:
                q[iq:iq + 3] = rg.normal(size=(3, n))
        elif JT_RUBX <= t <= JT_RUBU:
            a = rg.uniform(-np.pi, np.pi, n)
            q[iq], q[iq + 1] = np.cos(a), np.sin(a)
        else:
            q[iq] = rg.uniform(-1.0, 1.0, n)
    pitch = fn.frames(model, names, q)["rpy"][1]
    keep = np.flatnonzero((np.abs(pitch) <= np.pi / 2 - 0.1).all(0))[:Bn]
    assert len(keep) == Bn
    return np.ascontiguousarray(q[:, keep]), rg.normal(size=(model.nv, Bn))


def run_kinematics(call, plan, q, v, dtype, model_lane=None, mask=None, prefill=np.nan, with_prev=True) -> dict:
    """`call(q, v, model_lane, mask, pose, pose_prev, rpy, vel)` on fresh outputs `[rows][K][B]`."""
    K, Bn = plan.n_frames, q.shape[1]
    out = {k: np.full((rows, K, Bn), prefill, dtype=dtype) for k, rows in (("pose", 7), ("pose_prev", 7), ("rpy", 3), ("vel", 6))}
    if not with_prev:
        out["pose_prev"] = None
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype=dtype)     # noqa: E731
    call(cast(q), cast(v), cast(model_lane), mask, out["pose"], out["pose_prev"], out["rpy"], out["vel"])
    return out


def emu_call(plan):
    desc, keep = plan.desc()

    def call(q, v, model_lane, mask, pose, pose_prev, rpy, vel):
        assert keep
        emu.kinematics(desc, q, v, model_lane, mask, pose, pose_prev, rpy, vel)
    return call


EPS32 = 1.2e-7      # (float32: the same bound with the precision of that format, which also covers the rounding of q and v)


def kinematics_errors(got: dict, want: dict, plan, where=slice(None), eps: float = EPS) -> dict:
    """Largest error of every output in units of its bound 64 * depth * eps * max(|want|, 1) (depth per frame)."""
    bound = (64 * eps * np.asarray(plan.depth, dtype=np.float64))[None, :, None]
    pose, ref = got["pose"].astype(np.float64), want["pose"]
    assert np.isfinite(pose).all()
    e_pos = np.abs(pose[:3] - ref[:3]) / np.maximum(np.abs(ref[:3]), 1.0)
    e_quat = np.minimum(np.abs(pose[3:] - ref[3:]).max(0), np.abs(pose[3:] + ref[3:]).max(0))[None]
    d = got["rpy"].astype(np.float64) - want["rpy"]
    e_rpy = np.abs((d + np.pi) % (2 * np.pi) - np.pi) / np.maximum(np.abs(want["rpy"]), 1.0)
    errs = {"position": e_pos, "quaternion": e_quat, "rpy": e_rpy, "velocity": _rel(got["vel"], want["vel"])}
    return {k: float((e / bound)[..., where].max()) for k, e in errs.items()}


def alternating_modes(K: int) -> list:
    return [fn.LOCAL if k % 2 == 0 else fn.LOCAL_WORLD_ALIGNED for k in range(K)]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_emulated_kinematics_match_the_numpy_forward_kinematics(name):
    model = MODELS[name]()
    names = model_frames(name, model)
    Bn = 32
    q, v = random_state(model, names, Bn, seed=11)
    modes = alternating_modes(len(names))
    plan = frames.build_plan(model, names, modes)
    want = fn.frames(model, names, q, v, modes)
    got = run_kinematics(emu_call(plan), plan, q, v, np.float64)
    errs = kinematics_errors(got, want, plan)
    print(f"{name}: {len(names)} frames, depth {max(plan.depth)}, kinds {sorted(set(int(k) for k in plan.arrays['seg_kind']))}, "
          f"errors / bound {errs}")
    assert max(errs.values()) <= 1.0, errs
    assert np.array_equal(got["pose_prev"], got["pose"])
    # the velocity is the derivative of the pose along v: central difference of the numpy pose at eps = 1e-6
    fd = fn.finite_difference_velocity(model, names, q, v, modes, 1e-6)
    e = float(_rel(got["vel"], fd).max())
    print(f"{name}: velocity against the central difference {e:.2e}")
    assert e <= 1e-8
    # every output may be left out, and the velocity rows are not read without it
    only = run_kinematics(lambda q_, v_, ml, m, pose, prev, rpy, vel: emu.kinematics(plan.desc()[0], q_, None, ml, m, pose, None, None, None),
                          plan, q, v, np.float64, with_prev=False)
    assert np.array_equal(only["pose"], got["pose"]) and np.isnan(only["rpy"]).all() and np.isnan(only["vel"]).all()
    # float32: the same walk in single precision
    got32 = run_kinematics(emu_call(plan), plan, q, v, np.float32)
    e32 = kinematics_errors(got32, want, plan, eps=EPS32)
    print(f"{name} float32: errors / bound {e32}")
    assert max(e32.values()) <= 1.0, e32


def biased_model_lane(model, Bn: int, seed: int) -> np.ndarray:
    import torch

    from jiminy_amd.randomization import sample_model_lane
    g = torch.Generator(device="cpu").manual_seed(seed)
    return sample_model_lane(model, Bn, {"relativePositionBodiesBiasStd": 0.05}, generator=g).numpy()


@pytest.mark.parametrize("name", ["biped", "anymal"])
def test_emulated_kinematics_with_per_lane_placements(name):
    model = MODELS[name]()
    names = model_frames(name, model)
    Bn = 16
    q, v = random_state(model, names, Bn, seed=12)
    modes = alternating_modes(len(names))
    plan = frames.build_plan(model, names, modes)
    ml = biased_model_lane(model, Bn, seed=4)
    want = fn.frames(model, names, q, v, modes, model_lane=ml)
    nominal = fn.frames(model, names, q, v, modes)
    assert float(np.abs(want["pose"][:3] - nominal["pose"][:3]).max()) > 1e-3      # (the placements do move the frames)
    errs = kinematics_errors(run_kinematics(emu_call(plan), plan, q, v, np.float64, model_lane=ml), want, plan)
    print(f"{name} with per-lane placements: errors / bound {errs}")
    assert max(errs.values()) <= 1.0, errs


def test_emulated_kinematics_lane_mask():
    model = load_builtin("anymal")
    names = model_frames("anymal", model)
    q, v = random_state(model, names, 16, seed=13)
    plan = frames.build_plan(model, names)
    mask = np.arange(16) % 3 == 0
    full = run_kinematics(emu_call(plan), plan, q, v, np.float64)
    got = run_kinematics(emu_call(plan), plan, q, v, np.float64, mask=mask, prefill=7.25)
    for k in got:
        assert np.array_equal(got[k][..., mask], full[k][..., mask]), k
        assert (got[k][..., ~mask] == 7.25).all(), k


# ------------------------------------------------------------------------------------------- plan, ABI, Python surface
def _anymal_arrays() -> dict:
    model = load_builtin("anymal")
    return {k: np.array(v) for k, v in frames.build_plan(model, ["root_joint"] + list(model.contacts), [0, 1, 2, 0, 1]).arrays.items()}


def _prebuilt(model):
    path = codegen.lib_path(model)
    if not os.path.exists(path):
        pytest.skip(f"{os.path.basename(path)} not built (run __graft_entry__.build())")
    return _lib.load_for(model, allow_build=False)


def _last_error(lib) -> str:
    buf = C.create_string_buffer(1024)
    lib.L.jm_last_error(buf, 1024)
    return buf.value.decode()


def _set_at(index, value):
    def f(a):
        a = a.copy()
        a.reshape(-1)[index] = value
        return a
    return f


def _rejections(good: dict) -> list:
    """(changes of the description, what the message must say) for every rejection of `jm_frames_plan_create`."""
    kinds = good["seg_kind"]
    s_ff = int(np.flatnonzero(kinds == 7)[0])
    s_rev = int(np.flatnonzero((kinds >= 1) & (kinds <= 4))[0])
    n_seg, K = len(kinds), len(good["frame_mode"])
    deep = np.concatenate([[0], np.full(K, n_seg)])        # (n_seg segments in the first frame, none in the others)
    return [
        (dict(frame_mode=lambda a: np.zeros(0, int)), "bad sizes"),
        (dict(nq=lambda a: -1), "bad sizes"),
        (dict(njoints=lambda a: 0), "bad sizes"),
        (dict(frame_seg_start=_set_at(0, 1)), "frame_seg_start"),
        (dict(frame_seg_start=lambda a: deep), "segment count"),
        (dict(frame_seg_start=lambda a: np.array([0, 300]), frame_mode=lambda a: a[:1], **{
            k: (lambda a: np.concatenate([a] * (300 // len(a) + 1))[:300]) for k in ("seg_kind", "seg_joint", "seg_q_index", "seg_v_index",
                                                                                     "seg_rot", "seg_trans", "seg_axis")}),
         "segment count"),
        (dict(seg_q_index=_set_at(s_ff, int(good["nq"]) - 6)), "q rows"),
        (dict(seg_q_index=_set_at(s_rev, -1)), "q rows"),
        (dict(seg_v_index=_set_at(s_ff, int(good["nv"]) - 5)), "v rows"),
        (dict(seg_v_index=_set_at(s_rev, int(good["nv"]))), "v rows"),
        (dict(seg_joint=_set_at(s_rev, int(good["njoints"]))), "joint index"),
        (dict(seg_joint=_set_at(s_rev, -1)), "joint index"),
        (dict(seg_kind=_set_at(s_rev, 12)), "unknown joint kind"),
        (dict(seg_kind=_set_at(s_rev, -1)), "unknown joint kind"),
        (dict(frame_mode=_set_at(1, 3)), "reference frame mode"),
        (dict(seg_rot=_set_at(4, np.nan)), "not finite"),
        (dict(seg_trans=_set_at(1, np.inf)), "not finite"),
        (dict(seg_axis=_set_at(3 * s_rev, np.nan)), "not finite"),
    ]


def _broken(good: dict, change: dict):
    arrays = {k: np.array(v) for k, v in good.items()}
    for k, f in change.items():
        arrays[k] = f(arrays[k])
    for k in ("nq", "nv", "njoints"):
        arrays[k] = int(arrays[k])
    desc, keep = frames.make_desc(**arrays)
    if "frame_mode" in change and len(arrays["frame_mode"]) == 0:
        desc.n_frames = 0
    return desc, keep


def test_plan_validation_rejects_every_malformed_description():
    good = _anymal_arrays()
    desc, keep = frames.make_desc(**good)
    emu.pack(desc)
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    for field in ("frame_seg_start", "frame_mode", "seg_kind", "seg_joint", "seg_q_index", "seg_v_index", "seg_rot", "seg_trans", "seg_axis"):
        d, keep_ = frames.make_desc(**good)
        setattr(d, field, None)
        with pytest.raises(ValueError, match="null array"):
            emu.pack(d)
    for change, message in _rejections(good):
        d, keep_ = _broken(good, change)
        with pytest.raises(ValueError, match=message):
            emu.pack(d)


def test_plan_create_validates_before_touching_the_device():
    """The same rejections through the C ABI of a built library, on a machine without a device: JM_EINVAL and a message."""
    lib = _prebuilt(load_builtin("cartpole"))
    good = _anymal_arrays()
    h = C.c_void_p()
    assert lib.L.jm_frames_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = frames.make_desc(**good)
    assert lib.L.jm_frames_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.seg_trans = None
    assert lib.L.jm_frames_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)
    for change, message in _rejections(good):
        d, keep_ = _broken(good, change)
        rc = lib.L.jm_frames_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and message in _last_error(lib), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)


def test_abi_version_symbols_and_the_plans_of_the_other_blocks():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    assert "typedef struct jm_frames_desc" in header
    assert [f[0] for f in _abi.FramesDesc._fields_] == ["n_frames", "nq", "nv", "njoints", "frame_seg_start", "frame_mode", "n_seg",
                                                         "seg_kind", "seg_joint", "seg_q_index", "seg_v_index", "seg_rot", "seg_trans",
                                                         "seg_axis"]
    # the segment table the other plans are made of keeps its lists and its kinds; the new table only adds to it
    from jiminy_amd import _plan
    assert sorted(vars(_plan.SegmentTable())) == ["axis", "frame_seg_start", "index", "kind", "ratio", "rot"]
    assert issubclass(_plan.PlacedSegmentTable, _plan.SegmentTable)
    assert (_plan.SEG_NONE, _plan.SEG_X, _plan.SEG_AXIS, _plan.SEG_UNBOUNDED, _plan.SEG_QUAT) == (0, 1, 4, 5, 6)
    # ANYmal's attitude plan: the free-flyer orientation (q rows 3 .. 6), then the frame of the IMU
    a = attitude.build_plan(load_builtin("anymal")).arrays
    assert sorted(a) == ["frame_seg_start", "ki", "kp", "nq", "rel_quat", "seg_axis", "seg_kind", "seg_q_index", "seg_rot"]
    assert list(a["seg_kind"])[0] == _plan.SEG_QUAT and list(a["seg_q_index"])[0] == 3 and list(a["frame_seg_start"])[0] == 0
    assert np.array(a["seg_rot"]).shape == (len(a["seg_kind"]), 3, 3)
    # the deformation plan of the flexible arm: encoders and constant rotations only, a ratio per segment
    d = deformation.build_plan(rd.flex_arm(False), rd.imu_frames(False)[::-1], ["f23", "f45", "f12", "elbow"]).arrays
    assert {"seg_kind", "seg_enc", "seg_rot", "seg_axis", "seg_ratio"} <= set(d)
    assert len(d["seg_ratio"]) == len(d["seg_kind"]) and max(d["seg_kind"]) <= _plan.SEG_AXIS


def test_python_surface_on_the_host():
    from types import SimpleNamespace

    import torch

    from jiminy_amd import blocks
    from jiminy_amd.envs import WalkerVecEnv
    model = load_builtin("anymal")
    with pytest.raises(LookupError, match="no_such_frame"):
        frames.build_plan(model, ["root_joint", "no_such_frame"])
    with pytest.raises(ValueError):
        frames.build_plan(model, ["root_joint"], ["LOCAL", "LOCAL"])
    with pytest.raises(ValueError, match="SIDEWAYS"):
        frames.build_plan(model, ["root_joint"], ["SIDEWAYS"])
    assert frames.build_plan(model, ["root_joint", "LF_FOOT"], ["ODOMETRY", "LOCAL_WORLD_ALIGNED"]).modes == [2, 1]
    # a frame on the universe is one constant segment
    fixed = load_builtin("cartpole")
    on_universe = [n for n, f in fixed.frames.items() if int(f.parent_joint) == 0]
    if on_universe:
        assert frames.build_plan(fixed, on_universe[:1]).depth == [1]
    # ODOMETRY is a frame of the step average: refused before anything is allocated
    stub = SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4,
                           _lib=SimpleNamespace(L=None, check=None))
    with pytest.raises(NotImplementedError, match="ODOMETRY"):
        blocks.FrameKinematics(stub, ["root_joint"], reference_frames=["ODOMETRY"])
    names = blocks.frame_fieldnames(["root_joint", "LF_FOOT"], True, True, True)
    assert sorted(names) == ["average_velocity", "pose", "pose_mean", "quat_no_yaw", "rpy", "velocity"]
    assert names["pose"][6] == ["root_joint.QuatW", "LF_FOOT.QuatW"] and names["rpy"][1] == ["root_joint.Pitch", "LF_FOOT.Pitch"]
    assert names["velocity"][3] == ["root_joint.AngX", "LF_FOOT.AngX"] and names["quat_no_yaw"][0][1] == "LF_FOOT.QuatX"
    assert sorted(blocks.frame_fieldnames(["a"], False, False, False)) == ["pose"]
    # the environment adds what its terminations read
    got = WalkerVecEnv.frame_kinematics_config(model, dict(frame_names=["LF_FOOT"], reference_frames=["LOCAL_WORLD_ALIGNED"], average=True),
                                               dict(base_roll_pitch=(-0.5, 0.5, 0.0)))
    assert got[0] == ["LF_FOOT", "root_joint"] + [c for c in model.contacts if c != "LF_FOOT"]
    assert got[1] == ["LOCAL_WORLD_ALIGNED"] + ["LOCAL"] * len(model.contacts) and got[2] == dict(average=True, compute_rpy=True)
    got = WalkerVecEnv.frame_kinematics_config(model, dict(frame_names=["imu_link"]), {})
    assert got == (["imu_link"], None, {})


# ------------------------------------------------------------------------------------------------------------ device
class DeviceFrames:
    """A plan on the device and the two calls on numpy arrays (copied in and out)."""

    def __init__(self, lib, arrays: dict, device):
        import torch
        self.torch, self.lib, self.device = torch, lib, device
        desc, keep = frames.make_desc(**arrays)
        self.h = C.c_void_p()
        with torch.cuda.device(device):
            lib.check(lib.L.jm_frames_plan_create(C.byref(desc), C.byref(self.h)))

    def close(self):
        self.lib.L.jm_frames_plan_destroy(self.h)

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

    def kinematics(self, q, v, model_lane, mask, pose, pose_prev, rpy, vel):
        L, h, Bn = self.lib.L, self.h, pose.shape[-1]
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._run(lambda p, s: L.jm_block_frame_kinematics(h, self._code(pose), Bn, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], s),
                  [q, v, model_lane, m, pose, pose_prev, rpy, vel], (4, 5, 6, 7))

    def average(self, prev, pose, inv_dt, v_avg, pose_mean, quat_no_yaw):
        L, h, Bn = self.lib.L, self.h, pose.shape[-1]
        self._run(lambda p, s: L.jm_block_frame_average(h, self._code(pose), Bn, p[0], p[1], float(inv_dt), p[2], p[3], p[4], s),
                  [prev, pose, v_avg, pose_mean, quat_no_yaw], (0, 2, 3, 4))


_STATES: dict = {}


def device_case(name: str):
    """Model, frames, 300 lanes of state and the numpy kinematics of every frame, computed once per model."""
    if name not in _STATES:
        model = MODELS[name]()
        names = model_frames(name, model)
        q, v = random_state(model, names, 300, seed=21)
        modes = alternating_modes(len(names))
        _STATES[name] = (model, names, modes, q, v, fn.frames(model, names, q, v, modes))
    return _STATES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["arm7", "cartpole", "flex_arm", "anymal", "hydra"])
def test_device_kinematics_match_the_numpy_forward_kinematics(name, gpu_device):
    """B = 300: two blocks, the second one partial; every frame of the case in one plan and its last frame alone."""
    lib = _prebuilt(load_builtin("cartpole"))
    model, names, modes, q, v, want = device_case(name)
    for cols in (list(range(len(names))), [len(names) - 1]):
        plan = frames.build_plan(model, [names[k] for k in cols], [modes[k] for k in cols])
        ref = {k: a[:, cols] for k, a in want.items() if k != "rot"}
        dev = DeviceFrames(lib, plan.arrays, gpu_device)
        try:
            for dtype, eps in ((np.float64, EPS), (np.float32, EPS32)):
                got = run_kinematics(dev.kinematics, plan, q, v, dtype)
                errs = kinematics_errors(got, ref, plan, eps=eps)
                print(f"{name} K={len(cols)} {np.dtype(dtype).name}: device errors / bound {errs}")
                assert max(errs.values()) <= 1.0, errs
                assert np.array_equal(got["pose_prev"], got["pose"])
        finally:
            dev.close()


@pytest.mark.gpu
def test_device_kinematics_with_per_lane_placements(gpu_device):
    lib = _prebuilt(load_builtin("cartpole"))
    model, names, modes, q, v, _ = device_case("anymal")
    q, v = q[:, :64], v[:, :64]
    plan = frames.build_plan(model, names, modes)
    ml = biased_model_lane(model, 64, seed=5)
    want = fn.frames(model, names, q, v, modes, model_lane=ml)
    dev = DeviceFrames(lib, plan.arrays, gpu_device)
    try:
        for dtype, eps in ((np.float64, EPS), (np.float32, EPS32)):
            errs = kinematics_errors(run_kinematics(dev.kinematics, plan, q, v, dtype, model_lane=ml), want, plan, eps=eps)
            print(f"anymal with per-lane placements {np.dtype(dtype).name}: device errors / bound {errs}")
            assert max(errs.values()) <= 1.0, errs
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_average_matches_the_reference(name, gpu_device):
    lib = _prebuilt(load_builtin("cartpole"))
    c = _case(name)
    dev = DeviceFrames(lib, _plain_arrays(c["modes"]), gpu_device)
    try:
        for dtype in (np.float64, np.float32):
            bounds, ref = average_bounds(name, c, dtype)
            got = run_average(dev.average, c, dtype)
            errs = average_errors(got, c, name)
            print(f"{name} {np.dtype(dtype).name}: device {errs} | numpy restatement {ref}")
            assert all(errs[k] <= bounds[k] for k in errs), (errs, bounds)
            if name == "rest":
                check_rest_lanes(got, c, dtype)
    finally:
        dev.close()


def _anymal_engine(Bn: int, q, v, device):
    import torch

    from jiminy_amd.engine import BatchedEngine
    eng = BatchedEngine(load_builtin("anymal"), Bn, dtype=torch.float64, device=device)
    eng.set_options({"contacts": {"model": "spring_damper"}})
    eng.start(torch.from_numpy(q), torch.from_numpy(v))
    return eng


@pytest.mark.gpu
def test_device_lane_mask_and_block_surface(gpu_device):
    """B = 300, every third lane masked: `reset(mask)` writes those lanes of every tensor (the previous pose included) and
    leaves the others bit for bit; the tensors keep their identity; a tensor of the wrong kind is refused."""
    import torch

    from jiminy_amd import blocks
    model, names, modes, q, v, want = device_case("anymal")
    eng = _anymal_engine(300, q, v, gpu_device)
    fk = blocks.FrameKinematics(eng, names, reference_frames=modes, compute_rpy=True, average=True)
    assert fk.fieldnames == blocks.frame_fieldnames(names, True, True, True)
    tensors = dict(pose=fk.pose, pose_prev=fk.pose_prev, rpy=fk.rpy, velocity=fk.velocity, average_velocity=fk.average_velocity,
                   pose_mean=fk.pose_mean, quat_no_yaw=fk.quat_no_yaw)
    fk.reset()
    full = {k: t.clone() for k, t in tensors.items()}
    ref = {k: a for k, a in want.items() if k != "rot"}
    got = dict(pose=full["pose"].cpu().numpy(), rpy=full["rpy"].cpu().numpy(), vel=full["velocity"].cpu().numpy())
    assert max(kinematics_errors(got, ref, fk.plan).values()) <= 1.0
    assert torch.equal(full["pose_prev"], full["pose"])
    for t in tensors.values():
        t.fill_(7.25)
    mask = torch.arange(300, device=gpu_device) % 3 == 0
    fk.reset(mask)
    for k, t in tensors.items():
        assert t is getattr(fk, k)
        assert torch.equal(t[..., ~mask], torch.full_like(t[..., ~mask], 7.25)), k
        if k in ("pose", "pose_prev", "rpy", "velocity"):
            assert torch.equal(t[..., mask], full[k][..., mask]), k
    fk.refresh()
    assert torch.equal(fk.pose, full["pose"]) and torch.equal(fk.velocity, full["velocity"])
    assert torch.equal(fk.pose_prev[..., ~mask], torch.full_like(fk.pose_prev[..., ~mask], 7.25))      # (refresh leaves it alone)
    fk.pose_prev.copy_(fk.pose)
    fk.refresh_average(0.04)
    assert torch.equal(fk.average_velocity, torch.zeros_like(fk.average_velocity)) and torch.equal(fk.pose_mean, fk.pose)
    with pytest.raises(NotImplementedError, match="ODOMETRY"):
        blocks.FrameKinematics(eng, ["root_joint"], reference_frames=["ODOMETRY"])
    with pytest.raises(LookupError, match="no_such_frame"):
        blocks.FrameKinematics(eng, ["no_such_frame"])
    keep = fk.pose
    fk.pose = fk.pose.to(torch.float32)
    with pytest.raises(ValueError, match="pipeline block tensors"):
        fk.refresh()
    fk.pose = keep
    eng.stop()


def contact_state(Bn: int, seed: int):
    """ANYmal states with random small tilts, joint angles and velocities, the base height drawn so that the two lower feet
    are below the flat ground by at most 5 mm and the two others above it; no foot within 1e-9 of the ground."""
    model = load_builtin("anymal")
    rg = np.random.default_rng(seed)
    feet = list(model.contacts)
    keep_q = []
    while len(keep_q) < Bn:
        n = 2 * Bn
        q = np.tile(model.neutral()[:, None], (1, n))
        yaw, tilt = rg.uniform(-np.pi, np.pi, n), rg.uniform(-0.01, 0.01, n)
        ang = rg.uniform(-np.pi, np.pi, n)
        for b in range(n):
            half = np.array([np.cos(ang[b]) * np.sin(tilt[b] / 2), np.sin(ang[b]) * np.sin(tilt[b] / 2), 0.0, np.cos(tilt[b] / 2)])
            z = np.array([0.0, 0.0, np.sin(yaw[b] / 2), np.cos(yaw[b] / 2)])
            q[3:7, b] = fn.quat_multiply(z, half)
        q[0:2] = rg.normal(size=(2, n))
        q[2] = 0.0
        q[7:] += rg.uniform(-0.005, 0.005, (model.nq - 7, n))
        h = np.sort(fn.frames(model, feet, q)["pose"][2], axis=0)       # foot heights with the base at z = 0, ascending
        q[2] = -(h[1] + rg.uniform(0.2, 0.8, n) * (h[2] - h[1]))
        low = h + q[2]
        ok = (low[0] >= -5e-3) & (np.abs(low) >= 1e-9).all(0)
        keep_q += [q[:, b] for b in np.flatnonzero(ok)]
    return model, np.ascontiguousarray(np.stack(keep_q[:Bn], 1)), rg.normal(scale=0.5, size=(model.nv, Bn))


@pytest.mark.gpu
def test_device_frames_against_the_sensors_and_contact_forces_of_the_physics_kernels(gpu_device):
    """ANYmal, B = 64, spring-damper contacts; `start` leaves every field evaluated at the given state.  (a) the LOCAL angular
    velocity of every IMU frame is the gyroscope of the `imu` field within 1e-8 relative to max(|omega|, 1), the bar
    tests/test_gpu_parity.py holds sensors to; (b) a contact point carries a normal force only below the ground."""
    import torch

    from jiminy_amd import blocks
    Bn = 64
    model, q, v = contact_state(Bn, seed=31)
    eng = _anymal_engine(Bn, q, v, gpu_device)
    imus = [s["frame"] for s in model.sensors["ImuSensor"]]
    feet = list(model.contacts)
    fk = blocks.FrameKinematics(eng, imus + feet)
    fk.refresh()
    torch.cuda.synchronize(gpu_device)
    vel, pose = fk.velocity.cpu().numpy(), fk.pose.cpu().numpy()
    gyro = eng.field("imu").cpu().numpy().reshape(len(imus), 6, Bn)[:, :3]           # [n_imu][3][B]
    omega = vel[3:, :len(imus)].transpose(1, 0, 2)
    e = float((np.abs(omega - gyro) / np.maximum(np.abs(gyro), 1.0)).max())
    print(f"IMU gyroscope against the LOCAL angular velocity of the block: {e:.2e}; |omega| up to {np.abs(gyro).max():.2f}")
    assert np.abs(gyro).max() > 0.1 and e <= 1e-8
    # normal force of every contact point in the world frame (the field is in the contact frame; flat ground: +z)
    f_local = eng.field("contact_forces").cpu().numpy().reshape(len(feet), 6, Bn)[:, :3]
    rot = fn.frames(model, feet, q)["rot"]                                             # [K][B][3][3]
    f_n = np.einsum("kbj,kjb->kb", rot[:, :, 2, :], f_local)
    z = pose[2, len(imus):]
    left_out = np.abs(z) < 1e-9
    assert left_out.mean() <= 0.01 and not left_out.any()       # (the draw keeps every foot away from the ground plane)
    below = z < 0
    print(f"{below.mean():.2f} of the feet below the ground, deepest {z.min() * 1e3:.2f} mm; {np.mean(f_n > 0):.2f} carry a normal force")
    assert 0.3 <= below.mean() <= 0.7 and z.min() >= -5e-3 - 1e-9
    assert (z[(f_n > 0) & ~left_out] < 0).all()
    assert (np.abs(f_local).sum(1)[~below & ~left_out] == 0.0).all()
    assert (f_n > 0).any()
    eng.stop()


@pytest.mark.gpu
def test_environment_with_frames_and_terminations(gpu_device, monkeypatch):
    """`make_anymal_env(64, frame_kinematics=..., terminations=...)`, three steps; every lane starts 0.5 m above the ground (no
    contact during the test), every fourth with 1.0 rad of roll, the others with 0.1 rad (away from the roll -> 0 corner of
    `remove_yaw_from_quat`, where the reference itself keeps eight digits)."""
    import torch

    from jiminy_amd.envs import VecJiminyEnv, make_anymal_env
    B = 64
    model = load_builtin("anymal")
    rolled = torch.arange(B, device=gpu_device) % 4 == 0
    sample = VecJiminyEnv._sample_state

    def lifted_and_rolled(self, n):
        q, v = sample(self, n)
        q = q.clone()
        q[2] += 0.5
        roll = torch.where(rolled, 1.0, 0.1).to(q.dtype)
        q[3], q[6] = torch.sin(roll / 2), torch.cos(roll / 2)
        return q, v
    monkeypatch.setattr(VecJiminyEnv, "_sample_state", lifted_and_rolled)
    names = ["root_joint", "LF_FOOT", "imu_link", "root_joint"]
    modes = ["LOCAL", "LOCAL_WORLD_ALIGNED", "LOCAL", "ODOMETRY"]
    cfg = dict(frame_names=names, reference_frames=modes, average=True)
    with pytest.raises(ValueError, match="frame_kinematics"):
        make_anymal_env(B, device=gpu_device, terminations=dict(base_roll_pitch=(-0.5, 0.5, 0.0)))
    env = make_anymal_env(B, device=gpu_device, auto_reset=False, frame_kinematics=cfg,
                          terminations=dict(base_roll_pitch=(-0.5, 0.5, 0.0), min_base_height=(0.05, 0.0)))
    graceful = make_anymal_env(B, device=gpu_device, auto_reset=False, frame_kinematics=cfg,
                               terminations=dict(base_roll_pitch=(-0.5, 0.5, 1.0)))
    plain = make_anymal_env(B, device=gpu_device, auto_reset=False)
    assert plain.frames is None and env.frames.frame_names == names + [c for c in model.contacts if c != "LF_FOOT"]
    assert env.frames.compute_rpy and graceful.frames.frame_names == env.frames.frame_names
    envs = (env, graceful, plain)
    for e in envs:
        e.reset(seed=7)
    fk = env.frames
    K = len(fk.frame_names)
    mode_ids = fk.plan.modes

    def root_pose_error():
        q = env.engine.robot_state.q[:7].cpu().numpy()
        pose = fk.pose[:, fk.index("root_joint")].cpu().numpy()
        e_quat = np.minimum(np.abs(pose[3:] - q[3:]).max(0), np.abs(pose[3:] + q[3:]).max(0)).max()
        return max(float(np.abs(pose[:3] - q[:3]).max()), float(e_quat))
    assert root_pose_error() <= TOL and torch.equal(fk.pose_prev, fk.pose)
    g = torch.Generator(device="cpu").manual_seed(2)
    worst = 0.0
    for i in range(3):
        before = fk.pose.cpu().numpy()
        action = (0.3 * torch.randn(B, model.nmotors, generator=g, dtype=torch.float64)).to(gpu_device)
        out = [e.step(action) for e in envs]
        terminated = out[0][2]
        assert torch.equal(terminated, rolled), i                                  # the rolled lanes, and only those
        assert not bool(out[1][2].any()) and not bool(out[2][2].any())              # grace period of one second; no termination at all
        assert root_pose_error() <= TOL
        # the step average is the restatement applied to the pose snapshots (each within 1e-13 of the reference: 2e-13)
        want = fn.average_step(before, fk.pose.cpu().numpy(), 1.0 / env.step_dt, mode_ids)
        errs = [float(_rel(fk.average_velocity.cpu().numpy(), want["v_avg"]).max()),
                float(_rel(fk.pose_mean.cpu().numpy(), want["pose_mean"]).max()),
                float(_rel(fk.quat_no_yaw.cpu().numpy(), want["quat_no_yaw"]).max())]
        worst = max(worst, *errs)
        assert max(errs) <= 2 * TOL, errs
        assert float(np.abs(want["v_avg"]).max()) > 0.1 and mode_ids[:4] == [0, 1, 0, 2]
        assert torch.equal(fk.pose_prev, fk.pose)
    print(f"environment: step average against the numpy restatement {worst:.2e}")
    # the block does not touch the physics: the environment without it steps to the same bits
    for e in (env, graceful):
        assert torch.equal(e.engine.robot_state.q, plain.engine.robot_state.q)
        assert torch.equal(e.engine.robot_state.v, plain.engine.robot_state.v)
    # relative height: root z over the lowest contact frame
    z = fn.frames(model, ["root_joint"] + list(model.contacts), env.engine.robot_state.q.cpu().numpy())["pose"][2]
    assert float(np.abs(env.base_relative_height().cpu().numpy() - (z[0] - z[1:].min(0))).max()) <= TOL
    # a partial reset: the average of the reset lanes starts from their reset pose, the other lanes keep every bit
    mask = torch.zeros(B, dtype=torch.bool, device=gpu_device)
    mask[::2] = True
    tensors = dict(pose=fk.pose, pose_prev=fk.pose_prev, rpy=fk.rpy, velocity=fk.velocity, average_velocity=fk.average_velocity,
                   pose_mean=fk.pose_mean, quat_no_yaw=fk.quat_no_yaw)
    kept = {k: t.clone() for k, t in tensors.items()}
    env.reset_lanes(mask)
    for k, t in tensors.items():
        assert t is getattr(fk, k) and torch.equal(t[..., ~mask], kept[k][..., ~mask]), k
    assert root_pose_error() <= TOL and torch.equal(fk.pose_prev[..., mask], fk.pose[..., mask])
    q0 = lifted_and_rolled(env, B)[0][:3]
    assert float((fk.pose_prev[:3, 0] - q0)[..., mask].abs().max()) <= TOL
    before = fk.pose_prev.cpu().numpy()
    action = torch.zeros(B, model.nmotors, dtype=torch.float64, device=gpu_device)
    env.step(action)
    want = fn.average_step(before, fk.pose.cpu().numpy(), 1.0 / env.step_dt, mode_ids)
    assert float(_rel(fk.average_velocity.cpu().numpy(), want["v_avg"]).max()) <= 2 * TOL
    assert K == fk.pose.shape[1]
    for e in envs:
        e.close()
