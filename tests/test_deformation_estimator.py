"""The DeformationEstimator observer block: kernel body (host emulation and device), plan builder, C ABI, Python surface.

The specification is the reference's own output (tests/golden/ref_deformation.npz, written by
tools/make_ref_deformation_fixtures.py from the reference's functions) and, for `ignore_twist=False`, a law: fed with the
true IMU orientations the block returns the quaternions of the flexibility joints.

Tolerances.
* float64 against the fixture: 1e-13 relative to max(|want|, 1), the bar of tests/test_reference_blocks.py.  The cases
  whose name ends in a branch of `swing_from_vector` (`_xy`, `_ratio_x`, ...) put one IMU of every second lane into the
  singular region of that function (tilt within 5e-6 of -e_z).  There the reference's own formulas are ill-conditioned:
  they take sqrt((1 + v_z) / 2) with 1 + v_z between 1e-11 and 5e-6, where v_z carries the rounding of a value near 1
  (1.1e-16), and divide tilt components of 1e-6 .. 1e-3 that carry the same absolute rounding.  One ulp of v_z moves the
  result by 1e-16 / (4 sqrt(w_2)) = up to 2e-11.  Such a case is bounded at max(1e-13, 4 x the error the numpy float64
  restatement of tests/deformation_numpy.py shows on the same case).  Measured (host emulation | numpy restatement, quat):
  `*_swing_xy` 2.2e-11 .. 2.4e-11 | 2.6e-11 .. 3.2e-11; `ratio_x` 1.1e-13 | 6.9e-14; `ratio_y` 1.1e-13 | 1.1e-13;
  `general_x` 2.1e-13 | 1.9e-13; `general_y` 3.6e-13 | 3.8e-13; every regular case <= 1e-15 for both.
  On the MI355X: `*_swing_xy` 1.9e-11 .. 2.1e-11, `ratio_x` 8.2e-14, `ratio_y` 1.1e-13, `general_x` 3.7e-13 (rpy 1.2e-12 under a
  bound of 2.5e-12: the closest any case comes), `general_y` 3.7e-13, regular cases <= 7e-16 (rpy 1.4e-15).
* float32 against the float64 fixture: measured, not chosen: 4 x the error of the numpy float32 restatement, taken case
  by case (which is never more than 4 x the largest over the fixture, the bound the comparison was asked to keep).
  Measured largest over the fixture (quat | rpy): numpy float32 3.3e-4 | 1.9e-3 (`arm4_swing_general_*`), emulated kernel
  3.3e-4 | 1.9e-3 (device kernel 3.3e-4 | 1.3e-3); regular cases: 2.2e-7 .. 3.0e-7 | 3.4e-7 .. 5.1e-7 for both (device 1.9e-7 ..
  3.1e-7 | 2.7e-7 .. 4.7e-7).
"""
from __future__ import annotations

import builtins
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, codegen, deformation, load_builtin
from jiminy_amd.model import JT_FREEFLYER, JT_SPHERICAL
from tests import deformation_numpy as dn
from tests import robots_deformation as rd
from tests.hostemu import deform as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_deformation.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_deformation_fixtures.py")
TOL = 1e-13
DESC_KEYS = ("n_imu", "n_enc", "ignore_twist", "chain_nflex", "chain_orphan", "chain_imu", "chain_imu_frame", "flex_frame",
             "flex_flipped", "frame_seg_start", "seg_kind", "seg_enc", "seg_rot", "seg_axis", "seg_ratio")
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["est_cases"]]
CHAIN_CASES = json.loads(str(FX["chain_cases"]))


def _case(name: str):
    arrays = {k: FX[f"est.{name}.{k}"] for k in DESC_KEYS}
    return arrays, FX[f"est.{name}.enc"], FX[f"est.{name}.imu_quat"], FX[f"est.{name}.quat"], FX[f"est.{name}.rpy"]


def _err(got: np.ndarray, want: np.ndarray) -> float:
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)))


def _bounds64(name: str, arrays, enc, imu, want_q, want_r):
    """1e-13; for a singular-branch case no less than 4 x what the numpy float64 restatement shows on it."""
    nq, nr = dn.estimate(arrays, enc, imu)
    eq, er = _err(nq, want_q), _err(nr, want_r)
    if not str(FX[f"est.{name}.singular"]):
        assert eq <= TOL and er <= TOL, (name, eq, er)      # the restatement itself keeps the bar on the regular cases
        return TOL, TOL, eq, er
    return max(TOL, 4 * eq), max(TOL, 4 * er), eq, er


def _bounds32(arrays, enc, imu, want_q, want_r):
    nq, nr = dn.estimate(arrays, enc, imu, dtype=np.float32)
    eq, er = _err(nq, want_q), _err(nr, want_r)
    return 4 * eq, 4 * er, eq, er


# ----------------------------------------------------------------------------------------------- fixture, kernel body
def test_fixture_covers_what_it_claims():
    hits = sum(FX[f"est.{c}.m2q_hits"] for c in CASES)
    assert (hits > 0).all(), hits                                         # every branch of matrices_to_quat
    swing = {}
    for c in CASES:
        for k, v in json.loads(str(FX[f"est.{c}.swing_hits"])).items():
            swing[k] = swing.get(k, 0) + v
    assert set(swing) == {"regular", "xy", "ratio_x", "ratio_y", "general_x", "general_y"} and min(swing.values()) >= 32
    orphans = {tuple(FX[f"est.{c}.chain_orphan"].reshape(-1, 2)[k]) for c in CASES for k in range(len(FX[f"est.{c}.chain_nflex"]))}
    assert orphans == {(0, 0), (0, 1)}
    assert {int(k) for c in CASES for k in FX[f"est.{c}.chain_nflex"]} == {1, 2, 4}
    assert any(len(FX[f"est.{c}.chain_nflex"]) == 2 for c in CASES)       # two chains in one robot
    assert {int(FX[f"est.{c}.ignore_twist"]) for c in CASES} == {0, 1}
    assert any(0 < FX[f"est.{c}.flex_flipped"].sum() < len(FX[f"est.{c}.flex_flipped"]) for c in CASES)     # flags mixed
    assert all(FX[f"est.{c}.quat"].shape[-1] <= 64 for c in CASES) and os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_float64_matches_the_reference(name):
    arrays, enc, imu, want_q, want_r = _case(name)
    desc, keep = deformation.make_desc(**arrays)
    q, r = emu.run(desc, enc, imu)
    bq, br, nq, nr = _bounds64(name, arrays, enc, imu, want_q, want_r)
    eq, er = _err(q, want_q), _err(r, want_r)
    print(f"{name}: kernel quat {eq:.2e} rpy {er:.2e} | numpy restatement {nq:.2e} {nr:.2e} | bounds {bq:.2e} {br:.2e}")
    assert eq <= bq and er <= br, (name, eq, er, bq, br)
    q_only, none = emu.run(desc, enc, imu, compute_rpy=False)
    assert none is None and np.array_equal(q_only, q)


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_float32_within_the_measured_bound(name):
    arrays, enc, imu, want_q, want_r = _case(name)
    desc, keep = deformation.make_desc(**arrays)
    q, r = emu.run(desc, enc, imu, dtype=np.float32)
    bq, br, nq, nr = _bounds32(arrays, enc, imu, want_q, want_r)
    eq, er = _err(q, want_q), _err(r, want_r)
    print(f"{name}: kernel float32 quat {eq:.2e} rpy {er:.2e} | numpy float32 {nq:.2e} {nr:.2e}")
    assert eq <= bq and er <= br, (name, eq, er, bq, br)


# ------------------------------------------------------------------------------------------------------- plan builder
def _tree_args(tree):
    parents = [p for _, p in tree["joints"]]
    names = [n for n, _ in tree["joints"]]
    return parents, bool(tree["root_free"]), {n: names.index(n) for n in tree["flex"]}, dict(tree["imu"])


@pytest.mark.parametrize("name", sorted(CHAIN_CASES))
def test_chain_extraction_matches_the_reference_function(name):
    case = CHAIN_CASES[name]
    assert case["tier"] == "B"
    args = _tree_args(case["tree"])
    if "error" in case["result"]:
        cls, message = case["result"]["error"]
        with pytest.raises(getattr(builtins, cls)) as e:
            deformation.flexibility_imu_frame_chains(*args)
        assert str(e.value) == message
    else:
        got = deformation.flexibility_imu_frame_chains(*args)
        assert [[list(f), list(i), list(fl)] for f, i, fl in got] == case["result"]["chains"]


@pytest.mark.parametrize("has_freeflyer", [False, True])
def test_plan_of_the_authored_arm(has_freeflyer):
    model = rd.flex_arm(has_freeflyer)
    case = CHAIN_CASES["flex_arm_ff" if has_freeflyer else "flex_arm"]
    # the recorded tree IS the compiled model's
    assert [n for n, _ in case["tree"]["joints"]] == model.joint_names
    assert [p for _, p in case["tree"]["joints"]] == [int(p) for p in model.parents]
    assert case["tree"]["imu"] == {n: int(model.frame(n).parent_joint) for n in rd.imu_frames(has_freeflyer)}
    # names given out of order: the plan follows the chain, not the user (deformation_estimator.py:613-616)
    plan = deformation.build_plan(model, rd.imu_frames(has_freeflyer)[::-1], ["f23", "f45", "f12", "elbow"])
    (flexs, imus, flipped), = case["result"]["chains"]
    frame_of = {"elbowFlexibility": "elbow"}
    assert plan.chains == [([frame_of.get(f, f) for f in flexs], imus, flipped)]
    assert plan.flexibility_frame_names == ["f45", "elbow", "f23", "f12"]
    assert plan.is_chain_orphan == [(False, not has_freeflyer)]
    sensors = [s["frame"] for s in model.sensors["ImuSensor"]]
    assert plan.imu_indices == [tuple(sensors.index(n) for n in imus if n)]
    # the flexibility point is represented by its nearest mechanical ancestor (:776-788)
    assert plan.parent_flex_joint_names == ["elbow", "shoulder", "shoulder", "shoulder"]
    a = plan.arrays
    assert a["n_imu"] == len(sensors) and a["n_enc"] == 2 and a["chain_orphan"] == [[0, int(not has_freeflyer)]]
    ratio = {s["name"]: 1.0 / s["reduction"] for s in model.sensors["EncoderSensor"]}
    enc_names = [s["name"] for s in model.sensors["EncoderSensor"]]
    for k, e, r in zip(a["seg_kind"], a["seg_enc"], a["seg_ratio"]):
        assert (k == 0 and e == -1) or r == ratio[enc_names[e]]
    assert ratio["shoulder"] == 0.1 and ratio["elbow"] == 1.0


def test_plan_error_cases():
    fixed, ff = rd.flex_arm(False), rd.flex_arm(True)
    flex = list(rd.FLEX_FRAMES)
    for imus, flexs in (([], flex), (rd.imu_frames(False), [])):        # deformation_estimator.py:550-552
        with pytest.raises(RuntimeError, match="^Please specify at least one IMU and one deformation point.$"):
            deformation.build_plan(fixed, imus, flexs)
    # a flexibility frame the compiled model does not have: this repository's one deviation from the reference
    with pytest.raises(NotImplementedError, match="no flexibility joint at frame 'shoulder'"):
        deformation.build_plan(fixed, rd.imu_frames(False), flex + ["shoulder"])
    with pytest.raises(LookupError):
        deformation.build_plan(fixed, rd.imu_frames(False), flex + ["no_such_frame"])
    # :297-307 through the block
    with pytest.raises(ValueError, match="^There must be an IMU frame attached to all the leaf joints"):
        deformation.build_plan(fixed, ["imu2", "imu3", "imu4"], flex)
    with pytest.raises(ValueError, match="^There must not be an IMU frame attached to the root joint"):
        deformation.build_plan(fixed, rd.imu_frames(False) + ["imu1"], flex)
    # :606-611
    with pytest.raises(NotImplementedError, match="^Freeflyer estimator is not supported for now.$"):
        deformation.build_plan(ff, rd.imu_frames(False), flex)
    # :678-682
    short = rd.flex_arm(False)
    short.sensors["EncoderSensor"].pop()
    with pytest.raises(ValueError, match="^The robot must have one encoder per mechanical joints.$"):
        deformation.build_plan(short, rd.imu_frames(False), flex)
    # :692-694
    with pytest.raises(ValueError, match="^Revolute unbounded joints are not supported for now.$"):
        deformation.build_plan(rd.flex_arm(False, continuous_elbow=True), rd.imu_frames(False), flex)


# ------------------------------------------------------------------------------------------------------------ the law
def sample_configurations(model, B: int, seed: int) -> np.ndarray:
    """Mechanical angles within their bounds, flexibility quaternions up to 0.5 rad, any free-flyer pose."""
    rg = np.random.default_rng(seed)
    q = np.zeros((model.nq, B))
    for j in range(1, model.njoints):
        t, iq = int(model.jtypes[j]), int(model.idx_q[j])
        if t in (JT_SPHERICAL, JT_FREEFLYER):
            o = iq if t == JT_SPHERICAL else iq + 3
            axis = rg.normal(size=(3, B))
            axis /= np.linalg.norm(axis, axis=0)
            angle = rg.uniform(-0.5, 0.5, B) if t == JT_SPHERICAL else rg.uniform(-3.0, 3.0, B)
            q[o:o + 3], q[o + 3] = axis * np.sin(angle / 2), np.cos(angle / 2)
            if t == JT_FREEFLYER:
                q[iq:iq + 3] = rg.normal(size=(3, B))
        else:
            q[iq] = rg.uniform(model.position_lower[iq], model.position_upper[iq], B)
    return q


def encoder_field(model, q: np.ndarray) -> np.ndarray:
    """The raw encoder field `[n_enc][2][B]` of a robot at rest in configuration q (motor-side encoders read angle x reduction)."""
    enc = np.zeros((len(model.sensors["EncoderSensor"]), 2, q.shape[1]))
    for i, s in enumerate(model.sensors["EncoderSensor"]):
        enc[i, 0] = q[int(model.idx_q[s["joint"]])] * (1.0 if s["joint_side"] else s["reduction"])
    return enc


def flexibility_quaternions(model, plan, q: np.ndarray) -> np.ndarray:
    """Quaternions of the spherical joints in the order of the plan's outputs, `[4][n_flex][B]`."""
    cols = []
    for name in plan.flexibility_frame_names:
        iq = int(model.idx_q[deformation._flexibility_joint(model, name)])
        cols.append(q[iq:iq + 4])
    return np.array(cols).transpose(1, 0, 2)


def sign_free_error(got: np.ndarray, want: np.ndarray) -> float:
    return float(np.minimum(np.abs(got - want).max(0), np.abs(got + want).max(0)).max())


@pytest.mark.parametrize("has_freeflyer", [False, True])
def test_true_imu_orientations_give_back_the_flexibility_quaternions(has_freeflyer):
    """`ignore_twist=False` is an exact kinematic identity (2.4e-15 through the reference's own functions): 1e-12 covers
    256 draws and the kernel's own sincos chain.  Measured here: 8e-16."""
    model = rd.flex_arm(has_freeflyer)
    plan = deformation.build_plan(model, rd.imu_frames(has_freeflyer), list(rd.FLEX_FRAMES), ignore_twist=False)
    q = sample_configurations(model, 256, seed=3 + has_freeflyer)
    desc, keep = plan.desc()
    est, rpy = emu.run(desc, encoder_field(model, q), dn.imu_quaternions(model, q))
    want = flexibility_quaternions(model, plan, q)
    assert np.abs(2 * np.arctan2(np.linalg.norm(want[:3], axis=0), np.abs(want[3]))).max() > 0.4     # really deformed
    err = sign_free_error(est, want)
    print(f"flex_arm{'_ff' if has_freeflyer else ''}: identity error {err:.2e}")
    assert err <= 1e-12
    assert np.isfinite(rpy).all()


def test_rotated_flexibility_placement_conjugates_the_estimate():
    """The kinematic rotation that stands for a flexibility point is that of its nearest non-flexibility ancestor JOINT
    (deformation_estimator.py:776-788), not of the point's own placement.  With f23 placed under a rotation R_p, the
    estimates at f23 and at the elbow flexibility (whose nearest such ancestor is the shoulder as well) are the true
    quaternions conjugated by R_p; those at f12 (in front of it) and f45 (behind the elbow joint, whose frame carries R_p)
    are the true ones."""
    model = rd.flex_arm(False, rotated_placement=True)
    plan = deformation.build_plan(model, rd.imu_frames(False), list(rd.FLEX_FRAMES), ignore_twist=False)
    q = sample_configurations(model, 256, seed=11)
    desc, keep = plan.desc()
    est, _ = emu.run(desc, encoder_field(model, q), dn.imu_quaternions(model, q))
    true = flexibility_quaternions(model, plan, q)
    R_p = model.placement_R[model.joint_names.index("f23")]
    assert not np.allclose(R_p, np.eye(3))
    conj = true.copy()
    conj[:3] = np.einsum("ij,jkb->ikb", R_p, true[:3])      # q_p (x) q (x) conj(q_p): the rotation vector turned by R_p
    for k, name in enumerate(plan.flexibility_frame_names):
        if name in ("f23", "elbow"):
            assert sign_free_error(est[:, k:k + 1], conj[:, k:k + 1]) <= 1e-12, name
            assert sign_free_error(est[:, k:k + 1], true[:, k:k + 1]) > 1e-3, name
        else:
            assert sign_free_error(est[:, k:k + 1], true[:, k:k + 1]) <= 1e-12, name


# --------------------------------------------------------------------------------------------------------- provenance
def test_fixture_generator_is_committed_and_names_the_reference_functions():
    text = open(TOOL).read()
    for name in ("flexibility_estimator", "_compute_orientation_error", "_compute_deformation_from_deviation",
                 "get_flexibility_imu_frame_chains", "compute_tilt_from_quat", "swing_from_vector", "matrices_to_quat",
                 "quat_multiply", "quat_to_rpy", "blocks/deformation_estimator.py", "utils/math.py"):
        assert f'"{name}"' in text, name
    # the tool holds no copy of them: it reads them where the reference lies
    assert "def flexibility_estimator" not in text and "def swing_from_vector" not in text and "ast.parse" in text


def test_fixture_regenerates_from_the_reference_tree(tmp_path):
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        return      # (nothing to compare with where the reference tree is absent; the committed fixture stands)
    out = tmp_path / "ref_deformation.npz"
    subprocess.check_call([sys.executable, TOOL, str(out)], stdout=subprocess.DEVNULL)
    new = np.load(out)
    assert sorted(new.files) == sorted(FX.files)
    for k in FX.files:
        assert np.array_equal(new[k], FX[k]), k


# ---------------------------------------------------------------------------------------------------------------- ABI
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
    good, *_ = _case("two_chains_twist")
    h = C.c_void_p()
    assert lib.L.jm_deform_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = deformation.make_desc(**good)
    assert lib.L.jm_deform_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.seg_rot = None
    assert lib.L.jm_deform_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)

    def broken(**change):
        arrays = {k: np.array(v) for k, v in good.items()}
        for k, f in change.items():
            arrays[k] = f(arrays[k])
        d, keep_ = deformation.make_desc(**arrays)
        rc = lib.L.jm_deform_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value
        with pytest.raises(ValueError):
            lib.check(rc)
        return _last_error(lib)

    def set_at(index, value):
        def f(a):
            a = a.copy()
            a.reshape(-1)[index] = value
            return a
        return f
    joint_seg = int(np.flatnonzero(good["seg_kind"])[0])
    assert "names encoder 2 out of range [0, 2)" in broken(seg_enc=set_at(joint_seg, 2))
    assert "names encoder -1 out of range" in broken(seg_enc=set_at(joint_seg, -1))
    assert "IMU index 5 out of range [0, 5)" in broken(chain_imu=set_at(1, 5))
    assert "misses its first IMU" in broken(chain_orphan=set_at(2, 1))
    assert "has no flexibility point" in broken(chain_nflex=set_at(0, 0))
    assert "unknown joint kind" in broken(seg_kind=set_at(0, 7))
    assert "flexibility frame out of range" in broken(flex_frame=set_at(0, 99))
    assert "frame_seg_start" in broken(frame_seg_start=set_at(-1, 3))
    empty, keep2 = deformation.make_desc(**{**good, "chain_nflex": [], "chain_orphan": [], "flex_frame": [], "flex_flipped": []})
    assert lib.L.jm_deform_plan_create(C.byref(empty), C.byref(h)) == _abi.JM_EINVAL
    assert lib.L.jm_deform_plan_destroy(None) == _abi.JM_OK
    # the calls themselves check their arguments first as well
    assert lib.L.jm_block_deformation_estimator(None, _abi.JM_F64, 4, None, None, None, None, None) == _abi.JM_EINVAL
    # the host emulation runs the same check
    d, keep3 = deformation.make_desc(**{**good, "chain_imu": set_at(1, 5)(good["chain_imu"])})
    with pytest.raises(ValueError, match="IMU index 5 out of range"):
        emu.run(d, FX["est.two_chains_twist.enc"], FX["est.two_chains_twist.imu_quat"])


# ================================================================================================================ GPU
def _device_call(lib, arrays, enc, imu, dtype, device, compute_rpy=True):
    import torch
    desc, keep = deformation.make_desc(**arrays)
    h = C.c_void_p()
    with torch.cuda.device(device):
        lib.check(lib.L.jm_deform_plan_create(C.byref(desc), C.byref(h)))
    try:
        t_enc = torch.as_tensor(np.ascontiguousarray(enc), dtype=dtype, device=device).contiguous()
        t_imu = torch.as_tensor(np.ascontiguousarray(imu), dtype=dtype, device=device).contiguous()
        Bn = t_imu.shape[-1]
        quat = torch.full((4, desc.n_flex, Bn), float("nan"), dtype=dtype, device=device)
        rpy = torch.full((3, desc.n_flex, Bn), float("nan"), dtype=dtype, device=device) if compute_rpy else None
        vp = C.c_void_p
        lib.check(lib.L.jm_block_deformation_estimator(
            h, _abi.JM_F64 if dtype == torch.float64 else _abi.JM_F32, Bn, vp(t_enc.data_ptr()), vp(t_imu.data_ptr()),
            vp(quat.data_ptr()), None if rpy is None else vp(rpy.data_ptr()), vp(torch.cuda.current_stream(device).cuda_stream)))
        torch.cuda.synchronize(device)
        return quat.cpu().numpy(), None if rpy is None else rpy.cpu().numpy()
    finally:
        lib.L.jm_deform_plan_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_kernel_matches_the_reference(name, gpu_device):
    """`jm_block_deformation_estimator` through the C ABI: float64 at 1e-13 (singular-branch cases: module docstring),
    float32 at the measured bound, bit-identical when repeated and when the lanes are permuted."""
    import torch
    lib = _prebuilt(load_builtin("cartpole"))
    arrays, enc, imu, want_q, want_r = _case(name)
    q, r = _device_call(lib, arrays, enc, imu, torch.float64, gpu_device)
    bq, br, nq, nr = _bounds64(name, arrays, enc, imu, want_q, want_r)
    eq, er = _err(q, want_q), _err(r, want_r)
    print(f"{name}: device quat {eq:.2e} rpy {er:.2e} | numpy restatement {nq:.2e} {nr:.2e} | bounds {bq:.2e} {br:.2e}")
    assert eq <= bq and er <= br, (name, eq, er, bq, br)
    q32, r32 = _device_call(lib, arrays, enc, imu, torch.float32, gpu_device)
    bq, br, nq, nr = _bounds32(arrays, enc, imu, want_q, want_r)
    eq, er = _err(q32, want_q), _err(r32, want_r)
    print(f"{name}: device float32 quat {eq:.2e} rpy {er:.2e} | numpy float32 {nq:.2e} {nr:.2e}")
    assert eq <= bq and er <= br, (name, eq, er, bq, br)
    # lane independence: the same bits again, with the lanes permuted (and the batch no multiple of the block size)
    q2, r2 = _device_call(lib, arrays, enc, imu, torch.float64, gpu_device)
    assert np.array_equal(q, q2) and np.array_equal(r, r2)
    perm = np.random.default_rng(0).permutation(enc.shape[-1] * 5)[:300] % enc.shape[-1]
    qp, rp = _device_call(lib, arrays, enc[..., perm], imu[..., perm], torch.float64, gpu_device)
    assert np.array_equal(qp, q[..., perm]) and np.array_equal(rp, r[..., perm])
    q_only, none = _device_call(lib, arrays, enc, imu, torch.float64, gpu_device, compute_rpy=False)
    assert none is None and np.array_equal(q_only, q)


@pytest.mark.gpu
def test_engine_and_block_recover_the_simulated_deformations(gpu_device):
    """The authored arm in a BatchedEngine of 4 096 lanes, random bounded motor torques held per lane, 200 RK4 steps of
    1 ms; the block fed with the TRUE IMU orientations (test-side forward kinematics of `robot_state.q`) must return the
    flexibility quaternions of `robot_state.q` up to sign to 1e-10 on EVERY lane (round-off is 1e-15, a wrong frame or
    sign shows at 1e-2), and the batch must really be deformed."""
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.engine import BatchedEngine
    model = rd.flex_arm(False, stiffness=60.0, damping=1.0)      # (soft enough to bend by several 1e-2 rad under its weight)
    B, dt = 4096, 1e-3
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device)
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": dt,
                                 "sensorsUpdatePeriod": dt}})
    g = torch.Generator(device="cpu").manual_seed(4)
    torque = (torch.rand((model.nmotors, B), generator=g, dtype=torch.float64) * 2 - 1) * torch.tensor([[0.3], [0.05]], dtype=torch.float64)
    q0 = torch.as_tensor(model.neutral(), dtype=torch.float64)[:, None].expand(-1, B).contiguous()
    eng.set_command(torque.to(gpu_device))
    eng.start(q0.to(gpu_device), torch.zeros((model.nv, B), dtype=torch.float64, device=gpu_device))
    for _ in range(200):
        eng.step(dt)
    torch.cuda.synchronize(gpu_device)
    assert bool((eng.status == 0).all()), "every lane must stay finite and inside its bounds"
    q = eng.robot_state.q.cpu().numpy()
    assert np.isfinite(q).all()
    block = blocks.DeformationEstimator(eng, rd.imu_frames(False), list(rd.FLEX_FRAMES), ignore_twist=False)
    assert block.flexibility_frame_names == ["f45", "elbow", "f23", "f12"]
    assert block.fieldnames["quat"][3][0] == "f45.Quatw" and block.fieldnames["rpy"][1][-1] == "f12.Pitch"
    assert torch.equal(block.quat[3], torch.ones_like(block.quat[3])) and not bool(block.quat[:3].any())
    # the encoders the block reads are the engine's own
    enc = eng.field("encoder").cpu().numpy().reshape(2, 2, B)
    assert np.abs(enc[:, 0] - encoder_field(model, q)[:, 0]).max() <= 1e-12
    block.refresh(torch.as_tensor(dn.imu_quaternions(model, q), device=gpu_device).contiguous())
    torch.cuda.synchronize(gpu_device)
    est = block.quat.cpu().numpy()
    want = flexibility_quaternions(model, block.plan, q)
    angle = 2 * np.arctan2(np.linalg.norm(want[:3], axis=0), np.abs(want[3]))
    err = sign_free_error(est, want)
    print(f"largest deformation {angle.max():.3e} rad, smallest per-lane largest {angle.max(0).min():.3e}; identity error {err:.2e}")
    assert angle.max() > 1e-2
    assert err <= 1e-10
    assert np.isfinite(block.rpy.cpu().numpy()).all()


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


@pytest.mark.gpu
def test_environment_plumbing(gpu_device, monkeypatch):
    import torch

    from jiminy_amd.envs import PDControlledWalkerVecEnv
    model = rd.flex_arm(True)
    B, n_flex = 64, 4
    cfg = dict(imu_frame_names=rd.imu_frames(True), flex_frame_names=list(rd.FLEX_FRAMES), ignore_twist=True, compute_rpy=True)

    def make(**kw):
        return PDControlledWalkerVecEnv(model, B, step_dt=0.01, control_dt=0.005, kp=[20.0, 20.0], kd=[0.05, 0.05],
                                        device=gpu_device, engine_options={"stepper": {"odeSolver": "runge_kutta_4", "dtMax": 1e-3}},
                                        auto_reset=False, **kw)      # (the arm falls freely: a walker would restart at once)
    # (every library call of the environments goes through a counting proxy: installed before they cache the handle)
    counts = _counting_library(monkeypatch, _lib.load_for(model))
    plain, tick, step = make(), make(deformation_estimator=dict(cfg, update_ratio=1)), make(deformation_estimator=dict(cfg, update_ratio=-1))
    graphed = make(deformation_estimator=dict(cfg, update_ratio=1))
    graphed.enable_graph()
    envs = (plain, tick, step, graphed)
    for e in envs:
        e.reset(seed=2)
    g = torch.Generator(device="cpu").manual_seed(0)
    obs0 = tick.observation()["features"]["deformation_estimator"]
    assert tuple(obs0["quat"].shape) == (B, 4, n_flex) and tuple(obs0["rpy"].shape) == (B, 3, n_flex)
    assert torch.equal(obs0["quat"][:, 3], torch.ones_like(obs0["quat"][:, 3])) and not bool(obs0["quat"][:, :3].any())
    assert plain.engine._lib is tick.engine._lib is graphed.engine._lib     # (one library object per topology)
    per_env = []
    for i in range(20):
        action = (0.5 * torch.randn(B, 2, generator=g, dtype=torch.float64)).to(gpu_device)
        outs = []
        for e in envs:
            counts.clear()
            outs.append(e.step(action)[0])
            if i == 3:
                per_env.append(dict(counts))
        assert sorted(outs[0]) == ["actions", "features", "measurements", "states", "t"]
        assert sorted(outs[0]["features"]) == ["mahony_filter"]
        assert sorted(outs[1]["features"]) == ["deformation_estimator", "mahony_filter"]
        est = outs[1]["features"]["deformation_estimator"]
        assert sorted(est) == ["quat", "rpy"] and bool(torch.isfinite(est["quat"]).all()) and bool(torch.isfinite(est["rpy"]).all())
        assert float((est["quat"].norm(dim=1) - 1).abs().max()) <= 1e-6
        # the estimator only observes: same physics with and without it; eager and graph replay agree bit for bit
        for o in outs[1:]:
            assert torch.equal(o["states"]["agent"]["q"], outs[0]["states"]["agent"]["q"])
        assert torch.equal(outs[3]["features"]["deformation_estimator"]["quat"], est["quat"])
        assert torch.equal(outs[3]["features"]["deformation_estimator"]["rpy"], est["rpy"])
        # once per step = the last of the per-tick updates
        assert torch.equal(outs[2]["features"]["deformation_estimator"]["quat"], est["quat"])
        if i == 9:
            mask = torch.zeros(B, dtype=torch.bool, device=gpu_device)
            mask[::5] = True
            before = tick._deform.quat.clone()
            for e in envs:
                e.reset_lanes(mask)
            after = tick._deform.quat
            assert torch.equal(after[:, :, ~mask], before[:, :, ~mask])
            assert torch.equal(after[3][:, mask], torch.ones_like(after[3][:, mask])) and not bool(after[:3][:, :, mask].any())
            assert not bool(tick._deform.rpy[:, :, mask].any())
    assert graphed._graph is not None
    assert float(tick._deform.quat[:3].abs().max()) > 1e-4      # the free-falling arm does deform
    # launches of one environment step (two controller ticks): unchanged without the argument, + one per tick / per step with it
    n_plain, n_tick, n_step, n_graph = per_env
    assert n_plain.get("jm_block_pd_adapter") == 1 and n_plain.get("jm_block_pd_controller") == 2
    assert n_plain.get("jm_block_mahony_filter") == 2 and n_plain.get("jm_batch_step", 0) >= 2
    assert "jm_block_deformation_estimator" not in n_plain
    assert {k: v for k, v in n_tick.items() if k != "jm_block_deformation_estimator"} == n_plain
    assert {k: v for k, v in n_step.items() if k != "jm_block_deformation_estimator"} == n_plain
    assert n_tick["jm_block_deformation_estimator"] == 2 and n_step["jm_block_deformation_estimator"] == 1
    assert not any(k.startswith(("jm_block", "jm_batch_step")) for k in n_graph)     # (replayed, not issued)
