"""Foot pose quantities on the device (csrc/jm_footposes.h behind `jm_block_foot_poses`, `blocks.FootPoseQuantities`, the
`foot_positions` / `foot_orientations` reward terms of `WalkerVecEnv`).

Specification: the reference's own output, tests/golden/ref_footposes.npz (tools/make_ref_footposes_fixtures.py executes the
reference's functions; six cases of 64 lanes).  Comparison rule: with three feet or more the mean and every relative quaternion
of a lane are multiplied by the sign of (got mean quaternion . wanted mean quaternion) first -- LAPACK's sign is arbitrary --
and compared as they are with one or two feet.  float64 within 1e-13 relative to max(|want|, 1) on every lane and output;
float32 within 4 x the error of the float32 numpy restatement (tests/footposes_numpy.py, `np.linalg.eigh` in float32) on the
same case and part, plus 4 x 1.2e-7 on the parts downstream of the eigenvector only (two eigen solvers need not round alike).
An output the case has no expectation for (no reference: the tracking error and the rewards) must stay unwritten.

Measured on the host (error relative to max(|want|, 1), largest over the six cases and the lanes):
  float64, host emulation | numpy restatement
    mean_pose 6.7e-16 | 6.7e-16   mean_odom_pose 5.3e-15 | 4.9e-15   relative_pose 3.3e-15 | 3.1e-15
    tracking_error 3.6e-15 | 3.6e-15   scalars 1.6e-14 | 1.2e-14
  float32, host emulation | numpy restatement
    mean_pose 1.7e-7 | 1.2e-7   mean_odom_pose 1.2e-6 | 4.6e-7   relative_pose 1.0e-6 | 3.7e-7
    tracking_error 6.8e-7 | 5.0e-7   scalars 1.5e-6 | 6.8e-7
  the float32 Jacobi eigenvector is about 3 x further from the float64 one than LAPACK's float32 one.
  ‖M q - lambda q‖ of the emulated mean quaternion on 4096 draws of four feet: 3.1e-15 against 6.4e-15 of `np.linalg.eigh`;
  |‖q‖ - 1| 2.2e-16 against 7.8e-16.

Measured on the device (MI355X; the same six cases through the C ABI, largest over the cases and the lanes):
  float64  mean position 0   mean quaternion 6.7e-16   mean yaw 6.3e-15   relative_pose 3.3e-15   tracking_error 3.3e-15
           scalars 2.0e-14
  float32  mean position 1.2e-7   mean quaternion 1.7e-7   mean yaw 7.5e-7   relative_pose 9.1e-7   tracking_error 9.6e-7
           scalars 2.5e-6; largest ratio error / bound of one case and part: 0.78 (scalars, `tracking`: 2.51e-6 against
           4 x 6.83e-7 + 4 x 1.2e-7)
  walking ANYmal (64 lanes, 4 steps of random actions): the front and hind knees bend opposite ways, the four foot frames form
  two pairs and the two largest eigenvalues nearly coincide: relative gap down to 6.4e-6 (median 1.1e-4).  Device against the
  host composition on the same tensors: mean_pose 3.0e-11, mean_odom_pose 4.8e-11, relative_pose 4.1e-11, tracking_error 8.1e-11,
  at most 0.07 of the lane's bar 1e-13 x 0.1 / gap (`conditioning`).  Laws, device | host composition: mean position 0 | 0;
  mean o relative pose = foot pose 3.9e-16 | 1.8e-15; ‖M q - lambda q‖ 7.0e-16 | 2.2e-15; |‖q‖ - 1| 1.1e-16 | 6.7e-16.
  Environment: reward against the numpy restatement at most 0.014 of its lane's bar.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, codegen, footposes, load_builtin
from tests import footposes_numpy as fp
from tests.hostemu import footposes as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_footposes.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_footposes_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
TOL = 1e-13
EPS = 2.2e-16
EIGEN_SLACK = 4.0 * 1.2e-7
NEW_SYMBOLS = ("jm_footposes_plan_create", "jm_footposes_plan_destroy", "jm_block_foot_poses")
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["cases"]]
_CASES: dict = {}
# (label, output, rows, downstream of the eigenvector when there are three feet or more)
PARTS = (("mean position", "mean_pose", slice(0, 3), False), ("mean quaternion", "mean_pose", slice(3, 7), True),
         ("mean odometry x y", "mean_odom_pose", slice(0, 2), False), ("mean yaw", "mean_odom_pose", slice(2, 3), True),
         ("relative_pose", "relative_pose", slice(None), True), ("tracking_error", "tracking_error", slice(None), True),
         ("scalars", "scalars", slice(None), True))


def case(name: str):
    """plan, inputs, expected and the two numpy restatements of a case, computed once."""
    if name not in _CASES:
        plan, inputs, expected = fp.load_case(FX, name)
        _CASES[name] = (plan, inputs, expected, fp.quantities(plan, inputs, np.float64), fp.quantities(plan, inputs, np.float32))
    return _CASES[name]


def n_feet(plan: dict) -> int:
    return len(plan["foot_column"])


def rel_error(got: np.ndarray, want: np.ndarray) -> float:
    """Largest error relative to max(|want|, 1); everything finite."""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    if not want.size:
        return 0.0
    return float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)).max())


def lane_error(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """`rel_error` per lane (the last axis)."""
    assert got.shape == want.shape and np.isfinite(got).all()
    e = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
    return e.reshape(-1, e.shape[-1]).max(0) if e.size else np.zeros(e.shape[-1])


def conditioning(quats: np.ndarray) -> np.ndarray:
    """Per lane, how much further than on the fixture two backward-stable eigen solvers may lie apart: the fixture's bar holds
    for a relative gap (lambda_1 - lambda_2) / lambda_1 >= 0.1 of sum q q^T; the error of the eigenvector of a matrix known to
    eps ‖M‖ grows like ‖M‖ / (lambda_1 - lambda_2) (Davis-Kahan), so a lane with a smaller gap g gets 0.1 / g times the bar.
    The feet of a quadruped whose front and hind knees bend opposite ways are such a case: two pairs of orientations, two
    nearly equal largest eigenvalues, a mean orientation that is itself ill defined."""
    lam = np.linalg.eigvalsh(fp.gram(quats))
    return np.maximum(1.0, 0.1 * lam[:, -1] / (lam[:, -1] - lam[:, -2]))


def reward_sensitivity(error: np.ndarray, cutoff: float) -> np.ndarray:
    """Per lane, |d reward / d error| <= 2 ln(100) ‖error‖ / cutoff^2 (the reward is at most 1), at least 1."""
    return np.maximum(1.0, 2.0 * np.log(100.0) * np.sqrt(np.sum(error ** 2, (0, 1))) / cutoff ** 2)


def aligned(plan: dict, got: dict, want: dict) -> dict:
    """The comparison rule: the sign of the mean quaternion is only defined up to LAPACK's with three feet or more."""
    return fp.align_sign(got, want) if n_feet(plan) >= 3 else got


def check_against_the_fixture(name: str, run, label: str) -> None:
    """`run(plan, inputs, dtype) -> outputs` (unwritten entries NaN) against the fixture in both dtypes."""
    plan, inputs, expected, _, n32 = case(name)
    n32 = aligned(plan, n32, expected)
    for dtype in (np.float64, np.float32):
        got = run(plan, inputs, dtype)
        for out in fp.OUTPUTS:
            if out not in expected:
                assert np.isnan(got[out]).all(), (name, out)           # no reference: not written
        got = aligned(plan, {k: v for k, v in got.items() if k in expected}, expected)
        for part, out, rows, downstream in PARTS:
            if out not in expected:
                continue
            e = rel_error(got[out][rows], expected[out][rows])
            if dtype is np.float64:
                print(f"{label} {name} float64 {part}: {e:.2e}")
                assert e <= TOL, (name, part, e)
            else:
                e_np = rel_error(n32[out][rows], expected[out][rows])
                bound = 4.0 * e_np + (EIGEN_SLACK if downstream and n_feet(plan) >= 3 else 0.0)
                print(f"{label} {name} float32 {part}: {e:.2e} (numpy float32 {e_np:.2e}, bound {bound:.2e})")
                assert e <= bound, (name, part, e, e_np)


# ------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_from_the_reference_tree():
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        pytest.skip("the reference tree is not here: the committed fixture stands")
    subprocess.check_call([sys.executable, TOOL, "--check"], stdout=subprocess.DEVNULL)


def test_fixture_holds_the_designed_cases():
    assert CASES == ["one_foot", "two_feet", "three_feet", "four_feet", "four_feet_wide", "tracking"]
    assert os.path.getsize(FIXTURE) <= 1 << 20
    feet = dict(one_foot=1, two_feet=2, three_feet=3, four_feet=4, four_feet_wide=4, tracking=4)
    permuted = False
    for name in CASES:
        plan, inputs, expected, _, _ = case(name)
        F, cols = n_feet(plan), [int(c) for c in plan["foot_column"]]
        K = int(plan["n_frames"])
        assert F == feet[name] and K > F and inputs["pose"].shape == (7, K, 64)
        assert len(set(cols)) == F and min(cols) >= 0 and max(cols) < K
        permuted |= cols != sorted(cols) or cols != list(range(F))
        assert ("reference_relative_pose" in inputs) == (name == "tracking")
        assert sorted(expected) == sorted(["mean_pose", "mean_odom_pose", "relative_pose"] +
                                          (["tracking_error", "scalars"] if name in ("one_foot", "tracking") else []))
        assert all(np.isfinite(v).all() for v in expected.values())
        quats = inputs["pose"][3:, cols]
        assert np.abs(np.linalg.norm(quats, axis=0) - 1.0).max() <= 1e-15
        if F >= 2:
            assert (quats[3] < 0).any() and (np.sum(quats[:, 0] * quats[:, 1], 0) < 0).any()      # q and -q are one orientation
        # the condition on the inputs: the two largest eigenvalues of sum q q^T are at least 0.1 apart, relative to the largest
        if F >= 3:
            lam = np.linalg.eigvalsh(fp.gram(quats))
            gap = (lam[:, -1] - lam[:, -2]) / lam[:, -1]
            print(f"{name}: smallest relative gap {gap.min():.3f}")
            assert gap.min() >= 0.1, (name, gap.min())
    assert permuted
    # one foot: a copy, no relative column, both rewards 1
    plan, inputs, expected, _, _ = case("one_foot")
    assert np.array_equal(expected["mean_pose"], inputs["pose"][:, int(plan["foot_column"][0])])
    assert expected["relative_pose"].shape == (7, 0, 64) and expected["tracking_error"].shape == (6, 0, 64) and (expected["scalars"] == 1.0).all()
    # two feet: a dot product of exactly 0 on lane 0 (the mean is quat1 / sqrt(2)), a negative one on lane 1
    plan, inputs, expected, _, _ = case("two_feet")
    q1, q2 = (inputs["pose"][3:, int(c)] for c in plan["foot_column"])
    assert list(q1[:, 0]) == [0.0, 0.0, 0.0, 1.0] and list(q2[:, 0]) == [1.0, 0.0, 0.0, 0.0]
    assert np.array_equal(expected["mean_pose"][3:, 0], q1[:, 0] / np.sqrt(2.0)) and float(np.sum(q1[:, 1] * q2[:, 1])) < 0.0
    # tracking: inside the cutoffs; lane 0 is the reference code's own output; lane 1 has a residual quaternion with w < 0
    plan, inputs, expected, _, _ = case("tracking")
    err = expected["tracking_error"]
    assert (np.sum(err[:3] ** 2, (0, 1)) <= 4.0 * plan["position_cutoff"] ** 2).all()
    assert (np.sum(err[3:] ** 2, (0, 1)) <= 4.0 * plan["orientation_cutoff"] ** 2).all()
    assert np.array_equal(inputs["reference_relative_pose"][..., 0], expected["relative_pose"][..., 0])
    # (the position error is exactly 0; `quat_multiply` leaves a few 1e-17 of conj(q) q, which the rewards do not see)
    assert (err[:3, :, 0] == 0.0).all() and np.abs(err[3:, :, 0]).max() <= 1e-16 and (expected["scalars"][:, 0] == 1.0).all()
    assert (expected["scalars"][:, 1:] < 1.0).all() and (expected["scalars"] > 1e-9).all()
    residual = fp.quat_mul_conj_left(expected["relative_pose"][3:], inputs["reference_relative_pose"][3:])
    assert residual[3, 0, 1] < 0.0 and (residual[3] > 0.0).any()


# ------------------------------------------------------------------------------------------------------ the host side
@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    plan, inputs, expected, n64, n32 = case(name)
    n64, n32 = aligned(plan, n64, expected), aligned(plan, n32, expected)
    assert sorted(n64) == sorted(expected)
    for out in expected:
        assert rel_error(n64[out], expected[out]) <= TOL, out
        assert rel_error(n32[out], expected[out]) <= 2e-6, out      # (sixteen roundings of 6e-8: the yardstick is sane)


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name):
    check_against_the_fixture(name, lambda plan, inputs, dtype: emu.run(plan, inputs, dtype), "emulation")


def test_emulated_mean_quaternion_has_the_defined_sign():
    for name in ("three_feet", "four_feet", "four_feet_wide", "tracking"):
        plan, inputs, _, _, _ = case(name)
        first = inputs["pose"][3:, int(plan["foot_column"][0])]
        for dtype in (np.float64, np.float32):
            mean = emu.run(plan, inputs, dtype, outputs=("mean_pose",))["mean_pose"][3:]
            assert (np.sum(mean * first, 0) >= 0.0).all() and np.abs(np.linalg.norm(mean.astype(np.float64), axis=0) - 1.0).max() <= 4 * np.finfo(dtype).eps


def check_null_outputs_lane_mask_and_cutoffs(run) -> None:
    """`run(plan, inputs, outputs=, mask=, fill=, position_cutoff=, orientation_cutoff=) -> every output` (those not asked for
    keep `fill`), on the `tracking` case."""
    plan, inputs, _, _, _ = case("tracking")
    full = run(plan, inputs, fill=7.25)
    assert all((v != 7.25).all() for v in full.values())
    # an output that is not asked for is not written; the others do not change
    for asked in (("mean_pose",), ("relative_pose", "scalars"), ("tracking_error",), ("mean_odom_pose",), ()):
        got = run(plan, inputs, outputs=asked, fill=7.25)
        for k, v in got.items():
            assert np.array_equal(v, full[k]) if k in asked else (v == 7.25).all(), (asked, k)
    # without a reference neither the error nor the rewards are written
    got = run(plan, {"pose": inputs["pose"]}, fill=7.25)
    assert (got["tracking_error"] == 7.25).all() and (got["scalars"] == 7.25).all()
    assert all(np.array_equal(got[k], full[k]) for k in ("mean_pose", "mean_odom_pose", "relative_pose"))
    # a non-positive cutoff: that reward row is not written
    got = run(plan, inputs, fill=7.25, position_cutoff=0.0)
    assert (got["scalars"][0] == 7.25).all() and np.array_equal(got["scalars"][1], full["scalars"][1])
    got = run(plan, inputs, fill=7.25, orientation_cutoff=-1.0)
    assert (got["scalars"][1] == 7.25).all() and np.array_equal(got["scalars"][0], full["scalars"][0])
    assert np.array_equal(got["tracking_error"], full["tracking_error"])
    # masked lanes only, the others bit for bit
    mask = np.arange(64) % 3 == 0
    got = run(plan, inputs, mask=mask, fill=7.25)
    for k, v in got.items():
        assert np.array_equal(v[..., mask], full[k][..., mask]) and (v[..., ~mask] == 7.25).all(), k
    # one foot: both rewards are 1 without a reference, unless their cutoff is not positive
    plan, inputs, _, _, _ = case("one_foot")
    got = run(plan, inputs, fill=7.25, orientation_cutoff=0.0)
    assert (got["scalars"][0] == 1.0).all() and (got["scalars"][1] == 7.25).all()


def _emu_run(plan, inputs, outputs=fp.OUTPUTS, fill=np.nan, **kw):
    got = emu.run(plan, inputs, outputs=outputs, fill=fill, **kw)
    return {k: got.get(k, np.full(fp.output_shape(k, plan, 64), fill)) for k in fp.OUTPUTS}


def test_emulated_null_pointers_lane_mask_and_cutoffs():
    check_null_outputs_lane_mask_and_cutoffs(_emu_run)


def _good() -> dict:
    plan = case("four_feet")[0]
    return {k: np.array(plan[k]) for k in emu.DESC_KEYS}


def _set_at(index, value):
    def f(a):
        a = a.copy()
        a.reshape(-1)[index] = value
        return a
    return f


def _rejections() -> list:
    """(changes of the description, what the message must say) for every rejection of `jm_footposes_plan_create`."""
    value = lambda v: (lambda a: v)      # noqa: E731
    return [
        (dict(foot_column=lambda a: np.zeros(0, int)), "bad sizes"),
        (dict(foot_column=lambda a: np.arange(65), n_frames=value(100)), "bad sizes"),
        (dict(n_frames=value(0)), "bad sizes"),
        (dict(n_frames=value(3)), "bad sizes"),
        (dict(foot_column=_set_at(0, -1)), "foot_column"),
        (dict(foot_column=_set_at(3, 7)), "out of range"),
        (dict(foot_column=lambda a: np.array([a[0], a[1], a[0], a[3]])), "repeats the column"),
    ]


def _broken(change: dict):
    arrays = _good()
    for k, f in change.items():
        arrays[k] = f(arrays[k])
    desc, keep = footposes.make_desc(**arrays)
    return desc, keep


def test_plan_validation_rejects_every_malformed_description():
    desc, keep = footposes.make_desc(**_good())
    emu.pack(desc)
    d, keep_ = footposes.make_desc(foot_column=np.arange(64), n_frames=64)       # (the cap itself is accepted)
    emu.pack(d)
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    d, keep_ = footposes.make_desc(**_good())
    d.foot_column = None
    with pytest.raises(ValueError, match="null array"):
        emu.pack(d)
    for change, message in _rejections():
        d, keep_ = _broken(change)
        with pytest.raises(ValueError, match=message):
            emu.pack(d)


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
    assert lib.L.jm_footposes_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = footposes.make_desc(**_good())
    assert lib.L.jm_footposes_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.foot_column = None
    assert lib.L.jm_footposes_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)
    for change, message in _rejections():
        d, keep_ = _broken(change)
        rc = lib.L.jm_footposes_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and message in _last_error(lib), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    io = _abi.FootPosesIO()
    assert lib.L.jm_block_foot_poses(None, _abi.JM_F64, 64, C.byref(io), 0.0, 0.0, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    assert "typedef struct jm_footposes_desc" in header and "typedef struct jm_footposes_io" in header
    assert [f[0] for f in _abi.FootPosesDesc._fields_] == ["n_frames", "n_feet", "foot_column"]
    # the order of the pointers of jm_footposes_io in the header is the order of the ctypes mirror
    body = header.split("typedef struct jm_footposes_io")[1].split("} jm_footposes_io;")[0]
    order = [line.split("*")[1].strip(" ;") for line in body.splitlines() if "*" in line]
    assert order == list(_abi.FOOTPOSES_IO_FIELDS)
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


@pytest.mark.parametrize("name, feet", [("anymal", ["LF_KFE", "LH_KFE", "RF_KFE", "RH_KFE"]), ("atlas", ["l_leg_akx", "r_leg_akx"])])
def test_host_plan_of_the_builtin_walkers(name, feet):
    model = load_builtin(name)
    names = ["root_joint"] + feet[::-1] + list(model.contacts)
    plan = footposes.build_plan(model, names)
    assert plan.foot_frame_names == feet and plan.n_feet == len(feet) and plan.n_frames == len(names)
    assert list(plan.arrays["foot_column"]) == list(range(len(feet), 0, -1))           # sorted names, wherever their columns are
    emu.pack(plan.desc()[0])
    one = footposes.build_plan(model, names, foot_frame_names=feet[1:2])
    assert one.foot_frame_names == feet[1:2] and list(one.arrays["foot_column"]) == [names.index(feet[1])]


def test_python_surface_refusals_on_the_host():
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.envs import WalkerVecEnv
    model = load_builtin("anymal")
    feet = ["LF_KFE", "LH_KFE", "RF_KFE", "RH_KFE"]
    with pytest.raises(ValueError, match="lacks the foot frames.*RH_KFE"):
        footposes.build_plan(model, ["root_joint"] + feet[:3])
    with pytest.raises(ValueError, match="end-effectors"):
        footposes.build_plan(model, feet, foot_frame_names=["root_joint"])
    with pytest.raises(ValueError, match="At least one frame"):
        footposes.build_plan(model, feet, foot_frame_names=[])
    with pytest.raises(ValueError, match="floating base"):
        footposes.build_plan(load_builtin("arm7"), feet)

    def engine(model=model):
        return SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _fields={},
                               _lib=SimpleNamespace(L=None, check=None))

    def frames_of(eng, frame_names=feet):
        return SimpleNamespace(_eng=eng, frame_names=list(frame_names), index=list(frame_names).index)
    make = blocks.FootPoseQuantities
    eng = engine(model=load_builtin("arm7"))
    with pytest.raises(ValueError, match="free-flyer"):
        make(eng, frames_of(eng))
    eng = engine()
    with pytest.raises(ValueError, match="another engine"):
        make(eng, frames_of(engine()))
    with pytest.raises(ValueError, match="lacks the foot frames.*LF_KFE"):
        make(eng, frames_of(eng, feet[1:]))
    with pytest.raises(ValueError, match="cutoff must be positive"):
        make(eng, frames_of(eng), position_cutoff=0.0)
    with pytest.raises(ValueError, match="cutoff must be positive"):
        make(eng, frames_of(eng), orientation_cutoff=-0.5)
    names_ = blocks.footposes_fieldnames(feet)
    assert names_["scalars"] == ["reward_foot_positions", "reward_foot_orientations"] and len(names_["relative_pose"][0]) == 3
    assert names_["relative_pose"][6][2] == "RF_KFE.RelativeQuatW" and names_["tracking_error"][3][0] == "LF_KFE.ErrorAngX"
    assert names_["mean_odom_pose"][2] == "FootMeanOdom.Yaw" and names_["mean_pose"][0] == "FootMean.X"
    # the environment adds the foot frames to what the frames block evaluates; without the argument nothing changes
    contacts = ["root_joint"] + list(model.contacts)
    assert WalkerVecEnv.frame_kinematics_config(model, {}, {}, None, {}) == (feet, None, {})
    assert WalkerVecEnv.frame_kinematics_config(model, dict(frame_names=["imu_link", "RF_KFE"], reference_frames=["LOCAL", 1]), {}, None,
                                                dict(position_cutoff=0.1)) == (["imu_link", "RF_KFE", "LF_KFE", "LH_KFE", "RH_KFE"],
                                                                               ["LOCAL", 1, "LOCAL", "LOCAL", "LOCAL"], {})
    assert WalkerVecEnv.frame_kinematics_config(model, {}, {}, dict(momentum=False), dict(foot_frame_names=feet[:2])) == \
        (contacts + feet[:2], None, {})
    assert WalkerVecEnv.frame_kinematics_config(model, {}, {}, dict(momentum=False)) == (contacts, None, {})


# ------------------------------------------------------------------------------------------------------------ device
class DeviceFootPoses:
    """A plan on the device and the launch on numpy arrays (copied in and out)."""

    def __init__(self, lib, plan: dict, device):
        import torch
        self.torch, self.lib, self.device, self.plan = torch, lib, device, plan
        desc, keep = emu.plan_desc(plan)
        self.h = C.c_void_p()
        with torch.cuda.device(device):
            lib.check(lib.L.jm_footposes_plan_create(C.byref(desc), C.byref(self.h)))

    def close(self):
        self.lib.L.jm_footposes_plan_destroy(self.h)

    def run(self, inputs: dict, dtype=np.float64, outputs=fp.OUTPUTS, mask=None, fill=np.nan, position_cutoff=None, orientation_cutoff=None):
        torch = self.torch
        B = inputs["pose"].shape[-1]
        io, held, out = _abi.FootPosesIO(), [], {}
        for name, a in inputs.items():
            t = torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=self.device)
            held.append(t)
            setattr(io, name, t.data_ptr() if t.numel() else None)
        if mask is not None:
            held.append(torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device=self.device))
            io.lane_mask = held[-1].data_ptr()
        for name in fp.OUTPUTS:
            out[name] = torch.full(fp.output_shape(name, self.plan, B), fill, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device=self.device)
            if name in outputs and out[name].numel():
                setattr(io, name, out[name].data_ptr())
        pc = self.plan["position_cutoff"] if position_cutoff is None else position_cutoff
        oc = self.plan["orientation_cutoff"] if orientation_cutoff is None else orientation_cutoff
        self.lib.check(self.lib.L.jm_block_foot_poses(self.h, _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B, C.byref(io),
                                                      float(pc), float(oc), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        del held
        return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, gpu_device):
    """Every fixture case through the C ABI at B = 64, both dtypes."""
    dev = DeviceFootPoses(_prebuilt(load_builtin("cartpole")), case(name)[0], gpu_device)
    try:
        check_against_the_fixture(name, lambda plan, inputs, dtype: dev.run(inputs, dtype), "device")
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_is_independent_of_the_batch_mates(gpu_device):
    """`four_feet` tiled to B = 70 (a full wave and a partial second one), the lanes rotated by 29: lane b of the tiled batch
    gives the bits lane (b + 29) % 64 gives at B = 64, in both dtypes."""
    plan, inputs = case("four_feet")[:2]
    dev = DeviceFootPoses(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        lanes = (np.arange(70) + 29) % 64
        tiled = {k: np.ascontiguousarray(v[..., lanes]) for k, v in inputs.items()}
        for dtype in (np.float64, np.float32):
            small, big = dev.run(inputs, dtype), dev.run(tiled, dtype)
            for out in ("mean_pose", "mean_odom_pose", "relative_pose"):
                assert big[out].shape[-1] == 70 and np.array_equal(big[out], small[out][..., lanes]), (out, dtype)
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_null_outputs_cutoffs_and_lane_mask(gpu_device):
    """An output that is not asked for keeps its poison; a non-positive cutoff or a null reference leaves the reward rows;
    with a mask the other lanes keep every bit."""
    lib = _prebuilt(load_builtin("cartpole"))
    devs = {name: DeviceFootPoses(lib, case(name)[0], gpu_device) for name in ("tracking", "one_foot")}
    try:
        check_null_outputs_lane_mask_and_cutoffs(lambda plan, inputs, **kw: devs["tracking" if n_feet(plan) == 4 else "one_foot"].run(inputs, **kw))
    finally:
        for dev in devs.values():
            dev.close()


def _walked_anymal(device, B=64, steps=4, seed=3, **kw):
    """An ANYmal environment with constraint contacts after a few steps of random actions (the feet leave their neutral poses)."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    env = make_anymal_env(B, device=device, contact_model="constraint", auto_reset=False, **kw)
    env.reset(seed=seed)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    out = None
    for _ in range(steps):
        action = (0.5 * (2.0 * torch.rand(B, env.model.nmotors, generator=gen, dtype=torch.float64) - 1.0)).to(device)
        out = env.step(action)
    return env, out


def _block_inputs(env) -> dict:
    """The tensors the block of an environment read at its last refresh, as numpy arrays in the layout of the kernel's inputs."""
    return dict(pose=env.frames.pose.cpu().numpy(), reference_relative_pose=env.foot_poses.reference_relative_pose.cpu().numpy())


def _block_plan(env) -> dict:
    b = env.foot_poses
    return dict(b.plan.arrays, position_cutoff=b.position_cutoff or 0.0, orientation_cutoff=b.orientation_cutoff or 0.0)


def _hamilton(l, r):
    lx, ly, lz, lw = l
    rx, ry, rz, rw = r
    return np.stack([lw * rx + lx * rw + ly * rz - lz * ry, lw * ry - lx * rz + ly * rw + lz * rx,
                     lw * rz + lx * ry - ly * rx + lz * rw, lw * rw - lx * rx - ly * ry - lz * rz])


@pytest.mark.gpu
def test_block_laws_on_a_walking_anymal(gpu_device):
    """`make_anymal_env(64, contact_model="constraint", foot_poses=...)`, 4 steps of random actions.  The device against the
    host composition (the numpy restatement on the tensors the block read) within 1e-13 times the conditioning of the lane's
    eigenvector (`conditioning`: the knees of ANYmal bend opposite ways, front and hind), and three laws on the block's tensors,
    each within 4 x the error the host composition leaves against the same law, plus 4 x 2.2e-16: the mean position is the mean
    of the foot positions; the mean composed with relative pose i gives back foot pose i; the mean quaternion is a unit
    eigenvector of sum q q^T."""
    import torch

    from jiminy_amd import blocks
    env, _ = _walked_anymal(gpu_device, foot_poses=dict(position_cutoff=0.2, orientation_cutoff=0.5))
    block = env.foot_poses
    assert env.frames.frame_names == block.foot_frame_names == ["LF_KFE", "LH_KFE", "RF_KFE", "RH_KFE"]
    assert block.fieldnames == blocks.footposes_fieldnames(block.foot_frame_names)
    # the reference of some lanes: their current relative pose; the others keep the initial one (zero positions, unit quaternions)
    lane = torch.arange(64, device=gpu_device)
    assert (block.reference_relative_pose[:6] == 0).all() and (block.reference_relative_pose[6] == 1).all()
    ref_tensor = block.reference_relative_pose
    block.set_reference_from_current(lane % 2 == 0)
    assert block.reference_relative_pose is ref_tensor
    assert torch.equal(ref_tensor[..., 0::2], block.relative_pose[..., 0::2]) and (ref_tensor[:6, :, 1::2] == 0).all()
    block.refresh()
    torch.cuda.synchronize(gpu_device)
    inputs, plan = _block_inputs(env), _block_plan(env)
    host = fp.quantities(plan, inputs)
    dev = {k: getattr(block, k).cpu().numpy() for k in fp.OUTPUTS}
    cols = [int(c) for c in plan["foot_column"]]
    factor = conditioning(inputs["pose"][3:, cols])
    print(f"walking ANYmal: 0.1 / relative gap of the two largest eigenvalues up to {factor.max():.3g} (median {np.median(factor):.3g})")
    amplify = {k: 1.0 for k in fp.OUTPUTS}
    amplify["scalars"] = np.maximum(reward_sensitivity(host["tracking_error"][:3], plan["position_cutoff"]),
                                    reward_sensitivity(host["tracking_error"][3:], plan["orientation_cutoff"]))
    for k in fp.OUTPUTS:
        e = lane_error(dev[k], host[k])
        print(f"walking ANYmal, device against the host composition, {k}: {e.max():.2e}, over its lane's bar {(e / (TOL * factor * amplify[k])).max():.3f}")
        assert (e <= TOL * factor * amplify[k]).all(), k
    assert (dev["tracking_error"][:3, :, 0::2] == 0).all() and (dev["scalars"][:, 0::2] == 1.0).all() and (dev["scalars"][:, 1::2] < 1.0).all()
    p, q = inputs["pose"][:3, cols], inputs["pose"][3:, cols]
    assert np.abs(p[:, 0] - p[:, 3]).max() > 0.3 and np.abs(q[:, 0] - q[:, 1]).max() > 1e-3       # four distinct feet

    def law(name, value):
        e_dev, e_host = value(dev), value(host)
        print(f"law {name}: device {e_dev:.2e}, host composition {e_host:.2e}")
        assert e_dev <= 4.0 * e_host + 4.0 * EPS, (name, e_dev, e_host)
    law("mean position = mean of the foot positions", lambda o: rel_error(o["mean_pose"][:3], p.sum(1) / 4.0))

    def recomposed(o):
        R = fp.quat_matrix(o["mean_pose"][3:])
        back_p = o["mean_pose"][:3, None] + np.einsum("ijb,jfb->ifb", R, o["relative_pose"][:3])
        back_q = _hamilton(o["mean_pose"][3:, None], o["relative_pose"][3:])
        back_q = back_q * np.sign(np.sum(back_q * q[:, :-1], 0))
        return max(rel_error(back_p, p[:, :-1]), rel_error(back_q, q[:, :-1]))
    law("mean o relative pose i = foot pose i", recomposed)
    M = fp.gram(q)

    def eigen_residual(o):
        m = o["mean_pose"][3:].T
        lam = np.einsum("bi,bij,bj->b", m, M, m)
        return float(np.linalg.norm(np.einsum("bij,bj->bi", M, m) - lam[:, None] * m, axis=1).max())
    law("‖M q - lambda q‖ of the mean quaternion", eigen_residual)
    law("|‖q‖ - 1| of the mean quaternion", lambda o: float(np.abs(np.linalg.norm(o["mean_pose"][3:], axis=0) - 1.0).max()))
    assert (np.sum(dev["mean_pose"][3:] * q[:, 0], 0) >= 0).all()
    # `reset(lane_mask)`: the masked lanes are evaluated, the others keep every tensor bit for bit
    tensors = {k: getattr(block, k) for k in fp.OUTPUTS}
    full = {k: t.clone() for k, t in tensors.items()}
    for t in tensors.values():
        t.fill_(7.25)
    mask = lane % 3 == 0
    block.reset(mask)
    for k, t in tensors.items():
        assert t is getattr(block, k)
        assert torch.equal(t[..., ~mask], torch.full_like(t[..., ~mask], 7.25)) and torch.equal(t[..., mask], full[k][..., mask]), k
    block.refresh()
    assert all(torch.equal(t, full[k]) for k, t in tensors.items())
    with pytest.raises(ValueError, match="lane_mask must have shape"):
        block.reset(mask[:5])
    env.close()


def _same(a, b) -> bool:
    """Two step results (nested tuples / dictionaries of tensors) hold the same bits."""
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return bool((a == b).all()) if hasattr(a, "shape") else a == b


@pytest.mark.gpu
def test_environment_tracking_rewards(gpu_device):
    """`make_anymal_env(32, contact_model="constraint", foot_poses=..., reward_mixture={'foot_positions': 0.5, 'foot_orientations':
    0.25})` with `set_reference_from_current()` at reset: the reward is its weights at step 0 and the numpy restatement on the
    block's tensors afterwards; the block does not touch the physics, and an environment without the keyword has no block."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    B, steps = 32, 4
    mixture = {"foot_positions": 0.5, "foot_orientations": 0.25}
    cfg = dict(position_cutoff=0.2, orientation_cutoff=0.5)
    common = dict(device=gpu_device, contact_model="constraint", auto_reset=False)
    with pytest.raises(ValueError, match="foot_poses"):
        make_anymal_env(B, reward_mixture={"foot_positions": 1.0}, **common)
    with pytest.raises(ValueError, match="orientation_cutoff"):
        make_anymal_env(B, reward_mixture={"foot_orientations": 1.0}, foot_poses=dict(position_cutoff=0.1), **common)
    env = make_anymal_env(B, foot_poses=cfg, reward_mixture=mixture, **common)
    plain, plain2 = make_anymal_env(B, **common), make_anymal_env(B, **common)
    assert plain.foot_poses is None and plain.frames is None and env.locomotion is None and env.actuation is None
    envs = (env, plain, plain2)
    for e in envs:
        e.reset(seed=11)
    block = env.foot_poses
    block.set_reference_from_current()
    block.refresh()
    reward0 = env.compute_reward(torch.zeros(B, dtype=torch.bool, device=gpu_device))
    assert (block.scalars == 1.0).all() and (reward0 == 0.75).all()
    gen = torch.Generator(device="cpu").manual_seed(5)
    plan, worst = _block_plan(env), 0.0
    for i in range(steps):
        action = (0.5 * (2.0 * torch.rand(B, env.model.nmotors, generator=gen, dtype=torch.float64) - 1.0)).to(gpu_device)
        out = [e.step(action) for e in envs]
        inputs = _block_inputs(env)
        host = fp.quantities(plan, inputs)
        want = 0.5 * host["scalars"][0] + 0.25 * host["scalars"][1]
        # (per lane: the bar of the fixture times the conditioning of the lane's eigenvector and the slope of the rewards)
        bar = TOL * conditioning(inputs["pose"][3:, [int(c) for c in plan["foot_column"]]]) * np.maximum(
            reward_sensitivity(host["tracking_error"][:3], plan["position_cutoff"]),
            reward_sensitivity(host["tracking_error"][3:], plan["orientation_cutoff"]))
        e = lane_error(out[0][1].cpu().numpy(), want)
        worst = max(worst, float((e / bar).max()))
        assert (e <= bar).all(), (i, float(e.max()), float(bar.min()))
        assert _same(out[1], out[2]), i
        assert torch.equal(env.engine.robot_state.q, plain.engine.robot_state.q) and torch.equal(env.engine.robot_state.v, plain.engine.robot_state.v)
        assert _same(out[0][0], out[1][0]) and _same(out[0][2:4], out[1][2:4]), i
    print(f"environment: reward against the numpy restatement, largest error over its lane's bar {worst:.3f}; last rewards {float(out[0][1].min()):.3f} .. {float(out[0][1].max()):.3f}")
    assert float(out[0][1].max()) < 0.75 and float(out[0][1].min()) > 0.0            # the feet moved, inside the cutoffs' reach
    # a partial reset: the reset lanes are evaluated at their reset state, the others keep every bit
    mask = torch.arange(B, device=gpu_device) % 2 == 0
    tensors = {k: getattr(block, k) for k in fp.OUTPUTS}
    kept = {k: t.clone() for k, t in tensors.items()}
    env.reset_lanes(mask)
    for k, t in tensors.items():
        assert t is getattr(block, k) and torch.equal(t[..., ~mask], kept[k][..., ~mask]), k
    assert not torch.equal(block.mean_pose[..., mask], kept["mean_pose"][..., mask])
    for e in envs:
        e.close()
