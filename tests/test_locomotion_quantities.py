"""Locomotion quantities on the device (csrc/jm_locomotion.h behind `jm_block_locomotion`, `blocks.LocomotionQuantities`, the
`flying` / `impact_force` terminations and the `momentum` / `friction` reward terms of `WalkerVecEnv`).

Specification: the reference's own output, tests/golden/ref_locomotion.npz (tools/make_ref_locomotion_fixtures.py executes the
reference's functions; five cases of 64 lanes).  float64 within 1e-13 relative to max(|want|, 1) on every lane and output, NaN
positions identical (the NaN lanes of `free_fall` are exactly the designed ones, every other lane of every output is finite);
float32 within 4 x the error of the float32 numpy restatement (tests/locomotion_numpy.py) on the same case and quantity.

Measured on the host (error relative to max(|want|, 1), largest over the five cases and the lanes):
  float64, host emulation | numpy restatement
    com 0 | 0   vcom 0 | 0   odom_pose 2.2e-16 | 0   zmp 1.1e-15 | 0   dcm 1.1e-15 | 0   h_angular 4.6e-16 | 4.6e-16
    contact_force_rel 0 | 0   foot_force_vertical 0 | 0   scalars 1.1e-16 | 1.1e-16
  float32, host emulation | numpy restatement (the error is that of rounding the inputs to float32)
    com 5.9e-8 | 5.9e-8   vcom 9.6e-8 | 9.6e-8   odom_pose 1.1e-7 | 1.4e-7   zmp 7.6e-7 | 7.6e-7   dcm 7.1e-7 | 7.2e-7
    h_angular 3.9e-7 | 3.9e-7   contact_force_rel 1.4e-7 | 1.4e-7   foot_force_vertical 1.8e-7 | 1.8e-7   scalars 1.5e-7 | 1.5e-7
  largest ratio emulation / restatement of one case and quantity in float32: 1.8 (dcm, `regular`).

Physics laws (ANYmal, 64 lanes, constraint contacts, settled on flat ground under zero action): the bound of every law is
4 x the error of the host composition -- the numpy restatement evaluated on the tensors the block read -- against the same
law, plus 4 x 2.2e-16 for the roundings of the law's own right-hand side (a division by the weight, a 3 x 3 rotation).

Measured on the device (MI355X; the same five cases through the C ABI, largest over the cases and the lanes):
  float64  com 0   vcom 0   odom_pose 2.5e-16   zmp 1.8e-15   dcm 1.2e-15   h_angular 4.3e-16   contact_force_rel 0
           foot_force_vertical 0   scalars 2.2e-16
  float32  com 5.9e-8   vcom 9.6e-8   odom_pose 1.5e-7   zmp 8.5e-7   dcm 7.2e-7   h_angular 3.3e-7   contact_force_rel 1.4e-7
           foot_force_vertical 1.8e-7   scalars 1.4e-7; largest ratio device / numpy float32 of one case and quantity: 1.47 (dcm)
  settled ANYmal, device against the host composition on the same tensors: 0 on every output but the scalars (1.1e-16, `pow`).
  Laws, device | host composition: sum of foot_force_vertical = 1: 4.70e-7 | 4.70e-7 (|dhg_linear_z| / weight is 4.70e-7: what
  the solver leaves); contact_force_rel = R contact_forces / weight: 5.6e-17 | 5.6e-17; com = centroidal: 0 | 0;
  vcom = hg_linear / mass: 5.4e-20 | 5.4e-20.  Environment: reward against the numpy restatement 1.3e-16; the dropped lanes
  show 10.1 times the weight on one contact point at the end of step 8, the standing ones 0.25 to 0.26.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, codegen, load_builtin, locomotion
from tests import frames_numpy as fn
from tests import locomotion_numpy as ln
from tests.hostemu import locomotion as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_locomotion.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_locomotion_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
TOL = 1e-13
EPS = 2.2e-16
NEW_SYMBOLS = ("jm_locomotion_plan_create", "jm_locomotion_plan_destroy", "jm_block_locomotion")
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["cases"]]
_CASES: dict = {}


def case(name: str):
    """plan, inputs, expected, designed NaN lanes and the two numpy restatements of a case, computed once."""
    if name not in _CASES:
        plan, inputs, expected, designed = ln.load_case(FX, name)
        _CASES[name] = (plan, inputs, expected, designed, ln.quantities(plan, inputs, np.float64), ln.quantities(plan, inputs, np.float32))
    return _CASES[name]


def rel_error(got: np.ndarray, want: np.ndarray, designed_nan=None) -> float:
    """Largest error relative to max(|want|, 1); NaN positions must be identical, and the designed ones where given."""
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and not np.isinf(got).any()
    if designed_nan is not None:
        assert np.array_equal(nan, np.broadcast_to(designed_nan, nan.shape))
    e = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
    return float(np.where(nan, 0.0, e).max())


def check_against_the_fixture(name: str, run, label: str) -> None:
    """`run(plan, inputs, dtype) -> outputs` against the fixture in both dtypes."""
    plan, inputs, expected, designed, _, n32 = case(name)
    for dtype in (np.float64, np.float32):
        got = run(plan, inputs, dtype)
        for out in ln.OUTPUTS:
            designed_nan = designed if out == "zmp" else np.zeros_like(designed)
            e = rel_error(got[out], expected[out], designed_nan)
            if dtype is np.float64:
                print(f"{label} {name} float64 {out}: {e:.2e}")
                assert e <= TOL, (name, out, e)
            else:
                e_np = rel_error(n32[out], expected[out], designed_nan)
                print(f"{label} {name} float32 {out}: {e:.2e} (numpy float32 {e_np:.2e})")
                assert e <= 4.0 * e_np, (name, out, e, e_np)


# ------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_from_the_reference_tree():
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        pytest.skip("the reference tree is not here: the committed fixture stands")
    subprocess.check_call([sys.executable, TOOL, "--check"], stdout=subprocess.DEVNULL)


def test_fixture_holds_the_designed_cases():
    assert CASES == ["regular", "grouped", "one", "free_fall", "per_lane_model"] and os.path.getsize(FIXTURE) <= 1 << 20
    for name in CASES:
        plan, inputs, expected, designed, _, _ = case(name)
        assert inputs["centroidal"].shape == (15, 64) and designed.shape == (64,)
        assert ("model_lane" in inputs) == (name == "per_lane_model")
        nan = {k: np.isnan(v) for k, v in expected.items()}
        assert all(not m.any() for k, m in nan.items() if k != "zmp")
        assert np.array_equal(nan["zmp"], np.broadcast_to(designed, (2, 64)))                 # no lane left out anywhere else
        assert designed.any() == (name == "free_fall")
        # the draw of the issue
        c = inputs["centroidal"]
        mass = np.sum(inputs["model_lane"][0::13][1:], 0) if "model_lane" in inputs else np.sum(plan["body_mass"][1:])
        r = (c[11] + mass * plan["gravity"]) / (mass * plan["gravity"])
        assert ((r >= 0.2) & (r <= 3.0))[~designed].all() and (r[designed] == 0.0).all()
        assert np.abs(c[:2]).max() <= 2.0 and c[2].min() >= 0.2 and c[2].max() <= 1.5
        assert (np.sum(expected["h_angular"] ** 2, 0) <= 4.0 * plan["momentum_cutoff"] ** 2 * (1 + 1e-12)).all()
        assert (np.sum(expected["contact_force_rel"][:2] ** 2, (0, 1)) <= 4.0 * plan["friction_cutoff"] ** 2).all()
    assert list(FX["regular.plan.contact_foot"]) == [0, 1, 2, 3] and list(FX["grouped.plan.contact_foot"]) == [0, 0, 0, -1, 1, 1, 1, 1]
    assert list(FX["one.plan.contact_foot"]) == [0] and list(np.flatnonzero(FX["free_fall.designed_nan"])) == list(range(1, 64, 2))
    assert ((FX["grouped.con_flags"] & 1) == 0).any() and ((FX["regular.con_flags"] & 1) == 1).all()


# ------------------------------------------------------------------------------------------------------ the host side
@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    plan, inputs, expected, designed, n64, n32 = case(name)
    for out in ln.OUTPUTS:
        assert rel_error(n64[out], expected[out]) <= TOL, out
        assert rel_error(n32[out], expected[out]) <= 2e-6, out      # (sixteen roundings of 6e-8: the yardstick is sane)


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name):
    check_against_the_fixture(name, lambda plan, inputs, dtype: emu.run(plan, inputs, dtype), "emulation")


def test_emulated_null_pointers_lane_mask_and_cutoffs():
    plan, inputs, expected, _, _, _ = case("grouped")
    full = emu.run(plan, inputs)
    # an output that is not asked for is not written; the others do not change
    some = emu.run(plan, inputs, outputs=("zmp", "scalars"))
    assert sorted(some) == ["scalars", "zmp"] and all(np.array_equal(some[k], full[k]) for k in some)
    # without the inputs of a part, its outputs keep the sentinel
    got = emu.run(plan, {k: v for k, v in inputs.items() if k not in ("con_lambda", "v_avg")})
    assert np.isnan(got["contact_force_rel"]).all() and np.isnan(got["foot_force_vertical"]).all() and np.isnan(got["h_angular"]).all()
    assert np.isnan(got["scalars"][[0, 2, 3]]).all() and np.array_equal(got["scalars"][1], full["scalars"][1])
    assert np.array_equal(got["zmp"], full["zmp"]) and np.array_equal(got["com"], full["com"])
    got = emu.run(plan, {k: v for k, v in inputs.items() if k != "q_root"})
    assert np.isnan(got["odom_pose"]).all() and np.isnan(got["dcm"]).all()        # (LOCAL: needs the odometry pose)
    assert np.array_equal(got["zmp"], full["zmp"])                                 # (LOCAL_WORLD_ALIGNED: does not)
    # a non-positive cutoff: that reward row is not written
    got = emu.run(plan, inputs, momentum_cutoff=0.0, friction_cutoff=-1.0)
    assert np.isnan(got["scalars"][2:]).all() and np.array_equal(got["scalars"][:2], full["scalars"][:2])
    # masked lanes only, the others bit for bit
    mask = np.arange(64) % 3 == 0
    into = {k: np.full_like(v, 7.25) for k, v in full.items()}
    emu.run(plan, inputs, mask=mask, into=into)
    for k, v in into.items():
        assert np.array_equal(v[..., mask], full[k][..., mask], equal_nan=True) and (v[..., ~mask] == 7.25).all(), k
    # a disabled contact contributes zero whatever its rows hold
    off = (inputs["con_flags"] & 1) == 0
    assert off.any() and (full["contact_force_rel"][:, off] == 0.0).all()
    assert (np.abs(inputs["con_lambda"].reshape(-1, 4, 64)[:, 2][off]) > 0).all()


def _good() -> dict:
    plan = case("grouped")[0]
    return {k: np.array(plan[k]) for k in emu.DESC_KEYS}


def _set_at(index, value):
    def f(a):
        a = a.copy()
        a.reshape(-1)[index] = value
        return a
    return f


def _rejections() -> list:
    """(changes of the description, what the message must say) for every rejection of `jm_locomotion_plan_create`."""
    value = lambda v: (lambda a: v)      # noqa: E731
    return [
        (dict(body_mass=lambda a: a[:1]), "bad sizes"),
        (dict(contact_foot=lambda a: np.zeros(0, int), contact_column=lambda a: np.zeros(0, int)), "bad sizes"),
        (dict(n_feet=value(0)), "bad sizes"),
        (dict(n_feet=value(9)), "bad sizes"),
        (dict(n_frames=value(0)), "bad sizes"),
        (dict(contact_foot=lambda a: np.zeros(300, int), contact_column=lambda a: np.zeros(300, int)), "bad sizes"),
        (dict(body_mass=_set_at(2, -1.0)), "body_mass"),
        (dict(body_mass=_set_at(3, np.nan)), "body_mass"),
        (dict(body_mass=lambda a: np.zeros_like(a)), "no mass"),
        (dict(root_inertia=_set_at(4, np.inf)), "root_inertia"),
        (dict(gravity=value(0.0)), "gravity"),
        (dict(gravity=value(-9.81)), "gravity"),
        (dict(gravity=value(np.nan)), "gravity"),
        (dict(omega=value(0.0)), "omega"),
        (dict(omega=value(np.inf)), "omega"),
        (dict(zmp_frame=value(2)), "Reference frame"),
        (dict(dcm_frame=value(-1)), "Reference frame"),
        (dict(root_column=value(-1)), "root_column"),
        (dict(root_column=value(10)), "root_column"),
        (dict(contact_foot=_set_at(0, 2)), "contact_foot"),
        (dict(contact_foot=_set_at(0, -2)), "contact_foot"),
        (dict(contact_column=_set_at(1, 10)), "contact_column"),
        (dict(contact_column=_set_at(1, -1)), "contact_column"),
        (dict(contact_foot=lambda a: np.array([0, 1, 0, -1, 1, 1, 1, 1])), "must be consecutive"),
        (dict(contact_foot=lambda a: np.array([0, 0, -1, 0, 1, 1, 1, 1])), "must be consecutive"),
        (dict(contact_foot=lambda a: np.array([0, 0, 0, -1, -1, -1, -1, -1])), "has no contact"),
    ]


def _broken(change: dict):
    arrays = _good()
    for k, f in change.items():
        arrays[k] = f(arrays[k])
    desc, keep = locomotion.make_desc(**arrays)
    if len(arrays["contact_foot"]) == 0:
        desc.n_contacts = 0
    return desc, keep


def test_plan_validation_rejects_every_malformed_description():
    desc, keep = locomotion.make_desc(**_good())
    emu.pack(desc)
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    for field in ("body_mass", "root_inertia", "contact_foot", "contact_column"):
        d, keep_ = locomotion.make_desc(**_good())
        setattr(d, field, None)
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
    assert lib.L.jm_locomotion_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = locomotion.make_desc(**_good())
    assert lib.L.jm_locomotion_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.contact_foot = None
    assert lib.L.jm_locomotion_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)
    for change, message in _rejections():
        d, keep_ = _broken(change)
        rc = lib.L.jm_locomotion_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and message in _last_error(lib), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    io = _abi.LocomotionIO()
    assert lib.L.jm_block_locomotion(None, _abi.JM_F64, 64, C.byref(io), 0.0, 0.0, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    assert "typedef struct jm_locomotion_desc" in header and "typedef struct jm_locomotion_io" in header
    assert [f[0] for f in _abi.LocomotionDesc._fields_] == ["njoints", "body_mass", "root_inertia", "gravity", "omega", "n_contacts",
                                                            "n_feet", "contact_foot", "contact_column", "n_frames", "root_column",
                                                            "zmp_frame", "dcm_frame"]
    # the order of the pointers of jm_locomotion_io in the header is the order of the ctypes mirror
    body = header.split("typedef struct jm_locomotion_io")[1].split("} jm_locomotion_io;")[0]
    order = [line.split("*")[1].strip(" ;") for line in body.splitlines() if "*" in line]
    assert order == list(_abi.LOCOMOTION_IO_FIELDS)
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


def _numpy_omega(model) -> float:
    """sqrt(g / (com_z - lowest contact z)) at the neutral configuration by the 4x4 forward kinematics of tests/frames_numpy.py."""
    q = model.neutral()[:, None]
    oMj = fn.joint_transforms(model, q[:, 0])
    com = sum(model.mass[j] * (oMj[j] @ np.append(model.com[j], 1.0))[:3] for j in range(1, model.njoints)) / model.mass[1:].sum()
    z = fn.frames(model, list(model.contacts), q)["pose"][2, :, 0]
    return float(np.sqrt(abs(model.gravity[2]) / (com[2] - z.min())))


@pytest.mark.parametrize("name, feet, grouping", [
    ("anymal", ["LF_KFE", "LH_KFE", "RF_KFE", "RH_KFE"], [0, 1, 2, 3]),
    ("atlas", ["l_leg_akx", "r_leg_akx"], [0] * 16 + [1] * 16),
])
def test_host_plan_of_the_builtin_walkers(name, feet, grouping):
    model = load_builtin(name)
    names = ["root_joint"] + list(model.contacts)
    plan = locomotion.build_plan(model, names)
    assert plan.foot_frame_names == feet and plan.contact_foot == grouping and plan.n_feet == len(feet)
    a = plan.arrays
    assert list(a["contact_column"]) == list(range(1, len(names))) and a["root_column"] == 0 and a["n_frames"] == len(names)
    assert a["gravity"] == 9.81 and (a["zmp_frame"], a["dcm_frame"]) == (0, 0)
    assert np.array_equal(a["body_mass"], model.mass) and a["root_inertia"][3] == model.inertia[1][1, 1]
    assert abs(plan.omega - _numpy_omega(model)) <= 1e-13 * plan.omega and 1.0 < plan.omega < 10.0
    emu.pack(plan.desc()[0])
    # the frames of the block in another order, named feet, the other reference frame
    other = locomotion.build_plan(model, names[::-1], foot_frame_names=feet[:1], zmp_reference_frame="LOCAL_WORLD_ALIGNED")
    assert other.arrays["root_column"] == len(names) - 1 and list(other.arrays["contact_column"]) == list(range(len(names) - 1))[::-1]
    assert other.n_feet == 1 and sorted(set(other.contact_foot)) == [-1, 0] and other.arrays["zmp_frame"] == 1


def test_host_plan_refusals():
    model = load_builtin("anymal")
    names = ["root_joint"] + list(model.contacts)
    with pytest.raises(ValueError, match="lacks the frames"):
        locomotion.build_plan(model, names[1:])
    with pytest.raises(ValueError, match="lacks the frames"):
        locomotion.build_plan(model, names[:-1])
    with pytest.raises(ValueError, match="end-effectors"):
        locomotion.build_plan(model, names, foot_frame_names=["root_joint"])
    with pytest.raises(ValueError, match="At least one frame"):
        locomotion.build_plan(model, names, foot_frame_names=[])
    with pytest.raises(ValueError, match="Reference frame must be"):
        locomotion.build_plan(model, names, zmp_reference_frame="ODOMETRY")
    with pytest.raises(ValueError, match="floating base"):
        locomotion.sanitize_foot_frame_names(load_builtin("arm7"))
    # contacts of one foot that are not consecutive (:1440-1449)
    import copy
    shuffled = copy.deepcopy(load_builtin("atlas"))
    shuffled.contacts = shuffled.contacts[:8] + shuffled.contacts[16:24] + shuffled.contacts[8:16] + shuffled.contacts[24:]
    with pytest.raises(ValueError, match="must be consecutive"):
        locomotion.build_plan(shuffled, ["root_joint"] + list(shuffled.contacts))


def test_python_surface_refusals_on_the_host():
    from types import SimpleNamespace

    import torch

    from jiminy_amd import blocks
    from jiminy_amd.envs import WalkerVecEnv
    model = load_builtin("anymal")
    names = ["root_joint"] + list(model.contacts)

    def engine(model=model, fields=("centroidal",), contacts="constraint", ground=None):
        return SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _fields={k: None for k in fields},
                               _options={"contacts": {"model": contacts}}, _ground=ground, _lib=SimpleNamespace(L=None, check=None))

    def frames_of(eng, frame_names=names, average=True, modes=None):
        return SimpleNamespace(_eng=eng, frame_names=list(frame_names), average=average, index=list(frame_names).index,
                               plan=SimpleNamespace(modes=modes or [0] * len(frame_names)))
    make = blocks.LocomotionQuantities
    eng = engine(model=load_builtin("arm7"))
    with pytest.raises(ValueError, match="free-flyer"):
        make(eng, frames_of(eng))
    eng = engine(fields=())
    with pytest.raises(ValueError, match="centroidal"):
        make(eng, frames_of(eng))
    eng = engine()
    with pytest.raises(ValueError, match="another engine"):
        make(eng, frames_of(engine()))
    with pytest.raises(ValueError, match="average=True"):
        make(eng, frames_of(eng, average=False))
    with pytest.raises(ValueError, match="lacks the frames.*root_joint"):
        make(eng, frames_of(eng, names[1:]))
    with pytest.raises(ValueError, match="lacks the frames.*RH_FOOT"):
        make(eng, frames_of(eng, names[:-1]))
    with pytest.raises(ValueError, match="LOCAL step-average"):
        make(eng, frames_of(eng, modes=[2, 0, 0, 0, 0]))
    with pytest.raises(ValueError, match="cutoff must be positive"):
        make(eng, frames_of(eng), momentum_cutoff=0.0)
    with pytest.raises(ValueError, match="switched off"):
        make(eng, frames_of(eng), friction_cutoff=0.5, forces=False)
    eng = engine(contacts="spring_damper")
    with pytest.raises(NotImplementedError, match="spring_damper"):
        make(eng, frames_of(eng))
    eng = engine(ground=torch.zeros(3, 3))
    with pytest.raises(NotImplementedError, match="flat ground"):
        make(eng, frames_of(eng))
    names_ = blocks.locomotion_fieldnames(model.contacts, ["LF_KFE"], True, True)
    assert names_["scalars"] == ["force_vertical_max", "ground_distance_min", "reward_momentum", "reward_friction"]
    assert names_["contact_force_rel"][5][0] == "LF_FOOT.AngZ" and names_["foot_force_vertical"] == ["LF_KFE.ForceVertical"]
    assert sorted(blocks.locomotion_fieldnames(model.contacts, [], False, False)) == ["com", "dcm", "odom_pose", "scalars", "vcom", "zmp"]
    # the environment adds what the block reads
    got = WalkerVecEnv.frame_kinematics_config(model, {}, {}, dict(momentum_cutoff=1.0))
    assert got == (names, None, dict(average=True))
    got = WalkerVecEnv.frame_kinematics_config(model, dict(frame_names=["imu_link"]), {}, dict(momentum=False))
    assert got == (["imu_link"] + names, None, {})


# ------------------------------------------------------------------------------------------------------------ device
class DeviceLocomotion:
    """A plan on the device and the launch on numpy arrays (copied in and out)."""

    def __init__(self, lib, plan: dict, device):
        import torch
        self.torch, self.lib, self.device, self.plan = torch, lib, device, plan
        desc, keep = emu.plan_desc(plan)
        self.h = C.c_void_p()
        with torch.cuda.device(device):
            lib.check(lib.L.jm_locomotion_plan_create(C.byref(desc), C.byref(self.h)))

    def close(self):
        self.lib.L.jm_locomotion_plan_destroy(self.h)

    def run(self, inputs: dict, dtype=np.float64, outputs=ln.OUTPUTS, mask=None, fill=np.nan, momentum_cutoff=None, friction_cutoff=None):
        torch = self.torch
        B = inputs["centroidal"].shape[-1]
        io, held, out = _abi.LocomotionIO(), [], {}
        for name, a in inputs.items():
            t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32 if name == "con_flags" else dtype), device=self.device)
            held.append(t)
            setattr(io, name, t.data_ptr())
        if mask is not None:
            held.append(torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device=self.device))
            io.lane_mask = held[-1].data_ptr()
        for name in ln.OUTPUTS:
            out[name] = torch.full(ln.output_shape(name, self.plan, B), fill, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device=self.device)
            if name in outputs:
                setattr(io, name, out[name].data_ptr())
        mc = self.plan["momentum_cutoff"] if momentum_cutoff is None else momentum_cutoff
        fc = self.plan["friction_cutoff"] if friction_cutoff is None else friction_cutoff
        self.lib.check(self.lib.L.jm_block_locomotion(self.h, _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B, C.byref(io),
                                                      float(mc), float(fc), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        del held
        return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, gpu_device):
    """Every fixture case through the C ABI at B = 64, both dtypes."""
    dev = DeviceLocomotion(_prebuilt(load_builtin("cartpole")), case(name)[0], gpu_device)
    try:
        check_against_the_fixture(name, lambda plan, inputs, dtype: dev.run(inputs, dtype), "device")
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_is_independent_of_the_batch_mates(gpu_device):
    """`regular` tiled to B = 193 (three full waves and one lane), the lanes rotated by 29: lane b of the tiled batch gives the
    bits lane (b + 29) % 64 gives at B = 64, in both dtypes."""
    plan, inputs = case("regular")[:2]
    dev = DeviceLocomotion(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        lanes = (np.arange(193) + 29) % 64
        tiled = {k: np.ascontiguousarray(v[..., lanes]) for k, v in inputs.items()}
        for dtype in (np.float64, np.float32):
            small, big = dev.run(inputs, dtype), dev.run(tiled, dtype)
            for out in ln.OUTPUTS:
                assert big[out].shape[-1] == 193 and np.array_equal(big[out], small[out][..., lanes]), (out, dtype)
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_null_outputs_cutoffs_and_lane_mask(gpu_device):
    """An output that is not asked for keeps its poison; a non-positive cutoff leaves its reward row; with a mask the other
    lanes keep every bit (B = 193: a partial last block)."""
    plan, inputs = case("grouped")[:2]
    dev = DeviceLocomotion(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        lanes = np.arange(193) % 64
        tiled = {k: np.ascontiguousarray(v[..., lanes]) for k, v in inputs.items()}
        full = dev.run(tiled)
        assert all(np.array_equal(full[k], emu.run(plan, tiled)[k]) or rel_error(full[k], emu.run(plan, tiled)[k]) <= TOL for k in full)
        for asked in (("zmp", "scalars"), ("contact_force_rel",), ()):
            got = dev.run(tiled, outputs=asked, fill=7.25)
            for k, v in got.items():
                assert np.array_equal(v, full[k]) if k in asked else (v == 7.25).all(), (asked, k)
        got = dev.run(tiled, fill=7.25, momentum_cutoff=0.0, friction_cutoff=-1.0)
        assert (got["scalars"][2:] == 7.25).all() and np.array_equal(got["scalars"][:2], full["scalars"][:2])
        got = dev.run({k: v for k, v in tiled.items() if k not in ("con_lambda", "pose")}, fill=7.25)
        assert (got["contact_force_rel"] == 7.25).all() and (got["foot_force_vertical"] == 7.25).all() and (got["scalars"][[0, 1, 3]] == 7.25).all()
        assert np.array_equal(got["h_angular"], full["h_angular"]) and np.array_equal(got["scalars"][2], full["scalars"][2])
        mask = np.arange(193) % 3 == 0
        got = dev.run(tiled, mask=mask, fill=7.25)
        for k, v in got.items():
            assert np.array_equal(v[..., mask], full[k][..., mask]) and (v[..., ~mask] == 7.25).all(), k
    finally:
        dev.close()


def _settled_anymal(device, B=64, steps=25, **kw):
    import torch

    from jiminy_amd.envs import make_anymal_env
    env = make_anymal_env(B, device=device, contact_model="constraint", auto_reset=False, **kw)
    env.reset(seed=3)
    action = torch.zeros(B, env.model.nmotors, dtype=torch.float64, device=device)
    for _ in range(steps):
        out = env.step(action)
    return env, out


def _block_inputs(env) -> dict:
    """The tensors the block of an environment read at its last refresh, as numpy arrays in the layout of the kernel's inputs."""
    eng, fk, lq = env.engine, env.frames, env.locomotion
    nc = lq.plan.n_contacts
    inputs = dict(centroidal=eng.field("centroidal"), q_root=eng.field("q")[:7],
                  con_lambda=eng.field("con_data")[lq._lambda_row:lq._lambda_row + 4 * nc],
                  con_flags=eng.field("con_flags")[lq._flag_row:lq._flag_row + nc], v_avg=fk.average_velocity, quat_no_yaw=fk.quat_no_yaw,
                  pose=fk.pose)
    return {k: v.cpu().numpy() for k, v in inputs.items()}


def _block_plan(env) -> dict:
    lq = env.locomotion
    return dict(lq.plan.arrays, momentum_cutoff=lq.momentum_cutoff or 0.0, friction_cutoff=lq.friction_cutoff or 0.0)


def _quat_matrices(q: np.ndarray) -> np.ndarray:
    """Rotation matrices `[..., 3, 3]` of quaternions xyzw `[4][...]`."""
    x, y, z, w = q
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


@pytest.mark.gpu
def test_physics_laws_on_settled_anymal(gpu_device):
    """`make_anymal_env(64, contact_model="constraint", locomotion_quantities=...)`, 25 steps (1 s) under zero action.  Every
    law is checked on the block's tensors within 4 x the error the host composition (the numpy restatement on the tensors the
    block read) leaves against the same law, plus 4 x 2.2e-16."""
    import torch
    env, _ = _settled_anymal(gpu_device, locomotion_quantities=dict(zmp_reference_frame="LOCAL_WORLD_ALIGNED", momentum_cutoff=1.0,
                                                                     friction_cutoff=0.5))
    lq, fk, eng, model = env.locomotion, env.frames, env.engine, env.model
    torch.cuda.synchronize(gpu_device)
    inputs, plan = _block_inputs(env), _block_plan(env)
    host = ln.quantities(plan, inputs)
    dev = {k: getattr(lq, k).cpu().numpy() for k in ln.OUTPUTS}
    for k in ln.OUTPUTS:
        print(f"settled ANYmal, device against the host composition, {k}: {rel_error(dev[k], host[k]):.2e}")
        assert rel_error(dev[k], host[k]) <= TOL, k
    assert ((inputs["con_flags"] & 1) == 1).all() and np.isfinite(dev["zmp"]).all()           # four feet on the ground, every lane
    weight = float(np.sum(model.mass[1:])) * 9.81

    def law(name, got, got_host, want):
        e_dev, e_host = rel_error(got, want), rel_error(got_host, want)
        print(f"law {name}: device {e_dev:.2e}, host composition {e_host:.2e}")
        assert e_dev <= 4.0 * e_host + 4.0 * EPS, (name, e_dev, e_host)
    # the feet carry the weight, up to the vertical acceleration the solver leaves: sum = 1 + dhg_linear_z / weight
    residual = np.abs(inputs["centroidal"][11]) / weight
    print(f"sum of the vertical foot forces - 1: {np.abs(dev['foot_force_vertical'].sum(0) - 1.0).max():.2e}; |dhg_z| / weight {residual.max():.2e}")
    law("sum of foot_force_vertical = 1", dev["foot_force_vertical"].sum(0), host["foot_force_vertical"].sum(0), np.ones(64))
    # the multipliers are the contact forces of the physics kernels, rotated into the world by the poses of the contact frames
    nc = lq.plan.n_contacts
    cols = [fk.index(c) for c in model.contacts]
    f_local = eng.field("contact_forces").cpu().numpy().reshape(nc, 6, 64)[:, :3]
    rot = _quat_matrices(inputs["pose"][3:7][:, cols])                                          # [nc][B][3][3]
    f_world = np.einsum("kbij,kjb->ikb", rot, f_local) / weight
    assert np.abs(f_world[2]).min() > 0.05
    law("contact_force_rel = R contact_forces / weight", dev["contact_force_rel"][:3], host["contact_force_rel"][:3], f_world)
    law("com = centroidal", dev["com"], host["com"], inputs["centroidal"][:3])
    law("vcom = hg_linear / mass", dev["vcom"], host["vcom"], inputs["centroidal"][3:6] / (weight / 9.81))
    # the ZMP (world axes) lies inside the bounding box of the contact positions
    xy = inputs["pose"][:2][:, cols]
    assert ((dev["zmp"] > xy.min(1)) & (dev["zmp"] < xy.max(1))).all()
    assert np.abs(dev["scalars"][1]).max() < 5e-3 and (dev["scalars"][0] < 0.5).all() and (dev["scalars"][2:] > 0.5).all()
    env.close()


@pytest.mark.gpu
def test_block_reset_keeps_the_unmasked_lanes_and_the_tensors(gpu_device):
    import torch

    from jiminy_amd import blocks
    env, _ = _settled_anymal(gpu_device, steps=2, locomotion_quantities=dict(momentum_cutoff=1.0, friction_cutoff=0.5))
    lq = env.locomotion
    assert lq.fieldnames == blocks.locomotion_fieldnames(env.model.contacts, lq.foot_frame_names, True, True)
    tensors = {k: getattr(lq, k) for k in ln.OUTPUTS}
    full = {k: t.clone() for k, t in tensors.items()}
    for t in tensors.values():
        t.fill_(7.25)
    mask = torch.arange(64, device=gpu_device) % 3 == 0
    lq.reset(mask)
    for k, t in tensors.items():
        assert t is getattr(lq, k)
        assert torch.equal(t[..., ~mask], torch.full_like(t[..., ~mask], 7.25)) and torch.equal(t[..., mask], full[k][..., mask]), k
    lq.refresh()
    assert all(torch.equal(t, full[k]) for k, t in tensors.items())
    with pytest.raises(ValueError, match="lane_mask must have shape"):
        lq.reset(mask[:5])
    env.close()


def _same(a, b) -> bool:
    """Two step results (nested tuples / dictionaries of tensors) hold the same bits."""
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return bool((a == b).all()) if hasattr(a, "shape") else a == b


@pytest.mark.gpu
def test_environment_terminations_and_rewards(gpu_device, monkeypatch):
    """`make_anymal_env(64, contact_model="constraint", locomotion_quantities=..., terminations=..., reward_mixture=...)`.
    Lanes b % 4 == 1 start 3 m above the ground (the lowest contact frame stays more than 1 m high for the 8 steps of the test:
    it falls 0.5 m in 0.32 s); lanes b % 4 == 0 are dropped from g t^2 / 2 with t = 0.316 s, so that they land 4 ms before the
    end of step 8 -- a termination sees the forces at the end of an environment step only, and the legs push back for some
    10 ms after a landing (measured on a sweep of drop heights: 2.5 to 19 times the weight on one contact point for landings
    2 to 6 ms before the end of a step, nothing once the robot has bounced off); the others stand.  `flying=(1.0, 0)` fires on
    the first kind at every step and on no other lane; `impact_force=(1.0, 0)` -- one contact point carrying the whole weight,
    four times what it carries at rest -- fires on the second kind at the landing and on no lane that stands; with a grace
    period of 10 s nothing fires."""
    import torch

    from jiminy_amd.envs import VecJiminyEnv, make_anymal_env
    B, steps = 64, 8
    lane = torch.arange(B, device=gpu_device)
    high, dropped = lane % 4 == 1, lane % 4 == 0
    sample = VecJiminyEnv._sample_state

    def lifted(self, n):
        q, v = sample(self, n)
        q = q.clone()
        q[2] += torch.where(high, 3.0, 0.0).to(q.dtype) + torch.where(dropped, 0.5 * 9.81 * 0.316 ** 2, 0.0).to(q.dtype)
        return q, v
    monkeypatch.setattr(VecJiminyEnv, "_sample_state", lifted)
    cfg = dict(momentum_cutoff=2.0, friction_cutoff=0.5)
    mixture = {"survival": 1.0, "momentum": 0.5, "friction": 0.25}
    common = dict(device=gpu_device, contact_model="constraint", auto_reset=False)
    with pytest.raises(ValueError, match="locomotion_quantities"):
        make_anymal_env(B, terminations=dict(flying=(1.0, 0.0)), frame_kinematics={}, **common)
    with pytest.raises(ValueError, match="locomotion_quantities"):
        make_anymal_env(B, reward_mixture={"momentum": 1.0}, **common)
    with pytest.raises(ValueError, match="momentum_cutoff"):
        make_anymal_env(B, reward_mixture={"momentum": 1.0}, locomotion_quantities={}, **common)
    with pytest.raises(ValueError, match="flying, impact_force"):
        make_anymal_env(B, terminations=dict(hovering=(1.0, 0.0)), **common)
    env = make_anymal_env(B, locomotion_quantities=cfg, reward_mixture=mixture,
                          terminations=dict(flying=(1.0, 0.0), impact_force=(1.0, 0.0)), **common)
    graceful = make_anymal_env(B, locomotion_quantities=cfg, terminations=dict(flying=(1.0, 10.0), impact_force=(1.0, 10.0)), **common)
    plain, plain2 = make_anymal_env(B, **common), make_anymal_env(B, **common)
    assert plain.locomotion is None and plain.frames is None and env.frames.average and "centroidal" not in plain.engine._fields
    assert env.frames.frame_names == ["root_joint"] + list(env.model.contacts)
    envs = (env, graceful, plain, plain2)
    for e in envs:
        e.reset(seed=7)
    lq = env.locomotion
    action = torch.zeros(B, env.model.nmotors, dtype=torch.float64, device=gpu_device)
    impact = torch.zeros(B, dtype=torch.bool, device=gpu_device)
    plan, worst = _block_plan(env), 0.0
    for i in range(steps):
        out = [e.step(action) for e in envs]
        flying = lq.ground_distance_min > 1.0
        hit = lq.force_vertical_max > 1.0
        print(f"step {i}: lowest contact of the high lanes {float(lq.ground_distance_min[high].min()):.3f} m; largest contact force "
              f"dropped {float(lq.force_vertical_max[dropped].max()):.2f}, standing {float(lq.force_vertical_max[~high & ~dropped].max()):.2f}")
        assert torch.equal(flying, high), i
        assert not bool(hit[~dropped].any()), i
        assert torch.equal(out[0][2], flying | hit), i                  # (no lane falls over or sinks within the test)
        assert not bool(out[1][2].any()) and not bool(out[2][2].any()), i
        impact |= hit
        # the two reward terms are the restatement on the block's tensors
        host = ln.quantities(plan, _block_inputs(env))
        want = 1.0 + 0.5 * host["scalars"][2] + 0.25 * host["scalars"][3]
        worst = max(worst, rel_error(out[0][1].cpu().numpy(), want))
        assert worst <= TOL, i
        # without the keyword: the same bits from two environments, and the block does not touch the physics
        assert _same(out[2], out[3]), i
        assert torch.equal(env.engine.robot_state.q, plain.engine.robot_state.q) and torch.equal(env.engine.robot_state.v, plain.engine.robot_state.v)
    print(f"environment: reward against the numpy restatement {worst:.2e}")
    assert torch.equal(impact, dropped)
    # a partial reset: the reset lanes are evaluated at their reset state, the others keep every bit
    mask = lane % 2 == 0
    tensors = {k: getattr(lq, k) for k in ln.OUTPUTS}
    kept = {k: t.clone() for k, t in tensors.items()}
    env.reset_lanes(mask)
    for k, t in tensors.items():
        # (bit for bit: the ZMP of a lane in free fall is NaN)
        assert t is getattr(lq, k) and torch.equal(t.view(torch.int64)[..., ~mask], kept[k].view(torch.int64)[..., ~mask]), k
    q0 = lifted(env, B)[0]
    assert float((lq.odom_pose[:2] - q0[:2])[..., mask].abs().max()) == 0.0
    for e in envs:
        e.close()
