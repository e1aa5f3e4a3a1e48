"""The tracking rewards block: `k_tracking_rewards` (jiminy_amd/csrc/jm_trackrewards.h) behind `jm_block_tracking_rewards` and
`blocks.TrackingRewards`.

The specification is tests/golden/ref_tracking_rewards.npz: what the reference's own `compute_height`, `quat_apply` and
`radial_basis_function` returned on seeded inputs (executed by tools/make_ref_tracking_rewards_fixtures.py), 64 lanes per case.
The kernel body is held to it on the host (tests/hostemu/trackrewards.cpp) and on the device in float64 and float32, inside
the bounds derived in tests/trackrewards_numpy.py; the designed lanes, lanes outside the mask and skipped terms bit for bit.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, codegen, load_builtin, trackrewards
from tests import trackrewards_numpy as rn
from tests.hostemu import trackrewards as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "make_ref_tracking_rewards_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
NEW_SYMBOLS = ("jm_trackrewards_plan_create", "jm_trackrewards_plan_destroy", "jm_block_tracking_rewards")
FX = rn.load_cases()
CASES = list(FX)
DTYPES = (np.float64, np.float32)
POISON = 7.0


def case(name: str):
    c = FX[name]
    plan = rn.plan_of(c)
    return plan, {k: c[k] for k in rn.INPUTS}, {k[9:]: v for k, v in c.items() if k.startswith("expected.")}, list(plan["cutoff"])


def check_case(name: str, run, dtype, label: str) -> None:
    plan, inputs, expected, cutoff = case(name)
    bounds = rn.run(plan, inputs, cutoff, dtype)
    got = run(plan, inputs, cutoff, dtype)
    for k in rn.OUTPUTS:
        worst = rn.compare(f"{label} {name} {np.dtype(dtype).name} {k}", got[k], expected[k], bounds["bound." + k])
        print(f"{label} {name} {np.dtype(dtype).name} {k}: worst error / bound {worst:.3f}")
    lane = {str(n): b for b, n in enumerate(np.load(rn.GOLDEN)["designed_lanes"])}
    # a zero error: the two sides agree to the bit and every reward is exactly 1
    assert (got["rewards"][:, lane["zero"]] == 1).all() and np.array_equal(got["value"][:, lane["zero"]], got["reference"][:, lane["zero"]])
    assert got["value"][0, lane["below"]] < 0


# ------------------------------------------------------------------------------------------------------------ fixture
def test_fixture_regenerates_from_the_reference_tree():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_ref_tracking_rewards_fixtures as tool
    finally:
        sys.path.pop(0)
    if not os.path.isdir(tool.COMMON):
        pytest.skip("the reference tree is not available")
    done = subprocess.run([sys.executable, TOOL, "--check"], capture_output=True, text=True, cwd=ROOT)
    assert done.returncode == 0, done.stdout + done.stderr


def test_fixture_holds_the_designed_lanes():
    z = np.load(rn.GOLDEN)
    assert CASES == ["quadruped", "one"] and os.path.getsize(rn.GOLDEN) < 200e3 and float(z["cutoff_esp"]) == rn.CUTOFF_ESP
    lane = {str(n): b for b, n in enumerate(z["designed_lanes"])}
    assert sorted(lane) == ["below", "cutoff", "tie", "zero"]
    for name in CASES:
        plan, inputs, expected, cutoff = case(name)
        assert all(a.shape[-1] == 64 for a in inputs.values())
        z_contacts = inputs["pose"][2][np.asarray(plan["contact_column"])]
        if len(plan["contact_column"]) > 1:
            low = np.sort(z_contacts[:, lane["tie"]])
            assert low[0] == low[1], "two contacts tie for the lowest"
        assert expected["value"][0, lane["below"]] < 0 and (inputs["pose"][2, plan["root_column"], lane["below"]] < z_contacts[:, lane["below"]]).all()
        assert (expected["rewards"][:, lane["zero"]] == 1.0).all()
        assert np.array_equal(expected["value"][:, lane["zero"]], expected["reference"][:, lane["zero"]])
        # the error equals the cutoff: the reward is CUTOFF_ESP within the bound of the float64 evaluation
        bound = rn.run(plan, inputs, cutoff)["bound.rewards"][:, lane["cutoff"]]
        assert (np.abs(expected["rewards"][:, lane["cutoff"]] - rn.CUTOFF_ESP) <= bound + 1e-14).all()
        e = expected["value"] - expected["reference"]
        for k, rows in rn.TERM_ROWS.items():
            assert (np.sum(e[rows] ** 2, axis=0) <= 4.0 * cutoff[k] ** 2 * (1 + 1e-9)).all(), "err^2 / cutoff^2 <= 4"
        assert 0.0 < expected["rewards"].min() < 1e-6 and expected["rewards"].max() == 1.0


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    plan, inputs, expected, cutoff = case(name)
    got = rn.run(plan, inputs, cutoff)
    for k in rn.OUTPUTS:
        rn.compare(f"{name} {k}", got[k], expected[k], got["bound." + k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name, dtype):
    check_case(name, lambda plan, inputs, cutoff, dt: emu.run(plan, inputs, cutoff, dt), dtype, "emulation")


def check_mask_and_skipped_terms(run) -> None:
    """What a launch must leave alone: lanes outside the mask, the rows of a term without a cutoff or without its inputs."""
    for dtype in DTYPES:
        plan, inputs, _, cutoff = case("quadruped")
        full = run(plan, inputs, cutoff, dtype, None, None)
        mask = np.arange(64) % 3 != 0
        into = {k: np.full_like(a, POISON) for k, a in full.items()}
        run(plan, inputs, cutoff, dtype, mask, into)
        for k, a in into.items():
            assert np.array_equal(a[:, mask], full[k][:, mask]) and (a[:, ~mask] == POISON).all(), k
        # a term without its cutoff, a term without its inputs: the rows are not written, the others keep their bits
        for term, rows in rn.TERM_ROWS.items():
            some = list(cutoff)
            some[term] = None
            lacking = {0: ("pose_reference",), 1: ("quat_no_yaw",), 2: ("dcm",), 3: ("position_reference",)}[term]
            for c, given in ((some, inputs), (cutoff, {k: v for k, v in inputs.items() if k not in lacking})):
                into = {k: np.full_like(a, POISON) for k, a in full.items()}
                run(plan, given, c, dtype, None, into)
                others = np.ones(full["value"].shape[0], dtype=bool)
                others[rows] = False
                assert (into["value"][rows] == POISON).all() and (into["reference"][rows] == POISON).all() and (into["rewards"][term] == POISON).all()
                assert np.array_equal(into["value"][others], full["value"][others])
                assert np.array_equal(np.delete(into["rewards"], term, 0), np.delete(full["rewards"], term, 0))
        # a contact height that is not a number makes the height one, as `np.min` does, whichever contact it is
        for c in range(len(plan["contact_column"])):
            bad = {k: v.copy() for k, v in inputs.items()}
            bad["pose"][2, plan["contact_column"][c], 5] = np.nan
            got = run(plan, bad, cutoff, dtype, None, None)
            assert np.isnan(got["value"][0, 5]) and np.isnan(got["rewards"][0, 5]) and np.isfinite(got["reference"][0, 5])
            assert np.array_equal(np.delete(got["value"][0], 5), np.delete(full["value"][0], 5))


def test_emulated_lane_mask_and_skipped_terms():
    check_mask_and_skipped_terms(lambda plan, inputs, cutoff, dtype, mask, into: emu.run(plan, inputs, cutoff, dtype, mask, into))


# ------------------------------------------------------------------------------------------------------ plan validation
def _good() -> dict:
    plan = case("quadruped")[0]
    return {k: plan[k] for k in rn.PLAN_KEYS}


def _rejections() -> list:
    p = _good()

    def change(key, at, value):
        a = np.array(p[key]).copy()
        a[at] = value
        return {key: a}
    return [
        (dict(n_motors=-1), "bad sizes"), (dict(n_motors=257), "bad sizes"), (dict(n_frames=-1), "bad sizes"),
        (dict(root_column=6), r"the root column is out of range \[0, 6\)"),
        (dict(root_column_reference=-1), r"the root column of the reference is out of range \[0, 5\)"),
        (change("contact_column", 2, 6), r"contact 2 has a column out of range \[0, 6\)"),
        (change("contact_column_reference", 0, 5), r"contact 0 has a column of the reference out of range \[0, 5\)"),
        (change("contact_column", 3, -1), "contact 3 has a column out of range"),
    ]


def test_plan_validation_rejects_every_malformed_description():
    for name in CASES:
        emu.pack(emu.plan_desc(case(name)[0])[0])
    with pytest.raises(ValueError, match="jm_trackrewards_plan_create: null description"):
        emu.pack(None)
    for change, message in _rejections():
        desc, keep = trackrewards.make_desc(**{**_good(), **change})
        with pytest.raises(ValueError, match=message):
            emu.pack(desc)
    for pointer in ("contact_column", "contact_column_reference"):
        desc, keep = trackrewards.make_desc(**_good())
        setattr(desc, pointer, None)
        with pytest.raises(ValueError, match="null array in the description"):
            emu.pack(desc)
    desc, keep = trackrewards.make_desc(**_good())
    desc.n_contacts = 65
    with pytest.raises(ValueError, match="bad sizes"):
        emu.pack(desc)
    with pytest.raises(ValueError, match="the same contact frames"):
        trackrewards.make_desc(**{**_good(), "contact_column": [0, 1]})
    del keep


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
    lib = _prebuilt(load_builtin("cartpole"))
    h = C.c_void_p()
    assert lib.L.jm_trackrewards_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    for change, message in _rejections():
        d, keep = trackrewards.make_desc(**{**_good(), **change})
        rc = lib.L.jm_trackrewards_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and re.search(message, _last_error(lib)), (message, _last_error(lib))
    assert lib.L.jm_block_tracking_rewards(None, _abi.JM_F64, 64, None, None, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    body = header.split("typedef struct jm_trackrewards_desc")[1].split("} jm_trackrewards_desc;")[0]
    order = [line.split(";")[0].split()[-1] for line in body.splitlines() if ";" in line]
    assert order == [f[0] for f in _abi.TrackRewardsDesc._fields_]
    body = header.split("typedef struct jm_trackrewards_io")[1].split("} jm_trackrewards_io;")[0]
    order = [line.split("*")[1].strip(" ;") for line in body.splitlines() if "*" in line]
    assert order == list(_abi.TRACKREWARDS_IO_FIELDS) and set(order) == set(rn.INPUTS + rn.OUTPUTS + ("lane_mask",))
    assert os.path.join(codegen.CSRC, "jm_trackrewards.h") in codegen._sources()
    assert "loco_rbf(" in open(os.path.join(codegen.CSRC, "jm_trackrewards.h")).read()
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


# ------------------------------------------------------------------------------------------------------------ host side
def test_build_plan_and_python_surface_refusals_on_the_host(monkeypatch):
    import torch

    from jiminy_amd import blocks
    model = load_builtin("anymal")
    names = ["root_joint"] + list(model.contacts)
    plan = trackrewards.build_plan(model, names + ["imu_link"], list(reversed(names)), 12)
    a = plan.arrays
    assert (a["n_frames"], a["root_column"], a["contact_column"]) == (6, 0, [1, 2, 3, 4]) and plan.rows == 18
    assert (a["n_frames_reference"], a["root_column_reference"], a["contact_column_reference"]) == (5, 4, [3, 2, 1, 0])
    emu.pack(plan.desc()[0])
    emu.pack(trackrewards.build_plan(model, None, None, 12).desc()[0])
    with pytest.raises(ValueError, match="lacks the frames.*root_joint"):
        trackrewards.build_plan(model, names[1:], names, 12)
    eng = SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _lib=SimpleNamespace(L=None, check=None))
    frames = lambda average=True, mode=0: SimpleNamespace(_eng=eng, frame_names=names, average=average, index=names.index,      # noqa: E731
                                                          plan=SimpleNamespace(modes=[mode] + [0] * 4))
    loco = lambda frame=0: SimpleNamespace(_eng=eng, plan=SimpleNamespace(arrays=dict(dcm_frame=frame)))      # noqa: E731
    make = blocks.TrackingRewards
    with pytest.raises(ValueError, match="cutoff must be positive"):
        make(eng, base_height_cutoff=0.0)
    with pytest.raises(ValueError, match="another engine"):
        make(eng, frames=SimpleNamespace(_eng=None))
    with pytest.raises(ValueError, match="pass frames and reference_frames"):
        make(eng, frames=frames(), base_height_cutoff=0.1)
    with pytest.raises(ValueError, match="average=True"):
        make(eng, frames=frames(), reference_frames=frames(average=False), odometry_velocity_cutoff=0.1)
    with pytest.raises(ValueError, match="LOCAL step-average"):
        make(eng, frames=frames(mode=2), reference_frames=frames(), odometry_velocity_cutoff=0.1)
    with pytest.raises(ValueError, match="pass locomotion and reference_locomotion"):
        make(eng, locomotion=loco(), capture_point_cutoff=0.1)
    with pytest.raises(ValueError, match="dcm_reference_frame='LOCAL'"):
        make(eng, locomotion=loco(), reference_locomotion=loco(1), capture_point_cutoff=0.1)
    with pytest.raises(ValueError, match="pass actuation and a trajectory"):
        make(eng, actuation=SimpleNamespace(_eng=eng, position=torch.zeros(12, 4)), joint_positions_cutoff=0.1)
    fields = blocks.tracking_rewards_fieldnames(["LF_HAA"])
    assert fields["value"] == fields["reference"] and fields["value"][0] == "BaseHeight" and fields["value"][-1] == "LF_HAA.Position"
    assert fields["rewards"] == ["reward_base_height", "reward_odometry_velocity", "reward_capture_point", "reward_joint_positions"]
    assert blocks.TRACKING_REWARD_TERMS == trackrewards.TERMS == rn.TERMS
    monkeypatch.setenv("JIMINY_AMD_TENSOR_BLOCKS", "1")
    with pytest.raises(NotImplementedError, match="no tensor-program form"):
        make(eng)


# ------------------------------------------------------------------------------------------------------------ device
class DeviceTrackRewards:
    """Plans on the device and the launch on numpy arrays (copied in and out), with the signature of `emu.run`."""

    def __init__(self, lib, device):
        import torch
        self.torch, self.lib, self.device, self.plans = torch, lib, device, []

    def close(self):
        for h in self.plans:
            self.lib.L.jm_trackrewards_plan_destroy(h)

    def run(self, plan, inputs, cutoff, dtype=np.float64, mask=None, into=None):
        torch = self.torch
        desc, keep = emu.plan_desc(plan)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            self.lib.check(self.lib.L.jm_trackrewards_plan_create(C.byref(desc), C.byref(h)))
        self.plans.append(h)
        n = next(iter(inputs.values())).shape[-1]
        up = lambda a, kind: torch.as_tensor(np.array(a, dtype=kind, order="C"), device=self.device)      # noqa: E731
        io = _abi.TrackRewardsIO()
        held = []
        for name in rn.INPUTS:
            if name in inputs:
                held.append(up(inputs[name], dtype))
                setattr(io, name, held[-1].data_ptr())
        if mask is not None:
            held.append(up(mask, np.uint8))
            io.lane_mask = held[-1].data_ptr()
        out = {}
        for name in rn.OUTPUTS:
            a = into[name] if into is not None else np.zeros((rn.rows_of(name, plan), n), dtype=dtype)
            assert a.shape == (rn.rows_of(name, plan), n) and a.dtype == np.dtype(dtype)
            out[name] = (a, up(a, dtype))
            setattr(io, name, out[name][1].data_ptr())
        c = (C.c_double * 4)(*[float(x) if x is not None else 0.0 for x in cutoff])
        self.lib.check(self.lib.L.jm_block_tracking_rewards(
            h, _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, n, C.byref(io), c,
            C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        for a, t in out.values():
            a[...] = t.cpu().numpy()
        del held, keep
        return {k: a for k, (a, _) in out.items()}


@pytest.fixture
def device_rewards(gpu_device):
    dev = DeviceTrackRewards(_prebuilt(load_builtin("cartpole")), gpu_device)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, device_rewards):
    """Every fixture case through the C ABI at B = 64, both dtypes."""
    for dtype in DTYPES:
        check_case(name, lambda plan, inputs, cutoff, dt: device_rewards.run(plan, inputs, cutoff, dt), dtype, "device")


@pytest.mark.gpu
def test_device_tail_block(device_rewards):
    """`quadruped` at B = 257: a second block of one lane; every lane repeats one of the 64 and gives its bits."""
    plan, inputs, _, cutoff = case("quadruped")
    lanes = np.arange(257) % 64
    wide = {k: v[..., lanes] for k, v in inputs.items()}
    for dtype in DTYPES:
        got, ref = device_rewards.run(plan, wide, cutoff, dtype), device_rewards.run(plan, inputs, cutoff, dtype)
        assert all(np.array_equal(got[k], ref[k][:, lanes]) for k in rn.OUTPUTS) and got["rewards"].shape == (4, 257)


@pytest.mark.gpu
def test_device_lane_mask_and_skipped_terms(device_rewards):
    check_mask_and_skipped_terms(lambda plan, inputs, cutoff, dtype, mask, into: device_rewards.run(plan, inputs, cutoff, dtype, mask, into))
