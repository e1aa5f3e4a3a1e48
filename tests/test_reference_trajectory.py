"""The reference trajectories block: `k_trajectory_state` (jiminy_amd/csrc/jm_trajectory.h) behind `jm_block_trajectory_state`,
`blocks.ReferenceTrajectory` and the `trajectory_database` keyword of `WalkerVecEnv`.

The specification is tests/golden/ref_trajectory.npz: the states the reference's own `Trajectory.get` returned (executed by
tools/make_ref_trajectory_fixtures.py on a stand-in for pinocchio), 64 lanes, a few query events per case.  The kernel body is
held to it on the host (tests/hostemu/trajectory.cpp) and on the device in float64 and float32: `status`, copied samples, lanes
outside the mask and absent outputs bit for bit, everything else inside the bounds derived in tests/trajectory_numpy.py.
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

from jiminy_amd import _abi, _lib, codegen, load_builtin, trajectory
from tests import trajectory_numpy as tn
from tests.hostemu import trajectory as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "make_ref_trajectory_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
NEW_SYMBOLS = ("jm_trajectory_plan_create", "jm_trajectory_plan_destroy", "jm_block_trajectory_state")
FX = tn.load_cases()
CASES = list(FX)
DTYPES = (np.float64, np.float32)
POISON = 7.0


def case(name: str):
    c = FX[name]
    return tn.plan_of(c), {k: c[k] for k in tn.EVENT_KEYS}, {k[9:]: v for k, v in c.items() if k.startswith("expected.")}


def fresh(plan, B, dtype):
    return {n: np.zeros((tn.rows_of(n, plan), B), dtype=tn.dtype_of(n, dtype)) for n in tn.OUTPUTS if tn.rows_of(n, plan)}


def check_case(name: str, run, dtype, label: str, lanes=None) -> float:
    """Every event of a case through `run(plan, time, trajectory, time_offset, mask, dtype, into)`, the tensors carried from
    event to event, against the fixture.  `lanes`: the fixture lane every lane of the batch replays (default: the 64 as they are)."""
    plan, events, expected = case(name)
    lanes = np.arange(events["time"].shape[1]) if lanes is None else np.asarray(lanes)
    bounds = tn.run_events(plan, events, dtype)
    into, worst = fresh(plan, len(lanes), dtype), 0.0
    for e in range(events["time"].shape[0]):
        run(plan, events["time"][e][lanes], events["trajectory"][e][lanes], events["time_offset"][e][lanes], events["mask"][e][lanes],
            dtype, into)
        for k, got in into.items():
            worst = max(worst, tn.compare(f"{label} {name} {np.dtype(dtype).name} event {e} {k}", got, expected[k][e][:, lanes],
                                          bounds["bound." + k][e][:, lanes]))
    print(f"{label} {name} {np.dtype(dtype).name}: worst error / bound {worst:.3f}")
    return worst


# ------------------------------------------------------------------------------------------------------------ fixture
def test_fixture_regenerates_from_the_reference_tree():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_ref_trajectory_fixtures as tool
    finally:
        sys.path.pop(0)
    if not os.path.isfile(tool.DYNAMICS):
        pytest.skip("the reference tree is not available")
    done = subprocess.run([sys.executable, TOOL, "--check"], capture_output=True, text=True, cwd=ROOT)
    assert done.returncode == 0, done.stdout + done.stderr


def test_fixture_holds_the_designed_lanes():
    z = np.load(tn.GOLDEN)
    assert CASES == ["anymal", "mixed", "fixed"] and os.path.getsize(tn.GOLDEN) < 500e3
    lane = {str(n): b for b, n in enumerate(z["designed_lanes"])}
    plan, events, expected = case("anymal")
    flags, n_steps, index = expected["status"][0]
    sample = lambda k, i: plan["data"][plan["sample_start"][k] + i, :plan["nq"]]      # noqa: E731
    q = expected["q"][0]
    # exactly on a sample and 2^-40 below it: that sample; the doubled timestamp: t-, the left one of the pair
    assert index[lane["on_sample"]] == index[lane["below_sample"]] == 3
    assert np.array_equal(q[:, lane["on_sample"]], sample(8, 3)) and np.array_equal(q[:, lane["below_sample"]], sample(8, 3))
    times5 = plan["times"][plan["sample_start"][5]:plan["sample_start"][6]]
    assert times5[2] == times5[3] and index[lane["doubled"]] == 2 and np.array_equal(q[:, lane["doubled"]], sample(5, 2))
    assert index[lane["t_start"]] == 1 and index[lane["t_end"]] == 8
    assert [int(flags[lane[n]]) for n in ("beyond_raise", "before_raise", "beyond_clip", "before_clip")] == [1, 1, 0, 0]
    assert [int(n_steps[lane[n]]) for n in ("beyond_wrap", "beyond_wrap3", "before_wrap", "stride_yaw", "stride_zero",
                                            "degenerate_wrap")] == [1, 3, -1, 3, 1, 0]
    assert abs(plan["stride"][7, 5] - 1.0) < 1e-12 and np.abs(plan["stride"][9]).max() < 1e-15
    assert plan["times"][plan["sample_start"][10]] == plan["times"][plan["sample_start"][11] - 1] and plan["mode"][10] == tn.WRAP
    # the grid of 2^-12: times, lane times and offsets (but the one designed lane 2^-40 below a sample)
    on_grid = lambda a: np.all(np.asarray(a) * 4096 == np.round(np.asarray(a) * 4096))      # noqa: E731
    for name in CASES:
        plan, events, expected = case(name)
        assert on_grid(plan["times"]) and on_grid(events["time_offset"]) and events["time"].shape[1] == 64
        off = ~np.isclose(events["time"] * 4096, np.round(events["time"] * 4096), atol=0, rtol=0)
        assert int(off.sum()) == (1 if name == "anymal" else 0)
        assert set(np.unique(plan["mode"])) == {tn.RAISE, tn.WRAP, tn.CLIP}
        assert (expected["status"][:, 0] == 1).any() and not events["mask"].all() and events["mask"][0].all()
    assert not tn.has_freeflyer(case("fixed")[0]) and "plan.stride" not in FX["fixed"] and case("fixed")[0]["fields"] == 0
    assert {int(k) for k in case("mixed")[0]["joint_kind"]} == {7, 6, 5, 8, 2}


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    plan, events, expected = case(name)
    got = tn.run_events(plan, events, np.float64)
    for k in expected:
        tn.compare(f"{name} {k}", got[k], expected[k], got["bound." + k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name, dtype):
    run = lambda plan, t, k, o, m, dt, into: emu.run(plan, t, k, o, mask=m, dtype=dt, into=into)      # noqa: E731
    check_case(name, run, dtype, "emulation")


def check_mask_nulls_and_absent(run) -> None:
    """What a launch must leave alone: lanes outside the mask (every bit), outputs that are null, outputs the plan lacks."""
    for dtype in DTYPES:
        plan, events, _ = case("anymal")
        t, k, o = events["time"][1], events["trajectory"][1], events["time_offset"][1]
        full = run(plan, t, k, o, None, dtype, None, tn.OUTPUTS, None)
        mask = np.arange(64) % 3 != 0
        into = {n: np.full_like(a, POISON) for n, a in full.items()}
        run(plan, t, k, o, mask, dtype, into, tn.OUTPUTS, None)
        for n, a in into.items():
            assert np.array_equal(a[:, mask], full[n][:, mask]) and (a[:, ~mask] == POISON).all(), n
        # only some outputs: the same bits as in the full launch
        some = run(plan, t, k, o, None, dtype, None, ("odom_pose", "position", "status"), None)
        assert set(some) == {"odom_pose", "position", "status"} and all(np.array_equal(some[n], full[n]) for n in some)
        # a trajectory index outside the dataset: flag bit 1, nothing else written
        bad = k.copy()
        bad[5], bad[6] = -1, len(plan["mode"])
        into = {n: np.full_like(a, POISON) for n, a in full.items()}
        run(plan, t, bad, o, None, dtype, into, tn.OUTPUTS, None)
        assert (into["status"][:, [5, 6]] == np.array([[2], [0], [0]])).all() and (into["q"][:, [5, 6]] == POISON).all()
        assert np.array_equal(into["q"][:, 7:], full["q"][:, 7:])
        # the case without a free-flyer and with q alone: the outputs it lacks are left alone
        plan, events, _ = case("fixed")
        absent = {"v": np.full((plan["nv"], 64), POISON, dtype), "a": np.full((plan["nv"], 64), POISON, dtype),
                  "command": np.full((plan["n_command"], 64), POISON, dtype), "odom_pose": np.full((3, 64), POISON, dtype)}
        run(plan, events["time"][0], events["trajectory"][0], events["time_offset"][0], None, dtype, None, tn.OUTPUTS, absent)
        assert all((a == POISON).all() for a in absent.values())


def test_emulated_lane_mask_null_pointers_and_absent_outputs():
    check_mask_nulls_and_absent(lambda plan, t, k, o, m, dt, into, outputs, absent:
                                emu.run(plan, t, k, o, mask=m, dtype=dt, into=into, outputs=outputs, absent=absent))


def test_emulated_time_that_is_not_finite_is_flagged():
    plan, events, _ = case("anymal")
    t = events["time"][1].copy()
    t[3], t[4] = np.nan, np.inf
    got = emu.run(plan, t, events["trajectory"][1], events["time_offset"][1])
    assert (got["status"][0, [3, 4]] == 1).all() and np.isfinite(got["q"]).all()


# ------------------------------------------------------------------------------------------------------ plan validation
def _good() -> dict:
    return dict(case("mixed")[0])


def _rejections() -> list:
    p = _good()
    S, N = len(p["times"]), len(p["mode"])
    nan_time, back_time = p["times"].copy(), p["times"].copy()
    nan_time[1], back_time[2] = np.nan, back_time[1] - 0.25
    short = p["sample_start"].copy()
    short[1] = 1
    bad_stride = p["stride"].copy()
    bad_stride[1, 4] = np.inf
    change = lambda key, at, value: {key: np.concatenate([p[key][:at], [value], p[key][at + 1:]]).astype(p[key].dtype)}      # noqa: E731
    return [
        (dict(nq=0), "bad sizes"), (dict(nv=-1), "bad sizes"), (dict(fields=8), "unknown field bits"),
        (dict(fields=tn.HAS_V | tn.HAS_COMMAND, n_command=0), "a present field has no rows"),
        (change("sample_start", 0, 1), "sample_start must run from 0 to n_samples"),
        (change("sample_start", N, S - 1), "sample_start must run from 0 to n_samples"),
        (dict(sample_start=short), "trajectory 0 needs at least 2 samples"),
        (dict(times=nan_time), r"trajectory 0 has a time that is not finite \(sample 1\)"),
        (dict(times=back_time), r"trajectory 0: time must not be decreasing between consecutive timesteps \(sample 2\)"),
        (change("mode", 2, 3), "trajectory 2 has an unknown time mode"), (change("mode", 0, -1), "trajectory 0 has an unknown time mode"),
        (change("joint_kind", 1, 12), "joint 1 has an unknown joint kind"), (change("joint_kind", 3, 0), "joint 3 has an unknown joint kind"),
        (change("joint_q_index", 1, 12), r"joint 1 reads q rows \[12, 16\) out of range \[0, 15\)"),
        (change("joint_q_index", 4, -1), r"joint 4 reads q rows \[-1, 0\) out of range"),
        (change("joint_kind", 1, 7), "joint 1: a free-flyer must be joint 0 at q row 0"),
        (change("motor_q_index", 0, 11), "motor 0 reads q row 11, which is not the row of a one-row joint"),
        (change("motor_q_index", 1, 15), "motor 1 reads q row 15"),
        (dict(stride=bad_stride), "trajectory 1 has a stride that is not finite"),
        (dict(stride=None), "a free-flyer needs the strides"),
    ]


def test_plan_validation_rejects_every_malformed_description():
    for name in CASES:
        for dtype in DTYPES:
            emu.pack(emu.plan_desc(case(name)[0], dtype)[0])
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    for change, message in _rejections():
        desc, keep = emu.plan_desc({**_good(), **change})
        with pytest.raises(ValueError, match=message):
            emu.pack(desc)
    desc, keep = emu.plan_desc(_good())
    for pointer in ("sample_start", "times", "mode", "data", "joint_kind", "joint_q_index", "motor_q_index"):
        d, _ = emu.plan_desc(_good())
        setattr(d, pointer, None)
        with pytest.raises(ValueError, match="null array in the description"):
            emu.pack(d)
    desc.dtype = 5
    with pytest.raises(ValueError, match="bad dtype"):
        emu.pack(desc)
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
    """The same rejections through the C ABI of a built library, on a machine without a device: JM_EINVAL and a message."""
    lib = _prebuilt(load_builtin("cartpole"))
    h = C.c_void_p()
    assert lib.L.jm_trajectory_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = emu.plan_desc(_good())
    assert lib.L.jm_trajectory_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    for change, message in _rejections():
        d, keep = emu.plan_desc({**_good(), **change})
        rc = lib.L.jm_trajectory_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and re.search(message, _last_error(lib)), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    io = _abi.TrajectoryIO()
    assert lib.L.jm_block_trajectory_state(None, _abi.JM_F64, 64, C.byref(io), None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    # the order of the fields in the header is the order of the ctypes mirrors
    body = header.split("typedef struct jm_trajectory_desc")[1].split("} jm_trajectory_desc;")[0]
    order = [line.split(";")[0].split()[-1] for line in body.splitlines() if ";" in line]
    assert order == [f[0] for f in _abi.TrajectoryDesc._fields_]
    assert set(tn.PLAN_KEYS) <= set(order)
    body = header.split("typedef struct jm_trajectory_io")[1].split("} jm_trajectory_io;")[0]
    order = [line.split("*")[1].strip(" ;") for line in body.splitlines() if "*" in line]
    assert order == list(_abi.TRAJECTORY_IO_FIELDS) and set(order) == set(tn.OUTPUTS + ("time", "trajectory", "time_offset", "lane_mask"))
    assert os.path.join(codegen.CSRC, "jm_trajectory.h") in codegen._sources()
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


# ------------------------------------------------------------------------------------------------------------ host side
def _anymal_dataset():
    """The trajectories of the fixture case `anymal` (whose layout is the built-in ANYmal's) as `Trajectory` objects."""
    plan = case("anymal")[0]
    out = {}
    for k in range(len(plan["mode"])):
        s = slice(plan["sample_start"][k], plan["sample_start"][k + 1])
        d = plan["data"][s]
        out[f"t{k}"] = (trajectory.Trajectory(plan["times"][s], d[:, :19], v=d[:, 19:37], command=d[:, 37:49]),
                        ("raise", "wrap", "clip")[int(plan["mode"][k])])
    return plan, out


def test_build_plan_of_the_builtin_anymal_and_its_refusals():
    model = load_builtin("anymal")
    want, dataset = _anymal_dataset()
    plan = trajectory.build_plan(model, dataset)
    assert plan.names == list(dataset) and plan.modes == list(want["mode"]) and plan.has_freeflyer and plan.fields == want["fields"]
    assert (plan.nq, plan.nv, plan.n_command, plan.n_motors) == (19, 18, 12, 12)
    a = plan.arrays
    for key in ("sample_start", "times", "data", "joint_q_index"):
        assert np.array_equal(np.asarray(a[key]), want[key]), key
    assert a["motor_q_index"] == [int(m.idx_q) for m in model.motors] and sorted(a["motor_q_index"]) == list(want["motor_q_index"])
    assert a["joint_kind"][0] == 7 and all(1 <= k <= 4 for k in a["joint_kind"][1:])
    starts = np.asarray(a["sample_start"])
    assert np.array_equal(plan.time_interval, np.stack([want["times"][starts[:-1]], want["times"][starts[1:] - 1]], axis=1))
    # the stride: float64 `log6(M_end * M_start^-1)` against the reference's own; two float64 evaluations of a few dozen
    # operations on magnitudes below 4: 64 eps (1 + |stride|)
    bound = 64 * np.finfo(np.float64).eps * (1 + np.abs(want["stride"]))
    assert (np.abs(a["stride"] - want["stride"]) <= bound).all()
    for dtype in DTYPES:
        emu.pack(plan.desc(dtype)[0])
    T = trajectory.Trajectory
    t, q = np.array([0.0, 0.5, 1.0]), want["data"][:3, :19]
    with pytest.raises(ValueError, match="Time must not be decreasing"):
        T([0.0, 0.5, 0.25], q)
    with pytest.raises(ValueError, match="at least 2 samples"):
        T([0.0], q[:1])
    with pytest.raises(ValueError, match="must be finite"):
        T([0.0, np.nan, 1.0], q)
    with pytest.raises(ValueError, match=r"q must have shape \[3\]\[rows\]"):
        T(t, q[:2])
    for name in ("u", "f_external", "lambda_c"):
        with pytest.raises(NotImplementedError, match=f"state field '{name}'"):
            T(t, q, **{name: np.zeros((3, 1))})
    with pytest.raises(TypeError, match="unexpected field"):
        T(t, q, torque=np.zeros((3, 1)))
    T([0.0, 0.5, 0.5], q)                       # (t-, t+)
    flipped = q.copy()
    flipped[1, 3:7] *= -1.0
    with pytest.raises(ValueError, match="trajectory 'flip': consecutive quaternions at q row 0 have a negative dot product"):
        trajectory.build_plan(model, {"flip": (T(t, flipped), "clip")})
    with pytest.raises(ValueError, match="q has 18 rows, the model 19"):
        trajectory.build_plan(model, {"a": (T(t, q[:, :18]), "clip")})
    with pytest.raises(ValueError, match="v has 3 rows, the model 18"):
        trajectory.build_plan(model, {"a": (T(t, q, v=np.zeros((3, 3))), "clip")})
    with pytest.raises(ValueError, match="carries other optional fields"):
        trajectory.build_plan(model, {"a": (T(t, q), "clip"), "b": (T(t, q, v=np.zeros((3, 18))), "clip")})
    with pytest.raises(ValueError, match="unknown time mode 'loop'"):
        trajectory.build_plan(model, {"a": (T(t, q), "loop")})
    with pytest.raises(ValueError, match="at least one trajectory"):
        trajectory.build_plan(model, {})
    with pytest.raises(ValueError, match=r"expected a pair \(Trajectory, mode\)"):
        trajectory.build_plan(model, {"a": T(t, q)})
    assert [trajectory.time_mode(m) for m in ("raise", "wrap", "clip", 2)] == [0, 1, 2, 2]


def test_python_surface_refusals_on_the_host(monkeypatch):
    from jiminy_amd import blocks
    monkeypatch.setenv("JIMINY_AMD_TENSOR_BLOCKS", "1")
    with pytest.raises(NotImplementedError, match="no tensor-program form"):
        blocks.ReferenceTrajectory(SimpleNamespace(), {})
    names = blocks.trajectory_fieldnames(load_builtin("anymal"), tn.HAS_V, ["m"])
    assert set(names) == {"q", "v", "odom_pose", "position", "status"} and names["status"] == ["flags", "n_steps", "index"]
    assert names["position"] == ["m.ReferencePosition"] and len(names["q"]) == 19


# ------------------------------------------------------------------------------------------------------------ device
class DeviceTrajectory:
    """Plans on the device and the launch on numpy arrays (copied in and out), with the signature of `emu.run`."""

    def __init__(self, lib, device):
        import torch
        self.torch, self.lib, self.device, self.plans = torch, lib, device, {}

    def handle(self, plan: dict, dtype):
        key = (id(plan["data"]), np.dtype(dtype).name)
        if key not in self.plans:
            desc, keep = emu.plan_desc(plan, dtype)
            h = C.c_void_p()
            with self.torch.cuda.device(self.device):
                self.lib.check(self.lib.L.jm_trajectory_plan_create(C.byref(desc), C.byref(h)))
            self.plans[key] = (h, plan)
        return self.plans[key][0]

    def close(self):
        for h, _ in self.plans.values():
            self.lib.L.jm_trajectory_plan_destroy(h)

    def run(self, plan, time, trajectory_, time_offset, mask=None, dtype=np.float64, into=None, outputs=tn.OUTPUTS, absent=None):
        torch = self.torch
        B = int(len(time))
        up = lambda a, kind: torch.as_tensor(np.ascontiguousarray(a, dtype=kind), device=self.device)      # noqa: E731
        io = _abi.TrajectoryIO()
        held = [up(time, np.float64), up(trajectory_, np.int32), up(time_offset, np.float64)]
        io.time, io.trajectory, io.time_offset = (t.data_ptr() for t in held)
        if mask is not None:
            held.append(up(mask, np.uint8))
            io.lane_mask = held[-1].data_ptr()
        out = {}
        for name in outputs:
            rows = tn.rows_of(name, plan)
            if not rows:
                continue
            kind = tn.dtype_of(name, dtype)
            a = into[name] if into is not None and name in into else np.full((rows, B), -1 if name == "status" else np.nan, dtype=kind)
            assert a.shape == (rows, B) and a.dtype == kind
            out[name] = (a, up(a, kind))
            setattr(io, name, out[name][1].data_ptr())
        left = {name: (a, up(a, a.dtype)) for name, a in (absent or {}).items()}
        for name, (_, t) in left.items():
            setattr(io, name, t.data_ptr())
        self.lib.check(self.lib.L.jm_block_trajectory_state(
            self.handle(plan, dtype), _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B, C.byref(io),
            C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        for a, t in list(out.values()) + list(left.values()):
            a[...] = t.cpu().numpy()
        del held
        return {k: a for k, (a, _) in out.items()}


@pytest.fixture
def device_trajectory(gpu_device):
    dev = DeviceTrajectory(_prebuilt(load_builtin("cartpole")), gpu_device)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, device_trajectory):
    """Every fixture case through the C ABI with the authored joint tables at B = 64, both dtypes."""
    run = lambda plan, t, k, o, m, dt, into: device_trajectory.run(plan, t, k, o, m, dt, into)      # noqa: E731
    for dtype in DTYPES:
        check_case(name, run, dtype, "device")


@pytest.mark.gpu
def test_device_partial_wavefront_mask_and_repeatability(device_trajectory):
    """`anymal` at B = 70: the fixture lanes and 6 repeats (a partial second wavefront, the mask path); two launches from the
    same inputs give the same bits; a dtype other than the plan's is refused."""
    lanes = np.concatenate([np.arange(64), [0, 7, 12, 15, 16, 63]])
    run = lambda plan, t, k, o, m, dt, into: device_trajectory.run(plan, t, k, o, m, dt, into)      # noqa: E731
    plan, events, _ = case("anymal")
    for dtype in DTYPES:
        check_case("anymal", run, dtype, "device B=70", lanes)
        args = (plan, events["time"][3][lanes], events["trajectory"][3][lanes], events["time_offset"][3][lanes])
        first, second = device_trajectory.run(*args, None, dtype), device_trajectory.run(*args, None, dtype)
        assert all(np.array_equal(first[k], second[k]) for k in first) and first["q"].shape == (19, 70)
        assert all(np.array_equal(v[:, 64:], v[:, lanes[64:]]) for v in first.values())
    io = _abi.TrajectoryIO()
    lib = device_trajectory.lib
    assert lib.L.jm_block_trajectory_state(device_trajectory.handle(plan, np.float64), _abi.JM_F32, 70, C.byref(io), None) == _abi.JM_EINVAL


@pytest.mark.gpu
def test_device_lane_mask_null_pointers_and_absent_outputs(device_trajectory):
    check_mask_nulls_and_absent(lambda plan, t, k, o, m, dt, into, outputs, absent:
                                device_trajectory.run(plan, t, k, o, m, dt, into, outputs, absent))


BLOCKS = dict(locomotion_quantities=dict(forces=False, momentum=False), foot_poses=dict(position_cutoff=0.1, orientation_cutoff=0.2),
              actuated_joints={})


@pytest.mark.gpu
def test_block_on_an_engine(gpu_device):
    """`blocks.ReferenceTrajectory` on the ANYmal engine: the fixture's dataset against the fixture through the block; `select`
    with a lane mask and a per-lane ratio; the odometry pose of a state copied from the engine equals
    `LocomotionQuantities.odom_pose` bit for bit."""
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.envs import make_anymal_env
    B = 64
    env = make_anymal_env(B, device=gpu_device, contact_model="constraint", auto_reset=False, **BLOCKS)
    env.reset(seed=5)
    plan, dataset = _anymal_dataset()
    _, events, expected = case("anymal")
    blk = blocks.ReferenceTrajectory(env.engine, dataset, actuation=env.actuation)
    assert blk.names == list(dataset) and blk.a is None and blk.q.shape == (19, B) and blk.command.shape == (12, B)
    assert blk.status.dtype == torch.int32 and blk.time_offset.dtype == torch.float64
    tensors = {k: getattr(blk, k) for k in ("q", "v", "command", "odom_pose", "position", "status", "trajectory", "time_offset")}
    address = {k: t.data_ptr() for k, t in tensors.items()}
    bounds = tn.run_events(plan, events, np.float64)
    motor_rows = torch.as_tensor([int(m.idx_q) for m in env.model.motors], device=gpu_device)
    for e in range(events["time"].shape[0]):
        blk.trajectory.copy_(torch.as_tensor(events["trajectory"][e], device=gpu_device))
        blk.time_offset.copy_(torch.as_tensor(events["time_offset"][e], device=gpu_device))
        blk.query(torch.as_tensor(events["time"][e], device=gpu_device), torch.as_tensor(events["mask"][e], device=gpu_device))
        torch.cuda.synchronize(gpu_device)
        for k in ("q", "v", "command", "odom_pose", "status"):
            tn.compare(f"block event {e} {k}", tensors[k].cpu().numpy(), expected[k][e], bounds["bound." + k][e])
        # (the motors in the order of the model's, which is not the order of their rows)
        assert torch.equal(blk.position, blk.q[motor_rows])
        assert np.array_equal(blk.out_of_range.cpu().numpy(), expected["status"][e][0] == 1)
    assert all(getattr(blk, k) is t and t.data_ptr() == address[k] for k, t in tensors.items())
    # select: by name on a mask with a per-lane ratio, the other lanes keep what they had
    lane = torch.arange(B, device=gpu_device)
    mask, ratio = lane % 3 == 0, (lane % 5).to(torch.float64) / 4.0
    before_k, before_o = blk.trajectory.clone(), blk.time_offset.clone()
    blk.select("t7", mask, ratio)
    t0, t1 = blk.plan.time_interval[7]
    want_o = torch.where(mask, t0 + ratio * (t1 - t0), before_o)
    assert torch.equal(blk.trajectory, torch.where(mask, torch.full_like(before_k, 7), before_k)) and torch.equal(blk.time_offset, want_o)
    blk.select(lane % 11, None, 0.5)
    iv = torch.as_tensor(blk.plan.time_interval, device=gpu_device)[lane % 11]
    assert torch.equal(blk.trajectory, (lane % 11).to(torch.int32)) and torch.equal(blk.time_offset, iv[:, 0] + 0.5 * (iv[:, 1] - iv[:, 0]))
    with pytest.raises(KeyError, match="no trajectory named 'nope'"):
        blk.select("nope")
    with pytest.raises(IndexError, match="out of range"):
        blk.select(lane)
    with pytest.raises(ValueError, match="contiguous float64 tensor"):
        blk.query(torch.zeros(B, device=gpu_device, dtype=torch.float32))
    # the engine's own q as a two-sample trajectory per lane, queried on the sample
    q = env.engine.field("q").cpu().numpy()
    own = {f"lane{b}": (trajectory.Trajectory([0.0, 1.0], np.stack([q[:, b], q[:, b]])), "clip") for b in range(B)}
    mine = blocks.ReferenceTrajectory(env.engine, own, actuation=env.actuation)
    assert mine.v is None and mine.command is None
    mine.select(lane)
    mine.query(torch.zeros(B, dtype=torch.float64, device=gpu_device))
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(mine.q, env.engine.field("q")) and torch.equal(mine.odom_pose, env.locomotion.odom_pose)
    assert torch.equal(mine.position, env.actuation.position) and (mine.status[0] == 0).all() and (mine.status[2] == 1).all()
    env.close()


@pytest.mark.gpu
def test_environment_replays_its_own_record(gpu_device):
    """`WalkerVecEnv` (ANYmal, 64 lanes, no randomisation, all five blocks): the state at the reset and after each of 6 steps
    of a fixed action is recorded and added as the trajectories of a database (one per lane).  Replaying the same actions,
    at every step the reference of the motor positions and of the relative foot poses equals the true value bit for bit (the
    same kernels on the same numbers), the two foot rewards are 1 and the drift and shift values 0.  Step 7 leaves the values
    of step 6 in mode "clip"; in mode "raise" it truncates every lane."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    B, steps = 64, 6
    windows = dict(odometry_horizon=0.08, foot_horizon=0.08, motor_horizon=0.08, odometry_cutoff=0.5)
    common = dict(device=gpu_device, contact_model="constraint", auto_reset=False, trajectory_tracking=windows,
                  reward_mixture={"survival": 1.0, "foot_positions": 1.0, "foot_orientations": 1.0}, **BLOCKS)
    gen = torch.Generator(device="cpu").manual_seed(3)
    action = (0.3 * (2.0 * torch.rand(B, 12, generator=gen, dtype=torch.float64) - 1.0)).to(gpu_device)
    lane = torch.arange(B, device=gpu_device)

    first = make_anymal_env(B, **common)
    assert first.trajectory is None
    first.reset(seed=11)
    state = lambda env: (env.engine.field("q").cpu().numpy().copy(), env.engine.field("v").cpu().numpy().copy())      # noqa: E731
    times, record = [float(first._lane_time()[0])], [state(first)]
    for _ in range(steps):
        first.step(action)
        times.append(float(first._lane_time()[0]))
        record.append(state(first))
    assert np.all(np.diff(times) > 0)

    def database(mode):
        return {f"lane{b}": (trajectory.Trajectory(times, np.stack([q[:, b] for q, _ in record]), v=np.stack([v[:, b] for _, v in record])),
                             mode) for b in range(B)}

    def replay(mode):
        env = make_anymal_env(B, trajectory_database=dict(dataset=database(mode)), **common)
        env.select_trajectory(lane)
        env.reset(seed=11)
        traj, out = env.trajectory, None

        def check(k):
            torch.cuda.synchronize(gpu_device)
            assert traj.position is env.tracking.reference_position and traj.odom_pose is env.tracking.reference_odom_pose
            assert torch.equal(traj.q, torch.as_tensor(record[k][0], device=gpu_device)), k
            assert torch.equal(env.tracking.reference_position, env.actuation.position), k
            assert torch.equal(env.foot_poses.reference_relative_pose, env.foot_poses.relative_pose), k
            assert torch.equal(env.tracking.reference_odom_pose, env.locomotion.odom_pose), k
            assert (env.foot_poses.reward_foot_positions == 1).all() and (env.foot_poses.reward_foot_orientations == 1).all(), k
            assert (env.tracking.scalars[[0, 1, 3, 4, 5]] == 0).all() and (env.tracking.reward_odom_pose == 1).all(), k
            assert not traj.out_of_range.any()
        check(0)
        for k in range(1, steps + 1):
            out = env.step(action)
            check(k)
            assert not out[3].any(), "no lane is truncated inside the trajectory"
        held = {n: getattr(traj, n).clone() for n in ("q", "v", "position", "odom_pose")}
        held["relative"] = env.foot_poses.reference_relative_pose.clone()
        out = env.step(action)
        torch.cuda.synchronize(gpu_device)
        return env, held, out

    env, held, out = replay("clip")
    assert all(torch.equal(getattr(env.trajectory, n), held[n]) for n in ("q", "v", "position", "odom_pose"))
    assert torch.equal(env.foot_poses.reference_relative_pose, held["relative"]) and not env.trajectory.out_of_range.any()
    assert (env.trajectory.status[2] == steps).all() and not out[3].any()
    with pytest.raises(NotImplementedError, match="whole-step graphs"):
        env.enable_graph(True, whole_step=True)
    env.close()
    env, held, out = replay("raise")
    assert env.trajectory.out_of_range.all() and out[3].all(), "every lane leaves the trajectory at step 7 and is truncated"
    assert torch.equal(env.trajectory.q, held["q"])
    env.close()
    first.close()


@pytest.mark.gpu
def test_environment_without_the_keyword_builds_no_trajectory_block(gpu_device):
    from jiminy_amd.envs import make_anymal_env
    env = make_anymal_env(8, device=gpu_device, contact_model="constraint", auto_reset=False, foot_poses={})
    assert env.trajectory is None and env._reference_frames is None and env._reference_foot_poses is None
    assert not hasattr(env, "_trajectory_time")
    with pytest.raises(RuntimeError, match="needs trajectory_database"):
        env.select_trajectory("a")
    env.close()
