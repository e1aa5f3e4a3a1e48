"""The centroidal state block: `k_centroidal_state` (jiminy_amd/csrc/jm_centroidal.h) behind `jm_block_centroidal_state`,
`blocks.CentroidalState` and `blocks.LocomotionQuantities(state=(q, centroidal))`.

The specification is the oracle: the `centroidal` rows `extra_terms` of oracle/oracle.cpp leaves for the state `(q, v, a)` it
reports.  The kernel body is held to them on the host (tests/hostemu/centroidal.cpp) and on the device, in float64 within the
tolerance tests/test_gpu_parity.py applies to `centroidal` between the engine and the oracle at `start` (1e-11 in its metric:
no integration lies between the state and the rows here, after a step either), in float32 within the bound derived in
tests/centroidal_numpy.py.

Which `a` the oracle's rows belong to: `test_oracle_rows_belong_to_the_reported_acceleration` evaluates the rows from the
reported `(q, v, a)` at `start` and after 3 RK4 steps, and both agree with the oracle's to round-off (measured 5e-16): the `a`
reported after a step is the one `extra_terms` saw, so the states after the steps are used as well.

The oracle's centre of mass is that of the subtree of joint 1 (oracle.cpp: "single root joint assumed by the reference"): on
the fixed-base `tree_arm`, where three joints hang on the universe, it is not the robot's.  That robot is held to the numpy
companion instead, which the floating-base robots tie to the oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, centroidal, codegen, load_builtin
from jiminy_amd.synthetic import sample_states
from oracle.oracle_py import OracleEngine
from tests import centroidal_numpy as cn
from tests import robots
from tests.helpers import rel_err
from tests.hostemu import centroidal as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
NEW_SYMBOLS = ("jm_centroidal_plan_create", "jm_centroidal_plan_destroy", "jm_block_centroidal_state")
DTYPES = (np.float64, np.float32)
TOL64 = 1e-11           # tests/test_gpu_parity.py: `centroidal` of the engine against the oracle, `rel_err`
POISON = 7.0
B = 64
MODELS = {"anymal": lambda: load_builtin("anymal"), "tree_arm_ff": lambda: robots.tree_arm(True),
          "tree_arm_flex_ff": lambda: robots.tree_arm_flexible(True), "tree_arm": lambda: robots.tree_arm(False),
          # 26 joints (free-flyer included) on a tree with two trunk branches (neck chain, tail) next to the limbs: against the numpy companion
          "hydra": robots.hydra}
ORACLE_MODELS = ("anymal", "tree_arm_ff", "tree_arm_flex_ff")
_CACHE: dict = {}


def model_of(name: str):
    if ("model", name) not in _CACHE:
        _CACHE["model", name] = MODELS[name]()
    return _CACHE["model", name]


def desc_of(name: str):
    if ("desc", name) not in _CACHE:
        _CACHE["desc", name] = centroidal.build_plan(model_of(name)).desc()
    return _CACHE["desc", name][0]


def oracle_states(name: str) -> dict:
    """64 sampled states with nonzero joint and base velocities through the oracle: `(q, v, a, centroidal)` `[rows][64]` at
    `start` ("start") and after 3 RK4 steps of 1 ms ("steps"), and the numpy companion's rows and bounds of both.  Computed
    once and never written to."""
    if ("states", name) in _CACHE:
        return _CACHE["states", name]
    model = model_of(name)
    st = sample_states(model, B, seed=3)
    assert np.abs(st["v"]).min(axis=1).max() > 0
    out = {}
    rows = {"start": [], "steps": []}
    for b in range(B):
        e = OracleEngine(model)
        e.start(st["q"][:, b], st["v"][:, b], st["command"][:, b] if model.nmotors else None)
        rows["start"].append([e.get(k).copy() for k in ("q", "v", "a", "centroidal")])
        for _ in range(3):
            e.step(1e-3)
        rows["steps"].append([e.get(k).copy() for k in ("q", "v", "a", "centroidal")])
    for when, lanes in rows.items():
        s = {k: np.ascontiguousarray(np.stack([lane[i] for lane in lanes], axis=1)) for i, k in enumerate(("q", "v", "a", "centroidal"))}
        for dtype in DTYPES:
            ref = cn.run(model, s["q"], s["v"], s["a"], dtype)
            s["numpy"], s["bound." + np.dtype(dtype).name] = ref["centroidal"], ref["bound"]
        for a in s.values():
            a.setflags(write=False)
        out[when] = s
    _CACHE["states", name] = out
    return out


def expected_of(name: str, s: dict) -> np.ndarray:
    return s["centroidal"] if name in ORACLE_MODELS else s["numpy"]


def check_states(name: str, run, label: str) -> None:
    """`run(desc, q, v, a, dtype)` on the states of a model against the expectation: float64 in the metric and tolerance of
    tests/test_gpu_parity.py, float32 inside the bound of the numpy companion."""
    for when, s in oracle_states(name).items():
        want = expected_of(name, s)
        got = run(desc_of(name), s["q"], s["v"], s["a"], np.float64)
        err = rel_err(got, want)
        print(f"{label} {name} {when} float64: rel_err {err:.3g}")
        assert err < TOL64, (name, when, err)
        got = run(desc_of(name), s["q"], s["v"], s["a"], np.float32)
        assert got.dtype == np.float32
        worst = float((np.abs(got.astype(np.float64) - want) / s["bound.float32"]).max())
        print(f"{label} {name} {when} float32: worst error / bound {worst:.3g}")
        assert worst <= 1.0, (name, when, worst)


# -------------------------------------------------------------------------------------------------------- specification
@pytest.mark.parametrize("name", ORACLE_MODELS)
def test_oracle_rows_belong_to_the_reported_acceleration(name):
    """The numpy companion from the reported `(q, v, a)` reproduces the oracle's rows at `start` and after the steps: the dhg
    rows (9 ..) depend on `a`, and are not small."""
    for when, s in oracle_states(name).items():
        assert np.abs(s["centroidal"][9:]).max() > 1e-2 and np.abs(s["a"]).max() > 1e-2
        err = rel_err(s["numpy"], s["centroidal"])
        print(f"numpy {name} {when}: rel_err {err:.3g}")
        assert err < TOL64, (when, err)
        # (with another acceleration the rows are another's: the test can tell)
        other = cn.run(model_of(name), s["q"], s["v"], 0.5 * s["a"])["centroidal"]
        assert rel_err(other, s["centroidal"]) > 1e-3


@pytest.mark.parametrize("name", list(MODELS))
def test_emulated_kernel_matches_the_oracle(name):
    check_states(name, lambda desc, q, v, a, dtype: emu.run(desc, q, v, a, dtype=dtype), "emulation")


def test_models_cover_every_joint_kind():
    kinds = set()
    for name in MODELS:
        kinds |= {int(k) for k in centroidal.build_plan(model_of(name)).arrays["seg_kind"]}
    print("segment kinds of the models:", sorted(kinds))
    # every kind of jm_frames_desc but 2, 8 and 10: aligned revolute and prismatic joints differ by the index of their axis alone
    assert kinds >= {0, 1, 3, 4, 5, 6, 7, 9, 11}, kinds


def _state_at(model, q, v, a, s, oracle):
    """The state on the curve through (q, v) with constant acceleration a, at parameter s: `integrate` of the oracle."""
    return oracle.integrate(q, s * v + 0.5 * s * s * a), v + s * a


@pytest.mark.parametrize("name", ["anymal", "tree_arm_ff", "tree_arm"])
def test_time_derivatives_converge_at_second_order(name):
    """d(com)/dt = hg_linear / mass and d(hg)/dt = dhg by central differences along the curve `integrate(q, s v + s^2 a / 2)`,
    `v + s a`: the error falls by about four times from h to h / 2 (between 3.5 and 4.5 on the worst row of 16 lanes).  No
    fixed bound: a wrong term in dhg leaves an error that does not fall at all.  The law holds for any acceleration: a seeded
    N(0, 2^2) one stands in for the oracle's, whose contact accelerations of 1e3 .. 1e4 rad/s^2 put h = 1e-2 outside the
    asymptotic range."""
    model = model_of(name)
    s = oracle_states(name)["start"]
    oracle = OracleEngine(model)
    desc, lanes = desc_of(name), range(16)
    mass = centroidal.build_plan(model).mass
    acc = 2.0 * np.random.default_rng(17).standard_normal((model.nv, 16))

    def rows_at(h):
        q, v = zip(*[_state_at(model, s["q"][:, b], s["v"][:, b], acc[:, b], h, oracle) for b in lanes])
        return emu.run(desc, np.stack(q, 1), np.stack(v, 1), None)

    base = emu.run(desc, s["q"][:, :16], s["v"][:, :16], acc)
    errors = []
    for h in (2e-2, 1e-2):
        d = (rows_at(h) - rows_at(-h)) / (2 * h)
        errors.append((np.abs(d[0:3] - base[3:6] / mass).max(), np.abs(d[3:9] - base[9:15]).max()))
    for k, label in enumerate(("d(com)/dt = hg_linear / mass", "d(hg)/dt = dhg")):
        coarse, fine = errors[0][k], errors[1][k]
        print(f"{name} {label}: error {coarse:.3g} at h, {fine:.3g} at h / 2, ratio {coarse / fine:.3f}")
        assert fine > 1e-12, "the differences are not resolved"
        assert 3.5 < coarse / fine < 4.5, (label, coarse, fine)


def check_designed_lanes(run) -> None:
    """What must hold to the bit: a state at rest, a null `a`, lanes outside the mask, an absent output."""
    for name in ("anymal", "tree_arm_ff"):
        s = oracle_states(name)["steps"]
        desc = desc_of(name)
        for dtype in DTYPES:
            zero = np.zeros_like(s["v"])
            rest = run(desc, s["q"], zero, zero, None, dtype, None)
            assert (rest[3:] == 0).all() and np.isfinite(rest[:3]).all() and np.abs(rest[:3]).max() > 0.1
            full = run(desc, s["q"], s["v"], s["a"], None, dtype, None)
            without = run(desc, s["q"], s["v"], None, None, dtype, None)
            with_zero = run(desc, s["q"], s["v"], zero, None, dtype, None)
            assert (without[9:] == 0).all() and np.array_equal(without[:9], with_zero[:9]) and np.array_equal(without[:9], full[:9])
            assert np.abs(with_zero[9:]).max() > 1e-3, "the velocity-product terms of dhg"
            mask = np.arange(B) % 3 != 0
            into = np.full((15, B), POISON, dtype=dtype)
            run(desc, s["q"], s["v"], s["a"], mask, dtype, into)
            assert np.array_equal(into[:, mask], full[:, mask]) and (into[:, ~mask] == POISON).all()
            assert run(desc, s["q"], s["v"], s["a"], None, dtype, "absent") is None


def test_emulated_designed_lanes():
    check_designed_lanes(lambda desc, q, v, a, mask, dtype, into:
                         emu.run(desc, q, v, a, mask=mask, dtype=dtype, absent=True) if isinstance(into, str)
                         else emu.run(desc, q, v, a, mask=mask, dtype=dtype, into=into))


# ------------------------------------------------------------------------------------------------------ plan validation
def _good() -> dict:
    return dict(centroidal.build_plan(model_of("tree_arm_ff")).arrays)


def _rejections() -> list:
    p = _good()
    n_seg, n_bodies = len(p["seg_kind"]), len(p["body_mass"])

    def change(key, at, value):
        a = np.array(p[key], dtype=np.float64 if key.startswith(("seg_rot", "seg_trans", "seg_axis", "body_")) and key != "body_seg_start"
                     else np.int64).copy()
        a[at] = value
        return {key: a}
    first_joint = next(i for i, k in enumerate(p["seg_kind"]) if k != 0)
    return [
        (dict(nq=-1), "bad sizes"), (dict(njoints=0), "bad sizes"),
        (change("body_seg_start", 0, 1), "body_seg_start must run from 0 to n_seg"),
        (change("body_seg_start", n_bodies, n_seg - 1), "body_seg_start must run from 0 to n_seg"),
        (change("body_seg_start", 1, 0), r"body 0 has a bad segment count \(1 .. 256\)"),
        (change("seg_kind", first_joint, 12), f"segment {first_joint} has an unknown joint kind"),
        (change("seg_kind", first_joint, -1), f"segment {first_joint} has an unknown joint kind"),
        (change("seg_q_index", first_joint, p["nq"]), rf"segment {first_joint} reads q rows \[{p['nq']}, .*\) out of range \[0, {p['nq']}\)"),
        (change("seg_q_index", first_joint, -1), rf"segment {first_joint} reads q rows \[-1, "),
        (change("seg_v_index", first_joint, p["nv"] - 1), rf"segment {first_joint} reads v rows .* out of range \[0, {p['nv']}\)"),
        (change("seg_joint", first_joint, p["njoints"]), rf"segment {first_joint} has joint index {p['njoints']} out of range"),
        (change("seg_rot", (1, 0, 0), np.nan), "segment 1 has a constant that is not finite"),
        (change("seg_trans", (0, 2), np.inf), "segment 0 has a constant that is not finite"),
        (change("body_mass", 1, np.nan), "body 1 has a constant that is not finite"),
        (change("body_com", (2, 1), np.inf), "body 2 has a constant that is not finite"),
        (change("body_inertia", (0, 5), np.nan), "body 0 has a constant that is not finite"),
        (change("body_mass", 2, -1.0), "body 2 has a negative mass"),
        (dict(body_mass=np.zeros(n_bodies)), "the bodies have no mass"),
    ]


POINTERS = ("body_seg_start", "seg_kind", "seg_joint", "seg_q_index", "seg_v_index", "seg_rot", "seg_trans", "seg_axis", "body_mass",
            "body_com", "body_inertia")


def test_plan_validation_rejects_every_malformed_description():
    for name in MODELS:
        emu.pack(desc_of(name))
    with pytest.raises(ValueError, match="jm_centroidal_plan_create: null description"):
        emu.pack(None)
    for change, message in _rejections():
        desc, keep = centroidal.make_desc(**{**_good(), **change})
        with pytest.raises(ValueError, match="jm_centroidal_plan_create: .*" + message):
            emu.pack(desc)
    for pointer in POINTERS:
        desc, keep = centroidal.make_desc(**_good())
        setattr(desc, pointer, None)
        with pytest.raises(ValueError, match="null array in the description"):
            emu.pack(desc)
    desc, keep = centroidal.make_desc(**_good())
    desc.n_bodies = 0
    with pytest.raises(ValueError, match="bad sizes"):
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
    assert lib.L.jm_centroidal_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = centroidal.make_desc(**_good())
    assert lib.L.jm_centroidal_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    for change, message in _rejections():
        d, keep = centroidal.make_desc(**{**_good(), **change})
        rc = lib.L.jm_centroidal_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and re.search(message, _last_error(lib)), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    assert lib.L.jm_block_centroidal_state(None, _abi.JM_F64, 64, None, None, None, None, None, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    # the order of the fields in the header is the order of the ctypes mirror
    body = header.split("typedef struct jm_centroidal_desc")[1].split("} jm_centroidal_desc;")[0]
    order = [line.split(";")[0].split()[-1] for line in body.splitlines() if ";" in line]
    assert order == [f[0] for f in _abi.CentroidalDesc._fields_]
    assert os.path.join(codegen.CSRC, "jm_centroidal.h") in codegen._sources()
    assert '#include "jm_centroidal.h"' in open(os.path.join(codegen.CSRC, "jm_lib_blocks.cpp")).read()
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


# ------------------------------------------------------------------------------------------------------------ host side
def test_build_plan_of_the_builtin_anymal():
    model = load_builtin("anymal")
    plan = centroidal.build_plan(model)
    assert plan.joints == list(range(1, model.njoints)) and plan.n_bodies == 13
    # a walk per body: its joints and the trailing constant segment -- 1 + 3 x 4 bodies at depths 1, 2, 3, 4
    assert plan.depth == [2] + [3, 4, 5] * 4 and sum(plan.depth) == 50
    assert abs(plan.mass - float(np.sum(model.mass[1:]))) < 1e-12
    a = plan.arrays
    assert np.array_equal(a["body_inertia"][0], np.asarray(model.inertia[1])[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]])
    assert np.array_equal(a["body_com"], model.com[1:]) and list(a["seg_kind"]).count(7) == 13
    with pytest.raises(ValueError, match="a model with mass"):
        centroidal.build_plan(SimpleNamespace(njoints=2, mass=np.zeros(2), inertia=np.zeros((2, 3, 3))))


def test_python_surface_refusals_on_the_host(monkeypatch):
    import torch

    from jiminy_amd import blocks
    model = load_builtin("anymal")
    eng = SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _fields={}, _ground=None,
                          _options={"contacts": {"model": "constraint"}}, _lib=SimpleNamespace(L=None, check=None))
    q, v = torch.zeros(model.nq, 4, dtype=torch.float64), torch.zeros(model.nv, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"state q must have shape \(19, 4\)"):
        blocks.CentroidalState(eng, state=(q[:7], v, None))
    with pytest.raises(ValueError, match=r"state v must have shape \(18, 4\)"):
        blocks.CentroidalState(eng, state=(q, None, None))
    with pytest.raises(ValueError, match=r"state a must have shape \(18, 4\)"):
        blocks.CentroidalState(eng, state=(q, v, q))
    names = ["root_joint"] + list(model.contacts)
    frames = SimpleNamespace(_eng=eng, frame_names=names, average=False, index=names.index, plan=SimpleNamespace(modes=[0] * 5),
                             _state=(q, v))
    rows = torch.zeros(15, 4, dtype=torch.float64)
    # a recorded trajectory carries no constraint multipliers
    with pytest.raises(NotImplementedError, match=r"no constraint multipliers \(`State.lambda_c`\)"):
        blocks.LocomotionQuantities(eng, frames, state=(q, rows))
    with pytest.raises(NotImplementedError, match="lambda_c"):
        blocks.LocomotionQuantities(eng, frames, state=(q, rows), forces=True, momentum=False)
    with pytest.raises(ValueError, match=r"state centroidal must have shape \(15, 4\)"):
        blocks.LocomotionQuantities(eng, frames, state=(q, rows[:9]), forces=False, momentum=False)
    with pytest.raises(ValueError, match="built on the same state"):
        blocks.LocomotionQuantities(eng, frames, state=(q.clone(), rows), forces=False, momentum=False)
    frames._state = None
    with pytest.raises(ValueError, match="built on the same state"):
        blocks.LocomotionQuantities(eng, frames, state=(q, rows), forces=False, momentum=False)
    # where the state has no acceleration the block has no `zmp` (built up to the plan on stand-ins for the library)
    import contextlib
    lib = SimpleNamespace(L=SimpleNamespace(jm_locomotion_plan_create=lambda desc, out: 0, jm_locomotion_plan_destroy=lambda plan: 0),
                          check=lambda rc: None)
    host = SimpleNamespace(**{**vars(eng), "_lib": lib})
    frames = SimpleNamespace(**{**vars(frames), "_eng": host, "_state": (q, v)})
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    for has in (False, True):
        state = object.__new__(blocks.CentroidalState)
        state.has_acceleration, state.centroidal = has, rows
        blk = blocks.LocomotionQuantities(host, frames, state=(q, state), forces=False, momentum=False)
        assert (blk.zmp is None) == (not has) and blk.dcm.shape == (2, 4) and blk.h_angular is None
        assert has is False or blk.zmp.shape == (2, 4)
    frames._eng, frames._state = eng, None
    # without the keyword the engine's field is still required
    with pytest.raises(ValueError, match="read the 'centroidal' output of the engine"):
        blocks.LocomotionQuantities(eng, frames, forces=False, momentum=False)
    monkeypatch.setenv("JIMINY_AMD_TENSOR_BLOCKS", "1")
    with pytest.raises(NotImplementedError, match="no tensor-program form"):
        blocks.CentroidalState(eng, state=(q, v, None))


# ------------------------------------------------------------------------------------------------------------ device
class DeviceCentroidal:
    """Plans on the device and the launch on numpy arrays (copied in and out)."""

    def __init__(self, lib, device):
        import torch
        self.torch, self.lib, self.device, self.plans = torch, lib, device, {}

    def handle(self, desc):
        if id(desc) not in self.plans:
            h = C.c_void_p()
            with self.torch.cuda.device(self.device):
                self.lib.check(self.lib.L.jm_centroidal_plan_create(C.byref(desc), C.byref(h)))
            self.plans[id(desc)] = (h, desc)
        return self.plans[id(desc)][0]

    def close(self):
        for h, _ in self.plans.values():
            self.lib.L.jm_centroidal_plan_destroy(h)

    def run(self, desc, q, v, a=None, mask=None, dtype=np.float64, into=None):
        torch = self.torch
        n = q.shape[1]
        up = lambda x, kind: None if x is None else torch.as_tensor(np.array(x, dtype=kind, order="C"), device=self.device)      # noqa: E731
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
        assert q.shape[0] == desc.nq and v.shape == (desc.nv, n) and (a is None or a.shape == (desc.nv, n))
        tq, tv, ta, tm = up(q, dtype), up(v, dtype), up(a, dtype), up(mask, np.uint8)
        absent = isinstance(into, str)
        out = None
        if not absent:
            out = np.full((15, n), np.nan, dtype=dtype) if into is None else into
            assert out.shape == (15, n) and out.dtype == np.dtype(dtype)
        to = up(out, dtype)
        self.lib.check(self.lib.L.jm_block_centroidal_state(
            self.handle(desc), _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, n, ptr(tq), ptr(tv), ptr(ta), ptr(tm),
            ptr(to), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        if absent:
            return None
        out[...] = to.cpu().numpy()
        return out


@pytest.fixture
def device_centroidal(gpu_device):
    dev = DeviceCentroidal(_prebuilt(load_builtin("cartpole")), gpu_device)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_device_matches_the_oracle(name, device_centroidal):
    """`k_centroidal_state` through the C ABI at B = 64 on the oracle states, both dtypes, same expectations and bounds."""
    check_states(name, lambda desc, q, v, a, dtype: device_centroidal.run(desc, q, v, a, dtype=dtype), "device")


@pytest.mark.gpu
def test_device_tail_block_and_repeatability(device_centroidal):
    """ANYmal at B = 257: a second block of one lane; every lane repeats one of the 64 states and gives its bits; two launches
    give the same bits."""
    s = oracle_states("anymal")["steps"]
    lanes = np.arange(257) % B
    desc = desc_of("anymal")
    for dtype in DTYPES:
        args = (desc, s["q"][:, lanes], s["v"][:, lanes], s["a"][:, lanes])
        first, second = device_centroidal.run(*args, dtype=dtype), device_centroidal.run(*args, dtype=dtype)
        assert first.shape == (15, 257) and np.array_equal(first, second) and np.isfinite(first).all()
        assert np.array_equal(first[:, B:], first[:, lanes[B:]])
        if dtype == np.float64:
            assert rel_err(first, s["centroidal"][:, lanes]) < TOL64


@pytest.mark.gpu
def test_device_designed_lanes(device_centroidal):
    check_designed_lanes(lambda desc, q, v, a, mask, dtype, into: device_centroidal.run(desc, q, v, a, mask, dtype, into))


def _anymal_engine(gpu_device, n):
    import torch

    from jiminy_amd.engine import BatchedEngine
    model = load_builtin("anymal")
    eng = BatchedEngine(model, n, dtype=torch.float64, device=gpu_device, extra_outputs=("centroidal",))
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": 1e-3, "controllerUpdatePeriod": 1e-3, "sensorsUpdatePeriod": 1e-3},
                     "contacts": {"model": "spring_damper"}})
    st = sample_states(model, n, seed=9)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    return eng


@pytest.mark.gpu
def test_block_reproduces_the_engines_own_rows(gpu_device):
    """The ANYmal engine (no model bias) with `extra_outputs=("centroidal",)`: at `start` and after 5 steps,
    `CentroidalState(state=(engine q, v, a))` reproduces the rows the physics kernels left, within the float64 tolerance; the
    tensor keeps its identity; a masked reset keeps the other lanes bit for bit; a captured graph of the refresh replays to the
    same bits as the eager launch."""
    import torch

    from jiminy_amd import blocks
    eng = _anymal_engine(gpu_device, B)
    blk = blocks.CentroidalState(eng, state=(eng.field("q"), eng.field("v"), eng.field("a")))
    rows, address = blk.centroidal, blk.centroidal.data_ptr()
    assert rows.shape == (15, B) and blk.has_acceleration and abs(blk.mass - float(np.sum(eng.model.mass[1:]))) < 1e-12
    assert len(blk.fieldnames["centroidal"]) == 15
    for k in range(6):
        if k:
            eng.step(1e-3)
        blk.refresh()
        torch.cuda.synchronize(gpu_device)
        got, want = rows.cpu().numpy(), eng.field("centroidal").cpu().numpy()
        err = rel_err(got, want)
        print(f"block against the engine's centroidal after {k} steps: rel_err {err:.3g}")
        assert err < TOL64 and np.abs(want[9:]).max() > 1e-2, (k, err)
    assert blk.centroidal is rows and rows.data_ptr() == address
    eager = rows.clone()
    rows.fill_(POISON)
    mask = torch.arange(B, device=gpu_device) % 2 == 0
    blk.reset(mask)
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(rows[:, mask], eager[:, mask]) and (rows[:, ~mask] == POISON).all()
    # graph capture: one launch, no allocation, copy or synchronisation
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.graph(graph):
        blk.refresh()
    rows.fill_(POISON)
    graph.replay()
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(rows, eager)


@pytest.mark.gpu
def test_locomotion_quantities_of_a_state(gpu_device):
    """`LocomotionQuantities(state=(q, centroidal))` on a copy of the engine's own state gives the engine-side block's `com`,
    `vcom`, `odom_pose`, `zmp`, `dcm` (the same kernel on rows that agree within the float64 tolerance: compared in the metric
    of that tolerance); without `a` the block has no `zmp`."""
    import torch

    from jiminy_amd import blocks
    eng = _anymal_engine(gpu_device, B)
    for _ in range(3):
        eng.step(1e-3)
    names = ["root_joint"] + list(eng.model.contacts)
    true_frames = blocks.FrameKinematics(eng, names)
    true = blocks.LocomotionQuantities(eng, true_frames, forces=False, momentum=False)
    q, v, a = (eng.field(k).clone() for k in ("q", "v", "a"))
    ref_frames = blocks.FrameKinematics(eng, names, state=(q, v))
    state = blocks.CentroidalState(eng, state=(q, v, a))
    ref = blocks.LocomotionQuantities(eng, ref_frames, forces=False, momentum=False, state=(q, state))
    for blk in (true_frames, true, ref_frames, state, ref):
        blk.refresh()
    torch.cuda.synchronize(gpu_device)
    for k in ("com", "vcom", "odom_pose", "zmp", "dcm"):
        got, want = getattr(ref, k).cpu().numpy(), getattr(true, k).cpu().numpy()
        # (the ZMP of a lane in free fall is NaN on both sides)
        held = ~np.isnan(want).any(axis=0)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and (held.all() or k == "zmp") and held.any(), (k, int(held.sum()))
        err = rel_err(got, want, held)
        print(f"state-side {k} against the engine-side block: rel_err {err:.3g} on {int(held.sum())} lanes")
        assert err < TOL64, (k, err)
    assert torch.equal(ref.odom_pose, true.odom_pose) and ref.h_angular is None and ref.contact_force_rel is None
    bare = blocks.CentroidalState(eng, state=(q, v, None))
    no_zmp = blocks.LocomotionQuantities(eng, ref_frames, forces=False, momentum=False, state=(q, bare))
    assert not bare.has_acceleration and no_zmp.zmp is None
    bare.refresh()
    no_zmp.refresh()
    torch.cuda.synchronize(gpu_device)
    assert (bare.centroidal[9:] == 0).all() and torch.equal(bare.centroidal[:9], state.centroidal[:9])
    assert torch.equal(no_zmp.dcm, ref.dcm) and torch.equal(no_zmp.com, ref.com)
    with pytest.raises(NotImplementedError, match="lambda_c"):
        blocks.LocomotionQuantities(eng, ref_frames, state=(q, state))
