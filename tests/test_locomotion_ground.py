"""Locomotion quantities on height-map ground (`locomotion_lane<T, true>` of csrc/jm_locomotion.h and csrc/jm_ground.h behind
`jm_block_locomotion_ground`, `blocks.LocomotionQuantities(ground_profile=True)`, `WalkerVecEnv(locomotion_quantities=
dict(ground_profile=True, ...))`).

Specification: the reference's own output, tests/golden/ref_locomotion_ground.npz (tools/make_ref_locomotion_ground_fixtures.py
executes the reference's functions; six cases of 64 lanes).  The bars are those of tests/test_locomotion_quantities.py:
float64 within 1e-13 relative to max(|want|, 1) on every lane and output, NaN positions identical (there is none); float32
within 4 x the error of the float32 numpy restatement (tests/locomotion_ground_numpy.py) on the same case and quantity.

Measured on the host (error relative to max(|want|, 1), largest over the six cases and the lanes):
  float64, host emulation | numpy restatement
    com 0 | 0   vcom 0 | 0   odom_pose 2.2e-16 | 0   zmp 2.7e-15 | 0   dcm 1.3e-15 | 0   h_angular 8.9e-16 | 8.9e-16
    contact_force_rel 0 | 0   foot_force_vertical 2.9e-16 | 2.9e-16   scalars 2.2e-16 | 2.2e-16   contact_ground 1.1e-16 | 1.1e-16
  float32, host emulation | numpy restatement (the error is that of rounding the inputs to float32)
    com 5.6e-8 | 5.6e-8   vcom 1.0e-7 | 1.0e-7   odom_pose 1.6e-7 | 1.5e-7   zmp 1.1e-6 | 1.4e-6   dcm 1.0e-6 | 1.0e-6
    h_angular 4.6e-7 | 4.6e-7   contact_force_rel 1.8e-7 | 1.8e-7   foot_force_vertical 3.0e-7 | 3.0e-7   scalars 1.8e-7 | 1.8e-7
    contact_ground 2.2e-7 | 2.2e-7
  largest ratio emulation / restatement of one case and quantity in float32: 1.34 (odom_pose, `edges`).

Newton's law on a slope (ANYmal, 64 lanes, constraint contacts, 25 steps under zero action on a plane of slope 0.2 with a
patch per lane): sum(foot_force_vertical) - 1 = dhg_linear_z / weight, the right-hand side from the `centroidal` rows.  Bound:
4 x the error of the host composition (the numpy restatement on the tensors the block read) against the same law, plus
4 x 2.2e-16.

Measured on the device (MI355X; the same six cases through the C ABI, largest over the cases and the lanes):
  float64  com 0   vcom 0   odom_pose 2.7e-16   zmp 2.2e-15   dcm 1.5e-15   h_angular 6.9e-16   contact_force_rel 0
           foot_force_vertical 3.5e-16   scalars 4.4e-16   contact_ground 3.9e-16
  float32  com 5.7e-8   vcom 1.0e-7   odom_pose 1.5e-7   zmp 1.4e-6   dcm 1.0e-6   h_angular 5.6e-7   contact_force_rel 1.8e-7
           foot_force_vertical 3.0e-7   scalars 1.8e-7   contact_ground 2.2e-7; largest ratio device / numpy float32 of one case
           and quantity: 2.31 (h_angular, `tiles`); of what looks at the ground: 1.15 (scalars, `edges`)
  `tiles` at B = 300 against the emulation on the same arrays: float64 at most 1.0e-15 (dcm), float32 at most 7.8e-7 (dcm, bound
  2.0e-6); a null structure and a structure without heights: the bits of `jm_block_locomotion`; the zero map against the flat
  kernel: 0 on every output in float64, 0 but 6.0e-8 on the scalars (the `powf` of a reward row) in float32.
  ANYmal on the slope, device against the host composition on the same tensors: at most 2.2e-16 (h_angular, scalars).  After
  25 steps 2 to 4 contacts per lane are enabled, the feet carry 0.886 to 1.374 times the weight, |dhg_linear_z| / weight is up
  to 0.374.  Law, device | host composition: 7.49e-16 | 7.49e-16 (bound 3.9e-15); the flat formula misses it by 9.7e-2.
  Raised ramp: distance to the ground of the standing lanes 0.010 to 0.019 m after the first step and -0.003 to -0.001 m after
  the second, of the lifted lanes 0.509 to 0.518 m and 0.486 to 0.494 m; the ground under the contacts is 0.442 to 0.557 m high.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, codegen, load_builtin
from tests import locomotion_ground_numpy as gn
from tests import locomotion_numpy as ln
from tests import test_locomotion_quantities as flat_tests
from tests.hostemu import locomotion as emu_flat
from tests.hostemu import locomotion_ground as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_locomotion_ground.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_locomotion_ground_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
TOL = 1e-13
EPS = 2.2e-16
MARGIN = 2.0 ** -10
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["cases"]]
_CASES: dict = {}
rel_error, _prebuilt, _last_error = flat_tests.rel_error, flat_tests._prebuilt, flat_tests._last_error


def case(name: str):
    """plan, inputs, ground, expected, designed contacts and the two numpy restatements of a case, computed once."""
    if name not in _CASES:
        plan, inputs, ground, expected, designed = gn.load_case(FX, name)
        _CASES[name] = (plan, inputs, ground, expected, designed, gn.quantities(plan, inputs, ground, np.float64),
                        gn.quantities(plan, inputs, ground, np.float32))
    return _CASES[name]


def check_against_the_fixture(name: str, run, label: str) -> None:
    """`run(plan, inputs, ground, dtype) -> outputs` against the fixture in both dtypes, every lane of every output."""
    plan, inputs, ground, expected, _, _, n32 = case(name)
    for dtype in (np.float64, np.float32):
        got = run(plan, inputs, ground, dtype)
        for out in gn.OUTPUTS:
            assert not np.isnan(expected[out]).any()
            e = rel_error(got[out], expected[out])
            if dtype is np.float64:
                print(f"{label} {name} float64 {out}: {e:.2e}")
                assert e <= TOL, (name, out, e)
            else:
                e_np = rel_error(n32[out], expected[out])
                print(f"{label} {name} float32 {out}: {e:.2e} (numpy float32 {e_np:.2e})")
                assert e <= 4.0 * e_np, (name, out, e, e_np)


# ------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_from_the_reference_tree():
    done = subprocess.run([sys.executable, TOOL, "--check"], capture_output=True, text=True)
    if "run this where the reference tree is available" in done.stderr:
        pytest.skip("the reference tree is not here: the committed fixture stands")
    assert done.returncode == 0, done.stdout + done.stderr


def test_fixture_holds_the_designed_cases_and_the_draw_conditions():
    assert CASES == ["ramp", "tiles", "edges", "steep", "zero_map", "per_lane_model"] and os.path.getsize(FIXTURE) <= 1 << 20
    for name in CASES:
        plan, inputs, ground, expected, designed, _, _ = case(name)
        nc = len(plan["contact_foot"])
        assert inputs["centroidal"].shape == (15, 64) and designed.shape == (nc, 64)
        assert ("model_lane" in inputs) == (name == "per_lane_model")
        assert all(v.shape[-1] == 64 and np.isfinite(v).all() for v in expected.values())       # no lane left out anywhere
        assert sorted(expected) == sorted(gn.OUTPUTS)
        # the draw of the flat tool
        c = inputs["centroidal"]
        mass = np.sum(inputs["model_lane"][0::13][1:], 0) if "model_lane" in inputs else np.sum(plan["body_mass"][1:])
        r = (c[11] + mass * plan["gravity"]) / (mass * plan["gravity"])
        assert ((r >= 0.2) & (r <= 3.0)).all()
        assert np.abs(c[:2]).max() <= 2.0 and c[2].min() >= 0.2 and c[2].max() <= 1.5
        assert (np.sum(expected["h_angular"] ** 2, 0) <= 4.0 * plan["momentum_cutoff"] ** 2 * (1 + 1e-12)).all()
        assert (np.sum(expected["contact_force_rel"][:2] ** 2, (0, 1)) <= 4.0 * plan["friction_cutoff"] ** 2).all()
        # the draw on the ground: clear of the cell lines outside the designed contacts, z - h in [-0.05, 0.5]
        pose = inputs["pose"][:, [int(k) for k in plan["contact_column"]]]
        off = ground.get("offsets", np.zeros((2, 64)))
        x, y = pose[0] + off[0], pose[1] + off[1]
        u, w = gn.grid_coordinates(ground, x, y)
        for g in (u, w):
            assert (np.abs(g - np.round(g)) >= MARGIN)[~designed].all()
        dz = pose[2] - expected["contact_ground"][0]
        assert dz.min() >= -0.05 and dz.max() <= 0.5
        assert designed.any() == (name == "edges")
        assert np.abs(np.linalg.norm(expected["contact_ground"][1:], axis=0) - 1.0).max() <= 4 * EPS
    ny_nx = {name: case(name)[2]["heights"].shape for name in CASES}
    assert ny_nx == dict(ramp=(3, 3), tiles=(4, 5), edges=(2, 2), steep=(4, 4), zero_map=(3, 3), per_lane_model=(4, 5))
    assert list(FX["ramp.plan.contact_foot"]) == [0, 1, 2, 3] and list(FX["tiles.plan.contact_foot"]) == [0, 0, 0, -1, 1, 1, 1, 1]
    # ramp: a plane (one normal everywhere); tiles: dx != dy, an origin, offsets, disabled constraints
    n = FX["ramp.expected.contact_ground"][1:]
    assert np.abs(n - n[:, :1, :1]).max() <= 4 * EPS and abs(n[0, 0, 0]) > 0.05
    g = case("tiles")[2]
    assert g["dx"] != g["dy"] and g["x0"] != 0.0 and g["y0"] != 0.0 and g["offsets"].shape == (2, 64) and np.abs(g["offsets"]).min() > 0
    assert ((FX["tiles.con_flags"] & 1) == 0).any() and "offsets" not in case("edges")[2] and "offsets" not in case("ramp")[2]
    # edges: powers of two, the designed contacts exact in float32: on a node, on a cell edge, past the four sides and a corner
    g, designed = case("edges")[2], case("edges")[4]
    assert all(np.log2(g[k]) == np.round(np.log2(g[k])) for k in ("dx", "dy"))
    plan, inputs = case("edges")[:2]
    p = inputs["pose"][:, int(plan["contact_column"][0])]
    assert designed[0, :10].all() and designed.sum() == 10
    assert np.array_equal(p[:2, :10].astype(np.float32).astype(np.float64), p[:2, :10])
    u, w = gn.grid_coordinates(g, p[0, :10], p[1, :10])
    got = set(zip(u.tolist(), w.tolist()))
    assert {(0.0, 0.0), (1.0, 1.0), (0.5, 0.0), (1.0, 0.25), (-0.5, 0.5), (1.5, 0.5), (0.5, -0.5), (0.5, 1.5), (1.5, 1.5)} <= got
    u32, w32 = gn.grid_coordinates(g, p[0, :10].astype(np.float32), p[1, :10].astype(np.float32), np.float32)
    assert np.array_equal(u32, u) and np.array_equal(w32, w)
    # steep: slopes above 1 and up to 2, lanes with n.y == 0 exactly
    n = FX["steep.expected.contact_ground"][1:]
    slope = np.abs(n[:2]) / n[2]
    assert 1.0 < slope.max() <= 2.0 * (1 + 1e-12) and (n[1][:, 0::4] == 0.0).all() and (n[1] != 0.0).any()
    # zero_map: offsets, and the flat ground's outputs
    g = case("zero_map")[2]
    assert not g["heights"].any() and np.abs(g["offsets"]).min() > 0


# ------------------------------------------------------------------------------------------------------ the host side
@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    _, _, _, expected, _, n64, n32 = case(name)
    for out in gn.OUTPUTS:
        assert rel_error(n64[out], expected[out]) <= TOL, out
        assert rel_error(n32[out], expected[out]) <= 3e-6, out      # (some twenty roundings of 6e-8: the yardstick is sane)


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name):
    check_against_the_fixture(name, lambda plan, inputs, ground, dtype: emu.run(plan, inputs, ground, dtype), "emulation")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_emulated_null_map_and_zero_map_equal_the_flat_variant(dtype):
    """`locomotion_lane<T, true>` without a map (a null structure, a structure without heights) and on the zero map gives the
    bits of `locomotion_lane<T>`; `contact_ground` is then height 0 and normal e_z."""
    for name in ("zero_map", "tiles"):
        plan, inputs, ground = case(name)[:3]
        want = emu_flat.run(plan, inputs, dtype)
        null = emu.run(plan, inputs, None, dtype)
        assert sorted(null) == sorted(ln.OUTPUTS) and all(np.array_equal(null[k], want[k]) for k in want), name
        no_map = emu.run(plan, inputs, dict(offsets=ground["offsets"]), dtype)
        assert all(np.array_equal(no_map[k], want[k]) for k in want), name
        assert (no_map["contact_ground"][:3] == 0).all() and (no_map["contact_ground"][3] == 1).all()
    plan, inputs, ground = case("zero_map")[:3]
    want, zero = emu_flat.run(plan, inputs, dtype), emu.run(plan, inputs, ground, dtype)
    assert all(np.array_equal(zero[k], want[k]) for k in want)
    assert (zero["contact_ground"][:3] == 0).all() and (zero["contact_ground"][3] == 1).all()
    # on a map the ground variant differs from the flat one where it should and nowhere else
    plan, inputs, ground = case("tiles")[:3]
    want, got = emu_flat.run(plan, inputs, dtype), emu.run(plan, inputs, ground, dtype)
    for k in ln.OUTPUTS:
        if k == "foot_force_vertical":
            assert not np.array_equal(got[k], want[k])
        elif k == "scalars":
            assert np.array_equal(got[k][[0, 2, 3]], want[k][[0, 2, 3]]) and not np.array_equal(got[k][1], want[k][1])
        else:
            assert np.array_equal(got[k], want[k]), k


def _ground_struct(**change):
    H = np.zeros((3, 3))
    g = _abi.LocomotionGround()
    g.heights, g.nx, g.ny, g.x0, g.y0, g.dx, g.dy = H.ctypes.data, 3, 3, 0.0, 0.0, 1.0, 1.0
    for k, v in change.items():
        setattr(g, k, v)
    return g, H


REJECTIONS = [(dict(nx=1), "2 x 2"), (dict(ny=1), "2 x 2"), (dict(nx=0, ny=0), "2 x 2"), (dict(nx=-3), "2 x 2"),
              (dict(x0=np.nan), "origin"), (dict(x0=np.inf), "origin"), (dict(y0=-np.inf), "origin"), (dict(y0=np.nan), "origin"),
              (dict(dx=0.0), "spacings"), (dict(dx=-1.0), "spacings"), (dict(dx=np.nan), "spacings"), (dict(dx=np.inf), "spacings"),
              (dict(dy=0.0), "spacings"), (dict(dy=-0.5), "spacings"), (dict(dy=np.nan), "spacings"), (dict(dy=np.inf), "spacings")]


def test_entry_point_validates_the_ground_before_touching_the_device():
    """Every malformed ground description through the C ABI of a built library, on a machine without a device: JM_EINVAL and
    a message.  The plan handle is a stand-in that is never dereferenced: the checks come before the launch."""
    lib = _prebuilt(load_builtin("cartpole"))
    fn = lib.L.jm_block_locomotion_ground
    stand_in = C.create_string_buffer(64)
    plan = C.c_void_p(C.addressof(stand_in))
    pose = np.zeros((7, 1, 64))
    io = _abi.LocomotionIO()
    io.pose = pose.ctypes.data
    g, keep = _ground_struct()
    assert fn(None, _abi.JM_F64, 64, C.byref(io), C.byref(g), 0.0, 0.0, None) == _abi.JM_EINVAL and "null argument" in _last_error(lib)
    assert fn(plan, _abi.JM_F64, 64, None, C.byref(g), 0.0, 0.0, None) == _abi.JM_EINVAL and "null argument" in _last_error(lib)
    assert fn(plan, _abi.JM_F64, 0, C.byref(io), C.byref(g), 0.0, 0.0, None) == _abi.JM_EINVAL and "bad sizes" in _last_error(lib)
    assert fn(plan, 7, 64, C.byref(io), C.byref(g), 0.0, 0.0, None) == _abi.JM_EINVAL and "bad dtype" in _last_error(lib)
    for change, message in REJECTIONS:
        g, keep = _ground_struct(**change)
        rc = fn(plan, _abi.JM_F32, 64, C.byref(io), C.byref(g), 0.0, 0.0, None)
        assert rc == _abi.JM_EINVAL and "jm_block_locomotion_ground" in _last_error(lib) and message in _last_error(lib), (change, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    # a height map without `pose`: its queries have nothing to read
    g, keep = _ground_struct()
    rc = fn(plan, _abi.JM_F64, 64, C.byref(_abi.LocomotionIO()), C.byref(g), 0.0, 0.0, None)
    assert rc == _abi.JM_EINVAL and "pose" in _last_error(lib)
    # the emulation runs the same check
    plan_, inputs, ground = case("ramp")[:3]
    for bad in (dict(ground, dx=0.0), dict(ground, heights=np.zeros((1, 3))), dict(ground, y0=np.nan)):
        with pytest.raises(ValueError, match="jm_block_locomotion_ground"):
            emu.run(plan_, inputs, bad)


def test_abi_version_and_symbol():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    assert "int32_t jm_block_locomotion_ground(" in header and "jm_block_locomotion_ground" in _lib.ABI_SYMBOLS
    assert "int32_t jm_block_locomotion_ground(" in open(os.path.join(codegen.CSRC, "jm_lib_blocks.cpp")).read()
    # the order and the types of the members of jm_locomotion_ground in the header are those of the ctypes mirror
    body = header.split("typedef struct jm_locomotion_ground")[1].split("} jm_locomotion_ground;")[0]
    members = [line.strip(" ;").rsplit(" ", 1) for line in body.splitlines() if line.strip().endswith(";")]
    ctype = {"const void *": C.c_void_p, "void *": C.c_void_p, "int32_t": C.c_int32, "double": C.c_double}
    assert [(name, ctype[kind]) for kind, name in members] == list(_abi.LocomotionGround._fields_)
    # jm_locomotion_io did not change
    assert [f[0] for f in _abi.LocomotionIO._fields_] == list(_abi.LOCOMOTION_IO_FIELDS) and len(_abi.LOCOMOTION_IO_FIELDS) == 18
    # one definition of the ground for the physics kernels and the block
    kernels = open(os.path.join(codegen.CSRC, "jm_kernels.h")).read()
    assert '#include "jm_ground.h"' in kernels and "void ground_profile(" not in kernels
    assert os.path.normpath(os.path.join(codegen.CSRC, "jm_ground.h")) in [os.path.normpath(p) for p in codegen._sources()]
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11 and lib.L.jm_block_locomotion_ground is not None


class _RecordingLibrary:
    """Stands for the C library on a machine without a device: records the launches."""

    def __init__(self):
        self.calls = []

    def jm_locomotion_plan_create(self, desc, out):
        return 0

    def jm_locomotion_plan_destroy(self, plan):
        return 0

    def jm_block_locomotion(self, *args):
        self.calls.append(("flat", args))
        return 0

    def jm_block_locomotion_ground(self, plan, dtype, B, io, ground, momentum_cutoff, friction_cutoff, stream):
        g = ground._obj
        self.calls.append(("ground", {k: getattr(g, k) for k, _ in _abi.LocomotionGround._fields_}))
        return 0


def test_python_surface_on_a_stand_in_engine(monkeypatch):
    from types import SimpleNamespace

    import torch

    from jiminy_amd import blocks
    model = load_builtin("anymal")
    names = ["root_joint"] + list(model.contacts)
    rows = _abi.constraint_rows(model)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())

    def engine(ground=None):
        fields = dict(centroidal=torch.zeros(15, 4, dtype=torch.float64), q=torch.zeros(model.nq, 4, dtype=torch.float64),
                      con_flags=torch.zeros(rows["con_flags"], 4, dtype=torch.int32),
                      con_data=torch.zeros(rows["con_data"], 4, dtype=torch.float64))
        eng = SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _fields=fields,
                              _options={"contacts": {"model": "constraint"}}, _ground=ground, _ground_grid=(-1.0, -2.0, 0.5, 0.25),
                              _lib=SimpleNamespace(L=_RecordingLibrary(), check=lambda rc: None), _stream=lambda: None)
        eng.field = fields.__getitem__
        return eng

    def frames_of(eng, state=None):
        K = len(names)
        return SimpleNamespace(_eng=eng, frame_names=list(names), average=True, index=names.index, plan=SimpleNamespace(modes=[0] * K),
                               _state=state, average_velocity=torch.zeros(6, K, 4, dtype=torch.float64),
                               quat_no_yaw=torch.zeros(4, K, 4, dtype=torch.float64), pose=torch.zeros(7, K, 4, dtype=torch.float64))
    make = blocks.LocomotionQuantities
    # the old refusal without the option, now naming the option
    eng = engine(ground=torch.zeros(3, 5, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="flat ground.*ground_profile=True"):
        make(eng, frames_of(eng))
    # the reference evaluates the ground distance in TRUE mode only
    q = torch.zeros(model.nq, 4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="TRUE mode"):
        make(eng, frames_of(eng, state=(q, None)), state=(q, torch.zeros(15, 4, dtype=torch.float64)), forces=False, ground_profile=True)
    # with the option and a map the block builds, and every launch goes through the new entry point with the engine's map
    lq = make(eng, frames_of(eng), ground_profile=True)
    assert tuple(lq.contact_ground.shape) == (4, 4, 4) and lq.ground_profile
    assert lq.fieldnames["contact_ground"][0][0] == "LF_FOOT.GroundHeight" and lq.fieldnames["contact_ground"][3][3] == "RH_FOOT.NormalZ"
    assert [row[0].split(".")[1] for row in lq.fieldnames["contact_ground"]] == ["GroundHeight", "NormalX", "NormalY", "NormalZ"]
    lq.refresh()
    kind, g = eng._lib.L.calls[-1]
    assert kind == "ground" and g["heights"] == eng._ground.data_ptr() and (g["nx"], g["ny"]) == (5, 3)
    assert (g["x0"], g["y0"], g["dx"], g["dy"]) == (-1.0, -2.0, 0.5, 0.25) and g["offsets"] is None
    assert g["contact_ground"] == lq.contact_ground.data_ptr()
    # the map, the grid and the offsets are read at every launch: bound and changed after the block was built
    eng._fields["ground_offset"] = torch.zeros(2, 4, dtype=torch.float64)
    eng._ground, eng._ground_grid = torch.zeros(2, 2, dtype=torch.float64), (0.0, 0.0, 1.0, 1.0)
    lq.reset(torch.tensor([True, False, True, False]))
    kind, g = eng._lib.L.calls[-1]
    assert kind == "ground" and g["heights"] == eng._ground.data_ptr() and (g["nx"], g["ny"], g["dx"]) == (2, 2, 1.0)
    assert g["offsets"] == eng._fields["ground_offset"].data_ptr()
    eng._ground = None
    lq.refresh()
    kind, g = eng._lib.L.calls[-1]
    assert kind == "ground" and g["heights"] is None and g["offsets"] is None and g["contact_ground"] == lq.contact_ground.data_ptr()
    # without the option nothing changes: no tensor, no names, the old entry point
    eng = engine()
    lq = make(eng, frames_of(eng))
    assert lq.contact_ground is None and "contact_ground" not in lq.fieldnames and not lq.ground_profile
    lq.refresh()
    assert eng._lib.L.calls[-1][0] == "flat"
    assert "contact_ground" not in blocks.locomotion_fieldnames(model.contacts, ["LF_KFE"], True, True)


# ------------------------------------------------------------------------------------------------------------ device
class DeviceLocomotionGround(flat_tests.DeviceLocomotion):
    """A plan on the device and the launch of `jm_block_locomotion_ground` on numpy arrays (copied in and out)."""

    def run(self, inputs: dict, ground, dtype=np.float64, outputs=gn.OUTPUTS, mask=None, fill=np.nan):
        torch = self.torch
        B = inputs["centroidal"].shape[-1]
        tdtype = torch.from_numpy(np.zeros(1, dtype)).dtype
        io, held, out = _abi.LocomotionIO(), [], {}

        def pointer(a):
            held.append(torch.as_tensor(a, device=self.device))
            return held[-1].data_ptr()
        for name, a in inputs.items():
            setattr(io, name, pointer(np.ascontiguousarray(a, dtype=np.int32 if name == "con_flags" else dtype)))
        if mask is not None:
            io.lane_mask = pointer(np.ascontiguousarray(mask, dtype=np.uint8))
        g = emu.ground_struct(ground, dtype, held, pointer)
        for name in gn.OUTPUTS:
            out[name] = torch.full(gn.output_shape(name, self.plan, B), fill, dtype=tdtype, device=self.device)
            if name in outputs and name != "contact_ground":
                setattr(io, name, out[name].data_ptr())
        if g is not None and "contact_ground" in outputs:
            g.contact_ground = out["contact_ground"].data_ptr()
        self.lib.check(self.lib.L.jm_block_locomotion_ground(
            self.h, _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B, C.byref(io), None if g is None else C.byref(g),
            float(self.plan["momentum_cutoff"]), float(self.plan["friction_cutoff"]),
            C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        del held
        return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, gpu_device):
    """Every fixture case through the C ABI at B = 64, both dtypes."""
    dev = DeviceLocomotionGround(_prebuilt(load_builtin("cartpole")), case(name)[0], gpu_device)
    try:
        check_against_the_fixture(name, lambda plan, inputs, ground, dtype: dev.run(inputs, ground, dtype), "device")
    finally:
        dev.close()


def _tiled(inputs: dict, ground: dict, lanes: np.ndarray):
    tiled = {k: np.ascontiguousarray(v[..., lanes]) for k, v in inputs.items()}
    return tiled, dict(ground, offsets=np.ascontiguousarray(ground["offsets"][:, lanes]))


@pytest.mark.gpu
def test_device_second_block_and_lane_mask_against_the_emulation(gpu_device):
    """`tiles` tiled to B = 300 (a second block of 256 threads, partly filled) with a lane mask: the masked lanes within the
    bars of the emulation on the same arrays, the other lanes untouched, in both dtypes."""
    plan, inputs, ground = case("tiles")[:3]
    dev = DeviceLocomotionGround(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        lanes = (np.arange(300) * 7 + 3) % 64
        tiled, tiled_ground = _tiled(inputs, ground, lanes)
        mask = np.arange(300) % 3 != 1
        assert mask[256:].any() and (~mask[256:]).any()
        for dtype in (np.float64, np.float32):
            want = emu.run(plan, tiled, tiled_ground, dtype)
            got = dev.run(tiled, tiled_ground, dtype, mask=mask, fill=7.25)
            n32 = gn.quantities(plan, tiled, tiled_ground, np.float32)
            n64 = gn.quantities(plan, tiled, tiled_ground, np.float64)
            for k in gn.OUTPUTS:
                assert (got[k][..., ~mask] == 7.25).all(), k
                e = rel_error(got[k][..., mask], want[k][..., mask])
                bound = TOL if dtype is np.float64 else 4.0 * rel_error(n32[k], n64[k])
                print(f"B = 300, device against the emulation, {np.dtype(dtype).name} {k}: {e:.2e} (bound {bound:.2e})")
                assert e <= bound, (k, dtype, e)
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_is_independent_of_the_batch_mates(gpu_device):
    """`steep` tiled to B = 193, the lanes rotated by 29: lane b of the tiled batch gives the bits lane (b + 29) % 64 gives at
    B = 64, in both dtypes."""
    plan, inputs, ground = case("steep")[:3]
    dev = DeviceLocomotionGround(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        lanes = (np.arange(193) + 29) % 64
        tiled, tiled_ground = _tiled(inputs, ground, lanes)
        for dtype in (np.float64, np.float32):
            small, big = dev.run(inputs, ground, dtype), dev.run(tiled, tiled_ground, dtype)
            for out in gn.OUTPUTS:
                assert big[out].shape[-1] == 193 and np.array_equal(big[out], small[out][..., lanes]), (out, dtype)
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_null_offsets_null_contact_ground_and_null_ground(gpu_device):
    """Without offsets the queries are made at the contact positions; an output that is not asked for keeps its poison and the
    others do not change; a null structure and a structure without heights give the bits of `jm_block_locomotion` (its kernel
    is launched).  On the zero map the kernel of the ground variant runs: what looks at the ground -- 0 lambda_x + 0 lambda_y +
    1 lambda_z and (z - 0) * 1, exact in any arithmetic -- has the flat kernel's bits, every other output is within the bars
    of the file (another instantiation may contract other products into fused multiply-adds)."""
    plan, inputs, ground = case("tiles")[:3]
    lib = _prebuilt(load_builtin("cartpole"))
    dev, dev_flat = DeviceLocomotionGround(lib, plan, gpu_device), flat_tests.DeviceLocomotion(lib, plan, gpu_device)
    try:
        full = dev.run(inputs, ground)
        no_off = {k: v for k, v in ground.items() if k != "offsets"}
        got, want = dev.run(inputs, no_off), gn.quantities(plan, inputs, no_off)
        assert all(rel_error(got[k], want[k]) <= TOL for k in gn.OUTPUTS)
        assert not np.array_equal(got["contact_ground"], full["contact_ground"])
        for asked in (ln.OUTPUTS, ("contact_ground",), ("scalars", "foot_force_vertical"), ()):
            got = dev.run(inputs, ground, outputs=asked, fill=7.25)
            for k, v in got.items():
                assert np.array_equal(v, full[k]) if k in asked else (v == 7.25).all(), (asked, k)
        zero_plan, zero_inputs, zero_ground = case("zero_map")[:3]
        for dtype in (np.float64, np.float32):
            flat = dev_flat.run(inputs, dtype)
            for g in (None, dict(offsets=ground["offsets"])):
                got = dev.run(inputs, g, dtype, fill=7.25)
                differ = [k for k in ln.OUTPUTS if not np.array_equal(got[k], flat[k])]
                assert not differ, (g is None, dtype, differ)
                c = got["contact_ground"]
                assert (c == 7.25).all() if g is None else ((c[:3] == 0).all() and (c[3] == 1).all())
        dev0, flat0 = DeviceLocomotionGround(lib, zero_plan, gpu_device), flat_tests.DeviceLocomotion(lib, zero_plan, gpu_device)
        try:
            for dtype in (np.float64, np.float32):
                got, flat = dev0.run(zero_inputs, zero_ground, dtype), flat0.run(zero_inputs, dtype)
                n64, n32 = case("zero_map")[5:7]
                for k in ln.OUTPUTS:
                    e = rel_error(got[k], flat[k])
                    bound = TOL if dtype is np.float64 else 4.0 * rel_error(n32[k], n64[k])
                    print(f"zero map against the flat kernel, {np.dtype(dtype).name} {k}: {e:.2e} (bound {bound:.2e})")
                    assert e <= bound, (k, dtype, e)
                assert np.array_equal(got["foot_force_vertical"], flat["foot_force_vertical"]), dtype
                assert np.array_equal(got["scalars"][1], flat["scalars"][1]), dtype
                assert (got["contact_ground"][:3] == 0).all() and (got["contact_ground"][3] == 1).all()
        finally:
            dev0.close()
            flat0.close()
    finally:
        dev.close()
        dev_flat.close()


SLOPE = 0.2


def _slope(x, y):
    return SLOPE * x


def _block_ground(env) -> dict:
    eng = env.engine
    x0, y0, dx, dy = eng._ground_grid
    return dict(heights=eng._ground.cpu().numpy(), x0=x0, y0=y0, dx=dx, dy=dy, offsets=eng.field("ground_offset").cpu().numpy())


@pytest.mark.gpu
def test_newtons_law_on_a_slope(gpu_device):
    """ANYmal, 64 lanes, constraint contacts, 25 steps under zero action on a plane of slope 0.2 that covers every lane's patch,
    the block built with `ground_profile=True`.  The feet carry the weight and what accelerates the centre of mass:
    sum(foot_force_vertical) - 1 = dhg_linear_z / weight, the right-hand side from the `centroidal` rows, which know nothing of
    the block's normals.  Bound: 4 x the error of the host composition (the numpy restatement on the tensors the block read)
    against the same law, plus 4 x 2.2e-16.  The flat formula misses the law by about 1 - cos(atan 0.2) plus the tangential
    share, about 2e-2.  Measured on the device: 7.49e-16, the host composition 7.49e-16 (bound 3.9e-15); the flat formula 9.7e-2
    (the lanes still rock on the slope: |dhg_linear_z| / weight is up to 0.374, and the tangential share grows with it)."""
    import torch
    env, _ = flat_tests._settled_anymal(gpu_device, locomotion_quantities=dict(ground_profile=True, momentum_cutoff=1.0, friction_cutoff=0.5),
                                        ground_profile=(_slope, (-6.0, 6.0), (-6.0, 6.0), 0.125), ground_patch_extent=(2.0, 2.0))
    lq, eng, model = env.locomotion, env.engine, env.model
    torch.cuda.synchronize(gpu_device)
    inputs, plan, ground = flat_tests._block_inputs(env), flat_tests._block_plan(env), _block_ground(env)
    assert ground["heights"].shape == (97, 97) and np.abs(ground["offsets"]).max() <= 2.0 and np.abs(ground["offsets"]).min() > 0
    host = gn.quantities(plan, inputs, ground)
    dev = {k: getattr(lq, k).cpu().numpy() for k in gn.OUTPUTS}
    for k in gn.OUTPUTS:
        print(f"ANYmal on the slope, device against the host composition, {k}: {rel_error(dev[k], host[k]):.2e}")
        assert rel_error(dev[k], host[k]) <= TOL, k
    # every contact point is on the plane's patch of its lane and on the ground
    n = dev["contact_ground"][1:]
    want_n = np.array([-SLOPE, 0.0, 1.0]) / np.sqrt(1.0 + SLOPE ** 2)
    assert np.abs(n - want_n[:, None, None]).max() <= 1e-12
    on = (inputs["con_flags"] & 1) == 1
    print(f"contacts enabled per lane {on.sum(0).min()} to {on.sum(0).max()}, distance to the ground {dev['scalars'][1].min():.2e} to "
          f"{dev['scalars'][1].max():.2e} m, sum of the vertical foot forces {dev['foot_force_vertical'].sum(0).min():.3f} to "
          f"{dev['foot_force_vertical'].sum(0).max():.3f}")
    # (the robots are put down from the highest ground under their footprint: after 1 s some still rock on the slope; the law
    # holds with the acceleration on its right-hand side, and is not vacuous where a foot is on the ground)
    assert on.any(0).all() and np.abs(dev["scalars"][1]).max() < 5e-3
    weight = float(np.sum(model.mass[1:])) * 9.81
    want = inputs["centroidal"][11] / weight
    e_dev = rel_error(dev["foot_force_vertical"].sum(0) - 1.0, want)
    e_host = rel_error(host["foot_force_vertical"].sum(0) - 1.0, want)
    flat = ln.quantities(plan, inputs)
    e_flat = rel_error(flat["foot_force_vertical"].sum(0) - 1.0, want)
    print(f"law sum(foot_force_vertical) - 1 = dhg_linear_z / weight: device {e_dev:.2e}, host composition {e_host:.2e}, "
          f"the flat formula {e_flat:.2e}; |dhg_linear_z| / weight {np.abs(want).max():.2e}")
    assert e_dev <= 4.0 * e_host + 4.0 * EPS, (e_dev, e_host)
    assert e_flat > 1e-2
    env.close()


RAISED = 0.5


def _raised_ramp(x, y):
    return RAISED + 0.04 * x


@pytest.mark.gpu
def test_flying_termination_on_raised_ground_and_partial_reset(gpu_device, monkeypatch):
    """A `WalkerVecEnv` on a ramp (slope 0.04) about 0.5 m high under the robots, `flying=(0.3, 0)`: no lane terminates while
    standing on it (the flat formula sees every contact 0.5 m high); lanes b % 4 == 1, lifted by 0.5 m, terminate.  A robot is
    put down at the highest ground within 1.125 m of its centre, at most 0.045 m + 0.016 m above the ground under its feet.  Then `reset(lane_mask)`
    of the block keeps the unmasked lanes bit for bit, and `reset_lanes` evaluates the reset lanes on their new patches."""
    import torch

    from jiminy_amd.envs import VecJiminyEnv, make_anymal_env
    B = 64
    lane = torch.arange(B, device=gpu_device)
    high = lane % 4 == 1
    sample = VecJiminyEnv._sample_state

    def lifted(self, n):
        q, v = sample(self, n)
        q = q.clone()
        q[2] += torch.where(high, 0.5, 0.0).to(q.dtype)
        return q, v
    monkeypatch.setattr(VecJiminyEnv, "_sample_state", lifted)
    env = make_anymal_env(B, device=gpu_device, contact_model="constraint", auto_reset=False,
                          locomotion_quantities=dict(ground_profile=True, momentum_cutoff=1.0, friction_cutoff=0.5),
                          terminations=dict(flying=(0.3, 0.0)), ground_profile=(_raised_ramp, (-4.0, 4.0), (-4.0, 4.0), 0.25),
                          ground_patch_extent=(1.0, 1.0))
    env.reset(seed=5)
    lq = env.locomotion
    ground_under = lq.contact_ground[0]
    assert float(ground_under.min()) > 0.3 and float(ground_under.max()) < 0.7
    action = torch.zeros(B, env.model.nmotors, dtype=torch.float64, device=gpu_device)
    for i in range(2):
        out = env.step(action)
        d = lq.ground_distance_min
        print(f"step {i}: distance to the ground, standing {float(d[~high].min()):.3f} to {float(d[~high].max()):.3f} m, lifted "
              f"{float(d[high].min()):.3f} to {float(d[high].max()):.3f} m; ground under the contacts {float(lq.contact_ground[0].min()):.3f} to "
              f"{float(lq.contact_ground[0].max()):.3f} m")
        assert torch.equal(out[2], high), i
        assert float(d[~high].max()) < 0.1 and float(d[high].min()) > 0.3
    # the block's own partial reset: the unmasked lanes keep every bit
    tensors = {k: getattr(lq, k) for k in gn.OUTPUTS}
    full = {k: t.clone() for k, t in tensors.items()}
    bits = lambda t: t.view(torch.int64)      # noqa: E731  (bit for bit: the ZMP of a lifted lane, in free fall, is NaN)
    for t in tensors.values():
        t.fill_(7.25)
    mask = lane % 3 == 0
    lq.reset(mask)
    for k, t in tensors.items():
        assert t is getattr(lq, k)
        assert torch.equal(t[..., ~mask], torch.full_like(t[..., ~mask], 7.25)), k
        assert torch.equal(bits(t)[..., mask], bits(full[k])[..., mask]), k
    lq.refresh()
    assert all(torch.equal(bits(t), bits(full[k])) for k, t in tensors.items())
    # the environment's partial reset: new patches for the reset lanes, which are evaluated on them
    offsets = env.engine.field("ground_offset").clone()
    env.reset_lanes(mask)
    new = env.engine.field("ground_offset")
    assert torch.equal(new[:, ~mask], offsets[:, ~mask]) and not torch.equal(new[:, mask], offsets[:, mask])
    for k, t in tensors.items():
        assert torch.equal(bits(t)[..., ~mask], bits(full[k])[..., ~mask]), k
    assert not torch.equal(lq.contact_ground[0][:, mask], full["contact_ground"][0][:, mask])
    torch.cuda.synchronize(gpu_device)
    host = gn.quantities(flat_tests._block_plan(env), flat_tests._block_inputs(env), _block_ground(env))
    m = mask.cpu().numpy()
    for k in ("contact_ground", "scalars", "foot_force_vertical"):
        rows = [1] if k == "scalars" else slice(None)
        assert rel_error(getattr(lq, k).cpu().numpy()[rows][..., m], host[k][rows][..., m]) <= TOL, k
    env.close()
