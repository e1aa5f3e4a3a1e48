"""Projected support polygon on the device (csrc/jm_support.h behind `jm_block_support_polygon`, `blocks.SupportPolygon`, the
`support_polygon` keyword and the `robustness` reward term of `WalkerVecEnv`).

Specification: the reference's own output, tests/golden/ref_support.npz (tools/make_ref_support_fixtures.py executes the
reference's hull, distance and sigmoid functions; eight cases of 64 lanes).  Comparison rule, on every lane of every case:
`n_vertices` and `vertex_index` equal the fixture exactly in float64, and in float32 equal the numpy restatement
(tests/support_numpy.py) run in float32 on the same float32 inputs; vertices, center, margin and reward within 1e-13 relative
to max(|want|, 1) in float64, and in float32 within 4 x the error of the float32 numpy restatement on the same case and
output; `-inf` margins and the NaN padding of `vertices` must be exactly that.  An output the case has no expectation for
(`polygon_only`: the scalars) must stay unwritten.

Measured on the host (error relative to max(|want|, 1), largest over the eight cases and the lanes):
  float64, host emulation | numpy restatement:  vertices 1.1e-16 | 0   center 8.3e-17 | 0   scalars 2.8e-16 | 1.1e-16
  float32, host emulation | numpy restatement:  vertices 1.6e-7 | 1.6e-7   center 1.4e-7 | 1.4e-7   scalars 7.2e-7 | 7.2e-7
  (the host build rounds every product on its own, as numpy does; the device build contracts the sums of two products)

Measured on the device (MI355X; the same eight cases through the C ABI, largest over the cases and the lanes):
  float64  vertices 1.1e-16   center 8.3e-17   scalars 1.3e-15; every index equal
  float32  vertices 1.9e-7   center 1.4e-7   scalars 9.1e-7; largest ratio error / bound of one case and output: 0.38 (scalars,
           `three_points`: 9.08e-7 against 4 x 6.0e-7); every index equal to the float32 restatement's
  standing ANYmal (64 lanes, each at its own place and yaw, 5 steps of the PD controller): device against the host composition on
  the same tensors at most 3.3e-16 (LOCAL_WORLD_ALIGNED) and 1.1e-16 (LOCAL); margin of the standing lanes 0.3009 .. 0.3012 m in
  both frames, LOCAL against LOCAL_WORLD_ALIGNED 2.2e-16; the lanes in free fall -inf and a reward of 0.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, codegen, load_builtin, support
from tests import support_numpy as sp
from tests.hostemu import support as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_support.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_support_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
TOL = 1e-13
NEW_SYMBOLS = ("jm_support_plan_create", "jm_support_plan_destroy", "jm_block_support_polygon")
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["cases"]]
FLOAT_OUTPUTS = ("vertices", "center", "scalars")
_CASES: dict = {}


def case(name: str):
    """plan, inputs, expected and the two numpy restatements of a case, computed once."""
    if name not in _CASES:
        plan, inputs, expected = sp.load_case(FX, name)
        _CASES[name] = (plan, inputs, expected, sp.quantities(plan, inputs, np.float64), sp.quantities(plan, inputs, np.float32))
    return _CASES[name]


def rel_error(got: np.ndarray, want: np.ndarray) -> float:
    """Largest error relative to max(|want|, 1).  Where `want` is NaN or infinite, `got` must be exactly that."""
    assert got.shape == want.shape, (got.shape, want.shape)
    got = got.astype(np.float64)
    special = ~np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN where a number is expected, or the reverse"
    assert np.array_equal(got[special & ~np.isnan(want)], want[special & ~np.isnan(want)]), "an infinite value differs"
    if not (~special).any():
        return 0.0
    with np.errstate(invalid="ignore"):
        return float((np.abs(got - want) / np.maximum(np.abs(want), 1.0))[~special].max())


def check_against_the_fixture(name: str, run, label: str) -> None:
    """`run(plan, inputs, dtype) -> outputs` (unwritten float entries 7.25, integer ones 7) against the fixture in both dtypes."""
    plan, inputs, expected, _, n32 = case(name)
    for dtype in (np.float64, np.float32):
        got = run(plan, inputs, dtype)
        index_want = expected if dtype is np.float64 else n32
        for out in sp.INT_OUTPUTS:
            assert got[out].dtype == np.int32 and np.array_equal(got[out], index_want[out]), (name, out, dtype)
        for out in FLOAT_OUTPUTS:
            if out not in expected:
                assert (got[out] == 7.25).all(), (name, out)           # no ZMP: not written
                continue
            e = rel_error(got[out], expected[out])
            if dtype is np.float64:
                print(f"{label} {name} float64 {out}: {e:.2e}")
                assert e <= TOL, (name, out, e)
            else:
                e_np = rel_error(n32[out], expected[out])
                print(f"{label} {name} float32 {out}: {e:.2e} (numpy float32 {e_np:.2e}, bound {4.0 * e_np:.2e})")
                assert e <= 4.0 * e_np, (name, out, e, e_np)


# ------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_from_the_reference_tree():
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        pytest.skip("the reference tree is not here: the committed fixture stands")
    subprocess.check_call([sys.executable, TOOL, "--check"], stdout=subprocess.DEVNULL)


def _is_short_binary(a: np.ndarray) -> bool:
    return bool(np.array_equal(a * 1024.0, np.round(a * 1024.0)))


def test_fixture_holds_the_designed_cases():
    assert CASES == ["quadruped_lwa", "quadruped_local", "biped_boxes", "three_points", "two_points", "one_point", "exact_ties",
                     "polygon_only"]
    assert os.path.getsize(FIXTURE) <= 1 << 20
    n_points = dict(quadruped_lwa=4, quadruped_local=4, biped_boxes=16, three_points=3, two_points=2, one_point=1, exact_ties=8,
                    polygon_only=7)
    local = {"quadruped_local", "one_point", "polygon_only"}
    for name in CASES:
        plan, inputs, expected, _, _ = case(name)
        cols = [int(c) for c in plan["point_column"]]
        n, K = len(cols), int(plan["n_frames"])
        assert n == n_points[name] and K > n and inputs["pose"].shape == (7, K, 64) and inputs["odom_pose"].shape == (3, 64)
        assert len(set(cols)) == n and min(cols) >= 0 and max(cols) < K
        assert (int(plan["reference_frame"]) == sp.LOCAL) == (name in local)
        assert ("zmp" in inputs) == (name != "polygon_only") == ("scalars" in expected)
        nv, idx, vert = expected["n_vertices"], expected["vertex_index"], expected["vertices"]
        assert nv.shape == (64,) and idx.shape == (16, 64) and vert.shape == (2, 16, 64) and expected["center"].shape == (2, 64)
        assert nv.min() >= 1 and nv.max() <= n
        for b in range(64):
            assert (idx[:nv[b], b] >= 0).all() and (idx[:nv[b], b] < n).all() and (idx[nv[b]:, b] == -1).all()
            assert np.isfinite(vert[:, :nv[b], b]).all() and np.isnan(vert[:, nv[b]:, b]).all()
            if n <= 3:
                pts = inputs["pose"][:2, cols, b]
                assert nv[b] == n and len({tuple(p) for p in pts.T}) == n            # no two points coincide
        if name == "polygon_only":
            continue
        margin, reward = expected["scalars"]
        nan = np.isnan(inputs["zmp"][0])
        assert np.array_equal(margin == -np.inf, nan) and np.array_equal(reward == 0.0, nan) and np.isfinite(margin[~nan]).all()
        assert ((reward >= 0.0) & (reward <= 1.0)).all()
        ci, co = float(plan["cutoff_inner"]), float(plan["cutoff_outer"])
        assert ci > 0 and co > 0 and (np.abs(np.where(margin > 0, margin / ci, margin / co))[~nan] <= 4.0).all()
        if name != "exact_ties":
            assert (np.abs(margin[~nan]) >= (1e-3 if name in local else 1e-6)).all()
        if name.startswith("quadruped"):
            assert list(np.flatnonzero(nan)) == list(range(7, 64, 8)) and (margin[~nan] > 0).any() and (margin[~nan] < 0).any()
        else:
            assert not nan.any()
    # the flat lanes of the biped: short binary fractions, every projected point there twice, bit for bit
    plan, inputs, expected, _, _ = case("biped_boxes")
    pts = inputs["pose"][:2, [int(c) for c in plan["point_column"]]]
    for b in range(64):
        distinct = len({tuple(p) for p in pts[:, :, b].T})
        assert (distinct == 8 and _is_short_binary(pts[:, :, b])) if b % 4 == 0 else distinct == 16
    assert expected["n_vertices"].max() > 4
    # three points: the sorted order is kept, so both orientations occur
    plan, inputs, expected, _, _ = case("three_points")
    v = expected["vertices"][:, :3]
    area = (v[0, 1] - v[0, 0]) * (v[1, 2] - v[1, 0]) - (v[1, 1] - v[1, 0]) * (v[0, 2] - v[0, 0])
    assert (area > 0).any() and (area < 0).any()
    # two points, one point: unsigned distances
    assert (case("two_points")[2]["scalars"][0] < 0).all() and (case("one_point")[2]["scalars"][0] < 0).all()
    # exact ties: binary fractions, one duplicate pair, a collinear run and an interior point (8 points, 4 vertices); queries
    # exactly on an edge or a vertex (margin -0.0 or 0.0) on lanes 0, 1 mod 3 and strictly inside on lanes 2 mod 3
    plan, inputs, expected, _, _ = case("exact_ties")
    pts = inputs["pose"][:2, [int(c) for c in plan["point_column"]]]
    assert _is_short_binary(pts) and _is_short_binary(inputs["zmp"]) and (expected["n_vertices"] == 4).all()
    assert all(len({tuple(p) for p in pts[:, :, b].T}) == 7 for b in range(64))
    margin = expected["scalars"][0]
    lane = np.arange(64)
    assert (margin[lane % 3 != 2] == 0.0).all() and (margin[lane % 3 == 2] > 0.0).all()
    assert (expected["scalars"][1][lane % 3 != 2] == 0.5).all()


# ------------------------------------------------------------------------------------------------------ the host side
@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    plan, inputs, expected, n64, n32 = case(name)
    assert sorted(n64) == sorted(expected)
    for out in sp.INT_OUTPUTS:
        assert np.array_equal(n64[out], expected[out]), out
    for out in FLOAT_OUTPUTS:
        if out in expected:
            assert rel_error(n64[out], expected[out]) <= TOL, out
            assert rel_error(n32[out], expected[out]) <= 2e-6, out      # (a dozen roundings of 6e-8: the yardstick is sane)


def _emu_run(plan, inputs, dtype=np.float64, outputs=sp.OUTPUTS, fill=7.25, **kw):
    got = emu.run(plan, inputs, dtype, outputs=outputs, fill=fill, **kw)
    return {k: got[k] if k in got else emu.new_output(k, plan, inputs["pose"].shape[-1], np.dtype(dtype), fill) for k in sp.OUTPUTS}


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name):
    check_against_the_fixture(name, _emu_run, "emulation")


def _untouched(name: str, a: np.ndarray) -> bool:
    return bool((a == (7 if name in sp.INT_OUTPUTS else 7.25)).all())


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_null_outputs_lane_mask_and_cutoffs(run) -> None:
    """`run(plan, inputs, outputs=, mask=, fill=, cutoff_inner=, cutoff_outer=) -> every output` (those not asked for keep
    `fill`: 7.25, the integer ones 7), on `quadruped_local` and `biped_boxes`."""
    for name in ("quadruped_local", "biped_boxes"):
        plan, inputs, _, _, _ = case(name)
        full = run(plan, inputs, fill=7.25)
        assert not any(_untouched(k, v) for k, v in full.items())
        # an output that is not asked for is not written; the others do not change
        for asked in (("n_vertices",), ("vertex_index", "scalars"), ("vertices",), ("center", "scalars"), ("scalars",), ()):
            got = run(plan, inputs, outputs=asked, fill=7.25)
            for k, v in got.items():
                assert _same_bits(v, full[k]) if k in asked else _untouched(k, v), (asked, k)
        # without a ZMP the scalars are not written
        got = run(plan, {k: v for k, v in inputs.items() if k != "zmp"}, fill=7.25)
        assert _untouched("scalars", got["scalars"]) and all(_same_bits(got[k], full[k]) for k in sp.OUTPUTS if k != "scalars")
        # a cutoff of zero: the reward row is not written, the margin is
        for zero in (dict(cutoff_inner=0.0), dict(cutoff_outer=0.0), dict(cutoff_inner=0.0, cutoff_outer=0.0)):
            got = run(plan, inputs, fill=7.25, **zero)
            assert (got["scalars"][1] == 7.25).all() and _same_bits(got["scalars"][0], full["scalars"][0]), zero
        # masked lanes only, the others bit for bit
        mask = np.arange(64) % 3 == 0
        got = run(plan, inputs, mask=mask, fill=7.25)
        for k, v in got.items():
            assert _same_bits(v[..., mask], full[k][..., mask]) and _untouched(k, v[..., ~mask]), k
    # LOCAL without the odometry pose: nothing is written
    plan, inputs, _, _, _ = case("quadruped_local")
    got = run(plan, {k: v for k, v in inputs.items() if k != "odom_pose"}, fill=7.25)
    assert all(_untouched(k, v) for k, v in got.items())


def test_emulated_null_pointers_lane_mask_and_cutoffs():
    check_null_outputs_lane_mask_and_cutoffs(lambda plan, inputs, **kw: _emu_run(plan, inputs, **kw))
    with pytest.raises(ValueError, match="cutoff thresholds must both be positive"):
        _emu_run(*case("quadruped_lwa")[:2], cutoff_inner=-0.1)
    with pytest.raises(ValueError, match="cutoff thresholds must both be positive"):
        _emu_run(*case("quadruped_lwa")[:2], cutoff_outer=float("nan"))


def poisoned(name: str):
    """The inputs of a case with NaN and infinite values in `pose` / `odom_pose` of the lanes 1 mod 4, and those lanes."""
    plan, inputs, _, _, _ = case(name)
    cols = [int(c) for c in plan["point_column"]]
    bad = np.arange(64) % 4 == 1
    inputs = {k: v.copy() for k, v in inputs.items()}
    values = (np.nan, np.inf, -np.inf)
    for b in np.flatnonzero(bad):
        kind = (b // 4) % 5
        if kind == 0:       # every coordinate
            inputs["pose"][:2, :, b] = np.nan
        elif kind == 1:     # one point
            inputs["pose"][b % 2, cols[b % len(cols)], b] = values[b % 3]
        elif kind == 2:     # every second point, mixed
            for i, c in enumerate(cols[::2]):
                inputs["pose"][:2, c, b] = values[(b + i) % 3]
        elif kind == 3:     # the odometry pose (read in LOCAL only)
            inputs["odom_pose"][b % 3, b] = values[b % 3]
            inputs["pose"][0, cols[0], b] = np.inf
        else:               # infinite coordinates of both signs
            inputs["pose"][0, cols, b] = np.where(np.arange(len(cols)) % 2 == 0, np.inf, -np.inf)
    return plan, inputs, bad


def check_failed_lanes(name: str, run) -> None:
    """Lanes with NaN / infinite `pose` or `odom_pose` terminate, keep their indices in range and leave the other lanes' bits."""
    plan, clean = case(name)[:2]
    n = len(plan["point_column"])
    _, inputs, bad = poisoned(name)
    for dtype in (np.float64, np.float32):
        want, got = run(plan, clean, dtype), run(plan, inputs, dtype)
        for k in sp.OUTPUTS:
            assert _same_bits(np.ascontiguousarray(got[k][..., ~bad]), np.ascontiguousarray(want[k][..., ~bad])), (name, k)
        nv, idx = got["n_vertices"][bad], got["vertex_index"][:, bad]
        assert nv.min() >= 0 and nv.max() <= 16 and idx.min() >= -1 and idx.max() < n, (name, nv.min(), nv.max(), idx.min(), idx.max())
        for j in range(nv.size):
            assert (idx[:nv[j], j] >= 0).all() and (idx[nv[j]:, j] == -1).all()


@pytest.mark.parametrize("name", ["quadruped_local", "biped_boxes", "three_points", "exact_ties", "polygon_only"])
def test_emulated_failed_lanes_terminate_and_stay_in_range(name):
    check_failed_lanes(name, _emu_run)


def _good() -> dict:
    plan = case("biped_boxes")[0]
    return {k: np.array(plan[k]) for k in emu.DESC_KEYS}


def _set_at(index, value):
    def f(a):
        a = a.copy()
        a.reshape(-1)[index] = value
        return a
    return f


def _rejections() -> list:
    """(changes of the description, what the message must say) for every rejection of `jm_support_plan_create`."""
    value = lambda v: (lambda a: v)      # noqa: E731
    return [
        (dict(point_column=lambda a: np.zeros(0, int)), "bad sizes"),
        (dict(point_column=lambda a: np.arange(17), n_frames=value(100)), "bad sizes"),
        (dict(n_frames=value(0)), "bad sizes"),
        (dict(n_frames=value(15)), "bad sizes"),
        (dict(point_column=_set_at(0, -1)), "point_column"),
        (dict(point_column=_set_at(3, 18)), "out of range"),
        (dict(point_column=lambda a: np.concatenate([a[:15], a[:1]])), "repeats the column"),
        (dict(reference_frame=value(2)), "Reference frame must be either"),
        (dict(reference_frame=value(-1)), "Reference frame must be either"),
    ]


def _broken(change: dict):
    arrays = _good()
    for k, f in change.items():
        arrays[k] = f(arrays[k])
    return support.make_desc(**arrays)


def test_plan_validation_rejects_every_malformed_description():
    desc, keep = support.make_desc(**_good())
    emu.pack(desc)
    d, keep_ = support.make_desc(point_column=np.arange(16), n_frames=16, reference_frame=0)       # (the cap itself is accepted)
    emu.pack(d)
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    d, keep_ = support.make_desc(**_good())
    d.point_column = None
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
    assert lib.L.jm_support_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = support.make_desc(**_good())
    assert lib.L.jm_support_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.point_column = None
    assert lib.L.jm_support_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)
    for change, message in _rejections():
        d, keep_ = _broken(change)
        rc = lib.L.jm_support_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and message in _last_error(lib), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    io = _abi.SupportIO()
    assert lib.L.jm_block_support_polygon(None, _abi.JM_F64, 64, C.byref(io), 0.1, 0.1, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    assert "typedef struct jm_support_desc" in header and "typedef struct jm_support_io" in header
    assert [f[0] for f in _abi.SupportDesc._fields_] == ["n_frames", "n_points", "reference_frame", "point_column"]
    # the order of the pointers of jm_support_io in the header is the order of the ctypes mirror
    body = header.split("typedef struct jm_support_io")[1].split("} jm_support_io;")[0]
    order = [line.split("*")[1].strip(" ;") for line in body.splitlines() if "*" in line]
    assert order == list(_abi.SUPPORT_IO_FIELDS)
    assert "jm_support.h" in open(os.path.join(ROOT, "jiminy_amd", "codegen.py")).read()
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


def test_builtin_atlas_is_over_the_bound():
    """The built-in Atlas carries two collision boxes per foot, 32 contact points: over the kernel's 16, so it is refused by
    name of the bound (the reference's pruning by the 3D hull of each foot would leave 24)."""
    model = load_builtin("atlas")
    assert len(model.contacts) == 32
    with pytest.raises(NotImplementedError, match="at most 16 contact points are supported, got 32"):
        support.build_plan(model, ["root_joint"] + list(model.contacts))


@pytest.mark.parametrize("name, n_points", [("anymal", 4), ("sixteen", 16)])
def test_host_plan_of_the_builtin_walkers(name, n_points):
    # (`sixteen`: a model at the bound itself; the plan reads the free-flyer flag and the contact names only)
    model = load_builtin(name) if name != "sixteen" else SimpleNamespace(has_freeflyer=True, contacts=[f"foot_{i}" for i in range(16)])
    names = ["root_joint"] + list(model.contacts)[::-1]
    plan = support.build_plan(model, names)
    assert plan.n_points == n_points == len(model.contacts) and plan.contact_names == list(model.contacts)
    assert plan.n_frames == n_points + 1 and plan.reference_frame == sp.LOCAL
    assert list(plan.arrays["point_column"]) == list(range(n_points, 0, -1))        # the model's contact order, wherever the columns are
    emu.pack(plan.desc()[0])
    assert support.build_plan(model, names, "LOCAL_WORLD_ALIGNED").reference_frame == sp.LOCAL_WORLD_ALIGNED
    assert support.build_plan(model, names, 1).reference_frame == sp.LOCAL_WORLD_ALIGNED
    with pytest.raises(ValueError, match="Reference frame must be either"):
        support.build_plan(model, names, "ODOMETRY")
    with pytest.raises(ValueError, match="lacks the contact frames"):
        support.build_plan(model, names[:-1])


def test_python_surface_refusals_on_the_host(monkeypatch):
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.envs import VecJiminyEnv, WalkerVecEnv
    model = load_builtin("anymal")
    with pytest.raises(RuntimeError, match="floating base"):
        support.build_plan(load_builtin("arm7"), [])
    no_contacts = SimpleNamespace(has_freeflyer=True, contacts=[])
    with pytest.raises(RuntimeError, match="at least one contact"):
        support.build_plan(no_contacts, [])
    many = SimpleNamespace(has_freeflyer=True, contacts=[f"c{i}" for i in range(17)])
    with pytest.raises(NotImplementedError, match="at most 16 contact points"):
        support.build_plan(many, many.contacts)

    def engine(model=model):
        return SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _fields={},
                               _lib=SimpleNamespace(L=None, check=None))

    def frames_of(eng):
        return SimpleNamespace(_eng=eng, frame_names=["root_joint"] + list(model.contacts))

    def loco_of(eng, frames, zmp_frame=0, zmp=True):
        return SimpleNamespace(_eng=eng, _frames=frames, plan=SimpleNamespace(arrays=dict(zmp_frame=zmp_frame)),
                               zmp=torch.zeros(2, 4, dtype=torch.float64) if zmp else None, odom_pose=torch.zeros(3, 4, dtype=torch.float64))
    make = blocks.SupportPolygon
    eng = engine(load_builtin("arm7"))
    fr = frames_of(eng)
    with pytest.raises(RuntimeError, match="free-flyer"):
        make(eng, fr, loco_of(eng, fr))
    for broken, error, message in ((no_contacts, RuntimeError, "at least one contact"), (many, NotImplementedError, "at most 16")):
        eng = engine(broken)
        fr = frames_of(eng)
        with pytest.raises(error, match=message):
            make(eng, fr, loco_of(eng, fr))
    eng = engine()
    fr = frames_of(eng)
    with pytest.raises(ValueError, match="frame kinematics block belongs to another engine"):
        make(eng, frames_of(engine()), loco_of(eng, fr))
    with pytest.raises(ValueError, match="locomotion quantities block belongs to another engine"):
        make(eng, fr, loco_of(engine(), fr))
    with pytest.raises(ValueError, match="reads another frame kinematics block"):
        make(eng, fr, loco_of(eng, frames_of(eng)))
    with pytest.raises(ValueError, match="must both be positive"):
        make(eng, fr, loco_of(eng, fr), cutoff_inner=-0.1, cutoff_outer=0.1)
    with pytest.raises(ValueError, match="must both be positive"):
        make(eng, fr, loco_of(eng, fr), cutoff_inner=0.1, cutoff_outer=-0.1)
    with pytest.raises(ValueError, match="cutoff_inner and cutoff_outer together"):
        make(eng, fr, loco_of(eng, fr), cutoff_inner=0.1)
    with pytest.raises(ValueError, match="cutoff_inner and cutoff_outer together"):
        make(eng, fr, loco_of(eng, fr), cutoff_outer=0.1)
    with pytest.raises(ValueError, match="a cutoff of zero is refused"):
        make(eng, fr, loco_of(eng, fr), cutoff_inner=0.0, cutoff_outer=0.1)
    with pytest.raises(ValueError, match="a cutoff of zero is refused"):
        make(eng, fr, loco_of(eng, fr), cutoff_inner=0.1, cutoff_outer=0.0)
    with pytest.raises(ValueError, match="LOCAL_WORLD_ALIGNED differs from the zmp_reference_frame LOCAL"):
        make(eng, fr, loco_of(eng, fr, zmp_frame=0), reference_frame="LOCAL_WORLD_ALIGNED")
    with pytest.raises(ValueError, match="LOCAL differs from the zmp_reference_frame LOCAL_WORLD_ALIGNED"):
        make(eng, fr, loco_of(eng, fr, zmp_frame=1), reference_frame=0)
    with pytest.raises(ValueError, match="Reference frame must be either"):
        make(eng, fr, loco_of(eng, fr), reference_frame="ODOMETRY")
    names_ = blocks.support_fieldnames(model.contacts)
    assert names_["scalars"] == ["stability_margin", "reward_robustness"] == list(support.SCALARS)
    assert len(names_["vertex_index"]) == 16 and len(names_["vertices"]) == 2 and names_["points"] == list(model.contacts)

    # the environment
    def bare_init(self, *args, **kw):
        self.model, self.num_envs, self.step_dt, self.dtype, self.device, self.engine = model, 4, 0.04, torch.float64, torch.device("cpu"), None
    monkeypatch.setattr(VecJiminyEnv, "__init__", bare_init)
    with pytest.raises(ValueError, match="the support polygon reads the locomotion quantities block: give locomotion_quantities"):
        WalkerVecEnv(support_polygon=dict(cutoff_inner=0.1, cutoff_outer=0.1))
    with pytest.raises(ValueError, match="the robustness reward term reads the support polygon block: give support_polygon"):
        WalkerVecEnv(reward_mixture={"robustness": 1.0})
    with pytest.raises(ValueError, match="give support_polygon"):
        WalkerVecEnv(reward_mixture={"robustness": 1.0}, locomotion_quantities={})
    for cfg in ({}, dict(cutoff_inner=0.1), dict(cutoff_outer=0.1), dict(cutoff_inner=None, cutoff_outer=0.2)):
        with pytest.raises(ValueError, match=r"reward_mixture\['robustness'\] needs support_polygon\['cutoff_inner'\] and"):
            WalkerVecEnv(reward_mixture={"robustness": 1.0}, locomotion_quantities={}, support_polygon=cfg)


# ------------------------------------------------------------------------------------------------------------ device
class DeviceSupport:
    """A plan on the device and the launch on numpy arrays (copied in and out)."""

    def __init__(self, lib, plan: dict, device):
        import torch
        self.torch, self.lib, self.device, self.plan = torch, lib, device, plan
        desc, keep = emu.plan_desc(plan)
        self.h = C.c_void_p()
        with torch.cuda.device(device):
            lib.check(lib.L.jm_support_plan_create(C.byref(desc), C.byref(self.h)))

    def close(self):
        self.lib.L.jm_support_plan_destroy(self.h)

    def run(self, inputs: dict, dtype=np.float64, outputs=sp.OUTPUTS, mask=None, fill=7.25, cutoff_inner=None, cutoff_outer=None):
        torch = self.torch
        B = inputs["pose"].shape[-1]
        io, held, out = _abi.SupportIO(), [], {}
        for name, a in inputs.items():
            t = torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=self.device)
            held.append(t)
            setattr(io, name, t.data_ptr())
        if mask is not None:
            held.append(torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device=self.device))
            io.lane_mask = held[-1].data_ptr()
        for name in sp.OUTPUTS:
            out[name] = torch.as_tensor(emu.new_output(name, self.plan, B, np.dtype(dtype), fill), device=self.device)
            if name in outputs:
                setattr(io, name, out[name].data_ptr())
        ci = self.plan.get("cutoff_inner", 0.0) if cutoff_inner is None else cutoff_inner
        co = self.plan.get("cutoff_outer", 0.0) if cutoff_outer is None else cutoff_outer
        self.lib.check(self.lib.L.jm_block_support_polygon(self.h, _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B,
                                                           C.byref(io), float(ci), float(co),
                                                           C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        del held
        return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, gpu_device):
    """Every fixture case through the C ABI at B = 64, both dtypes."""
    dev = DeviceSupport(_prebuilt(load_builtin("cartpole")), case(name)[0], gpu_device)
    try:
        check_against_the_fixture(name, lambda plan, inputs, dtype: dev.run(inputs, dtype), "device")
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["biped_boxes", "quadruped_local", "exact_ties"])
def test_device_is_independent_of_the_batch_mates(name, gpu_device):
    """The 64 lanes permuted and embedded in B = 192 (lane 3 b + 1 holds lane perm[b]; the other lanes hold lanes of the case
    in another order): the same bits as at B = 64, in both dtypes."""
    plan, inputs = case(name)[:2]
    dev = DeviceSupport(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        rg = np.random.default_rng(5)
        perm = rg.permutation(64)
        lanes = rg.integers(0, 64, 192)
        lanes[1::3] = perm
        big_inputs = {k: np.ascontiguousarray(v[..., lanes]) for k, v in inputs.items()}
        for dtype in (np.float64, np.float32):
            small, big = dev.run(inputs, dtype), dev.run(big_inputs, dtype)
            for out in sp.OUTPUTS:
                assert big[out].shape[-1] == 192
                assert _same_bits(np.ascontiguousarray(big[out][..., 1::3]), np.ascontiguousarray(small[out][..., perm])), (out, dtype)
                assert _same_bits(big[out], np.ascontiguousarray(small[out][..., lanes])), (out, dtype)
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_null_outputs_cutoffs_lane_mask_and_failed_lanes(gpu_device):
    """An output that is not asked for keeps its poison; a zero cutoff or a null ZMP leaves the rows; with a mask the other
    lanes keep every bit; lanes of NaN / infinite `pose` in the batch terminate, stay in range and disturb no other lane (the
    same source terminates on such lanes in `test_emulated_failed_lanes_terminate_and_stay_in_range`)."""
    lib = _prebuilt(load_builtin("cartpole"))
    names = ("quadruped_local", "biped_boxes", "exact_ties")
    devs = {len(case(name)[0]["point_column"]): DeviceSupport(lib, case(name)[0], gpu_device) for name in names}
    try:
        run = lambda plan, inputs, dtype=np.float64, **kw: devs[len(plan["point_column"])].run(inputs, dtype, **kw)      # noqa: E731
        check_null_outputs_lane_mask_and_cutoffs(run)
        for name in names:
            check_failed_lanes(name, run)
        io = _abi.SupportIO()
        rc = lib.L.jm_block_support_polygon(devs[4].h, _abi.JM_F64, 64, C.byref(io), -1.0, 0.1, None)
        assert rc == _abi.JM_EINVAL and "cutoff thresholds must both be positive" in _last_error(lib)
    finally:
        for dev in devs.values():
            dev.close()


def _anymal(device, monkeypatch, B=64, steps=5, **kw):
    """An ANYmal environment with constraint contacts under its PD controller (zero action); the lanes 1 mod 4 start 3 m above
    the ground and are in free fall for the steps of the test."""
    import torch

    from jiminy_amd.envs import VecJiminyEnv, make_anymal_env
    high = torch.arange(B, device=device) % 4 == 1
    sample = VecJiminyEnv._sample_state

    def lifted(self, n):
        q, v = sample(self, n)
        q = q.clone()
        q[2] += torch.where(high, 3.0, 0.0).to(q.dtype)
        # every lane somewhere else on the plane and turned about the vertical by its own angle (the odometry frame differs
        # from the world-aligned one): the root quaternion (x y z w) times a rotation about z from the left
        lane = torch.arange(B, device=device).to(q.dtype)
        yaw = 0.1 * lane - 3.0
        s, c = torch.sin(0.5 * yaw), torch.cos(0.5 * yaw)
        x, y, z, w_ = q[3].clone(), q[4].clone(), q[5].clone(), q[6].clone()
        q[3], q[4], q[5], q[6] = c * x - s * y, c * y + s * x, c * z + s * w_, c * w_ - s * z
        q[0] += 0.05 * lane
        q[1] -= 0.03 * lane
        return q, v
    if sample.__name__ != "lifted":         # (once per test, however many environments it builds)
        monkeypatch.setattr(VecJiminyEnv, "_sample_state", lifted)
    env = make_anymal_env(B, device=device, contact_model="constraint", auto_reset=False, **kw)
    env.reset(seed=3)
    action = torch.zeros(B, env.model.nmotors, dtype=torch.float64, device=device)
    out = None
    for _ in range(steps):
        out = env.step(action)
    return env, out, high, action


def _block_inputs(block) -> dict:
    """The tensors a block read at its last refresh, as numpy arrays in the layout of the kernel's inputs."""
    loco = block._locomotion
    return dict(pose=block._frames.pose.cpu().numpy(), odom_pose=loco.odom_pose.cpu().numpy(), zmp=loco.zmp.cpu().numpy())


def _block_plan(block) -> dict:
    return dict(block.plan.arrays, cutoff_inner=block.cutoff_inner or 0.0, cutoff_outer=block.cutoff_outer or 0.0)


def _bits(t):
    import torch
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.gpu
def test_block_laws_on_a_standing_anymal(gpu_device, monkeypatch):
    """`make_anymal_env(64, contact_model="constraint", locomotion_quantities=..., support_polygon=...)`, 5 steps of the PD
    controller.  The device margin against the numpy restatement on the tensors the block read, to 1e-13; a LOCAL and a
    LOCAL_WORLD_ALIGNED pair of blocks agree on the margin to 1e-12 and on `n_vertices`; a standing robot has a positive margin,
    a lane in free fall -inf and a reward of 0."""
    import torch

    from jiminy_amd import blocks
    cutoffs = dict(cutoff_inner=0.1, cutoff_outer=0.2)
    env, _, high, _ = _anymal(gpu_device, monkeypatch, locomotion_quantities=dict(zmp_reference_frame="LOCAL_WORLD_ALIGNED"),
                              support_polygon=cutoffs)
    block = env.support
    assert block.reference_frame == sp.LOCAL_WORLD_ALIGNED and block.contact_names == list(env.model.contacts)
    assert block.fieldnames == blocks.support_fieldnames(env.model.contacts)
    local_loco = blocks.LocomotionQuantities(env.engine, env.frames, zmp_reference_frame="LOCAL")
    local = blocks.SupportPolygon(env.engine, env.frames, local_loco, **cutoffs)
    assert local.reference_frame == sp.LOCAL
    with pytest.raises(ValueError, match="differs from the zmp_reference_frame"):
        blocks.SupportPolygon(env.engine, env.frames, local_loco, reference_frame="LOCAL_WORLD_ALIGNED")
    local_loco.refresh()
    local.refresh()
    torch.cuda.synchronize(gpu_device)
    high_ = high.cpu().numpy()
    for blk, label in ((block, "LOCAL_WORLD_ALIGNED"), (local, "LOCAL")):
        host = sp.quantities(_block_plan(blk), _block_inputs(blk))
        dev = {k: getattr(blk, k).cpu().numpy() for k in sp.OUTPUTS}
        for k in sp.INT_OUTPUTS:
            assert np.array_equal(dev[k], host[k]), (label, k)
        for k in FLOAT_OUTPUTS:
            e = rel_error(dev[k], host[k])
            print(f"standing ANYmal {label}, device against the host composition, {k}: {e:.2e}")
            assert e <= TOL, (label, k, e)
        margin, reward = dev["scalars"]
        print(f"standing ANYmal {label}: margin of the standing lanes {margin[~high_].min():.4f} .. {margin[~high_].max():.4f}, "
              f"reward {reward[~high_].min():.4f} .. {reward[~high_].max():.4f}")
        assert (margin[~high_] > 0.0).all() and (margin[high_] == -np.inf).all() and (reward[high_] == 0.0).all()
        assert (reward[~high_] > 0.5).all() and (dev["n_vertices"] == 4).all()
    a, b = block.stability_margin.cpu().numpy(), local.stability_margin.cpu().numpy()
    e = rel_error(b, a)
    print(f"standing ANYmal: LOCAL against LOCAL_WORLD_ALIGNED margin {e:.2e}")
    assert e <= 1e-12 and torch.equal(block.n_vertices, local.n_vertices)
    # `reset(lane_mask)`: the masked lanes are evaluated, the others keep every tensor bit for bit
    tensors = {k: getattr(block, k) for k in sp.OUTPUTS}
    full = {k: t.clone() for k, t in tensors.items()}
    for t in tensors.values():
        t.fill_(7)
    mask = torch.arange(64, device=gpu_device) % 3 == 0
    block.reset(mask)
    for k, t in tensors.items():
        assert t is getattr(block, k)
        assert (t[..., ~mask] == 7).all() and torch.equal(_bits(t[..., mask]), _bits(full[k][..., mask])), k
    block.refresh()
    assert all(torch.equal(_bits(t), _bits(full[k])) for k, t in tensors.items())
    with pytest.raises(ValueError, match="lane_mask must have shape"):
        block.reset(mask[:5])
    env.close()


@pytest.mark.gpu
def test_environment_robustness_reward(gpu_device, monkeypatch):
    """64 lanes: `reward_mixture={'robustness': w}` adds `w * env.support.reward_robustness` to what the same environment returns
    without the term; `reset_lanes` on half the lanes keeps the other half bit for bit; a captured graph of `support.refresh()`
    replays to the bits of the eager launch after its outputs are poisoned; without the keyword `env.support` is None."""
    import torch

    w = 0.375
    cfg = dict(locomotion_quantities={}, support_polygon=dict(cutoff_inner=0.1, cutoff_outer=0.2))
    env, out, high, action = _anymal(gpu_device, monkeypatch, reward_mixture={"survival": 1.0, "robustness": w}, **cfg)
    plain, out_plain, _, _ = _anymal(gpu_device, monkeypatch, reward_mixture={"survival": 1.0}, **cfg)
    bare, _, _, _ = _anymal(gpu_device, monkeypatch, steps=1)
    assert bare.support is None and bare.locomotion is None and plain.support is not None
    block = env.support
    assert block.reference_frame == sp.LOCAL and env.locomotion.zmp is not None
    for _ in range(2):
        assert torch.equal(out[1], out_plain[1] + w * block.reward_robustness)
        assert torch.equal(_bits(block.scalars), _bits(plain.support.scalars))
        assert float(block.reward_robustness[~high].min()) > 0.5 and float(block.reward_robustness[high].max()) == 0.0
        out, out_plain = env.step(action), plain.step(action)
    # a captured graph of the refresh
    tensors = {k: getattr(block, k) for k in sp.OUTPUTS}
    eager = {k: t.clone() for k, t in tensors.items()}
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.graph(graph):
        block.refresh()
    for t in tensors.values():
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize(gpu_device)
    for k, t in tensors.items():
        assert t is getattr(block, k) and torch.equal(_bits(t), _bits(eager[k])), k
    # a partial reset: the reset lanes are evaluated at their reset state, the others keep every bit
    mask = torch.arange(64, device=gpu_device) % 2 == 0
    env.reset_lanes(mask)
    for k, t in tensors.items():
        assert t is getattr(block, k) and torch.equal(_bits(t[..., ~mask]), _bits(eager[k][..., ~mask])), k
    assert not torch.equal(_bits(block.vertices[..., mask]), _bits(eager["vertices"][..., mask]))
    for e in (env, plain, bare):
        e.close()
