"""Reference-pinned fixtures of the locomotion quantities block on height-map ground: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_locomotion_fixtures.py, whose loader, flat-ground composition and draws this script
imports: the reference's `normalize_vertical_forces`, `normalize_spatial_forces`, `min_depth` and `radial_basis_function` (and
the functions of the flat quantities) are parsed where they lie and executed; nothing of the reference is copied into the
repository.  Only authored descriptions, seeded inputs and the outputs the reference's code produced for them are written, to
tests/golden/ref_locomotion_ground.npz.

Run where the reference tree is available:   python tools/make_ref_locomotion_ground_fixtures.py [output.npz]
                                             python tools/make_ref_locomotion_ground_fixtures.py --check   (regenerate and compare)

What this script RESTATES, and labels as such below: `FrameConstraint::setNormal` (core/src/constraints/frame_constraint.cc:
62-68), whose `rotationLocal_` gives the vertical transform of a contact (its third row, quantities/locomotion.py:1426-1436);
the ground under a point, which in the reference is a user's `groundProfile` callable and here the project's own definition of
`set_ground_heightmap` (bilinear patches, flat continuation outside the map); the per-lane offset of its queries
(`set_ground_offsets`); and the `refresh` bodies of `MultiFootNormalizedForceVertical` (:1468-1481) and
`_MultiContactMinGroundDistance` (compositions/locomotion.py:527-540) around the reference's functions.

Every case holds 64 lanes.  Next to the draw conditions of the flat tool: outside the designed contacts, the grid coordinates
of every contact stay at least 2^-10 of a cell from every cell line (the normal jumps across a line: float32 must land in the
same cell); the designed coordinates of `edges` are short binary fractions, exact in float32; `z - height` lies in
[-0.05, 0.5].
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_ref_locomotion_fixtures as flat      # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_locomotion_ground.npz")
B = flat.B
SEED = 20261020
LOCAL, LOCAL_WORLD_ALIGNED = flat.LOCAL, flat.LOCAL_WORLD_ALIGNED
OUTPUTS = flat.OUTPUTS + ("contact_ground",)
MARGIN = 2.0 ** -10


# ------------------------------------------------------------------------------------------------------ restated glue
def ground_patch(g: dict, x: float, y: float):
    """RESTATED: the project's own definition of `set_ground_heightmap` -- sample (iy, ix) at (x0 + ix dx, y0 + iy dy),
    bilinear patches, outside the map the height of the nearest edge sample and no slope across the edge.  Height, unit normal."""
    H = g["heights"]
    ny, nx = H.shape
    u, w = (x - g["x0"]) / g["dx"], (y - g["y0"]) / g["dy"]
    in_x, in_y = 0.0 <= u <= nx - 1, 0.0 <= w <= ny - 1
    u, w = min(max(u, 0.0), nx - 1.0), min(max(w, 0.0), ny - 1.0)
    ix, iy = min(max(int(u), 0), nx - 2), min(max(int(w), 0), ny - 2)
    fx, fy = u - ix, w - iy
    h00, h10, h01, h11 = (float(v) for v in (H[iy, ix], H[iy, ix + 1], H[iy + 1, ix], H[iy + 1, ix + 1]))
    h = (1.0 - fy) * ((1.0 - fx) * h00 + fx * h10) + fy * ((1.0 - fx) * h01 + fx * h11)
    dhdx = ((1.0 - fy) * (h10 - h00) + fy * (h11 - h01)) / g["dx"] if in_x else 0.0
    dhdy = ((1.0 - fx) * (h01 - h00) + fx * (h11 - h10)) / g["dy"] if in_y else 0.0
    normal = np.array([-dhdx, -dhdy, 1.0])
    return h, normal / np.sqrt(dhdx * dhdx + dhdy * dhdy + 1.0)


def set_normal(normal: np.ndarray) -> np.ndarray:
    """RESTATED `FrameConstraint::setNormal` (frame_constraint.cc:62-68): `rotationLocal_`."""
    rotation_local = np.zeros((3, 3))
    rotation_local[:, 2] = normal
    col1 = np.cross(normal, np.array([1.0, 0.0, 0.0]))
    rotation_local[:, 1] = col1 / np.linalg.norm(col1)
    rotation_local[:, 0] = np.cross(rotation_local[:, 1], rotation_local[:, 2])
    return rotation_local


def lane_quantities(ref: dict, plan: dict, lane: dict, g, offset) -> dict:
    """The flat tool's composition, then RESTATED `MultiFootNormalizedForceVertical.refresh` (:1468-1481) and
    `_MultiContactMinGroundDistance.refresh` (compositions/locomotion.py:527-540) on the ground `g` (None: flat) queried at the
    lane's offset (RESTATED: `set_ground_offsets`), around the reference's own functions."""
    out = flat.lane_quantities(ref, plan, lane)
    nc, n_feet = len(plan["contact_foot"]), int(plan["n_feet"])
    positions = np.asfortranarray(lane["pose"][:3][:, [int(k) for k in plan["contact_column"]]])
    heights, normals = np.zeros(nc), np.asfortranarray(np.tile(np.array([[0.0], [0.0], [1.0]]), (1, nc)))
    if g is not None:
        for c in range(nc):
            x, y = positions[0, c], positions[1, c]
            if offset is not None:
                x, y = x + offset[0], y + offset[1]
            heights[c], normals[:, c] = ground_patch(g, x, y)
    out["contact_ground"] = np.concatenate([heights[None], normals])
    if g is None:
        return out
    masses = lane["model_lane"][0::13] if "model_lane" in lane else plan["body_mass"]
    robot_weight = flat.robot_mass(masses) * abs(float(plan["gravity"]))
    lambda_c = (lane["con_lambda"].reshape(nc, 4) * ((lane["con_flags"] & 1) != 0)[:, None]).reshape(-1)
    feet = list(plan["contact_foot"])
    foot_slices = tuple((4 * feet.index(f), 4 * (len(feet) - feet[::-1].index(f))) for f in range(n_feet))
    # (the third row of every constraint's `local_rotation`, :1426-1436)
    vertical = tuple(np.asfortranarray(np.stack([set_normal(normals[:, c])[2] for c in range(s // 4, e // 4)], -1)) for s, e in foot_slices)
    foot_force = np.zeros(n_feet)
    ref["normalize_vertical_forces"](lambda_c, foot_slices, vertical, robot_weight, foot_force)
    out["foot_force_vertical"] = foot_force
    out["scalars"] = out["scalars"].copy()
    out["scalars"][1] = ref["min_depth"](positions, heights, normals)
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def clear_of_lines(rg: np.random.Generator, low: float, high: float) -> float:
    """A grid coordinate in [low, high] at least 2 MARGIN away from every integer."""
    while True:
        u = rg.uniform(low, high)
        if abs(u - round(u)) >= 2 * MARGIN:
            return u


def plane_map(nx, ny, x0, y0, dx, dy, a, b, c):
    X, Y = np.meshgrid(x0 + dx * np.arange(nx), y0 + dy * np.arange(ny))
    return a * X + b * Y + c


# label -> the arguments of the flat tool's make_case (foot of every contact, feet, ZMP frame, DCM frame, some contacts
# disabled, free fall, per-lane model)
CASES = (
    ("ramp", ((0, 1, 2, 3), 4, LOCAL, LOCAL, False, False, False)),
    ("tiles", ((0, 0, 0, -1, 1, 1, 1, 1), 2, LOCAL_WORLD_ALIGNED, LOCAL, True, False, False)),
    ("edges", ((0, 1, 2, 3), 4, LOCAL, LOCAL, False, False, False)),
    ("steep", ((0, 0, 1, 1), 2, LOCAL, LOCAL_WORLD_ALIGNED, False, False, False)),
    ("zero_map", ((0, 1, 2, 3), 4, LOCAL, LOCAL, True, False, False)),
    ("per_lane_model", ((0, 0, 1, 1), 2, LOCAL, LOCAL, False, False, True)),
)
# the designed contact of `edges` (contact 0 of lane k): grid coordinates on a node, on a cell edge, outside past each of the
# four sides and past a corner
EDGES_DESIGNED = ((0.0, 0.0), (1.0, 1.0), (0.5, 0.0), (1.0, 0.25), (-0.5, 0.5), (1.5, 0.5), (0.5, -0.5), (0.5, 1.5), (1.5, 1.5),
                  (-0.25, -0.75))


def make_ground(label: str, rg: np.random.Generator):
    """The height map of a case, whether its lanes carry offsets, and the range of the grid coordinates of its contacts."""
    if label == "ramp":
        return dict(heights=plane_map(3, 3, -3.0, -3.0, 3.0, 3.0, 0.2, -0.1, 0.3), x0=-3.0, y0=-3.0, dx=3.0, dy=3.0), False, 0.0
    if label in ("tiles", "per_lane_model"):
        return dict(heights=rg.uniform(-0.2, 0.4, (4, 5)), x0=-1.75, y0=0.6, dx=0.8, dy=1.3), True, 0.7
    if label == "edges":
        return dict(heights=np.array([[0.125, -0.25], [0.5, 0.0625]]), x0=-0.25, y0=0.5, dx=0.5, dy=0.25), False, 0.9
    if label == "steep":
        # a profile along x plus one along y, steps of at most 1.0 per 0.5: |dh/dx|, |dh/dy| <= 2; the first row of cells does
        # not vary along y: n.y == 0 exactly there
        along_x = np.cumsum(rg.uniform(-1.0, 1.0, 4))
        along_y = np.concatenate([[0.0, 0.0], np.cumsum(rg.uniform(-1.0, 1.0, 2))])
        return dict(heights=along_y[:, None] + along_x[None, :], x0=-1.0, y0=-0.5, dx=0.5, dy=0.5), True, 0.4
    if label == "zero_map":
        return dict(heights=np.zeros((3, 3)), x0=-1.0, y0=-1.0, dx=1.0, dy=1.0), True, 0.6
    raise KeyError(label)


def make_case(ref: dict, rg: np.random.Generator, label: str, args) -> dict:
    case = flat.make_case(ref, rg, *args)
    plan = {k[5:]: (v if v.ndim else v.item()) for k, v in case.items() if k.startswith("plan.")}
    g, with_offsets, outside = make_ground(label, rg)
    ny, nx = g["heights"].shape
    nc = len(plan["contact_foot"])
    cols = [int(k) for k in plan["contact_column"]]
    offsets = rg.uniform(-3.0, 3.0, (2, B)) if with_offsets else None
    designed = np.zeros((nc, B), dtype=bool)
    pose = case["pose"]
    for b in range(B):
        off = offsets[:, b] if with_offsets else np.zeros(2)
        for c in range(nc):
            u, w = clear_of_lines(rg, -outside, nx - 1 + outside), clear_of_lines(rg, -outside, ny - 1 + outside)
            if label == "steep" and b % 4 == 0:
                w = clear_of_lines(rg, 0.0, 1.0)
            if label == "edges" and c == 0 and b < len(EDGES_DESIGNED):
                (u, w), designed[c, b] = EDGES_DESIGNED[b], True
            x, y = g["x0"] + u * g["dx"] - off[0], g["y0"] + w * g["dy"] - off[1]
            h = ground_patch(g, x + off[0], y + off[1])[0]
            pose[0, cols[c], b], pose[1, cols[c], b], pose[2, cols[c], b] = x, y, h + rg.uniform(-0.05, 0.5)
    lanes = []
    for b in range(B):
        lane = {k: case[k][..., b] for k in flat.INPUTS if k in case}
        off = offsets[:, b] if with_offsets else None
        e = lane_quantities(ref, plan, lane, g, off)
        on_flat = lane_quantities(ref, plan, lane, None, None)
        for k in flat.OUTPUTS:       # (what does not look at the ground is what the flat tool wrote)
            if k not in ("foot_force_vertical", "scalars"):
                assert np.array_equal(e[k], case[f"expected.{k}"][..., b], equal_nan=True), k
        assert np.array_equal(e["scalars"][[0, 2, 3]], on_flat["scalars"][[0, 2, 3]])
        if label == "zero_map":
            assert all(np.array_equal(e[k], on_flat[k]) for k in OUTPUTS), "the zero map must give the flat ground's outputs"
        # the draw conditions
        for c in range(nc):
            x, y, z = lane["pose"][:3, cols[c]]
            if off is not None:
                x, y = x + off[0], y + off[1]
            u, w = (x - g["x0"]) / g["dx"], (y - g["y0"]) / g["dy"]
            if designed[c, b]:
                assert (u, w) == EDGES_DESIGNED[b] and all(float(np.float32(v)) == v for v in (x, y))
            else:
                assert abs(u - round(u)) >= MARGIN and abs(w - round(w)) >= MARGIN
            assert -0.05 <= z - e["contact_ground"][0, c] <= 0.5
        lanes.append(e)
    if label == "steep":
        ny_zero = np.stack([e["contact_ground"][2] for e in lanes], -1) == 0.0
        assert ny_zero[:, 0::4].all() and not ny_zero.all()
        slope = np.stack([np.abs(e["contact_ground"][1:3]) / e["contact_ground"][3] for e in lanes], -1)
        assert 1.0 < slope.max() <= 2.0 * (1 + 1e-12)
    case.update({f"expected.{k}": np.stack([e[k] for e in lanes], -1) for k in OUTPUTS})
    case.update({f"ground.{k}": np.asarray(v) for k, v in g.items()})
    if with_offsets:
        case["ground.offsets"] = offsets
    case["designed"] = designed
    del case["designed_nan"]
    return case


def generate() -> dict:
    ref = flat.load_reference_functions()
    rg = np.random.default_rng(SEED)
    out: dict = {}
    for label, args in CASES:
        for k, v in make_case(ref, rg, label, args).items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array([c[0] for c in CASES])
    out["tier"] = np.array("A: the reference's functions on the arrays they are written for; FrameConstraint::setNormal, the "
                           "bilinear height map, the per-lane offset and the refresh bodies around them are restated")
    return out


def main(out_path: str, verbose: bool = True) -> None:
    np.savez_compressed(out_path, **generate())
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(flat.COMMON):
        sys.exit(f"{flat.COMMON} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        fresh, have = generate(), np.load(OUT)
        same = sorted(fresh) == sorted(have.files) and all(
            np.asarray(fresh[k]).dtype == have[k].dtype and np.array_equal(fresh[k], have[k], equal_nan=have[k].dtype.kind == "f")
            for k in fresh)
        print("tests/golden/ref_locomotion_ground.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
