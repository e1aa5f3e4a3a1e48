"""Reference-pinned fixtures of the projected support polygon block: EXECUTES THE REFERENCE'S OWN PYTHON.

Same mechanism and rules as tools/make_ref_locomotion_fixtures.py: this script parses the reference files where they lie, takes
the function definitions named in SOURCES (decorators included) and the constant `CUTOFF_ESP`, and executes them with
`numba.jit` stubbed to the identity.  Nothing of the reference is copied into the repository: only authored descriptions,
seeded inputs and the outputs the reference's code produced for them, written to tests/golden/ref_support.npz.

Run where the reference tree is available:   python tools/make_ref_support_fixtures.py [output.npz]
                                             python tools/make_ref_support_fixtures.py --check     (regenerate and compare)

Tier A for the functions, a restated composition for the glue: `compute_convex_hull_vertices`, `compute_vectors_from_convex`,
`compute_distance_convex_to_point` (with `_amin_last_axis`, `_all_last_axis`), `sigmoid_normalization` and
`translate_position_odom` are the reference's, called on the arrays they are written for, one lane at a time.  What this script
RESTATES, and labels as such below: `ProjectedSupportPolygon.refresh` (toolbox/quantities/locomotion.py:146-160; the candidate
points are every contact point: the host-side pruning by the 3D hull of each body is not built),
`ConvexHull2D.__init__` / `.center` / the `npoints <= 2` branches of `.get_distance_to_point` (toolbox/math/qhull.py:366-457),
`StabilityMarginProjectedSupportPolygon.refresh` (:228-239) and the call of `MaximizeRobustness` (compositions/locomotion.py:
105-112).  `translate_position_odom` subtracts the reference position `[2]` from its first argument, which broadcasts as meant
for one position `[2]` only, so it is called once per point.

Every case holds 64 lanes.  The generator asserts its own conditions on every lane: with three points or fewer no two points
coincide; apart from the lanes of `exact_ties` every query lies at least 1e-6 from the border (1e-3 in LOCAL); in LOCAL every
orientation predicate the reference evaluates has |lhs - rhs| >= 1e-4 (|lhs| + |rhs|) (the device's translation may differ
from numpy's in the last bit, in float32 as well; the bar asked for is 1e-9); the argument of the reward stays within
|value_rel| <= 4.  A lane that misses a condition on random points is drawn again.
"""
from __future__ import annotations

import ast
import math
import os
import sys
import tempfile
import types
import typing

import numpy as np

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
COMMON = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common")
TOOLBOX = os.path.join(REF, "python/gym_jiminy/toolbox/gym_jiminy/toolbox")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_support.npz")

SOURCES = (
    (COMMON, "quantities/locomotion.py", ("translate_position_odom",)),
    (COMMON, "compositions/mixin.py", ("CUTOFF_ESP",)),
    (TOOLBOX, "math/qhull.py", ("_amin_last_axis", "_all_last_axis", "compute_convex_hull_vertices", "compute_vectors_from_convex",
                                "compute_distance_convex_to_point")),
    (TOOLBOX, "compositions/locomotion.py", ("sigmoid_normalization",)),
)
B = 64
SEED = 20261020
LOCAL, LOCAL_WORLD_ALIGNED = 0, 1
MAX_POINTS = 16
INPUTS = ("pose", "odom_pose", "zmp")
OUTPUTS = ("n_vertices", "vertex_index", "vertices", "center", "scalars")
BORDER, BORDER_LOCAL, PREDICATE_LOCAL, VALUE_REL_MAX = 1e-6, 1e-3, 1e-4, 4.0


def load_reference_functions() -> dict:
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    ns: dict = {"np": np, "nb": nb, "math": math, "ArrayOrScalar": typing.Any}
    ns.update({k: getattr(typing, k) for k in ("Optional", "Tuple", "Union", "List", "Sequence", "Dict", "Literal", "overload",
                                               "no_type_check")})
    for root, rel, names in SOURCES:
        path = os.path.join(root, rel)
        with open(path) as f:
            tree = ast.parse(f.read(), filename=path)
        found = set()
        for node in tree.body:
            is_function = isinstance(node, ast.FunctionDef) and node.name in names
            is_constant = (isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name)
                           and node.targets[0].id in names)
            if is_function or is_constant:
                exec(compile(ast.Module([node], []), path, "exec"), ns)
                found.add(node.name if is_function else node.targets[0].id)
        if set(names) - found:
            raise RuntimeError(f"{rel}: {sorted(set(names) - found)} not found")
    return ns


# ------------------------------------------------------------------------------------------------------ restated glue
def lane_quantities(ref: dict, plan: dict, lane: dict) -> dict:
    """RESTATED `ProjectedSupportPolygon.refresh`, `ConvexHull2D.__init__` / `.center` / `.get_distance_to_point`,
    `StabilityMarginProjectedSupportPolygon.refresh` and the reward of `MaximizeRobustness` for one lane, around the
    reference's own functions."""
    cols = [int(c) for c in plan["point_column"]]
    points = np.ascontiguousarray(lane["pose"][:2, cols].T)                # `_candidate_xy_batch`, [n][2]
    if plan["reference_frame"] == LOCAL:
        for point in points:
            ref["translate_position_odom"](point, lane["odom_pose"], point)
    npoints = len(points)
    indices = np.asarray(ref["compute_convex_hull_vertices"](points), dtype=np.int64)
    vertices = points[indices]
    nv = len(indices)
    out = dict(n_vertices=np.int32(nv), vertex_index=np.full(MAX_POINTS, -1, np.int32), vertices=np.full((2, MAX_POINTS), np.nan),
               center=np.mean(vertices, axis=0), points=points)
    out["vertex_index"][:nv] = indices
    out["vertices"][:, :nv] = vertices.T
    if "zmp" not in lane:
        return out
    zmp = lane["zmp"]
    if math.isnan(zmp[0]):
        margin = float("-inf")
    else:
        points2d = np.atleast_2d(zmp)
        if npoints > 2:
            vectors = ref["compute_vectors_from_convex"](vertices)
            dist2d = ref["compute_distance_convex_to_point"](vertices, vectors, points2d)
        elif npoints == 2:
            vec = vertices[1] - vertices[0]
            ratio = (points2d - vertices[0]) @ vec / np.dot(vec, vec)
            proj = vertices[0] + np.outer(np.clip(ratio, 0.0, 1.0), vec)
            dist2d = np.linalg.norm(points2d - proj, axis=1)
        else:
            dist2d = np.linalg.norm(points2d - vertices, axis=1)
        margin = - dist2d[0].item()
    reward = ref["sigmoid_normalization"](margin, -float(plan["cutoff_outer"]), float(plan["cutoff_inner"]), True)
    out["scalars"] = np.array([margin, reward])
    return out


def evaluated_predicates(points: np.ndarray, zmp) -> tuple:
    """RESTATED, for the generator's own assertion only: (lhs, rhs) of every orientation predicate the reference evaluates on
    these points (both chains, then the all-edges test of the query), and the vertices the chains give."""
    pairs = []
    order = np.argsort(points[:, 0], kind="mergesort")
    order = order[np.argsort(points[order, 1], kind="mergesort")]
    if len(points) <= 3:
        vertices = list(order)
    else:
        vertices = []
        for sequence in (order[::-1], order):
            chain = []
            for i in sequence:
                p = points[i]
                while len(chain) > 1:
                    a, b = points[chain[-2]], points[chain[-1]]
                    lhs, rhs = (b[0] - a[0]) * (p[1] - a[1]), (p[0] - a[0]) * (b[1] - a[1])
                    pairs.append((lhs, rhs))
                    if lhs > rhs:
                        break
                    chain.pop()
                    vertices.pop()
                if chain:
                    vertices.append(i)
                chain.append(i)
    if zmp is not None and len(points) > 2 and not math.isnan(zmp[0]):
        v = points[vertices]
        vectors = np.concatenate([v[-1:] - v[:1], v[:-1] - v[1:]])
        rel = zmp[None, :] - v
        pairs += list(zip(rel[:, 0] * vectors[:, 1], rel[:, 1] * vectors[:, 0]))
    return pairs, vertices


def conditions_hold(plan: dict, lane: dict, e: dict, ties: bool) -> bool:
    """The generator's conditions on one lane (see the module docstring)."""
    points, n = e["points"], len(e["points"])
    local = plan["reference_frame"] == LOCAL
    if n <= 3:
        for i in range(n):
            for j in range(i):
                if np.array_equal(points[i], points[j]):
                    return False
    zmp = lane.get("zmp")
    pairs, vertices = evaluated_predicates(points, zmp)
    assert list(vertices) == list(e["vertex_index"][:int(e["n_vertices"])])
    if local and any(abs(l - r) < PREDICATE_LOCAL * (abs(l) + abs(r)) for l, r in pairs):
        return False
    if zmp is not None and not math.isnan(zmp[0]):
        margin, reward = e["scalars"]
        if not ties and abs(margin) < (BORDER_LOCAL if local else BORDER):
            return False
        value_rel = margin / plan["cutoff_inner"] if margin > 0 else margin / plan["cutoff_outer"]
        if abs(value_rel) > VALUE_REL_MAX:
            return False
    return True


# ------------------------------------------------------------------------------------------------------------ cases
def filler_pose(rg: np.random.Generator, K: int) -> np.ndarray:
    """A `pose` tensor of one lane whose rows the block does not read are filled: heights and unit quaternions."""
    pose = np.empty((7, K))
    pose[:2] = rg.uniform(-3.0, 3.0, (2, K))
    pose[2] = rg.uniform(-0.01, 0.5, K)
    q = rg.normal(size=(4, K))
    pose[3:] = q / np.linalg.norm(q, axis=0)
    return pose


def rot2(yaw: float) -> np.ndarray:
    return np.array([[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]])


def query(rg: np.random.Generator, world_points: np.ndarray, b: int, every_nan: int) -> np.ndarray:
    """A query around the points: inside-ish on even lanes, outside-ish on odd ones, NaN on every `every_nan`-th lane."""
    if every_nan and b % every_nan == every_nan - 1:
        return np.array([float("nan"), float("nan")])
    c = world_points.mean(0)
    k = int(rg.integers(len(world_points)))
    u = rg.uniform(0.0, 0.7) if b % 2 == 0 else rg.uniform(1.2, 1.9)
    return c + u * (world_points[k] - c) + rg.uniform(-0.02, 0.02, 2)


def quadruped_points(rg, b):
    xy, yaw = rg.uniform(-2.0, 2.0, 2), rg.uniform(-np.pi, np.pi)
    feet = np.array([[0.35, 0.2], [0.35, -0.2], [-0.35, 0.2], [-0.35, -0.2]]) + rg.uniform(-0.06, 0.06, (4, 2))
    return xy + feet @ rot2(yaw).T, np.array([xy[0], xy[1], yaw]), None


def biped_points(rg, b):
    """Two feet of 8 box vertices each: a planar pose plus a tilt of up to 0.2 rad; every fourth lane exactly flat, in short
    binary fractions, so that the upper and lower vertices of a box coincide in projection bit for bit."""
    flat = b % 4 == 0
    box = np.array([[sx * 0.125, sy * 0.0625, sz * 0.03125] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)])
    base = rg.integers(-128, 128, 2) / 64.0 if flat else rg.uniform(-2.0, 2.0, 2)
    base_yaw = 0.0 if flat else rg.uniform(-np.pi, np.pi)
    points = []
    for side in (1.0, -1.0):
        if flat:
            centre, R = np.array([rg.integers(-8, 8) / 64.0, side * 0.125 + rg.integers(-2, 2) / 64.0, 0.03125]), np.eye(3)
        else:
            centre = np.array([rg.uniform(-0.15, 0.15), side * 0.12 + rg.uniform(-0.03, 0.03), 0.05])
            yaw, tilt, phi = rg.uniform(-0.3, 0.3), rg.uniform(0.0, 0.2), rg.uniform(-np.pi, np.pi)
            ax = np.array([math.cos(phi), math.sin(phi), 0.0])
            Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            Rt = np.eye(3) + math.sin(tilt) * Kx + (1 - math.cos(tilt)) * Kx @ Kx
            Rz = np.eye(3)
            Rz[:2, :2] = rot2(yaw)
            R = Rz @ Rt
        points.append((centre + box @ R.T)[:, :2])
    local = np.concatenate(points)
    world = base + local if flat else base + local @ rot2(base_yaw).T
    return world, np.array([base[0], base[1], base_yaw]), None


def few_points(n):
    def draw(rg, b):
        xy, yaw = rg.uniform(-2.0, 2.0, 2), rg.uniform(-np.pi, np.pi)
        return xy + rg.uniform(-0.4, 0.4, (n, 2)), np.array([xy[0], xy[1], yaw]), None
    return draw


def tie_points(rg, b):
    """8 points in short binary fractions: the corners of a rectangle, a collinear run of two points on one edge (one of them
    its midpoint), an interior point and a duplicate of one of the seven, in a random order; the query exactly on an edge
    (lanes 0 mod 3), on a vertex (1 mod 3) or strictly inside (2 mod 3)."""
    o = rg.integers(-64, 64, 2) / 32.0
    w, h = rg.integers(2, 9) / 8.0, rg.integers(2, 9) / 8.0
    corners = np.array([[0, 0], [w, 0], [w, h], [0, h]])
    e = int(rg.integers(4))
    a, c = corners[e], corners[(e + 1) % 4]
    run = [(a + c) / 2.0, a + (c - a) / 4.0]
    interior = np.array([w * rg.integers(1, 4) / 4.0, h * rg.integers(1, 4) / 4.0])
    seven = np.concatenate([corners, run, [interior]])
    pts = np.concatenate([seven, seven[[int(rg.integers(7))]]])[rg.permutation(8)] + o
    f = int(rg.integers(4))
    if b % 3 == 0:
        q = (corners[f] + corners[(f + 1) % 4]) / 2.0 if b % 2 else corners[f] + (corners[(f + 1) % 4] - corners[f]) / 8.0
    elif b % 3 == 1:
        q = corners[f]
    else:
        q = np.array([w * rg.integers(1, 8) / 8.0, h * rg.integers(1, 8) / 8.0])
    return pts, np.array([o[0], o[1], 0.0]), q + o


def random_points(n):
    def draw(rg, b):
        xy, yaw = rg.uniform(-2.0, 2.0, 2), rg.uniform(-np.pi, np.pi)
        return xy + rg.uniform(-0.5, 0.5, (n, 2)), np.array([xy[0], xy[1], yaw]), None
    return draw


def make_case(ref: dict, rg: np.random.Generator, draw, n: int, frame: int, cutoff_inner: float, cutoff_outer: float, with_zmp: bool,
              every_nan: int, ties: bool):
    K = n + 2
    plan = dict(point_column=rg.permutation(K)[:n].astype(np.int32), n_frames=K, reference_frame=frame, cutoff_inner=cutoff_inner,
                cutoff_outer=cutoff_outer)
    cols = [int(c) for c in plan["point_column"]]
    lanes, redrawn = [], 0
    for b in range(B):
        while True:
            world, odom_pose, q = draw(rg, b)
            assert world.shape == (n, 2)
            lane = dict(pose=filler_pose(rg, K), odom_pose=odom_pose)
            lane["pose"][:2, cols] = world.T
            if with_zmp:
                zmp = query(rg, world, b, every_nan) if q is None else np.asarray(q, dtype=np.float64)
                if frame == LOCAL and not math.isnan(zmp[0]):
                    # the ZMP of the locomotion block is in the odometry frame then
                    ref["translate_position_odom"](zmp, odom_pose, zmp)
                lane["zmp"] = zmp
            lane["expected"] = lane_quantities(ref, plan, lane)
            if conditions_hold(plan, lane, lane["expected"], ties):
                break
            assert not ties, "a designed lane misses the generator's conditions"
            redrawn += 1
            assert redrawn < 4 * B
        lanes.append(lane)
    case = {k: np.stack([lane[k] for lane in lanes], -1) for k in INPUTS if k in lanes[0]}
    case.update({f"expected.{k}": np.stack([lane["expected"][k] for lane in lanes], -1) for k in OUTPUTS if k in lanes[0]["expected"]})
    case.update({f"plan.{k}": np.asarray(v) for k, v in plan.items()})
    return case


CASES = (
    # label, points of a lane, n_points, frame, cutoff_inner, cutoff_outer, zmp, NaN on every n-th lane, designed ties
    ("quadruped_lwa", quadruped_points, 4, LOCAL_WORLD_ALIGNED, 0.08, 0.25, True, 8, False),
    ("quadruped_local", quadruped_points, 4, LOCAL, 0.08, 0.25, True, 8, False),
    ("biped_boxes", biped_points, 16, LOCAL_WORLD_ALIGNED, 0.05, 0.1, True, 0, False),
    ("three_points", few_points(3), 3, LOCAL_WORLD_ALIGNED, 0.1, 0.3, True, 0, False),
    ("two_points", few_points(2), 2, LOCAL_WORLD_ALIGNED, 0.1, 0.3, True, 0, False),
    ("one_point", few_points(1), 1, LOCAL, 0.1, 0.3, True, 0, False),
    ("exact_ties", tie_points, 8, LOCAL_WORLD_ALIGNED, 0.125, 0.25, True, 0, True),
    ("polygon_only", random_points(7), 7, LOCAL, 0.0, 0.0, False, 0, False),
)


def main(out_path: str, verbose: bool = True) -> None:
    ref = load_reference_functions()
    rg = np.random.default_rng(SEED)
    out: dict = {}
    for label, *args in CASES:
        for k, v in make_case(ref, rg, *args).items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array([c[0] for c in CASES])
    out["tier"] = np.array("A: the reference's hull, distance, sigmoid and odometry translation functions on the arrays they are "
                           "written for; the refresh bodies, ConvexHull2D's constructor, center and degenerate distances are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(COMMON) or not os.path.isdir(TOOLBOX):
        sys.exit(f"{COMMON} or {TOOLBOX} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_support.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_support.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
