"""Numpy restatement of the projected support polygon block (csrc/jm_support.h), lane by lane and in the dtype asked for: the
yardstick of the float32 comparisons and the host composition of the block-law tests.  It follows the reference's text
(toolbox/math/qhull.py, toolbox/quantities/locomotion.py:146-239, toolbox/compositions/locomotion.py:15-48) with Python lists
and numpy's own stable sorts, not the kernel's rank count and packed registers.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

CUTOFF_ESP = 1.0e-2
MAX_POINTS = 16
LOCAL, LOCAL_WORLD_ALIGNED = 0, 1
INPUTS = ("pose", "odom_pose", "zmp")
OUTPUTS = ("n_vertices", "vertex_index", "vertices", "center", "scalars")
INT_OUTPUTS = ("n_vertices", "vertex_index")


def output_shape(name: str, plan: Dict, B: int) -> tuple:
    return {"n_vertices": (B,), "vertex_index": (MAX_POINTS, B), "vertices": (2, MAX_POINTS, B), "center": (2, B), "scalars": (2, B)}[name]


def load_case(npz, label: str):
    """`plan`, `inputs`, `expected` of one case of tests/golden/ref_support.npz."""
    pre = label + "."
    keys = [k[len(pre):] for k in npz.files if k.startswith(pre)]
    plan = {k[5:]: npz[pre + k] for k in keys if k.startswith("plan.")}
    plan = {k: (v if v.ndim else v.item()) for k, v in plan.items()}
    inputs = {k: npz[pre + k] for k in keys if k in INPUTS}
    expected = {k[9:]: npz[pre + k] for k in keys if k.startswith("expected.")}
    return plan, inputs, expected


def hull_vertices(points: np.ndarray) -> list:
    """`compute_convex_hull_vertices` (math/qhull.py:71-123) on `[n][2]` points of any float dtype."""
    order = np.argsort(points[:, 0], kind="mergesort")
    order = order[np.argsort(points[order, 1], kind="mergesort")]
    if len(points) <= 3:
        return [int(i) for i in order]
    vertices: list = []
    for sequence in (order[::-1], order):
        chain: list = []
        for i in sequence:
            p = points[i]
            while len(chain) > 1:
                a, b = points[chain[-2]], points[chain[-1]]
                if (b[0] - a[0]) * (p[1] - a[1]) > (p[0] - a[0]) * (b[1] - a[1]):
                    break
                chain.pop()
                vertices.pop()
            if chain:
                vertices.append(int(i))
            chain.append(int(i))
    return vertices


def distance_to_point(n_points: int, vertices: np.ndarray, query: np.ndarray):
    """`ConvexHull2D.get_distance_to_point` (:416-457) of one query; the branch is on the number of points."""
    dtype = vertices.dtype
    zero, one = dtype.type(0), dtype.type(1)
    if n_points > 2:
        vectors = np.concatenate([vertices[-1:] - vertices[:1], vertices[:-1] - vertices[1:]])
        rel = query[None, :] - vertices
        inside = bool(np.all(rel[:, 0] * vectors[:, 1] > rel[:, 1] * vectors[:, 0]))
        ratios = np.sum(rel * vectors, axis=1) / np.sum(np.square(vectors), axis=1)
        ratios = np.minimum(np.maximum(ratios, zero), one)
        projs = ratios[:, None] * vectors + vertices
        dist = np.sqrt(np.min(np.sum(np.square(query[None, :] - projs), axis=1)))
        return (one - dtype.type(2) * dtype.type(inside)) * dist
    if n_points == 2:
        vec = vertices[1] - vertices[0]
        ratio = np.sum((query - vertices[0]) * vec) / np.sum(vec * vec)
        proj = vertices[0] + np.minimum(np.maximum(ratio, zero), one) * vec
        return np.sqrt(np.sum(np.square(query - proj)))
    return np.sqrt(np.sum(np.square(query - vertices[0])))


def sigmoid_normalization(value, cutoff_low, cutoff_high):
    """`sigmoid_normalization(..., is_asymmetric=True)` (compositions/locomotion.py:39-48) in the dtype of `value`."""
    t = type(value)
    value_rel = value / cutoff_high if value * cutoff_high > 0 else - value / cutoff_low
    with np.errstate(all="ignore"):
        factor = np.power(t(CUTOFF_ESP) / (t(1) - t(CUTOFF_ESP)), np.abs(value_rel))
        return t(1) / (t(1) + factor) if value_rel > 0 else factor / (t(1) + factor)


def lane_points(plan: Dict, pose_xy: np.ndarray, odom_pose) -> np.ndarray:
    """The candidate points `[n][2]` of one lane; `pose_xy`: rows 0 and 1 of the lane's `pose`, `[2][K]`."""
    points = np.ascontiguousarray(pose_xy[:, [int(c) for c in plan["point_column"]]].T)
    if int(plan["reference_frame"]) == LOCAL:
        # `translate_position_odom` (common/quantities/locomotion.py:904-910)
        rel = points - odom_pose[None, :2]
        cos_yaw, sin_yaw = np.cos(odom_pose[2]), np.sin(odom_pose[2])
        points = np.stack([cos_yaw * rel[:, 0] + sin_yaw * rel[:, 1], - sin_yaw * rel[:, 0] + cos_yaw * rel[:, 1]], axis=1)
    return points


def quantities(plan: Dict, inputs: Dict, dtype=np.float64, cutoff_inner=None, cutoff_outer=None) -> Dict[str, np.ndarray]:
    """Every output the inputs allow, `[rows][B]`; the float ones in `dtype`."""
    dtype = np.dtype(dtype)
    pose = np.asarray(inputs["pose"], dtype=dtype)
    B = pose.shape[-1]
    odom = np.asarray(inputs["odom_pose"], dtype=dtype) if "odom_pose" in inputs else None
    zmp = np.asarray(inputs["zmp"], dtype=dtype) if inputs.get("zmp") is not None else None
    ci = dtype.type(plan.get("cutoff_inner", 0.0) if cutoff_inner is None else cutoff_inner)
    co = dtype.type(plan.get("cutoff_outer", 0.0) if cutoff_outer is None else cutoff_outer)
    out = {"n_vertices": np.zeros(B, np.int32), "vertex_index": np.full((MAX_POINTS, B), -1, np.int32),
           "vertices": np.full((2, MAX_POINTS, B), np.nan, dtype), "center": np.zeros((2, B), dtype)}
    if zmp is not None:
        out["scalars"] = np.zeros((2, B), dtype)
    for b in range(B):
        points = lane_points(plan, pose[:2, :, b], None if odom is None else odom[:, b])
        index = hull_vertices(points)
        vertices = points[index]
        nv = len(index)
        out["n_vertices"][b] = nv
        out["vertex_index"][:nv, b] = index
        out["vertices"][:, :nv, b] = vertices.T
        total = vertices[0].copy()
        for v in vertices[1:]:
            total = total + v
        out["center"][:, b] = total / dtype.type(nv)
        if zmp is None:
            continue
        with np.errstate(all="ignore"):
            margin = dtype.type(-np.inf) if np.isnan(zmp[0, b]) else - distance_to_point(len(points), vertices, zmp[:, b])
        out["scalars"][0, b] = margin
        if ci > 0 and co > 0:
            out["scalars"][1, b] = sigmoid_normalization(margin, -co, ci)
    return out
