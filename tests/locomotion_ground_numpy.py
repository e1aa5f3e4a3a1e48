"""An authored numpy statement of what the locomotion quantities block computes on height-map ground (tests only), vectorised
over the lanes in the arithmetic of a given dtype (float64, float32): a second statement next to the reference's own output
(tests/golden/ref_locomotion_ground.npz) and the yardstick of the float32 tolerance.

`plan`, `inputs`: those of tests/locomotion_numpy.py.  `ground`: None (flat ground) or heights `[ny][nx]`, x0, y0, dx, dy and
offsets `[2][B]` (optional), the arguments of `set_ground_heightmap` / `set_ground_offsets`.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from tests import locomotion_numpy as ln

INPUTS = ln.INPUTS
OUTPUTS = ln.OUTPUTS + ("contact_ground",)
GROUND_KEYS = ("heights", "x0", "y0", "dx", "dy", "offsets")


def output_shape(name: str, plan: Dict, B: int) -> tuple:
    if name == "contact_ground":
        return (4, len(plan["contact_foot"]), B)
    return ln.output_shape(name, plan, B)


def load_case(npz, label: str):
    """`plan`, `inputs`, `ground`, `expected` and the designed contacts `[nc][B]` of one case of
    tests/golden/ref_locomotion_ground.npz."""
    pre = label + "."
    keys = [k[len(pre):] for k in npz.files if k.startswith(pre)]
    plan = {k[5:]: npz[pre + k] for k in keys if k.startswith("plan.")}
    plan = {k: (v if v.ndim else v.item()) for k, v in plan.items()}
    inputs = {k: npz[pre + k] for k in keys if k in INPUTS}
    ground = {k[7:]: npz[pre + k] for k in keys if k.startswith("ground.")}
    ground = {k: (v if v.ndim else v.item()) for k, v in ground.items()}
    expected = {k[9:]: npz[pre + k] for k in keys if k.startswith("expected.")}
    return plan, inputs, ground, expected, npz[pre + "designed"]


def grid_coordinates(ground: Dict, x, y, dtype=np.float64):
    """Grid coordinates (u, w) of world points, offsets already added, as the kernel computes them."""
    dtype = np.dtype(dtype).type
    return (x - dtype(ground["x0"])) / dtype(ground["dx"]), (y - dtype(ground["y0"])) / dtype(ground["dy"])


def ground_profile(ground: Dict, x, y, dtype=np.float64):
    """Height and unit normal `[3][...]` of the bilinear patches with flat continuation under (x, y)."""
    dtype = np.dtype(dtype).type
    H = np.asarray(ground["heights"], dtype=dtype)
    ny, nx = H.shape
    dx, dy, one, zero = dtype(ground["dx"]), dtype(ground["dy"]), dtype(1), dtype(0)
    u, w = grid_coordinates(ground, x, y, dtype)
    in_x, in_y = (u >= 0) & (u <= nx - 1), (w >= 0) & (w <= ny - 1)
    u, w = np.minimum(np.maximum(u, zero), dtype(nx - 1)), np.minimum(np.maximum(w, zero), dtype(ny - 1))
    ix, iy = np.clip(u.astype(np.int64), 0, nx - 2), np.clip(w.astype(np.int64), 0, ny - 2)
    fx, fy = u - ix.astype(dtype), w - iy.astype(dtype)
    h00, h10, h01, h11 = H[iy, ix], H[iy, ix + 1], H[iy + 1, ix], H[iy + 1, ix + 1]
    h = (one - fy) * ((one - fx) * h00 + fx * h10) + fy * ((one - fx) * h01 + fx * h11)
    dhdx = np.where(in_x, ((one - fy) * (h10 - h00) + fy * (h11 - h01)) / dx, zero)
    dhdy = np.where(in_y, ((one - fx) * (h01 - h00) + fx * (h11 - h10)) / dy, zero)
    inv = one / np.sqrt(dhdx * dhdx + dhdy * dhdy + one)
    return h, np.stack([-dhdx * inv, -dhdy * inv, inv])


def vertical_transform(n):
    """Third row (t0_z, t1_z, n_z) of `rotationLocal_` = [t0 t1 n]: t1 = (0, n_z, -n_y) / |.|, t0 = t1 x n."""
    inv = 1 / np.sqrt(n[2] * n[2] + n[1] * n[1])
    t1x, t1y, t1z = np.zeros_like(n[2]), n[2] * inv, -n[1] * inv
    return np.stack([t1x * n[1] - t1y * n[0], t1z, n[2]]).astype(n.dtype)


def robot_weight(plan: Dict, inp: Dict, B: int, dtype):
    """The weight as tests/locomotion_numpy.py forms it."""
    ml = inp.get("model_lane")
    if ml is None:
        mass64 = 0.0
        for m in np.asarray(plan["body_mass"], dtype=np.float64)[1:]:
            mass64 += float(m)
        mass = np.full(B, dtype(mass64))
    else:
        mass = np.zeros(B, dtype=dtype)
        for j in range(1, ml.shape[0] // 13):
            mass = mass + ml[13 * j]
    return mass * dtype(plan["gravity"])


def quantities(plan: Dict, inputs: Dict, ground: Optional[Dict] = None, dtype=np.float64) -> Dict[str, np.ndarray]:
    out = ln.quantities(plan, inputs, dtype)
    dtype = np.dtype(dtype).type
    nc, n_feet = len(plan["contact_foot"]), int(plan["n_feet"])
    B = inputs["centroidal"].shape[-1]
    flat = np.zeros((4, nc, B), dtype=dtype)
    flat[3] = 1
    out["contact_ground"] = flat
    if ground is None or ground.get("heights") is None:
        return out
    pose = np.asarray(inputs["pose"], dtype=dtype)[:, [int(k) for k in plan["contact_column"]]]
    x, y, z = pose[0], pose[1], pose[2]
    if ground.get("offsets") is not None:
        off = np.asarray(ground["offsets"], dtype=dtype)
        x, y = x + off[0], y + off[1]
    h, n = ground_profile(ground, x, y, dtype)
    out["contact_ground"] = np.concatenate([h[None], n])
    weight = robot_weight(plan, {k: np.asarray(v, dtype=dtype) for k, v in inputs.items() if k == "model_lane"}, B, dtype)
    lam = np.asarray(inputs["con_lambda"], dtype=dtype).reshape(nc, 4, B) * ((inputs["con_flags"] & 1) != 0)[:, None, :].astype(dtype)
    row = vertical_transform(n)
    foot = np.zeros((n_feet, B), dtype=dtype)
    for k, f in enumerate(plan["contact_foot"]):
        if f >= 0:
            foot[f] = foot[f] + (row[0, k] * lam[k, 0] + row[1, k] * lam[k, 1] + row[2, k] * lam[k, 2])
    out["foot_force_vertical"] = foot / weight
    out["scalars"] = out["scalars"].copy()
    out["scalars"][1] = ((z - h) * n[2]).min(0)
    assert all(v.dtype == dtype for v in out.values())
    return out
