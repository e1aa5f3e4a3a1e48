"""An authored numpy statement of what the locomotion quantities block computes (tests only), vectorised over the lanes in
the arithmetic of a given dtype (float64, float32): a second statement next to the reference's own output
(tests/golden/ref_locomotion.npz) and the yardstick of the float32 tolerance.

`plan`: body_mass, root_inertia, gravity, omega, contact_foot, contact_column, n_feet, n_frames, root_column, zmp_frame,
dcm_frame, momentum_cutoff, friction_cutoff.  `inputs`: centroidal `[15][B]`, q_root `[7][B]`, model_lane `[13 nj][B]`
(optional), con_lambda `[4 nc][B]`, con_flags `[nc][B]`, v_avg `[6][K][B]`, quat_no_yaw `[4][K][B]`, pose `[7][K][B]`.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from tests.frames_numpy import quat_apply

LOCAL, LOCAL_WORLD_ALIGNED = 0, 1
CUTOFF_ESP = 1.0e-2
INPUTS = ("centroidal", "q_root", "model_lane", "con_lambda", "con_flags", "v_avg", "quat_no_yaw", "pose")
OUTPUTS = ("com", "vcom", "odom_pose", "zmp", "dcm", "h_angular", "contact_force_rel", "foot_force_vertical", "scalars")
SHAPES = {"com": (3,), "vcom": (3,), "odom_pose": (3,), "zmp": (2,), "dcm": (2,), "h_angular": (3,), "scalars": (4,)}


def output_shape(name: str, plan: Dict, B: int) -> tuple:
    if name == "contact_force_rel":
        return (6, len(plan["contact_foot"]), B)
    if name == "foot_force_vertical":
        return (int(plan["n_feet"]), B)
    return (*SHAPES[name], B)


def load_case(npz, label: str):
    """`plan`, `inputs`, `expected` and the designed NaN lanes of one case of tests/golden/ref_locomotion.npz."""
    pre = label + "."
    keys = [k[len(pre):] for k in npz.files if k.startswith(pre)]
    plan = {k[5:]: npz[pre + k] for k in keys if k.startswith("plan.")}
    plan = {k: (v if v.ndim else v.item()) for k, v in plan.items()}
    inputs = {k: npz[pre + k] for k in keys if k in INPUTS}
    expected = {k[9:]: npz[pre + k] for k in keys if k.startswith("expected.")}
    return plan, inputs, expected, npz[pre + "designed_nan"]


def translate_position_odom(x, y, ref_x, ref_y, yaw):
    rx, ry = x - ref_x, y - ref_y
    cs, sn = np.cos(yaw), np.sin(yaw)
    return cs * rx + sn * ry, -sn * rx + cs * ry


def radial_basis_function(sq_norm, cutoff, dtype):
    return np.power(dtype(CUTOFF_ESP), sq_norm / np.power(dtype(cutoff), dtype(2)))


def quantities(plan: Dict, inputs: Dict, dtype=np.float64) -> Dict[str, np.ndarray]:
    dtype = np.dtype(dtype).type
    inp = {k: (v if k == "con_flags" else np.asarray(v, dtype=dtype)) for k, v in inputs.items()}
    c, q = inp["centroidal"], inp["q_root"]
    B = c.shape[-1]
    nc, n_feet, root = len(plan["contact_foot"]), int(plan["n_feet"]), int(plan["root_column"])
    ml = inp.get("model_lane")
    if ml is None:
        mass64 = 0.0
        for m in np.asarray(plan["body_mass"], dtype=np.float64)[1:]:
            mass64 += float(m)
        mass = np.full(B, dtype(mass64))
        inertia = [np.full(B, dtype(v)) for v in plan["root_inertia"]]
    else:
        mass = np.zeros(B, dtype=dtype)
        for j in range(1, ml.shape[0] // 13):
            mass = mass + ml[13 * j]
        inertia = [ml[13 + 4 + k] for k in range(6)]
    weight = mass * dtype(plan["gravity"])
    out = {"com": c[0:3].copy(), "vcom": c[3:6] / mass}

    qx, qy, qz, qw = q[3:7]
    yaw = np.arctan2(2 * (qy * qx + qz * qw), 1 - 2 * (qy * qy + qz * qz))
    out["odom_pose"] = np.stack([q[0], q[1], yaw])

    with np.errstate(divide="ignore", invalid="ignore"):
        f_z = c[11] + weight
        ratio = weight / f_z
        zx = c[0] * ratio - (c[13] + c[9] * c[2]) / f_z
        zy = c[1] * ratio + (c[12] - c[10] * c[2]) / f_z
        if plan["zmp_frame"] == LOCAL:
            zx, zy = translate_position_odom(zx, zy, q[0], q[1], yaw)
        free = np.abs(f_z) < dtype(np.finfo(np.float32).eps)
    out["zmp"] = np.where(free, dtype(np.nan), np.stack([zx, zy]))

    omega = dtype(plan["omega"])
    dx, dy = c[0] + out["vcom"][0] / omega, c[1] + out["vcom"][1] / omega
    if plan["dcm_frame"] == LOCAL:
        dx, dy = translate_position_odom(dx, dy, q[0], q[1], yaw)
    out["dcm"] = np.stack([dx, dy])

    xx, xy, xz, yy, yz, zz = inertia
    wx, wy, wz = inp["v_avg"][3:6, root]
    h = np.stack([xx * wx + xy * wy + xz * wz, xy * wx + yy * wy + yz * wz, xz * wx + yz * wy + zz * wz])
    h = quat_apply(inp["quat_no_yaw"][:, root], h)
    out["h_angular"] = h

    lam = inp["con_lambda"].reshape(nc, 4, B) * ((inp["con_flags"] & 1) != 0)[:, None, :].astype(dtype)
    rel = np.zeros((6, nc, B), dtype=dtype)
    rel[0:3] = np.moveaxis(lam[:, 0:3], 0, 1) / weight
    rel[5] = lam[:, 3] / weight
    out["contact_force_rel"] = rel
    foot = np.zeros((n_feet, B), dtype=dtype)
    for k, f in enumerate(plan["contact_foot"]):
        if f >= 0:
            foot[f] = foot[f] + lam[k, 2]
    out["foot_force_vertical"] = foot / weight

    sq_tangential = np.zeros(B, dtype=dtype)
    for k in range(nc):
        sq_tangential = sq_tangential + (rel[0, k] * rel[0, k] + rel[1, k] * rel[1, k])
    z_contacts = inp["pose"][2][[int(k) for k in plan["contact_column"]]]
    out["scalars"] = np.stack([rel[2].max(0), z_contacts.min(0),
                               radial_basis_function(h[0] * h[0] + h[1] * h[1] + h[2] * h[2], plan["momentum_cutoff"], dtype),
                               radial_basis_function(sq_tangential, plan["friction_cutoff"], dtype)])
    assert all(v.dtype == dtype for v in out.values())
    return out
