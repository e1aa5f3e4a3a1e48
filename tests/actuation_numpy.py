"""An authored numpy statement of what the actuated-joint quantities block computes (tests only), vectorised over the lanes in
the arithmetic of a given dtype (float64, float32): a second statement next to the reference's own output
(tests/golden/ref_actuation.npz), the expected value of the float32 tests and the home of the derived error bounds.

`plan`: idx_q, idx_v, reduction, position_low, position_high, nq, nv, generator_mode, max_stack, and the launch scalars of a
fixture case: motor_side, position_margin, velocity_max, power_cutoff.  `inputs`: q `[nq][B]`, v, a `[nv][B]`, command `[M][B]`.

A fixture case is a sequence of launches ("events"): `mode [E]` (0 restart, 1 push), `mask [E][B]`, the inputs `v`, `command`
per event (`q` and `a` are the same for every event of a case), and under `expected.` the tensors of the block after every
event -- a lane that an event's mask leaves out keeps what it had.  `position`, `acceleration`, `bound_low` and `bound_high`
follow `q` and `a` and are stored once.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

CUTOFF_ESP = 1.0e-2
CHARGE, LOST_EACH, LOST_GLOBAL, PENALIZE = range(4)
RESTART, PUSH = 0, 1
POWER, POWER_AVERAGE, REWARD_POWER = range(3)
INPUTS = ("q", "v", "a", "command")
PER_EVENT_INPUTS = ("v", "command")
KINEMATICS = ("position", "velocity", "acceleration", "bound_low", "bound_high")
OUTPUTS = KINEMATICS + ("safety", "scalars")
STATE = ("power_ring", "power_count")
CONSTANT_OUTPUTS = ("position", "acceleration", "bound_low", "bound_high")
PLAN_KEYS = ("idx_q", "idx_v", "reduction", "position_low", "position_high", "nq", "nv", "generator_mode", "max_stack")


def output_shape(name: str, plan: Dict, B: int) -> tuple:
    if name in KINEMATICS:
        return (len(plan["idx_q"]), B)
    return {"safety": (B,), "scalars": (3, B), "power_ring": (int(plan["max_stack"]), B), "power_count": (B,)}[name]


def output_dtype(name: str, dtype):
    return np.dtype(np.int32) if name in ("safety", "power_count") else np.dtype(dtype)


def load_case(npz, label: str):
    """`plan`, the inputs, `mode [E]`, `mask [E][B]` and `expected` of one case of tests/golden/ref_actuation.npz.  A case that
    names a `base` takes from it whatever it does not hold itself."""
    def keys_of(lab):
        pre = lab + "."
        return {k[len(pre):]: npz[k] for k in npz.files if k.startswith(pre)}
    own = keys_of(label)
    if "base" in own:
        own = {**keys_of(str(own.pop("base"))), **own}
    plan = {k[5:]: (v if v.ndim else v.item()) for k, v in own.items() if k.startswith("plan.")}
    inputs = {k: own[k] for k in INPUTS}
    expected = {k[9:]: v for k, v in own.items() if k.startswith("expected.")}
    return plan, inputs, own["mode"], own["mask"], expected


def event_inputs(inputs: Dict, e: int) -> Dict:
    return {k: (v[e] if k in PER_EVENT_INPUTS else v) for k, v in inputs.items()}


def new_state(plan: Dict, B: int, dtype=np.float64) -> Dict[str, np.ndarray]:
    return {"power_ring": np.zeros((int(plan["max_stack"]), B), dtype=dtype), "power_count": np.zeros(B, dtype=np.int32)}


def motor_powers(plan: Dict, inputs: Dict, dtype=np.float64) -> np.ndarray:
    """`[M][B]`: (v * reduction) * effort of every motor, in the arithmetic of `dtype`."""
    dtype = np.dtype(dtype).type
    v = np.asarray(inputs["v"], dtype=dtype)[np.asarray(plan["idx_v"], dtype=int)]
    ratio = np.asarray(plan["reduction"], dtype=np.float64).astype(dtype)[:, None]
    return (v * ratio) * np.asarray(inputs["command"], dtype=dtype)


def power(plan: Dict, inputs: Dict, dtype=np.float64) -> np.ndarray:
    """`compute_power` per lane: a running sum in motor order."""
    dtype = np.dtype(dtype).type
    p = motor_powers(plan, inputs, dtype)
    mode = int(plan["generator_mode"])
    if mode == LOST_EACH:
        p = np.maximum(p, dtype(0))
    elif mode == PENALIZE:
        p = np.abs(p)
    total = np.zeros(p.shape[1], dtype=dtype)
    for m in range(p.shape[0]):
        total = total + p[m]
    if mode == LOST_GLOBAL:
        total = np.where(total < 0, dtype(0), total)
    return total


def quantities(plan: Dict, inputs: Dict, state: Dict[str, np.ndarray], mode: int, mask: Optional[np.ndarray] = None,
               dtype=np.float64, motor_side=None, position_margin=None, velocity_max=None, power_cutoff=None
               ) -> Dict[str, np.ndarray]:
    """One launch.  Returns every output for every lane; `state` (ring and counter) is updated in place on the lanes of
    `mask` (all without one), and the rows of `scalars` that read it are meaningful on those lanes only."""
    dtype = np.dtype(dtype).type
    motor_side = bool(plan["motor_side"] if motor_side is None else motor_side)
    margin = dtype(plan["position_margin"] if position_margin is None else position_margin)
    vmax = dtype(plan["velocity_max"] if velocity_max is None else velocity_max)
    cutoff = dtype(plan["power_cutoff"] if power_cutoff is None else power_cutoff)
    iq, iv = np.asarray(plan["idx_q"], dtype=int), np.asarray(plan["idx_v"], dtype=int)
    ratio = np.asarray(plan["reduction"], dtype=np.float64).astype(dtype)[:, None]
    low = np.asarray(plan["position_low"], dtype=np.float64).astype(dtype)[:, None]
    high = np.asarray(plan["position_high"], dtype=np.float64).astype(dtype)[:, None]
    q, v, a = (np.asarray(inputs[k], dtype=dtype) for k in ("q", "v", "a"))
    B = q.shape[-1]
    mask = np.ones(B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    qj, vj, aj = q[iq], v[iv], a[iv]
    out = {"position": qj * ratio if motor_side else qj.copy(), "velocity": vj * ratio if motor_side else vj.copy(),
           "acceleration": aj * ratio if motor_side else aj.copy(), "bound_low": qj - low, "bound_high": high - qj}
    unsafe = ((out["bound_low"] < margin) & (vj < -vmax)) | ((out["bound_high"] < margin) & (vj > vmax))
    out["safety"] = unsafe.sum(0).astype(np.int32)
    p = power(plan, inputs, dtype)
    S = int(plan["max_stack"])
    ring, count = state["power_ring"], state["power_count"]
    assert ring.dtype == dtype and ring.shape == (S, B)
    new_count = np.zeros(B, dtype=np.int32) if mode == RESTART else count + 1
    slot = new_count % S
    lanes = np.flatnonzero(mask)
    count[lanes] = new_count[lanes]
    ring[slot[lanes], lanes] = p[lanes]
    n = np.minimum(count + 1, S)
    total = np.zeros(B, dtype=dtype)
    for k in range(S):       # (storage order, as `np.sum` of a short array)
        total = np.where(k < n, total + ring[k], total)
    average = total / n.astype(dtype)
    scalars = np.zeros((3, B), dtype=dtype)
    scalars[POWER], scalars[POWER_AVERAGE] = p, average
    if cutoff > 0:
        scalars[REWARD_POWER] = np.power(dtype(CUTOFF_ESP), (average * average) / np.power(cutoff, dtype(2)))
    out["scalars"] = scalars
    assert all(v_.dtype == output_dtype(k, dtype) for k, v_ in out.items())
    return out


def replay(plan: Dict, inputs: Dict, modes, masks, dtype=np.float64, step=None):
    """Every event of a case through `step(inputs of the event, state, mode, mask) -> outputs` (default: `quantities`), with
    the carry-over of the lanes an event leaves out.  Returns `[E]`-stacked outputs and states like the fixture's `expected`."""
    B = inputs["q"].shape[-1]
    state = new_state(plan, B, dtype)
    if step is None:
        step = lambda inp, st, mode, mask: quantities(plan, inp, st, mode, mask, dtype)      # noqa: E731
    held, rows = None, []
    for e, (mode, mask) in enumerate(zip(modes, masks)):
        got = step(event_inputs(inputs, e), state, int(mode), np.asarray(mask, dtype=bool))
        if held is None:
            assert np.all(mask), "the first event of a case launches every lane"
            held = {k: np.array(v) for k, v in got.items()}
        else:
            for k, v in got.items():
                held[k][..., mask] = v[..., mask]
        rows.append({**{k: v.copy() for k, v in held.items()}, **{k: v.copy() for k, v in state.items()}})
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# ---------------------------------------------------------------------------------------------------- the derived bounds
def power_bound(plan: Dict, inputs: Dict, eps: float) -> np.ndarray:
    """|got - want| <= 4 (M + 2) eps sum_m |v_m r_m e_m|: two roundings per term and M - 1 of the sum on either side
    (contraction and the order of a BLAS dot stay inside), factor 2 for the two sides, factor 2 margin."""
    p = np.abs(motor_powers(plan, inputs, np.float64))
    return 4.0 * (p.shape[0] + 2) * eps * p.sum(0)


def average_bound(power_bounds: np.ndarray, powers: np.ndarray, n: np.ndarray, eps: float) -> np.ndarray:
    """`power_bounds`, `powers` `[S][B]`: the bound and the value of every slot of the ring, `n [B]` the entries in use: the
    mean of the n per-entry bounds plus 2 n eps mean_k |p_k|."""
    use = np.arange(powers.shape[0])[:, None] < n[None, :]
    return np.where(use, power_bounds, 0.0).sum(0) / n + 2.0 * n * eps * np.where(use, np.abs(powers), 0.0).sum(0) / n


def reward_bound(reward: np.ndarray, average: np.ndarray, bound_average: np.ndarray, cutoff: float, eps: float) -> np.ndarray:
    """r ln(100) 2 |avg| bound_avg / cutoff^2 + 8 eps."""
    return reward * np.log(100.0) * 2.0 * np.abs(average) * bound_average / cutoff ** 2 + 8.0 * eps


def scalar_bounds(plan: Dict, inputs: Dict, modes, masks, expected_scalars: np.ndarray, eps: float) -> np.ndarray:
    """`[E][3][B]`: the bounds of the three rows of `scalars` after every event of a case, from float64 values."""
    B = inputs["q"].shape[-1]
    S = int(plan["max_stack"])
    ring_b, ring_p, count = np.zeros((S, B)), np.zeros((S, B)), np.zeros(B, dtype=int)
    held = np.zeros((3, B))
    out = []
    for e, (mode, mask) in enumerate(zip(modes, masks)):
        mask = np.asarray(mask, dtype=bool)
        inp = event_inputs(inputs, e)
        pb, p = power_bound(plan, inp, eps), power(plan, inp, np.float64)
        lanes = np.flatnonzero(mask)
        count[lanes] = 0 if int(mode) == RESTART else count[lanes] + 1
        ring_b[count[lanes] % S, lanes], ring_p[count[lanes] % S, lanes] = pb[lanes], p[lanes]
        ab = average_bound(ring_b, ring_p, np.minimum(count + 1, S), eps)
        rb = reward_bound(expected_scalars[e][REWARD_POWER], expected_scalars[e][POWER_AVERAGE], ab, float(plan["power_cutoff"]), eps)
        now = np.stack([pb, ab, rb])
        held[:, mask] = now[:, mask]
        out.append(held.copy())
    return np.stack(out)
