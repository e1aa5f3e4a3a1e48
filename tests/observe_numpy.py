"""Numpy restatement of the observation assembly (jiminy_amd/csrc/jm_observe.h, jiminy_amd/observe.py), for the tests: the
tables of a plan from a list of kept leaves, and the evaluation of a plan on numpy sources with its rolling history."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_MULTIPLIERS = 4
PLAN_KEYS = ("source_rows", "elem_slot", "elem_row", "elem_mult_start", "elem_mult_count", "elem_mean", "elem_scale", "multiplier",
             "num_stack", "pos_elem", "pos_age")


def make_plan(source_rows: Sequence[int], leaves: Sequence[Dict], num_stack: int) -> Dict:
    """The tables of a plan.  `leaves`, in flat order: `slot`, `rows` (one per element), `mults` (a list of factors per element),
    `mean`, `scale` (per element) and `stacked`.  The flat order is that of `FlattenObservation` over the stacked leaves: a
    stacked leaf is `[num_stack][elements]`, oldest first; another leaf appears once."""
    plan: Dict = {k: [] for k in PLAN_KEYS}
    plan["source_rows"], plan["num_stack"] = [int(r) for r in source_rows], int(num_stack)
    for leaf in leaves:
        e0, n = len(plan["elem_slot"]), len(leaf["rows"])
        for j in range(n):
            plan["elem_slot"].append(int(leaf["slot"]))
            plan["elem_row"].append(int(leaf["rows"][j]))
            plan["elem_mult_start"].append(len(plan["multiplier"]))
            plan["elem_mult_count"].append(len(leaf["mults"][j]))
            plan["multiplier"] += [float(f) for f in leaf["mults"][j]]
            plan["elem_mean"].append(float(leaf["mean"][j]))
            plan["elem_scale"].append(float(leaf["scale"][j]))
        stacked = bool(leaf["stacked"]) and num_stack > 1
        for frame in range(num_stack if stacked else 1):
            plan["pos_elem"] += list(range(e0, e0 + n))
            plan["pos_age"] += [num_stack - 1 - frame if stacked else 0] * n
    return plan


def stacked_elements(plan: Dict) -> np.ndarray:
    count = np.bincount(np.asarray(plan["pos_elem"]), minlength=len(plan["elem_slot"]))
    return (count == plan["num_stack"]) & (plan["num_stack"] > 1)


def current_values(plan: Dict, sources: Sequence[np.ndarray], dtype_in) -> np.ndarray:
    """`[D][B]`: every element read, multiplied by its chain (padded with 1.0 to 4 factors, each product rounded in `dtype_in`)
    and normalised, `(x - mean) / scale`."""
    dtype_in = np.dtype(dtype_in).type
    D, B = len(plan["elem_slot"]), sources[0].shape[-1]
    out = np.empty((D, B), dtype=dtype_in)
    for e in range(D):
        x = np.asarray(sources[plan["elem_slot"][e]], dtype=dtype_in).reshape(-1, B)[plan["elem_row"][e]].copy()
        start, count = plan["elem_mult_start"][e], plan["elem_mult_count"][e]
        for f in list(plan["multiplier"][start:start + count]) + [1.0] * (MAX_MULTIPLIERS - count):
            x = x * dtype_in(f)
        out[e] = (x - dtype_in(plan["elem_mean"][e])) / dtype_in(plan["elem_scale"][e])
    return out


def evaluate(plan: Dict, sources: Sequence[np.ndarray], hist: np.ndarray, shift: bool = True, reset_mask: Optional[np.ndarray] = None,
             dtype_in=np.float64, dtype_out=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """One launch: `(out [B][W], the history after it [num_stack][D][B])`.  The rows of an element that is not stacked stay as
    they are in the history."""
    S, D, W = plan["num_stack"], len(plan["elem_slot"]), len(plan["pos_elem"])
    B = sources[0].shape[-1]
    assert hist.shape == (S, D, B) and hist.dtype == np.dtype(dtype_in)
    value = current_values(plan, sources, dtype_in)
    stacked = stacked_elements(plan)
    frames = hist.copy()
    if shift:
        frames[:-1] = hist[1:]
    if reset_mask is not None:
        frames[:-1][:, :, np.asarray(reset_mask, dtype=bool)] = 0
    frames[-1] = value
    new_hist = hist.copy()
    new_hist[:, stacked] = frames[:, stacked]
    out = np.empty((B, W), dtype=dtype_out)
    for p in range(W):
        out[:, p] = frames[S - 1 - plan["pos_age"][p], plan["pos_elem"][p]].astype(dtype_out)
    return out, new_hist


def synthetic_case(B: int, D: int, num_stack: int, seed: int = 0) -> Tuple[Dict, List[np.ndarray]]:
    """3 sources (float64 `[rows][B]`), leaves of a few elements each that alternate between stacked and not, rows in a shuffled
    order, multiplier chains of length 0, 1 and 4, and every third leaf normalised."""
    rng = np.random.default_rng(seed + 1000 * B + D)
    source_rows = [max(1, D // 2), D + 3, 2]
    sources = [rng.uniform(-2.0, 2.0, (r, B)) for r in source_rows]
    leaves, e = [], 0
    while e < D:
        n = min(D - e, int(rng.integers(1, 8)))
        slot = len(leaves) % 3
        leaves.append(dict(slot=slot, rows=rng.integers(0, source_rows[slot], n),
                           mults=[list(rng.uniform(0.5, 3.0, (0, 1, 4)[(e + j) % 3])) for j in range(n)],
                           mean=rng.uniform(-1, 1, n) if len(leaves) % 3 == 0 else np.zeros(n),
                           scale=rng.uniform(0.5, 2, n) if len(leaves) % 3 == 0 else np.ones(n),
                           stacked=len(leaves) % 2 == 0))
        e += n
    return make_plan(source_rows, leaves, num_stack), sources
