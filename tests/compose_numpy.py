"""The composition layer (csrc/jm_compose.h) restated in numpy, lane by lane, in the scalar type asked for (tests only).

A plan is the dictionary of the arrays of `jm_compose_desc` (include/jiminy_hip.h); the inputs are `sources` (one array
`[rows][B]` per slot), `time`, `base_terminated`, `base_truncated` and `training`.  `load_case` reads both from the fixture
tests/golden/ref_compositions.npz."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

LEAF, SURVIVE, ADDITIVE, MULTIPLICATIVE = 0, 1, 2, 3
SRC_DTYPE, SRC_INT32, SRC_UINT8 = 0, 1, 2
COND_ARRAY, COND_TRUNCATION, COND_TRAINING_ONLY = 1, 2, 4
HAS_LOW, HAS_HIGH = 1, 2
PLAN_KEYS = ("source_kind", "source_rows", "node_kind", "node_terminal", "node_normalized", "node_slot", "node_row", "node_child_start",
             "node_child_count", "node_order", "child", "child_weight", "cond_elem_start", "cond_elem_count", "cond_flags", "cond_grace",
             "elem_slot", "elem_row", "elem_bounds", "elem_low", "elem_high")
OUTPUTS = ("reward", "node_value", "terminated", "truncated", "trigger", "violations")
FLOAT_OUTPUTS = ("reward", "node_value")
OUTPUT_DTYPES = dict(terminated=np.uint8, truncated=np.uint8, trigger=np.int32, violations=np.int32)
SOURCE_DTYPES = {SRC_INT32: np.int32, SRC_UINT8: np.uint8}


def load_case(fx, name: str) -> Tuple[Dict, Dict, Dict]:
    """plan, inputs and expected outputs of a fixture case (`expected['compare']`: the lanes whose values are compared)."""
    plan = {k: fx[f"{name}.plan.{k}"] for k in PLAN_KEYS}
    plan["node_names"] = [str(n) for n in fx[f"{name}.node_names"]]
    plan["condition_names"] = [str(n) for n in fx[f"{name}.condition_names"]]
    inputs = dict(sources=[fx[f"{name}.source{s}"] for s in range(len(plan["source_kind"]))], time=fx[f"{name}.time"],
                  base_terminated=fx[f"{name}.base_terminated"], base_truncated=fx[f"{name}.base_truncated"],
                  training=bool(fx[f"{name}.training"]))
    expected = {k: fx[f"{name}.expected.{k}"] for k in OUTPUTS}
    expected["compare"] = fx[f"{name}.compare"]
    return plan, inputs, expected


def cast_sources(plan: Dict, sources: List[np.ndarray], dtype) -> List[np.ndarray]:
    """The sources in the element kind of their slot (`dtype` for the engine-dtype slots)."""
    return [np.ascontiguousarray(a, dtype=SOURCE_DTYPES.get(int(k), dtype)) for k, a in zip(plan["source_kind"], sources)]


def output_shape(name: str, plan: Dict, B: int) -> tuple:
    return (len(plan["node_kind"]), B) if name == "node_value" else (B,)


def quantities(plan: Dict, inputs: Dict, dtype=np.float64, training: Optional[bool] = None) -> Dict[str, np.ndarray]:
    T = np.dtype(dtype).type
    sources = cast_sources(plan, inputs["sources"], dtype)
    B = sources[0].shape[-1]
    training = inputs["training"] if training is None else training
    time = np.asarray(inputs["time"], dtype=dtype)
    n_nodes = len(plan["node_kind"])
    out = dict(reward=np.zeros(B, dtype), node_value=np.full((n_nodes, B), np.nan, dtype), terminated=np.zeros(B, np.uint8),
               truncated=np.zeros(B, np.uint8), trigger=np.full(B, -1, np.int32), violations=np.zeros(B, np.int32))
    read = lambda slot, row, b: T(sources[slot][row, b])        # noqa: E731

    def node(n: int, terminated: bool, b: int, state: dict):
        """(value, evaluated) of node n ≙ `AbstractReward.__call__`."""
        kind = int(plan["node_kind"][n])
        if (int(plan["node_terminal"][n]) == 1) != terminated:
            return T(0), False
        if kind == LEAF:
            value = read(int(plan["node_slot"][n]), int(plan["node_row"][n]), b)
        elif kind == SURVIVE:
            value = T(1)
        else:
            start, count = int(plan["node_child_start"][n]), int(plan["node_child_count"][n])
            order = float(plan["node_order"][n])
            total, n_values = T(0) if kind == ADDITIVE else T(1), 0
            for k in range(start, start + count):
                v, ok = node(int(plan["child"][k]), terminated, b, state)
                if not ok:
                    continue
                if kind == ADDITIVE:
                    w = T(plan["child_weight"][k])
                    if np.isinf(order):
                        x = w * v
                        total = x if (n_values == 0 or x > total) else total
                    else:
                        total = total + w * np.power(v, T(order))
                else:
                    total = total * v
                n_values += 1
            if n_values == 0:
                return T(0), False
            if kind == ADDITIVE:
                value = total if np.isinf(order) else np.power(total, T(1.0 / order))
            else:
                value = np.power(total, T(1.0 / n_values))
        if plan["node_normalized"][n] and (value < 0 or value > 1) and state["violations"] == 0:
            state["violations"] = 1 << n
        out["node_value"][n, b] = value
        return value, True

    for b in range(B):
        terminated, truncated, trigger = bool(inputs["base_terminated"][b]), bool(inputs["base_truncated"][b]), -1
        if not (terminated or truncated):
            for c in range(len(plan["cond_flags"])):
                flags = int(plan["cond_flags"][c])
                if ((flags & COND_TRAINING_ONLY) and not training) or time[b] < T(plan["cond_grace"][c]):
                    continue
                fired = False
                for e in range(int(plan["cond_elem_start"][c]), int(plan["cond_elem_start"][c]) + int(plan["cond_elem_count"][c])):
                    v = read(int(plan["elem_slot"][e]), int(plan["elem_row"][e]), b)
                    bounds, low, high = int(plan["elem_bounds"][e]), T(plan["elem_low"][e]), T(plan["elem_high"][e])
                    if flags & COND_ARRAY:
                        fired |= bool((bounds & HAS_LOW) and not low <= v) or bool((bounds & HAS_HIGH) and not v <= high)
                    else:
                        fired |= bool((bounds & HAS_LOW) and low > v) or bool((bounds & HAS_HIGH) and v > high)
                if fired:
                    terminated = not flags & COND_TRUNCATION
                    truncated, trigger = not terminated, c
                    break
        out["terminated"][b], out["truncated"][b], out["trigger"][b] = terminated, truncated, trigger
        if n_nodes:
            state = dict(violations=0)
            with np.errstate(invalid="ignore"):
                out["reward"][b] = node(0, terminated, b, state)[0]
            out["violations"][b] = np.array(state["violations"], dtype=np.uint32).astype(np.int32)
    return out
