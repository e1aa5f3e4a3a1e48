"""Reference-pinned fixtures of the composition layer (csrc/jm_compose.h): EXECUTES THE REFERENCE'S OWN PYTHON CLASSES.

Same mechanism and rules as tools/make_ref_support_fixtures.py: this script parses the reference files where they lie, takes the
definitions named in SOURCES (classes and functions, decorators included) and executes them with `numba.jit` stubbed to the
identity.  Nothing of the reference is copied into the repository: only authored descriptions, seeded inputs and the outputs the
reference's code produced for them, written to tests/golden/ref_compositions.npz.

Run where the reference tree is available:   python tools/make_ref_compositions_fixtures.py [output.npz]
                                             python tools/make_ref_compositions_fixtures.py --check     (regenerate and compare)

Tier A for the whole composition logic: `AbstractReward.__call__`, `QuantityReward`, `MixtureReward`, `AdditiveMixtureReward`,
`MultiplicativeMixtureReward`, `SurviveReward`, `AbstractTerminationCondition.__call__`, `QuantityTermination`, `weighted_norm`,
`geometric_mean` and `_array_contains` are the reference's, constructed and called as `ComposedJiminyEnv` does, against a stub
environment: `quantities.add(name, creator)` returns an object whose `.get()` reads the current lane's rows, `training` and
`stepper_state.t` are attributes.  The flags of every mixture (`is_terminal`, `is_normalized`), its kept components and weights
are read off the reference's objects.  What this script RESTATES, and labels as such below: the loop of
`ComposedJiminyEnv.has_terminated` (bases/pipeline.py:777-797) and the call of `ComposedJiminyEnv.compute_reward` (:825-829).
Where the reference raises its "not normalized" ValueError, the expectation is the bit of the node whose `__call__` raised, and
the values of that lane are not compared.  `order='inf'` is handed over as `float('inf')`: the string of the reference's
signature is compared with `float('inf')` in `weighted_norm` and would reach `math.pow`.

Every case holds 64 lanes; each lane is one sequence of calls on one stub environment.  The generator asserts its own
conditions on every lane and redraws a lane that misses one: apart from the designed exact ties no compared element lies within
1e-3 (relative to max(|bound|, 1)) of a bound; every base handed to `math.pow` lies in [0, 4] (or is a NaN of `non_finite`), so
none is negative under a fractional order.
"""
from __future__ import annotations

import abc
import ast
import enum
import functools
import logging
import math
import os
import sys
import tempfile
import types
import typing

import numpy as np

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
COMMON = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_compositions.npz")

SOURCES = (
    ("utils/spaces.py", ("_array_contains",)),
    ("bases/compositions.py", ("AbstractReward", "QuantityReward", "MixtureReward", "EpisodeState", "AbstractTerminationCondition",
                               "QuantityTermination")),
    ("compositions/mixin.py", ("weighted_norm", "geometric_mean", "AdditiveMixtureReward", "MultiplicativeMixtureReward")),
    ("compositions/generic.py", ("SurviveReward",)),
)
B = 64
SEED = 20261020
SRC_DTYPE, SRC_INT32, SRC_UINT8 = 0, 1, 2
LEAF, SURVIVE, ADDITIVE, MULTIPLICATIVE = 0, 1, 2, 3
COND_ARRAY, COND_TRUNCATION, COND_TRAINING_ONLY = 1, 2, 4
HAS_LOW, HAS_HIGH = 1, 2
MARGIN, POW_MAX = 1e-3, 4.0
OUTPUTS = ("reward", "node_value", "terminated", "truncated", "trigger", "violations")
INF = float("inf")


class RecordingMath:
    """`math` for the reference's functions, with a `pow` that records its bases (the generator's own assertion)."""

    def __init__(self) -> None:
        self.bases: list = []

    def pow(self, x, y):
        self.bases.append(float(x))
        return math.pow(x, y)

    def __getattr__(self, name):
        return getattr(math, name)


class Subscriptable:
    def __class_getitem__(cls, item):
        return typing.Any


def load_reference() -> dict:
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    ns: dict = {"np": np, "nb": nb, "math": RecordingMath(), "partial": functools.partial, "ABCMeta": abc.ABCMeta,
                "abstractmethod": abc.abstractmethod, "IntEnum": enum.IntEnum, "LOGGER": logging.getLogger("reference"),
                "QuantityCreator": Subscriptable, "ValueT": typing.TypeVar("ValueT")}
    ns["LOGGER"].setLevel(logging.ERROR)
    ns.update({k: typing.Any for k in ("InterfaceJiminyEnv", "InfoType", "ArrayOrScalar", "ArrayLikeOrScalar", "Number")})
    ns.update({k: getattr(typing, k) for k in ("Optional", "Tuple", "Union", "List", "Sequence", "Dict", "Literal", "Callable", "Generic",
                                               "Any", "no_type_check")})
    for rel, names in SOURCES:
        path = os.path.join(COMMON, rel)
        with open(path) as f:
            tree = ast.parse(f.read(), filename=path)
        found = set()
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
                exec(compile(ast.Module([node], []), path, "exec"), ns)
                found.add(node.name)
        if set(names) - found:
            raise RuntimeError(f"{rel}: {sorted(set(names) - found)} not found")
    return ns


# ------------------------------------------------------------------------------------------------- the stub environment
class Handle:
    def __init__(self, env, creator) -> None:
        self.env, self.creator = env, creator

    def get(self):
        form, slot, rows = self.creator
        data = self.env.sources[slot]
        if form == "row":           # a reward leaf: one number
            return data[rows, self.env.lane]
        if form == "scalar":        # a 0-d quantity
            return np.array(data[rows[0], self.env.lane])
        return np.array(data[rows, self.env.lane])      # an array quantity [n]


class Quantities:
    def __init__(self, env) -> None:
        self.env, self.creators = env, {}

    def add(self, name, creator):
        assert name not in self.creators, name
        self.creators[name] = creator
        return Handle(self.env, creator)

    def discard(self, name):
        self.creators.pop(name, None)


class StubEnv:
    def __init__(self) -> None:
        self.training = True
        self.stepper_state = types.SimpleNamespace(t=0.0)
        self.quantities = Quantities(self)
        self.sources: list = []
        self.lane = 0


def raising_node(error: BaseException) -> str:
    """The name of the reward whose `AbstractReward.__call__` raised."""
    name, tb = None, error.__traceback__
    while tb is not None:
        if tb.tb_frame.f_code.co_name == "__call__" and hasattr(tb.tb_frame.f_locals.get("self"), "is_normalized"):
            name = tb.tb_frame.f_locals["self"].name
        tb = tb.tb_next
    assert name is not None
    return name


def composed_step(env, reward, terminations, base_terminated: bool, base_truncated: bool, names: list) -> dict:
    """RESTATED `ComposedJiminyEnv.has_terminated` (bases/pipeline.py:777-797) and `compute_reward` (:825-829) for the current
    lane of `env`, around the reference's own `__call__`s."""
    info: dict = {}
    terminated, truncated = base_terminated, base_truncated
    if not (terminated or truncated):
        for i, termination in enumerate(terminations):
            terminated, truncated = termination(info)
            if terminated:
                assert "terminated" not in info
                info["terminated"] = i
                break
            if truncated:
                assert "truncated" not in info
                info["truncated"] = i
                break
    out = dict(terminated=np.uint8(terminated), truncated=np.uint8(truncated),
               trigger=np.int32(info.get("terminated", info.get("truncated", -1))), violations=np.int32(0), compare=True)
    value = 0.0
    if reward is not None:
        try:
            value = reward(bool(terminated), info)
        except ValueError as e:
            assert "not normalized" in str(e), e
            out["violations"] = np.array(1 << names.index(raising_node(e)), dtype=np.uint32).astype(np.int32)
            out["compare"] = False
            value = float("nan")
    out["reward"] = np.float64(value)
    out["node_value"] = np.array([float(info.get(name, float("nan"))) for name in names])
    return out


# --------------------------------------------------------------------------------- the plan, read off the reference's objects
def flatten(ref: dict, env: StubEnv, reward, terminations) -> tuple:
    """The arrays of `jm_compose_desc` (include/jiminy_hip.h) of reference objects, nodes in pre-order, and their names."""
    nodes, child, weight = [], [], []

    def add(r) -> int:
        n = len(nodes)
        node = dict(name=r.name, kind=LEAF, terminal=-1 if r.is_terminal is None else int(bool(r.is_terminal)),
                    normalized=int(bool(r.is_normalized)), slot=0, row=0, start=0, count=0, order=1.0)
        nodes.append(node)
        if isinstance(r, ref["SurviveReward"]):
            node["kind"] = SURVIVE
        elif isinstance(r, ref["QuantityReward"]):
            _, node["slot"], node["row"] = env.quantities.creators[r.name]
        else:
            assert isinstance(r, ref["MixtureReward"])
            additive = isinstance(r, ref["AdditiveMixtureReward"])
            node["kind"] = ADDITIVE if additive else MULTIPLICATIVE
            node["order"] = float(r.order) if additive else 1.0
            indices = [add(c) for c in r.components]
            node["start"], node["count"] = len(child), len(indices)
            child.extend(indices)
            weight.extend(r.weights if additive else (1.0,) * len(indices))
        return n

    if reward is not None:
        add(reward)
    conds, elems = [], []
    for t in terminations:
        form, slot, rows = env.quantities.creators[t.name]
        n = len(rows)
        bound = lambda x: (np.zeros(n, bool), np.zeros(n)) if x is None else (np.ones(n, bool), np.broadcast_to(np.asarray(x, float), (n,)))  # noqa: E731
        (has_low, low), (has_high, high) = bound(t.low), bound(t.high)
        flags = (COND_ARRAY if form == "array" else 0) | (COND_TRUNCATION if t.is_truncation else 0) | \
                (COND_TRAINING_ONLY if t.training_only else 0)
        conds.append((len(elems), n, flags, float(t.grace_period)))
        elems += [(slot, int(r), HAS_LOW * int(hl) + HAS_HIGH * int(hh), float(lo), float(hi))
                  for r, hl, lo, hh, hi in zip(rows, has_low, low, has_high, high)]
    col = lambda rows, k, dtype: np.array([r[k] for r in rows], dtype=dtype)      # noqa: E731
    i32, f64 = np.int32, np.float64
    get = lambda key, dtype: np.array([n[key] for n in nodes], dtype=dtype)      # noqa: E731
    plan = dict(node_kind=get("kind", i32), node_terminal=get("terminal", i32), node_normalized=get("normalized", i32),
                node_slot=get("slot", i32), node_row=get("row", i32), node_child_start=get("start", i32),
                node_child_count=get("count", i32), node_order=get("order", f64), child=np.array(child, dtype=i32),
                child_weight=np.array(weight, dtype=f64), cond_elem_start=col(conds, 0, i32), cond_elem_count=col(conds, 1, i32),
                cond_flags=col(conds, 2, i32), cond_grace=col(conds, 3, f64), elem_slot=col(elems, 0, i32), elem_row=col(elems, 1, i32),
                elem_bounds=col(elems, 2, i32), elem_low=col(elems, 3, f64), elem_high=col(elems, 4, f64))
    return plan, [n["name"] for n in nodes], [t.name for t in terminations]


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    """An authored case: `kinds` / `rows` of the sources, `build(ref, env, leaf, term) -> (reward, terminations)`, `draw(rg, b)
    -> (list of source columns, time, base_terminated, base_truncated)`; `ties`: the lanes whose designed exact ties are exempt
    from the margin condition; `nan_ok`: NaN may reach `math.pow`."""

    def __init__(self, kinds, rows, build, draw, training=True, nan_ok=False) -> None:
        self.kinds, self.rows, self.build, self.draw, self.training, self.nan_ok = kinds, rows, build, draw, training, nan_ok


def margins_hold(plan: dict, kinds: list, columns: list, tie: bool) -> bool:
    """No element of a float source within MARGIN of a bound it is compared with, designed ties apart (integers are exact)."""
    if tie:
        return True
    for slot, row, flags, low, high in zip(plan["elem_slot"], plan["elem_row"], plan["elem_bounds"], plan["elem_low"], plan["elem_high"]):
        if kinds[slot] != SRC_DTYPE:
            continue
        v = float(columns[slot][row])
        for has, bound in ((flags & HAS_LOW, low), (flags & HAS_HIGH, high)):
            if has and not math.isnan(v) and abs(v - bound) < MARGIN * max(abs(bound), 1.0):
                return False
    return True


def make_case(ref: dict, rg: np.random.Generator, case: Case) -> dict:
    env = StubEnv()
    env.training = case.training
    leaf = lambda name, slot, row, normalized=True, terminal=False: ref["QuantityReward"](     # noqa: E731
        env, name, ("row", slot, row), None, normalized, terminal)
    term = lambda name, form, slot, rows, low, high, grace=0.0, **kw: ref["QuantityTermination"](     # noqa: E731
        env, name, (form, slot, list(rows)), low, high, grace, **kw)
    reward, terminations = case.build(ref, env, leaf, term)
    plan, names, cond_names = flatten(ref, env, reward, terminations)
    dtypes = {SRC_DTYPE: np.float64, SRC_INT32: np.int32, SRC_UINT8: np.uint8}
    env.sources = [np.zeros((r, B), dtype=dtypes[k]) for k, r in zip(case.kinds, case.rows)]
    time, base_term, base_trunc = np.zeros(B), np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    lanes, redrawn = [], 0
    for b in range(B):
        while True:
            columns, t, bt, btr, tie = case.draw(rg, b)
            for s, c in zip(env.sources, columns):
                s[:, b] = c
            env.lane, env.stepper_state.t = b, float(t)
            ref["math"].bases.clear()
            e = composed_step(env, reward, terminations, bool(bt), bool(btr), names)
            bases = ref["math"].bases
            ok = all((0.0 <= x <= POW_MAX) or (case.nan_ok and math.isnan(x)) for x in bases) and margins_hold(plan, case.kinds, columns, tie)
            if ok:
                break
            assert not tie, "a designed lane misses the generator's conditions"
            redrawn += 1
            assert redrawn < 4 * B
        time[b], base_term[b], base_trunc[b] = t, bt, btr
        lanes.append(e)
    out = {f"plan.{k}": v for k, v in plan.items()}
    out["plan.source_kind"] = np.array(case.kinds, dtype=np.int32)
    out["plan.source_rows"] = np.array(case.rows, dtype=np.int32)
    out.update({f"source{s}": a for s, a in enumerate(env.sources)})
    out.update(time=time, base_terminated=base_term, base_truncated=base_trunc, training=np.array(case.training),
               node_names=np.array(names, dtype=str), condition_names=np.array(cond_names, dtype=str),
               compare=np.array([e["compare"] for e in lanes]))
    out.update({f"expected.{k}": np.stack([e[k] for e in lanes], -1) for k in OUTPUTS})
    return out


def flags(b: int, every: int = 2):
    """Base flags of lane b: terminated on every `every`-th lane."""
    return int(b % every == 1), 0


def leaves_case(n: int, build, low=0.0, high=1.0, zero_every=0, terminated_every=2, poke=None, nan_ok=False) -> Case:
    """`n` leaves on one source of `n + 1` rows (the last is not read), values uniform in [low, high)."""
    def draw(rg, b):
        x = rg.uniform(low, high, n + 1)
        if zero_every and b % zero_every == 0:
            x[int(rg.integers(n))] = 0.0
        if poke is not None:
            poke(rg, b, x)
        bt, btr = flags(b, terminated_every)
        return [x], 0.0, bt, btr, False
    return Case([SRC_DTYPE], [n + 1], build, draw, nan_ok=nan_ok)


def additive(order, weights):
    def build(ref, env, leaf, term):
        parts = [leaf(f"leaf_{i}", 0, i) for i in range(len(weights))]
        return ref["AdditiveMixtureReward"](env, "total", parts, order, weights), []
    return build


def build_additive_inf(ref, env, leaf, term):
    parts = [leaf("a", 0, 0), leaf("b", 0, 1), ref["SurviveReward"](env), leaf("c", 0, 2)]
    return ref["AdditiveMixtureReward"](env, "total", parts, INF, (0.5, 1.0, 0.25, 0.75)), []


def build_multiplicative(ref, env, leaf, term):
    return ref["MultiplicativeMixtureReward"](env, "total", [leaf(f"leaf_{i}", 0, i) for i in range(4)]), []


def nested_reward(ref, env, leaf, with_terminal: bool):
    add2 = ref["AdditiveMixtureReward"](env, "add", [leaf("a", 0, 0), leaf("b", 0, 1)], 2, (0.5, 0.5))
    addinf = ref["AdditiveMixtureReward"](env, "last_resort", [leaf("c", 0, 2), ref["SurviveReward"](env)], INF, (1.0, 0.4))
    parts = [add2, addinf, leaf("d", 0, 3)]
    if with_terminal:
        parts.append(leaf("final", 0, 4, True, True))
    return ref["MultiplicativeMixtureReward"](env, "root", parts)


def build_nested(ref, env, leaf, term):
    return nested_reward(ref, env, leaf, False), []


def build_terminal_only(ref, env, leaf, term):
    parts = [leaf(f"final_{i}", 0, i, True, True) for i in range(3)]
    return ref["AdditiveMixtureReward"](env, "total", parts, 1, (0.5, 0.3, 0.2)), []


def build_mixed_terminal(ref, env, leaf, term):
    add2 = ref["AdditiveMixtureReward"](env, "add", [leaf("a", 0, 0), leaf("b", 0, 1)], 2, (0.5, 0.5))
    return ref["MultiplicativeMixtureReward"](env, "root", [add2, ref["SurviveReward"](env), leaf("final", 0, 2, True, True)]), []


def build_unnormalized(ref, env, leaf, term):
    parts = [leaf(f"cost_{i}", 0, i, False) for i in range(3)]
    return ref["AdditiveMixtureReward"](env, "total", parts, 1, (0.5, 0.25, 0.25)), []


def poke_violation(rg, b, x):
    if b % 4 == 2:
        x[int(rg.integers(4))] = rg.uniform(1.05, 1.5) if b % 8 == 2 else -rg.uniform(0.05, 0.5)


def build_non_finite(ref, env, leaf, term):
    linf = ref["AdditiveMixtureReward"](env, "linf", [leaf("a", 0, 0), leaf("b", 0, 1), leaf("c", 0, 2)], INF, (1.0, 0.8, 0.6))
    l1 = ref["AdditiveMixtureReward"](env, "l1", [leaf("d", 0, 3), leaf("e", 0, 4)], 1, (0.5, 0.5))
    return ref["AdditiveMixtureReward"](env, "root", [linf, l1], 1, (0.5, 0.5)), []


def poke_non_finite(rg, b, x):
    # lanes 1 mod 4: a NaN behind the first component of the L^inf mixture (Python's max keeps the total); 2 mod 4: in its
    # first component (the total starts as NaN and stays); 3 mod 4: under L^1 (propagates)
    if b % 4 == 1:
        x[1 + b % 2] = float("nan")
    elif b % 4 == 2:
        x[0] = float("nan")
    elif b % 4 == 3:
        x[3 + b % 2] = float("nan")


TIMES = (0.0, 0.125, 0.25, 0.375, 0.5, 0.75)


def build_terminations(ref, env, leaf, term):
    f = np.float64
    return None, [
        term("posture", "array", 0, (0, 1, 2), np.array([-0.5, -0.4, -1.0]), np.array([0.5, 0.6, 1.0]), 0.25),
        term("height", "scalar", 0, (3,), f(-1.0), f(1.0)),
        term("flying", "array", 0, (4, 5), None, 2.0, 0.5, is_truncation=True),
        term("safety", "scalar", 1, (1,), None, f(0.0)),
        term("progress", "scalar", 0, (6,), f(0.2), None, is_truncation=True),
        term("drift", "scalar", 0, (7,), f(-1.0), f(1.0), 0.25),
    ]


def draw_terminations(rg, b):
    x = np.empty(9)
    x[:3] = rg.uniform(-0.52, 0.52, 3)
    x[3] = rg.uniform(-1.15, 1.15)
    x[4:6] = rg.uniform(0.0, 3.0, 2)
    x[6] = rg.uniform(0.0, 1.5)
    x[7] = rg.uniform(-1.2, 1.2)
    x[8] = rg.uniform(-9.0, 9.0)            # (not read)
    safety = np.array([3, 1 if rg.uniform() < 0.15 else 0], dtype=np.int32)
    tie = False
    if b % 16 == 5:         # exact ties: on a bound is inside it
        x[:3], x[3], x[4:6], x[6], x[7], tie = [-0.5, 0.6, 1.0], 1.0, 2.0, 0.2, -1.0, True
    if b % 16 == 9:         # NaN: fires the array form, not the scalar form
        x[int(rg.integers(3))], tie = float("nan"), False
    if b % 16 == 13:
        x[3] = x[7] = float("nan")
    t = TIMES[int(rg.integers(len(TIMES)))]
    return [x, safety], t, int(b % 8 == 3), int(b % 8 == 6), tie


def build_training_only(ref, env, leaf, term):
    f = np.float64
    return None, [
        term("height", "scalar", 0, (0,), f(0.3), None, 0.25),
        term("effort", "array", 0, (1, 2), None, np.array([1.0, 2.0]), 0.0, training_only=True),
        term("timeout", "scalar", 0, (3,), None, f(0.5), 0.0, is_truncation=True, training_only=True),
        term("posture", "array", 0, (4, 5), -1.0, 1.0, 0.0),
    ]


def draw_training_only(rg, b):
    x = np.array([rg.uniform(0.1, 1.0), rg.uniform(0.0, 1.3), rg.uniform(0.0, 2.5), rg.uniform(0.0, 0.7), *rg.uniform(-1.25, 1.25, 2)])
    return [x], TIMES[int(rg.integers(len(TIMES)))], 0, 0, False


def build_combined(ref, env, leaf, term):
    f = np.float64
    return nested_reward(ref, env, leaf, True), [
        term("posture", "array", 0, (5, 6), np.array([-0.5, -0.5]), np.array([0.5, 0.5]), 0.25),
        term("flying", "scalar", 0, (7,), None, f(0.3), 0.0, is_truncation=True),
        term("safety", "scalar", 1, (0,), None, f(0.0), 0.125),
    ]


def draw_combined(rg, b):
    x = np.concatenate([rg.uniform(0.0, 1.0, 5), rg.uniform(-0.7, 0.7, 2), [rg.uniform(0.0, 0.4)]])
    safety = np.array([2 if rg.uniform() < 0.35 else 0], dtype=np.int32)
    return [x, safety], TIMES[int(rg.integers(len(TIMES)))], int(b % 16 == 7), int(b % 16 == 11), False


W5 = (0.3, 0.25, 0.2, 0.15, 0.1)
CASES = (
    ("additive_l1", leaves_case(5, additive(1, W5))),
    ("additive_l2", leaves_case(5, additive(2, W5))),
    ("additive_half", leaves_case(5, additive(0.5, W5))),
    ("additive_inf", leaves_case(3, build_additive_inf)),
    ("multiplicative", leaves_case(4, build_multiplicative, zero_every=5)),
    ("nested", leaves_case(4, build_nested)),
    ("terminal_only", leaves_case(3, build_terminal_only)),
    ("mixed_terminal", leaves_case(3, build_mixed_terminal)),
    ("zero_weight", leaves_case(5, additive(1, (0.4, 0.0, 0.6, 0.0, -0.5)))),
    ("unnormalized", leaves_case(3, build_unnormalized, low=1.0, high=3.5)),
    ("violation", leaves_case(4, additive(1, (0.25, 0.25, 0.25, 0.25)), poke=poke_violation)),
    ("non_finite", leaves_case(5, build_non_finite, poke=poke_non_finite, nan_ok=True, terminated_every=8)),
    ("terminations", Case([SRC_DTYPE, SRC_INT32], [9, 2], build_terminations, draw_terminations)),
    ("training_only_eval", Case([SRC_DTYPE], [6], build_training_only, draw_training_only, training=False)),
    ("training_only_train", Case([SRC_DTYPE], [6], build_training_only, draw_training_only, training=True)),
    ("combined", Case([SRC_DTYPE, SRC_INT32], [8, 1], build_combined, draw_combined)),
)


def main(out_path: str, verbose: bool = True) -> None:
    ref = load_reference()
    out: dict = {}
    for label, case in CASES:
        # (the two `training_only` cases draw the same inputs)
        rg = np.random.default_rng([SEED, sum(map(ord, label.replace("_eval", "").replace("_train", "")))])
        for k, v in make_case(ref, rg, case).items():
            out[f"{label}.{k}"] = v
    out["cases"] = np.array([c[0] for c in CASES])
    out["tier"] = np.array("A: the reference's reward, mixture and termination classes, weighted_norm, geometric_mean and "
                           "_array_contains, executed against a stub environment; the loop of ComposedJiminyEnv.has_terminated and "
                           "the call of compute_reward are restated")
    np.savez_compressed(out_path, **out)
    if verbose:
        print(f"wrote {os.path.relpath(out_path)}: {os.path.getsize(out_path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if not os.path.isdir(COMMON):
        sys.exit(f"{COMMON} not found: run this where the reference tree is available")
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            fresh = os.path.join(tmp, "ref_compositions.npz")
            main(fresh, verbose=False)
            same = open(fresh, "rb").read() == open(OUT, "rb").read()
        print("tests/golden/ref_compositions.npz " + ("regenerates identically" if same else "DIFFERS from a fresh run"))
        sys.exit(0 if same else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
