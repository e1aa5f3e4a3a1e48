"""Reference-pinned fixtures of the layout, filter and scale wrappers (jiminy_amd/wrappers.py): EXECUTES THE REFERENCE'S OWN
PYTHON FUNCTIONS AND CLASSES.

Same mechanism and rules as tools/make_ref_compositions_fixtures.py: this script parses the reference files where they lie, takes
the definitions named in SOURCES and executes them with what is not installed stubbed.  Nothing of the reference is copied into
the repository: only authored specifications, seeded inputs and what the reference's code produced for them, written to
tests/golden/ref_wrappers.npz.

Run where the reference tree is available:   python tools/make_ref_wrappers_fixtures.py [output.npz]
                                             python tools/make_ref_wrappers_fixtures.py --check     (regenerate and compare)

What runs is the reference's: `_adapt_layout`, `FilterObservation.__init__`, `_split_nested_key_and_slice`, `_array_scale`,
`ScaleObservation.__init__` / `transform_observation`, `ScaleAction.__init__` with its `_array_scale_chunks`, and the whole of
`jiminy_py/tree.py` (pure Python) behind them.  What is stubbed: `numba.jit` (identity), `gymnasium` (an empty `Space`: the data
are arrays, not spaces), the base classes of the wrappers (they keep `env`), `multi_array_copyto` / `array_copyto` (element-wise
assignment), `copy` of utils/spaces.py (RESTATED: `unflatten_as(data, flatten(data))`, its one line), `build_reduce` (RESTATED for
an action that is one array: the function it is given, called on `(factor list, env.action, action)`), and `OrderedDict`, whose
keys go through `repr` where they are not hashable (a `slice` is hashable from Python 3.12 on only; the order of insertion,
`get`, `move_to_end`, `items` and `values` are those of the real one).

Recorded per case (keys `<case>/<name>`): the paths of the leaves of the result as the reference's `flatten_with_path` gives them
(`paths`, their `repr`), the skeleton of its containers (`skeleton`: the `repr` of the result with every leaf replaced by its
number), the leaves (`leaf<i>`); for `ScaleObservation` the sequence of its scale operations -- the leaf each writes, the mask of
the elements it covers, whether it reads the base leaf, and its factor -- and for `ScaleAction` the factor list of the action
with the masks of its blocks.
"""
from __future__ import annotations

import __future__ as future
import ast
import collections
import functools
import operator
import os
import sys
import tempfile
import types
import typing

import numpy as np

REF = os.environ.get("JIMINY_REFERENCE", "/root/reference")
WRAPPERS = os.path.join(REF, "python/gym_jiminy/common/gym_jiminy/common/wrappers")
TREE = os.path.join(REF, "python/jiminy_py/src/jiminy_py/tree.py")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_wrappers.npz")
SEED = 20261021

SOURCES = (
    ("observation_layout.py", ("_adapt_layout", "FilterObservation")),
    ("scale.py", ("_array_scale", "_split_nested_key_and_slice", "ScaleObservation", "ScaleAction")),
)

# ---- the authored cases (tests/test_observe_wrappers.py holds the same specifications and checks them against `spec`)
LAYOUTS = {
    "layout_aggregate": [((), ("x2", "y2")), ((0,), ("x1",))],
    "layout_blocks": [(("A", "B1"), ("x2", "y2", 1)), (("A", "B2"), ("x1", 0, [(), (1, 4), (1, 3)]))],
    "layout_subtrees": [((), ("x2",)), (("y1", "z2"), ("x1",))],
    "layout_noncontiguous": [(("a",), ("x1", 0, [(1, 6), 2, (), (0, 3)])), (("a",), ("x2", "y2", 1, [(), 1])), (("b", "c"), ("x2", "y1", "z1"))],
}
FILTER_KEYS = [("x2", "y2", 2), ("x2", "y2", 0), ("x1",)]
SCALES = {
    "scale_two_full": [(("a", "p"), 2.0), (("a",), 3.0), (("a", "p"), 0.7)],
    "scale_block_around_full": [(("a", "q", [(0, 2), ()]), 1.5), (("a", "q"), 0.7), (("a", "q", [1, (1, 3)]), 2.5)],
    "scale_overlapping_blocks": [(("b", [(0, 3)]), 3.0), (("b", [(2, 5)]), 7.0), (("b", [(1, 4)]), 0.3)],
    "scale_combined": [(("a", "q", [(0, 2), ()]), 1.5), (("a",), 3.0), (("b", [(0, 3)]), 3.0), (("a", "q"), 0.7), (("b",), 1.1),
                       (("b", [(2, 5)]), 7.0), (("a", "q", [1, (1, 3)]), 2.5), (("a", "p"), 2.0)],
}
ACTION_SCALES = {
    "action_two_full": [((), 2.0), ((), 0.3)],
    "action_block_around_full": [(([(0, 4)],), 1.5), ((), 0.7), (([(2, 6)],), 2.5)],
    "action_repeated_block": [(([(1, 5)],), 3.0), (([(0, 2)],), 7.0), (([(1, 5)],), 0.3), ((), 1.7)],
}
ACTION_SIZE = 6


def layout_input(rng) -> dict:
    """The observation of the docstrings of observation_layout.py:333-347, as arrays (a `Discrete` leaf is a 0-d array)."""
    return {"x1": (rng.standard_normal((7, 6, 5, 4)),),
            "x2": {"y1": {"z1": np.array(rng.standard_normal())},
                   "y2": (np.array(rng.standard_normal()), rng.standard_normal((2, 3)), np.array(rng.standard_normal()))}}


def scale_input(rng) -> dict:
    return {"a": {"p": rng.standard_normal(6), "q": rng.standard_normal((3, 4))}, "b": rng.standard_normal(5)}


class ReprKeyedOrderedDict:
    """`collections.OrderedDict` for keys that may hold a `slice` (hashable from Python 3.12 on only)."""

    def __init__(self) -> None:
        self._d: collections.OrderedDict = collections.OrderedDict()

    @staticmethod
    def _k(key):
        try:
            hash(key)
            return key
        except TypeError:
            return repr(key)

    def get(self, key, default=None):
        return self._d.get(self._k(key), (None, default))[1]

    def __setitem__(self, key, value) -> None:
        self._d[self._k(key)] = (key, value)

    def move_to_end(self, key, last=True) -> None:
        self._d.move_to_end(self._k(key), last=last)

    def items(self):
        return tuple(self._d.values())

    def values(self):
        return tuple(v for _, v in self._d.values())

    def __class_getitem__(cls, item):
        return cls


class Subscriptable:
    def __class_getitem__(cls, item):
        return cls


class GenericStub:
    def __class_getitem__(cls, item):
        return object


class BaseTransform(Subscriptable):
    def __init__(self, env) -> None:
        self.env = env
        if hasattr(env, "action"):       # (the action buffer of the wrapper itself, of the structure of the environment's)
            self.action, self.action_space = np.zeros_like(env.action), None


def load_reference() -> dict:
    tree = types.ModuleType("jiminy_py.tree")
    with open(TREE) as f:
        exec(compile(f.read(), TREE, "exec"), tree.__dict__)
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    gym = types.ModuleType("gymnasium")
    gym.Space = type("Space", (Subscriptable,), {})
    gym.spaces = types.SimpleNamespace(Box=type("Box", (gym.Space,), {}), Dict=dict, Tuple=tuple)

    def copyto(dst, src):
        dst[...] = src

    def multi_copyto(dsts, srcs):
        for d, s in zip(dsts, srcs):
            d[...] = s

    calls: list = []

    def build_reduce(fn, op, dataset, space, arity, forward_bounds):       # RESTATED for an action that is one array
        calls.append(dataset[0])
        return lambda action: fn(dataset[0], dataset[1], action)

    ns: dict = {"np": np, "nb": nb, "gym": gym, "getitem": operator.getitem, "reduce": functools.reduce,
                "OrderedDict": ReprKeyedOrderedDict, "cast": typing.cast, "overload": typing.overload,
                "flatten_with_path": tree.flatten_with_path, "issubclass_mapping": tree.issubclass_mapping,
                "issubclass_sequence": tree.issubclass_sequence, "unflatten_as": tree.unflatten_as,
                "copy": lambda data: tree.unflatten_as(data, tree.flatten(data)),          # RESTATED (utils/spaces.py:383)
                "array_copyto": copyto, "multi_array_copyto": multi_copyto, "build_reduce": build_reduce,
                "BaseTransformObservation": BaseTransform, "BaseTransformAction": BaseTransform, "Generic": GenericStub,
                "deepcopy": __import__("copy").deepcopy, "tree": tree, "build_reduce_calls": calls}
    ns.update({k: typing.Any for k in ("NestedObs", "Obs", "Act", "ScaledObs", "ScaledAct", "NestedKey")})      # (named in the class bases, in a `cast`)
    for rel, names in SOURCES:
        path = os.path.join(WRAPPERS, rel)
        with open(path) as f:
            module = ast.parse(f.read(), filename=path)
        found = set()
        for node in module.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
                # (annotations are not evaluated: most of the names they use are not defined here)
                exec(compile(ast.Module([node], []), path, "exec", flags=future.annotations.compiler_flag), ns)
                found.add(node.name)
        if set(names) - found:
            raise RuntimeError(f"{rel}: {sorted(set(names) - found)} not found")
    return ns


def skeleton(data, counter=None) -> str:
    counter = counter if counter is not None else [0]
    if isinstance(data, dict):
        return "{" + ", ".join(f"{k!r}: {skeleton(v, counter)}" for k, v in data.items()) + "}"
    if isinstance(data, (list, tuple)):
        body = ", ".join(skeleton(v, counter) for v in data)
        return f"[{body}]" if isinstance(data, list) else f"({body},)"
    counter[0] += 1
    return str(counter[0] - 1)


def record_tree(out: dict, case: str, ns: dict, data) -> None:
    leaves = ns["flatten_with_path"](data)
    out[f"{case}/paths"] = np.array([repr(tuple(p)) for p, _ in leaves])
    out[f"{case}/skeleton"] = np.array(skeleton(data))
    for i, (_, leaf) in enumerate(leaves):
        out[f"{case}/leaf{i}"] = np.array(leaf, dtype=np.float64)


def covered(array: np.ndarray, view: np.ndarray) -> np.ndarray:
    """The mask of the elements of `array` that `view` is a view of."""
    saved = array.copy()
    array[...] = 0.0
    view[...] = 1.0
    mask = array != 0.0
    array[...] = saved
    return mask


def generate() -> dict:
    ns = load_reference()
    rng = np.random.default_rng(SEED)
    out: dict = {}
    data = layout_input(rng)
    record_tree(out, "layout_input", ns, data)
    for case, layout in LAYOUTS.items():
        record_tree(out, case, ns, ns["_adapt_layout"](data, layout))
    env = types.SimpleNamespace(observation=data, observation_space=data)
    record_tree(out, "filter", ns, ns["FilterObservation"](env, FILTER_KEYS).observation)
    for case, nested_scale in SCALES.items():
        base = scale_input(rng)
        record_tree(out, f"{case}/input", ns, base)
        wrapper = ns["ScaleObservation"](types.SimpleNamespace(observation=base), nested_scale)
        leaves = [leaf for _, leaf in ns["flatten_with_path"](wrapper.observation)]
        bases = [leaf for _, leaf in ns["flatten_with_path"](base)]
        ops = []
        for k, (dst, src, factor) in enumerate(wrapper._scale_ops):
            i = next(i for i, leaf in enumerate(leaves) if np.shares_memory(leaf, dst))
            out[f"{case}/op{k}_mask"] = covered(leaves[i], dst)
            ops.append((i, int(np.shares_memory(src, bases[i])), factor))
        out[f"{case}/op_leaf"] = np.array([o[0] for o in ops], dtype=np.int64)
        out[f"{case}/op_reads_base"] = np.array([o[1] for o in ops], dtype=np.int64)
        out[f"{case}/op_factor"] = np.array([o[2] for o in ops], dtype=np.float64)
        wrapper.transform_observation()
        record_tree(out, case, ns, wrapper.observation)
    for case, nested_scale in ACTION_SCALES.items():
        action_env, action = np.zeros(ACTION_SIZE), rng.standard_normal(ACTION_SIZE)
        ns["build_reduce_calls"].clear()
        wrapper = ns["ScaleAction"](types.SimpleNamespace(action=action_env), nested_scale)
        factors = ns["build_reduce_calls"][0]
        probe = np.zeros(ACTION_SIZE)
        for k, (slices, factor) in enumerate(factors):
            out[f"{case}/op{k}_mask"] = np.ones(ACTION_SIZE, dtype=bool) if slices is None else covered(probe, probe[slices])
        out[f"{case}/op_factor"] = np.array([f for _, f in factors], dtype=np.float64)
        out[f"{case}/op_full"] = np.array([s is None for s, _ in factors], dtype=np.int64)
        wrapper.transform_action(action)
        out[f"{case}/input"], out[f"{case}/scaled"] = action, action_env.copy()
    out["spec"] = np.array(repr({"layouts": LAYOUTS, "filter_keys": FILTER_KEYS, "scales": SCALES, "action_scales": ACTION_SCALES}))
    return out


def main() -> None:
    args = sys.argv[1:]
    data = generate()
    if args and args[0] == "--check":
        with np.load(OUT) as f:
            assert sorted(f.files) == sorted(data), (sorted(set(f.files) ^ set(data)))
            for k in f.files:
                a, b = f[k], data[k]
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
        print(f"{os.path.relpath(OUT)}: regenerated identically ({len(data)} arrays)")
        return
    path = args[0] if args else OUT
    with tempfile.NamedTemporaryFile(dir=os.path.dirname(os.path.abspath(path)), suffix=".npz", delete=False) as tmp:
        np.savez_compressed(tmp, **data)
    os.replace(tmp.name, path)
    print(f"wrote {os.path.relpath(path)}: {len(data)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
