"""`AdaptLayoutObservation`, `FilterObservation`, `ScaleObservation` and `ScaleAction` (jiminy_amd/wrappers.py) against what the
reference's own `_adapt_layout`, `FilterObservation`, `ScaleObservation` and `ScaleAction` produced
(tests/golden/ref_wrappers.npz, written by tools/make_ref_wrappers_fixtures.py, which executes them): the paths and the
containers exactly, the arrays bit for bit in float64.  The inputs of the fixture have no batch axis; here they get one of two
lanes, the second holding twice the first (exact), so that a block spec that addressed the batch axis would show."""
from __future__ import annotations

import ast
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from jiminy_amd import wrappers as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_wrappers.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_wrappers_fixtures.py")
FX = np.load(FIXTURE)
SPEC = ast.literal_eval(str(FX["spec"]))


def tree_of(case: str):
    """The input a case records, with batch-first tensors of two lanes as leaves: the observation of the reference's docstrings
    (observation_layout.py:333-347) or the small tree of the scale cases."""
    leaves = []
    while f"{case}/leaf{len(leaves)}" in FX.files:
        a = FX[f"{case}/leaf{len(leaves)}"]
        leaves.append(torch.from_numpy(np.stack([a, 2.0 * a])))
    if case == "layout_input":
        tree = {"x1": (leaves[0],), "x2": {"y1": {"z1": leaves[1]}, "y2": (leaves[2], leaves[3], leaves[4])}}
    else:
        tree = {"a": {"p": leaves[0], "q": leaves[1]}, "b": leaves[2]}
    assert skeleton(tree) == str(FX[f"{case}/skeleton"])
    return tree, leaves


def skeleton(data, counter=None) -> str:
    counter = counter if counter is not None else [0]
    if isinstance(data, dict):
        return "{" + ", ".join(f"{k!r}: {skeleton(v, counter)}" for k, v in data.items()) + "}"
    if isinstance(data, (list, tuple)):
        body = ", ".join(skeleton(v, counter) for v in data)
        return f"[{body}]" if isinstance(data, list) else f"({body},)"
    counter[0] += 1
    return str(counter[0] - 1)


def check_tree(case: str, got) -> None:
    leaves = W._leaves_in_order(got)
    assert [repr(p) for p, _ in leaves] == [str(p) for p in FX[f"{case}/paths"]], case
    assert skeleton(got) == str(FX[f"{case}/skeleton"]), case
    for i, (path, x) in enumerate(leaves):
        want = FX[f"{case}/leaf{i}"]
        assert x.dtype == torch.float64 and tuple(x.shape) == (2,) + want.shape, (case, path)
        assert x[0].numpy().tobytes() == want.tobytes() and np.array_equal(x[1].numpy(), 2.0 * want), (case, path)


class Env:
    def __init__(self, obs) -> None:
        self.obs, self.actions = obs, []

    def observation(self):
        return self.obs

    def reset(self):
        return self.obs, {}

    def step(self, action):
        self.actions.append(action)
        return self.obs, None, None, None, {}


def test_fixture_regenerates_from_the_reference_tree():
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        pytest.skip("the reference tree is not here: the committed fixture stands")
    subprocess.check_call([sys.executable, TOOL, "--check"], stdout=subprocess.DEVNULL)


def test_fixture_holds_the_designed_cases():
    assert list(SPEC["layouts"]) == ["layout_aggregate", "layout_blocks", "layout_subtrees", "layout_noncontiguous"]
    # the three layouts of the reference's docstring (observation_layout.py:349-392)
    assert SPEC["layouts"]["layout_aggregate"] == [((), ("x2", "y2")), ((0,), ("x1",))]
    assert SPEC["layouts"]["layout_blocks"] == [(("A", "B1"), ("x2", "y2", 1)), (("A", "B2"), ("x1", 0, [(), (1, 4), (1, 3)]))]
    assert SPEC["layouts"]["layout_subtrees"] == [((), ("x2",)), (("y1", "z2"), ("x1",))]
    assert FX["layout_blocks/leaf1"].shape == (7, 3, 2, 4)
    # a block that is not contiguous in memory: an index in the middle and a slice behind it
    assert FX["layout_noncontiguous/leaf0"].shape == (5, 5, 3) and not FX["layout_input/leaf0"][1:6, 2, :, 0:3].flags.c_contiguous
    assert SPEC["filter_keys"] == [("x2", "y2", 2), ("x2", "y2", 0), ("x1",)]
    assert list(SPEC["scales"]) == ["scale_two_full", "scale_block_around_full", "scale_overlapping_blocks", "scale_combined"]
    assert FX["scale_two_full/op_leaf"].tolist() == [1, 0]                       # three full factors on ('a', 'p'): one operation
    assert FX["scale_block_around_full/op_reads_base"].tolist() == [1, 0, 0]     # the full operation comes first
    masks = [FX[f"scale_overlapping_blocks/op{k}_mask"] for k in range(3)]
    assert (masks[0] & masks[1]).any() and (masks[1] & masks[2]).any() and (masks[0] & masks[2]).any()
    assert list(SPEC["action_scales"]) == ["action_two_full", "action_block_around_full", "action_repeated_block"]


@pytest.mark.parametrize("case", list(SPEC["layouts"]))
def test_adapt_layout_matches_the_reference(case):
    obs, leaves = tree_of("layout_input")
    env = W.AdaptLayoutObservation(Env(obs), SPEC["layouts"][case])
    got = env.observation()
    check_tree(case, got)
    # extracted leaves are views, not copies
    for _, x in W._leaves_in_order(got):
        assert any(x.untyped_storage().data_ptr() == leaf.untyped_storage().data_ptr() for leaf in leaves)
    assert W._leaves_in_order(env.reset()[0])[0][1].shape == W._leaves_in_order(got)[0][1].shape


def test_adapt_layout_errors():
    obs, _ = tree_of("layout_input")
    with pytest.raises(ValueError, match="The resulting observation space must not be empty."):
        W.AdaptLayoutObservation(Env(obs), [])
    with pytest.raises(ValueError, match="Input nested keys must not be empty."):
        W.AdaptLayoutObservation(Env(obs), [(("a",), ())]).observation()
    with pytest.raises(KeyError, match=r"Nested key '\('x2', 'nope'\)' is missing."):
        W.AdaptLayoutObservation(Env(obs), [(("a",), ("x2", "nope"))]).observation()
    # a string key for the output is one key
    got = W.AdaptLayoutObservation(Env(obs), [("a", ("x2", "y1", "z1"))]).observation()
    assert list(got) == ["a"] and got["a"].shape == (2,)


def test_filter_observation_matches_the_reference():
    obs, _ = tree_of("layout_input")
    check_tree("filter", W.FilterObservation(Env(obs), SPEC["filter_keys"]).observation())
    # a duplicate key keeps its leaf once; the order of the keys does not matter
    check_tree("filter", W.FilterObservation(Env(obs), [("x1",), ("x2", "y2", 0), ("x1", 0), ("x2", "y2", 2)]).observation())
    with pytest.raises(ValueError, match="At least one observation leaf must be preserved."):
        W.FilterObservation(Env(obs), [("nope",)]).observation()


@pytest.mark.parametrize("case", list(SPEC["scales"]))
def test_scale_observation_matches_the_reference(case):
    obs, _ = tree_of(f"{case}/input")
    paths = [p for p, _ in W.flatten_with_path(obs)]
    assert [repr(p) for p in paths] == [str(p) for p in FX[f"{case}/paths"]]
    # the operations of every leaf, in the reference's order: the elements each covers and its factor
    ops = W.observation_scale_ops(paths, SPEC["scales"][case])
    want = {i: [] for i in range(len(paths))}
    for k, (leaf, reads_base, factor) in enumerate(zip(FX[f"{case}/op_leaf"], FX[f"{case}/op_reads_base"], FX[f"{case}/op_factor"])):
        want[int(leaf)].append((FX[f"{case}/op{k}_mask"], bool(reads_base), float(factor)))
    for i, path in enumerate(paths):
        got = ops.get(path, [])
        assert len(got) == len(want[i]), (case, path)
        for (block, factor), (mask, reads_base, want_factor) in zip(got, want[i]):
            hit = np.zeros(mask.shape, dtype=bool)
            hit[() if block is None else block] = True
            assert np.array_equal(hit, mask) and (block is None) == reads_base, (case, path)
            assert np.float64(factor).tobytes() == np.float64(want_factor).tobytes(), (case, path, factor, want_factor)
    untouched = [x.clone() for _, x in W.flatten_with_path(obs)]
    check_tree(case, W.ScaleObservation(Env(obs), SPEC["scales"][case]).observation())
    for (_, x), before in zip(W.flatten_with_path(obs), untouched):       # (the base observation is not scaled in place)
        assert torch.equal(x, before)


@pytest.mark.parametrize("case", list(SPEC["action_scales"]))
def test_scale_action_matches_the_reference(case):
    nested_scale = SPEC["action_scales"][case]
    # the reference's key of a block of the one action array is `(block spec,)`; `((), block spec)` names the same
    for spelled in (nested_scale, [(((), *key), scale) if key else (key, scale) for key, scale in nested_scale]):
        ops = W.action_scale_ops(spelled)
        assert len(ops) == len(FX[f"{case}/op_factor"])
        for k, (block, factor) in enumerate(ops):
            hit = np.zeros(6, dtype=bool)
            hit[() if block is None else block] = True
            assert np.array_equal(hit, FX[f"{case}/op{k}_mask"]) and (block is None) == bool(FX[f"{case}/op_full"][k])
            assert np.float64(factor).tobytes() == FX[f"{case}/op_factor"][k].tobytes()
        inner = Env({"x": torch.zeros(2, 1, dtype=torch.float64)})
        action = torch.from_numpy(np.stack([FX[f"{case}/input"], 2.0 * FX[f"{case}/input"]]))
        before = action.clone()
        W.ScaleAction(inner, spelled).step(action)
        assert inner.actions[0][0].numpy().tobytes() == FX[f"{case}/scaled"].tobytes()
        assert np.array_equal(inner.actions[0][1].numpy(), 2.0 * FX[f"{case}/scaled"]) and torch.equal(action, before)


def test_scale_errors():
    obs, _ = tree_of("scale_two_full/input")
    with pytest.raises(ValueError, match=r"Nested key \('a', 'z'\) not found in base observation space."):
        W.ScaleObservation(Env(obs), [(("a", "z"), 2.0)]).observation()
    with pytest.raises(ValueError, match=r"Nested key \('a',\) not found in base action space."):
        W.ScaleAction(Env(obs), [(("a",), 2.0)])
    with pytest.raises(ValueError, match="must not be zero"):
        W.ScaleObservation(Env(obs), [(("a",), 0.0)]).observation()
