"""Reward mixtures and termination conditions on the device (csrc/jm_compose.h behind `jm_block_compose`,
`jiminy_amd.compositions`, `blocks.Composition`, the `reward` / `termination_conditions` keywords of `WalkerVecEnv`).

Specification: the reference's own output, tests/golden/ref_compositions.npz (tools/make_ref_compositions_fixtures.py executes
the reference's reward, mixture and termination classes against a stub environment; sixteen cases of 64 lanes).  Comparison
rule, on every lane of every case: `terminated`, `truncated`, `trigger`, `violations` and the NaN pattern of `node_value` equal
the fixture exactly in float64, and in float32 equal the numpy restatement (tests/compose_numpy.py) run in float32 on the same
float32 inputs; `reward` and `node_value` within 1e-13 relative to max(|want|, 1) in float64, and in float32 within
max(4 x the error of the float32 numpy restatement on the same case and output, FLOOR32).  The values of a lane on which the
reference raised its "not normalized" ValueError (the violation bit is the expectation there) are not compared.

FLOOR32 = 2 float32 epsilons (2.4e-7).  Why a floor: the error of the restatement is whatever the rounding of the inputs to
float32 leaves (half an epsilon, 6e-8, on most cases; 0 on `terminations` and the two `training_only` cases, which have no
reward), and where a case is exact or nearly exact in numpy (`additive_inf`, `terminal_only`: no `powf` that is not an
identity) 4 x that error may fall under what a device `powf`, which is not correctly rounded, costs.  The largest device error
measured is 1.72e-7 = 1.44 epsilons (`unnormalized`, values up to 3.1), so the floor sits just above it at 2 epsilons.  As
measured, no case needs it: every device error below also lies within 4 x the restatement's error of its own case.

Measured on the host (error relative to max(|want|, 1), largest over the sixteen cases and the compared lanes):
  float64, host emulation | numpy restatement:  reward 0 | 1.1e-16   node_value 0 | 1.1e-16
  float32, host emulation | numpy restatement:  reward 1.3e-7 | 1.3e-7   node_value 1.3e-7 | 1.3e-7   (both `additive_half`)
  every flag, trigger index, violation word and NaN pattern equal, in both dtypes

Measured on the device (MI355X; the same sixteen cases through the C ABI, largest over the cases and the compared lanes):
  float64  reward 2.8e-16   node_value 2.8e-16 (`additive_half`); every flag, index, violation word and NaN pattern equal
  float32  reward 1.72e-7   node_value 1.72e-7 (`unnormalized`, against a restatement error of 1.05e-7); `additive_inf` 2.8e-8 and
           `terminal_only` 6.6e-8, against restatement errors of 2.8e-8 and 4.6e-8; largest ratio error / bound of one case and
           output: 0.41 (`unnormalized`, reward and node_value: 1.72e-7 against 4 x 1.05e-7); every flag, index, violation word
           and NaN pattern equal to the float32 restatement's
  independence of the batch-mates (`nested`, `terminations`, `combined` alone and as lanes 193 .. 256 of B = 257): equal bits
  ANYmal (64 lanes, each at its own place and yaw, every fourth in free fall, 5 steps of the PD controller; a nested mixture
  over `momentum`, `power`, `foot_positions` and survive, `base_roll_pitch`, `flying` as a truncation, `mechanical_safety`):
  device against the numpy restatement on the tensors read back, reward 5.6e-17 and node_value 1.1e-16, every flag and index
  equal; an L^1 mixture with normalised weights against `reward_mixture` with the same weights on the live lanes, 1.1e-16.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from jiminy_amd import _abi, _lib, codegen, compositions, load_builtin
from tests import compose_numpy as cn
from tests.hostemu import compose as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_compositions.npz")
TOOL = os.path.join(ROOT, "tools", "make_ref_compositions_fixtures.py")
HEADER = os.path.join(ROOT, "include", "jiminy_hip.h")
TOL = 1e-13
FLOOR32 = 2.0 * float(np.finfo(np.float32).eps)
NEW_SYMBOLS = ("jm_compose_plan_create", "jm_compose_plan_destroy", "jm_block_compose")
FX = np.load(FIXTURE)
CASES = [str(c) for c in FX["cases"]]
FLAG_OUTPUTS = ("terminated", "truncated", "trigger", "violations")
_CASES: dict = {}


def case(name: str):
    """plan, inputs, expected and the two numpy restatements of a case, computed once."""
    if name not in _CASES:
        plan, inputs, expected = cn.load_case(FX, name)
        _CASES[name] = (plan, inputs, expected, cn.quantities(plan, inputs, np.float64), cn.quantities(plan, inputs, np.float32))
    return _CASES[name]


def rel_error(got: np.ndarray, want: np.ndarray) -> float:
    """Largest error relative to max(|want|, 1).  Where `want` is NaN, `got` must be NaN, and nowhere else."""
    assert got.shape == want.shape, (got.shape, want.shape)
    got, want = got.astype(np.float64), want.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN where a number is expected, or the reverse"
    number = ~np.isnan(want)
    if not number.any():
        return 0.0
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1.0))[number].max())


def check_against_the_fixture(name: str, run, label: str) -> None:
    """`run(plan, inputs, dtype) -> outputs` against the fixture in both dtypes."""
    plan, inputs, expected, _, n32 = case(name)
    compared = expected["compare"]
    for dtype in (np.float64, np.float32):
        got = run(plan, inputs, dtype)
        flags_want = expected if dtype is np.float64 else n32
        for out in FLAG_OUTPUTS:
            assert got[out].dtype == cn.OUTPUT_DTYPES[out] and np.array_equal(got[out], flags_want[out]), (name, out, dtype)
        for out in cn.FLOAT_OUTPUTS:
            want = expected[out][..., compared]
            e = rel_error(got[out][..., compared], want)
            if dtype is np.float64:
                print(f"{label} {name} float64 {out}: {e:.2e}")
                assert e <= TOL, (name, out, e)
            else:
                e_np = rel_error(n32[out][..., compared], want)
                bound = max(4.0 * e_np, FLOOR32)
                print(f"{label} {name} float32 {out}: {e:.2e} (numpy float32 {e_np:.2e}, bound {bound:.2e}, ratio {e / bound:.2f})")
                assert e <= bound, (name, out, e, e_np)


# ------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_from_the_reference_tree():
    ref = os.environ.get("JIMINY_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "python", "gym_jiminy")):
        pytest.skip("the reference tree is not here: the committed fixture stands")
    subprocess.check_call([sys.executable, TOOL, "--check"], stdout=subprocess.DEVNULL)


def test_fixture_holds_the_designed_cases():
    assert CASES == ["additive_l1", "additive_l2", "additive_half", "additive_inf", "multiplicative", "nested", "terminal_only",
                     "mixed_terminal", "zero_weight", "unnormalized", "violation", "non_finite", "terminations", "training_only_eval",
                     "training_only_train", "combined"]
    assert os.path.getsize(FIXTURE) <= 1 << 20
    lane = np.arange(64)
    for name in CASES:
        plan, inputs, expected, _, _ = case(name)
        n = len(plan["node_kind"])
        assert expected["reward"].shape == (64,) and expected["node_value"].shape == (n, 64) and inputs["time"].shape == (64,)
        assert all(s.shape == (r, 64) for s, r in zip(inputs["sources"], plan["source_rows"]))
        assert len(set(plan["node_names"])) == n and expected["compare"].all() == (name != "violation")
        assert not (expected["terminated"] & expected["truncated"]).any()
    order = lambda name: float(case(name)[0]["node_order"][0])       # noqa: E731
    assert (order("additive_l1"), order("additive_l2"), order("additive_half"), order("additive_inf")) == (1.0, 2.0, 0.5, np.inf)
    for name in ("additive_l1", "additive_l2", "additive_half"):
        plan, inputs, expected, _, _ = case(name)
        assert list(plan["node_kind"]) == [cn.ADDITIVE] + [cn.LEAF] * 5 and abs(plan["child_weight"].sum() - 1.0) < 1e-12
        assert 24 <= int(expected["terminated"].sum()) <= 40 and (expected["reward"][expected["terminated"] == 1] == 0.0).all()
        assert np.isnan(expected["node_value"][:, expected["terminated"] == 1]).all()
    assert cn.SURVIVE in case("additive_inf")[0]["node_kind"]
    # a geometric mean with an exact zero among the values
    plan, inputs, expected, _, _ = case("multiplicative")
    zero = (inputs["sources"][0][:4] == 0.0).any(0)
    assert zero.any() and (expected["reward"][zero] == 0.0).all() and plan["node_kind"][0] == cn.MULTIPLICATIVE
    # depth 3: multiplicative over [additive L2, additive L^inf with survive, leaf]
    plan = case("nested")[0]
    assert list(plan["node_kind"]) == [3, 2, 0, 0, 2, 0, 1, 0] and list(plan["node_order"][[1, 4]]) == [2.0, np.inf]
    # terminal leaves: evaluated on the terminated lanes only
    plan, inputs, expected, _, _ = case("terminal_only")
    assert (plan["node_terminal"] == 1).all()
    assert np.array_equal(np.isnan(expected["node_value"][0]), expected["terminated"] == 0) and (expected["reward"][expected["terminated"] == 1] > 0).all()
    # behaviour 1: the mixed mixture is indefinite, skipped as a whole at termination, and filters its terminal child elsewhere
    plan, inputs, expected, _, _ = case("mixed_terminal")
    assert list(plan["node_terminal"]) == [-1, 0, 0, 0, 0, 1] and plan["node_names"][-1] == "final"
    done = expected["terminated"] == 1
    assert np.isnan(expected["node_value"][:, done]).all() and (expected["reward"][done] == 0.0).all()
    assert np.isnan(expected["node_value"][5]).all() and not np.isnan(expected["node_value"][:5, ~done]).any()
    # dropped components do not exist in the plan
    plan = case("zero_weight")[0]
    assert plan["node_names"] == ["total", "leaf_0", "leaf_2"] and list(plan["child_weight"]) == [0.4, 0.6]
    plan, inputs, expected, _, _ = case("unnormalized")
    assert not plan["node_normalized"].any() and (expected["violations"] == 0).all() and (inputs["sources"][0][:3] > 1.0).all()
    # the reference's ValueError as the bit of the leaf that left [0, 1]
    plan, inputs, expected, _, _ = case("violation")
    assert np.array_equal(expected["violations"] != 0, lane % 4 == 2) and np.array_equal(expected["compare"], lane % 4 != 2)
    x = inputs["sources"][0][:4]
    for b in np.flatnonzero(lane % 4 == 2):
        (leaf,) = np.flatnonzero((x[:, b] < 0) | (x[:, b] > 1))
        assert expected["violations"][b] == 1 << (leaf + 1)
    # behaviour 3: NaN under L^1 propagates, under L^inf Python's max keeps the total behind the first component
    plan, inputs, expected, _, _ = case("non_finite")
    value, live = expected["node_value"], expected["terminated"] == 0
    behind, first, l1 = live & (lane % 4 == 1), live & (lane % 4 == 2), live & (lane % 4 == 3)
    assert behind.any() and first.any() and l1.any()
    assert not np.isnan(value[1, behind]).any() and np.isnan(value[1, first]).all() and np.isnan(value[5, l1]).all()
    assert np.isnan(value[0, first | l1]).all() and not np.isnan(value[0, behind]).any() and (expected["violations"] == 0).all()
    # six conditions of every kind; every one fires somewhere, base flags pass through, ties and NaN lanes are there
    plan, inputs, expected, _, _ = case("terminations")
    assert len(plan["cond_flags"]) == 6 and list(plan["source_kind"]) == [cn.SRC_DTYPE, cn.SRC_INT32]
    assert list(plan["cond_flags"]) == [1, 0, 1 | 2, 0, 2, 0] and list(plan["cond_grace"]) == [0.25, 0.0, 0.5, 0.0, 0.0, 0.25]
    assert list(plan["elem_bounds"]) == [3, 3, 3, 3, 2, 2, 2, 1, 3] and len(set(plan["elem_low"][:3])) == 3
    assert set(expected["trigger"]) == {-1, 0, 1, 2, 3, 4, 5} and set(inputs["time"]) == {0.0, 0.125, 0.25, 0.375, 0.5, 0.75}
    base = (inputs["base_terminated"] | inputs["base_truncated"]) == 1
    assert base.any() and (expected["trigger"][base] == -1).all()
    assert np.array_equal(expected["terminated"][base], inputs["base_terminated"][base])
    n64 = case("terminations")[3]
    assert np.array_equal(expected["truncated"] == 1, (inputs["base_truncated"] == 1) | np.isin(expected["trigger"], (2, 4)))
    # (the order decides: a lane on which more than one condition would fire alone)
    several = 0
    for b in np.flatnonzero(~base):
        fires = []
        alone = {k: v if k == "training" else [s[:, b:b + 1] for s in v] if k == "sources" else v[b:b + 1] for k, v in inputs.items()}
        for c in range(6):
            # (condition c alone: the others are made `training_only` and the lane is evaluated outside training)
            only = dict(plan, cond_flags=np.where(np.arange(6) == c, plan["cond_flags"], plan["cond_flags"] | 4))
            fires.append(int(cn.quantities(only, alone, training=False)["trigger"][0]) == c)
        several += sum(fires) > 1
        assert n64["trigger"][b] == (fires.index(True) if any(fires) else -1)
    assert several >= 4
    nan_array, nan_scalar, ties = lane % 16 == 9, lane % 16 == 13, lane % 16 == 5
    assert np.isnan(inputs["sources"][0][:3, nan_array]).any(0).all() and np.isnan(inputs["sources"][0][3, nan_scalar]).all()
    late = inputs["time"] >= 0.25
    assert (expected["trigger"][nan_array & late & ~base] == 0).all() and (nan_array & late & ~base).any()
    assert not np.isin(expected["trigger"][nan_scalar], (1, 5)).any()
    assert (inputs["sources"][0][3, ties] == 1.0).all() and not np.isin(expected["trigger"][ties], (0, 1, 2, 4, 5)).any()
    # the same plan and inputs in evaluation and in training mode
    (p_eval, i_eval, e_eval, _, _), (p_train, i_train, e_train, _, _) = case("training_only_eval"), case("training_only_train")
    assert all(np.array_equal(p_eval[k], p_train[k]) for k in cn.PLAN_KEYS) and list(p_eval["cond_flags"]) == [0, 1 | 4, 2 | 4, 1]
    assert np.array_equal(i_eval["sources"][0], i_train["sources"][0]) and not i_eval["training"] and i_train["training"]
    assert not np.isin(e_eval["trigger"], (1, 2)).any() and np.isin(e_train["trigger"], (1, 2)).any()
    # terminations feeding the reward
    plan, inputs, expected, _, _ = case("combined")
    assert len(plan["cond_flags"]) == 3 and plan["node_names"][-1] == "final" and set(expected["trigger"]) == {-1, 0, 1, 2}
    done = expected["terminated"] == 1
    assert (expected["reward"][done] == 0.0).all() and (expected["reward"][~done] > 0.0).all() and (expected["truncated"][~done] == 1).any()


# ------------------------------------------------------------------------------------------------------ the host side
@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference(name):
    plan, inputs, expected, n64, n32 = case(name)
    compared = expected["compare"]
    for out in FLAG_OUTPUTS:
        assert np.array_equal(n64[out], expected[out]) and np.array_equal(n32[out], expected[out]), out
    for out in cn.FLOAT_OUTPUTS:
        assert rel_error(n64[out][..., compared], expected[out][..., compared]) <= TOL, out
        assert rel_error(n32[out][..., compared], expected[out][..., compared]) <= 1e-6, out      # (the yardstick is sane)


def _emu_run(plan, inputs, dtype=np.float64, **kw):
    return emu.run(plan, inputs, dtype, **kw)


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_matches_the_reference(name):
    check_against_the_fixture(name, _emu_run, "emulation")


def _untouched(name: str, a: np.ndarray) -> bool:
    return bool((a == (7 if name in cn.OUTPUT_DTYPES else 7.25)).all())


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_null_outputs_and_lane_mask(run) -> None:
    """`run(plan, inputs, dtype, outputs=, mask=) -> the outputs asked for` on `combined` and `terminations`: an output that is
    not asked for changes no other; with a mask, with NaN and garbage in the inputs of the other lanes, those lanes keep every
    row; without the optional inputs the time is 0 and the base flags are clear."""
    for name in ("combined", "terminations"):
        plan, inputs, _, _, _ = case(name)
        for dtype in (np.float64, np.float32):
            full = run(plan, inputs, dtype)
            assert sorted(full) == sorted(cn.OUTPUTS)
            assert not any(_untouched(k, v) for k, v in full.items() if v.size)
            for asked in (("reward",), ("node_value", "trigger"), ("terminated", "truncated"), ("violations",), ("trigger", "reward"), ()):
                got = run(plan, inputs, dtype, outputs=asked)
                assert sorted(got) == sorted(asked) and all(_same_bits(got[k], full[k]) for k in asked), asked
            mask = np.arange(64) % 3 == 0
            poisoned = dict(inputs, sources=[s.copy() for s in inputs["sources"]], time=inputs["time"].copy())
            poisoned["sources"][0][:, ~mask] = np.where(np.arange(64)[~mask] % 2 == 0, np.nan, -3.0e38)
            poisoned["sources"][1][:, ~mask] = -2 ** 31
            poisoned["time"][~mask] = np.nan
            got = run(plan, poisoned, dtype, mask=mask)
            for k, v in got.items():
                assert _same_bits(v[..., mask], full[k][..., mask]) and _untouched(k, v[..., ~mask]), (name, k)
            bare = run(plan, {k: v for k, v in inputs.items() if k in ("sources", "training")}, dtype)
            want = cn.quantities(plan, dict(inputs, time=np.zeros(64), base_terminated=np.zeros(64, np.uint8),
                                            base_truncated=np.zeros(64, np.uint8)), dtype)
            assert all(np.array_equal(bare[k], want[k]) for k in FLAG_OUTPUTS)


def test_emulated_null_outputs_and_lane_mask():
    check_null_outputs_and_lane_mask(_emu_run)


def _good() -> dict:
    plan = case("combined")[0]
    return {k: np.array(plan[k]) for k in cn.PLAN_KEYS}


def _set_at(index, value):
    def f(a):
        a = a.copy()
        a.reshape(-1)[index] = value
        return a
    return f


def _chain(n_levels: int) -> dict:
    """A chain of `n_levels - 1` multiplicative mixtures of one child each over one leaf."""
    n, i32 = n_levels, np.int32
    return dict(_good(), node_kind=np.array([3] * (n - 1) + [0], i32), node_terminal=np.zeros(n, i32), node_normalized=np.ones(n, i32),
                node_slot=np.zeros(n, i32), node_row=np.zeros(n, i32), node_child_start=np.array(list(range(n - 1)) + [0], i32),
                node_child_count=np.array([1] * (n - 1) + [0], i32), node_order=np.ones(n), child=np.arange(1, n, dtype=i32),
                child_weight=np.ones(n - 1))


def _wide(n_leaves: int) -> dict:
    n, i32 = n_leaves + 1, np.int32
    return dict(_good(), node_kind=np.array([2] + [0] * n_leaves, i32), node_terminal=np.zeros(n, i32), node_normalized=np.ones(n, i32),
                node_slot=np.zeros(n, i32), node_row=np.zeros(n, i32), node_child_start=np.zeros(n, i32),
                node_child_count=np.array([n_leaves] + [0] * n_leaves, i32), node_order=np.ones(n), child=np.arange(1, n, dtype=i32),
                child_weight=np.ones(n_leaves))


def _conditions(n_conditions: int, n_each: int) -> dict:
    n, i32 = n_conditions * n_each, np.int32
    return dict(_good(), cond_elem_start=np.arange(n_conditions, dtype=i32) * n_each, cond_elem_count=np.full(n_conditions, n_each, i32),
                cond_flags=np.ones(n_conditions, i32), cond_grace=np.zeros(n_conditions), elem_slot=np.zeros(n, i32),
                elem_row=np.zeros(n, i32), elem_bounds=np.full(n, 3, i32), elem_low=np.zeros(n), elem_high=np.ones(n))


def _rejections() -> list:
    """(the arrays of a malformed description, what the message must say) for every rejection of `jm_compose_plan_create`.
    The good description is `combined`: nodes root(3) [add(2) [a, b], last_resort(2) [c, survive], d, final], two sources."""
    change = lambda **kw: {**_good(), **{k: f(_good()[k]) for k, f in kw.items()}}       # noqa: E731
    return [
        (change(node_slot=_set_at(2, 2)), "node 2 reads slot 2, out of range"),
        (change(node_slot=_set_at(2, -1)), "node 2 reads slot -1"),
        (change(node_row=_set_at(3, 8)), "node 3 reads row 8, out of range"),
        (change(elem_slot=_set_at(0, 5)), "element 0 reads slot 5"),
        (change(elem_row=_set_at(3, 1)), "element 3 reads row 1, out of range"),
        (change(child=_set_at(0, 9)), "child 9, out of range"),
        (change(child=_set_at(0, -1)), "child -1, out of range"),
        (change(child=_set_at(0, 1)), "a cycle"),                               # (node 1 its own child)
        (change(child=_set_at(2, 0)), "a cycle"),                               # (the root below node 4)
        (change(child=_set_at(1, 2)), "not the child of exactly one node"),     # (node 2 twice, node 3 never)
        (change(node_child_start=_set_at(1, 7)), "child entries out of range"),
        (change(node_child_count=_set_at(1, 0)), "At least one reward component"),
        (change(node_kind=_set_at(2, 4)), "unknown kind"),
        (change(node_terminal=_set_at(2, 2)), "is_terminal"),
        (_chain(5), "depth of 4 levels"),
        (_wide(32), "at most 32 reward nodes are supported, got 33"),
        (_conditions(17, 1), "at most 16 termination conditions are supported, got 17"),
        (_conditions(5, 13), "at most 64 termination elements are supported, got 65"),
        (change(node_order=_set_at(1, 0.0)), "'order' must be strictly positive"),
        (change(node_order=_set_at(1, -2.0)), "'order' must be strictly positive"),
        (change(node_order=_set_at(4, float("nan"))), "'order' must be strictly positive"),
        (change(child_weight=_set_at(0, 0.0)), "weight that is not positive"),
        (change(elem_low=_set_at(0, 0.75)), "low bound above its high bound"),
        (change(cond_elem_start=_set_at(2, 4)), "condition 2 has elements out of range"),
        (change(cond_elem_count=_set_at(1, 0)), "condition 1 has elements out of range"),
        (change(cond_elem_count=_set_at(1, 2)), "scalar form and has more than one element"),
        (change(cond_flags=_set_at(0, 8)), "unknown flags"),
        (change(elem_bounds=_set_at(0, 4)), "unknown bound flags"),
        (change(source_kind=_set_at(1, 3)), "element kind other than"),
        (change(source_rows=_set_at(0, 0)), "has no rows"),
        (change(source_kind=lambda a: np.zeros(17, np.int32), source_rows=lambda a: np.ones(17, np.int32)), "at most 16 sources"),
    ]


def test_plan_validation_rejects_every_malformed_description():
    emu.pack(compositions.make_desc(**_good())[0])
    for accepted in (_chain(4), _wide(31), _conditions(16, 4)):         # (the caps themselves are accepted)
        d, keep = compositions.make_desc(**accepted)
        emu.pack(d)
    with pytest.raises(ValueError, match="null description"):
        emu.pack(None)
    for key in cn.PLAN_KEYS:
        d, keep = compositions.make_desc(**_good())
        setattr(d, key, None)
        with pytest.raises(ValueError, match="null array"):
            emu.pack(d)
    for arrays, message in _rejections():
        d, keep = compositions.make_desc(**arrays)
        with pytest.raises(ValueError, match=message):
            emu.pack(d)


def _prebuilt(model):
    path = codegen.lib_path(model)
    if not os.path.exists(path):
        pytest.skip(f"{os.path.basename(path)} not built (run __graft_entry__.build())")
    return _lib.load_for(model, allow_build=False)


def _last_error(lib) -> str:
    buf = C.create_string_buffer(1024)
    lib.L.jm_last_error(buf, 1024)
    return buf.value.decode()


def test_plan_create_validates_before_touching_the_device():
    """The same rejections through the C ABI of a built library, on a machine without a device: JM_EINVAL and a message."""
    lib = _prebuilt(load_builtin("cartpole"))
    h = C.c_void_p()
    assert lib.L.jm_compose_plan_create(None, C.byref(h)) == _abi.JM_EINVAL and "null description" in _last_error(lib)
    desc, keep = compositions.make_desc(**_good())
    assert lib.L.jm_compose_plan_create(C.byref(desc), None) == _abi.JM_EINVAL
    desc.child = None
    assert lib.L.jm_compose_plan_create(C.byref(desc), C.byref(h)) == _abi.JM_EINVAL and "null array" in _last_error(lib)
    for arrays, message in _rejections():
        d, keep_ = compositions.make_desc(**arrays)
        rc = lib.L.jm_compose_plan_create(C.byref(d), C.byref(h))
        assert rc == _abi.JM_EINVAL and not h.value and message in _last_error(lib), (message, _last_error(lib))
        with pytest.raises(ValueError):
            lib.check(rc)
    io = _abi.ComposeIO()
    assert lib.L.jm_block_compose(None, _abi.JM_F64, 64, C.byref(io), 1, None) == _abi.JM_EINVAL
    assert "null argument" in _last_error(lib)


def test_abi_version_and_symbols():
    header = open(HEADER).read()
    assert _abi.ABI_VERSION == 11
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in header and name in _lib.ABI_SYMBOLS, name
    # the order of the fields in the header is the order of the ctypes mirrors
    body = header.split("typedef struct jm_compose_desc")[1].split("} jm_compose_desc;")[0]
    order = [line.split(";")[0].split()[-1] for line in body.splitlines() if ";" in line]
    assert order == [f[0] for f in _abi.ComposeDesc._fields_]
    body = header.split("typedef struct jm_compose_io")[1].split("} jm_compose_io;")[0]
    order = [line.split(";")[0].split()[-1].split("[")[0] for line in body.splitlines() if ";" in line]
    assert order == list(_abi.COMPOSE_IO_FIELDS) and "const void * source[16];" in body and _abi.COMPOSE_MAX_SOURCES == 16
    assert "jm_compose.h" in open(os.path.join(ROOT, "jiminy_amd", "codegen.py")).read()
    lib = _prebuilt(load_builtin("cartpole"))
    assert lib.L.jm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert getattr(lib.L, name) is not None


# ------------------------------------------------------------------------------------------------- the Python surface
def _describe(name: str, torch):
    """The reward and the terminations of a fixture case as descriptions of `jiminy_amd.compositions` on CPU tensors."""
    from jiminy_amd.compositions import AdditiveMixtureReward as Add, MultiplicativeMixtureReward as Mul, RewardTerm, SurviveReward, Termination
    plan, inputs, _, _, _ = case(name)
    src = [torch.as_tensor(np.ascontiguousarray(a)) for a in cn.cast_sources(plan, inputs["sources"], np.float64)]
    x = src[0]
    if name in ("nested", "combined"):
        parts = [Add("add", [RewardTerm("a", x[0]), RewardTerm("b", x[1])], 2, (0.5, 0.5)),
                 Add("last_resort", [RewardTerm("c", x[2]), SurviveReward()], "inf", (1.0, 0.4)), RewardTerm("d", x[3])]
        if name == "combined":
            parts.append(RewardTerm("final", x[4], is_terminal=True))
        reward = Mul("root", parts)
    elif name == "mixed_terminal":
        reward = Mul("root", [Add("add", [RewardTerm("a", x[0]), RewardTerm("b", x[1])], 2, (0.5, 0.5)), SurviveReward(),
                              RewardTerm("final", x[2], is_terminal=True)])
    elif name == "zero_weight":
        reward = Add("total", [RewardTerm(f"leaf_{i}", x[i]) for i in range(5)], 1, (0.4, 0.0, 0.6, 0.0, -0.5))
    elif name == "unnormalized":
        reward = Add("total", [RewardTerm(f"cost_{i}", x[i], is_normalized=False) for i in range(3)], 1, (0.5, 0.25, 0.25))
    else:
        reward = None
    terminations = []
    if name == "combined":
        terminations = [Termination("posture", x[5:7], [-0.5, -0.5], [0.5, 0.5], 0.25),
                        Termination("flying", x[7], None, 0.3, is_truncation=True), Termination("safety", src[1][0], None, 0, 0.125)]
    elif name == "terminations":
        terminations = [Termination("posture", x[:3], [-0.5, -0.4, -1.0], [0.5, 0.6, 1.0], 0.25), Termination("height", x[3], -1.0, 1.0),
                        Termination("flying", x[4:6], None, 2.0, 0.5, is_truncation=True), Termination("safety", src[1][1], None, 0.0),
                        Termination("progress", x[6], 0.2, None, is_truncation=True), Termination("drift", x[7], -1.0, 1.0, 0.25)]
    return reward, terminations, src


@pytest.mark.parametrize("name", ["nested", "mixed_terminal", "zero_weight", "unnormalized", "terminations", "combined"])
def test_descriptions_build_the_plan_of_the_reference_objects(name, caplog):
    """The description classes derive `is_terminal` / `is_normalized`, drop and order what the reference's constructors do: the
    plan `build_plan` packs equals, array for array, the one the fixture tool read off the reference's objects."""
    import torch
    with caplog.at_level(logging.WARNING, logger="jiminy_amd.compositions"):
        reward, terminations, src = _describe(name, torch)
    assert ("is not normalized" in caplog.text) == (name == "unnormalized")
    plan = compositions.build_plan(reward, terminations, 64, torch.float64)
    want = case(name)[0]
    assert plan.node_names == want["node_names"] and plan.condition_names == want["condition_names"]
    for key in cn.PLAN_KEYS:
        assert np.array_equal(np.asarray(plan.arrays[key], dtype=want[key].dtype), want[key]), key
    assert plan.source_ptr == [s.data_ptr() for s in src[:len(plan.source_ptr)]]
    emu.pack(plan.desc()[0])


def test_description_errors():
    import torch
    from jiminy_amd.compositions import AdditiveMixtureReward as Add, MultiplicativeMixtureReward as Mul, RewardTerm, SurviveReward, Termination
    x = torch.zeros(8, 4, dtype=torch.float64)
    leaf = lambda i, **kw: RewardTerm(f"leaf_{i}", x[i], **kw)       # noqa: E731
    build = lambda reward=None, terminations=(): compositions.build_plan(reward, terminations, 4, torch.float64)       # noqa: E731
    for order in (0, -1.0, "sup"):
        with pytest.raises(ValueError, match="'order' must be strictly positive or 'inf'."):
            Add("total", [leaf(0)], order)
    with pytest.raises(ValueError, match="Exactly one weight per reward component must be specified."):
        Add("total", [leaf(0), leaf(1)], 1, (1.0,))
    with pytest.raises(ValueError, match="At least one reward component"):
        Mul("total", [])
    with pytest.raises(ValueError, match="At least one reward component"):
        Add("total", [leaf(0), leaf(1)], 1, (0.0, -1.0))
    with pytest.raises(KeyError, match="Key 'leaf_0' already reserved in 'info'"):
        build(Mul("total", [leaf(0), Add("add", [leaf(0)])]))
    with pytest.raises(KeyError, match="already reserved"):
        build(Mul("total", [SurviveReward(), Add("add", [SurviveReward()])]))
    # derived flags
    assert Add("t", [leaf(0), leaf(1)], 1, (0.5, 0.5)).is_normalized and not Add("t", [leaf(0), leaf(1)], 1, (0.5, 0.6)).is_normalized
    assert Add("t", [leaf(0), leaf(1)], "inf", (1.0, 0.6)).is_normalized and not Add("t", [leaf(0), leaf(1)], "inf", (0.5, 0.6)).is_normalized
    assert Add("t", [leaf(0), leaf(1)], float("inf"), (1.0, 0.6)).order == float("inf")
    assert not Mul("t", [leaf(0), leaf(1, is_normalized=False)]).is_normalized
    assert Mul("t", [leaf(0, is_terminal=True), leaf(1, is_terminal=True)]).is_terminal is True
    assert Mul("t", [leaf(0, is_terminal=True), leaf(1)]).is_terminal is None and Mul("t", [leaf(0, is_terminal=None)]).is_terminal is None
    assert Mul("t", [leaf(0), SurviveReward()]).is_terminal is False
    # the bounds of the kernel, by name
    deep = leaf(0)
    for level in range(4):
        deep = Mul(f"level_{level}", [deep])
    with pytest.raises(ValueError, match="deeper than 4 levels"):
        build(deep)
    build(deep.components[0])
    with pytest.raises(ValueError, match="at most 32 reward nodes"):
        build(Mul("root", [Mul(f"m{j}", [RewardTerm(f"l{j}_{i}", x[i]) for i in range(8)]) for j in range(4)]))
    term = lambda i, rows=None, **kw: Termination(f"term_{i}", x[0] if rows is None else rows, 0.0, 1.0, **kw)       # noqa: E731
    with pytest.raises(ValueError, match="at most 16 termination conditions are supported, got 17"):
        build(terminations=[term(i) for i in range(17)])
    with pytest.raises(ValueError, match="at most 64 termination elements in total are supported, got 72"):
        build(terminations=[term(i, x) for i in range(9)])
    with pytest.raises(KeyError, match="share a name"):
        build(terminations=[term(0), term(0)])
    with pytest.raises(ValueError, match="a low bound lies above its high bound"):
        build(terminations=[Termination("t", x[:2], [0.0, 2.0], 1.0)])
    with pytest.raises(ValueError, match="expected one bound or one per element"):
        build(terminations=[Termination("t", x[:3], [0.0, 2.0], None)])
    with pytest.raises(ValueError, match="at most 16 source tensors"):
        build(Mul("root", [RewardTerm(f"r{i}", torch.zeros(4, dtype=torch.float64)) for i in range(17)]))
    with pytest.raises(ValueError, match="expected a view"):
        build(terminations=[Termination("t", x[:, :2], 0.0, None)])
    with pytest.raises(ValueError, match="does not start on a row"):
        build(terminations=[Termination("t", x.reshape(-1)[2:6], 0.0, None)])
    with pytest.raises(ValueError, match="engine dtype, int32, uint8 or bool"):
        build(terminations=[Termination("t", torch.zeros(4, dtype=torch.float32), 0.0, None)])
    with pytest.raises(ValueError, match="expected one row"):
        build(RewardTerm("r", x[:2]))
    # strided views: every element finds its row
    plan = build(terminations=[Termination("t", x.view(2, 4, 4)[:, 1], 0.0, None), Termination("b", torch.zeros(4, dtype=torch.bool), None, 0)])
    assert plan.arrays["elem_row"] == [1, 5, 0] and plan.arrays["elem_slot"] == [0, 0, 1] and plan.arrays["source_kind"] == [0, 2]
    assert plan.arrays["cond_flags"] == [1, 0] and plan.arrays["source_rows"] == [8, 1]


# ------------------------------------------------------------------------------------------------------------ device
class DeviceCompose:
    """A plan on the device and the launch on numpy arrays (copied in and out)."""

    def __init__(self, lib, plan: dict, device):
        import torch
        self.torch, self.lib, self.device, self.plan = torch, lib, device, plan
        desc, keep = emu.plan_desc(plan)
        self.h = C.c_void_p()
        with torch.cuda.device(device):
            lib.check(lib.L.jm_compose_plan_create(C.byref(desc), C.byref(self.h)))

    def close(self):
        self.lib.L.jm_compose_plan_destroy(self.h)

    def run(self, inputs: dict, dtype=np.float64, outputs=cn.OUTPUTS, mask=None, fill=7.25, training=None, as_tensors=False):
        torch, plan = self.torch, self.plan
        sources = cn.cast_sources(plan, inputs["sources"], dtype)
        B = sources[0].shape[-1]
        io, held, out = _abi.ComposeIO(), [], {}
        put = lambda a: held.append(torch.as_tensor(np.ascontiguousarray(a), device=self.device)) or held[-1].data_ptr()      # noqa: E731
        for s, a in enumerate(sources):
            io.source[s] = put(a)
        for name, kind in (("time", dtype), ("base_terminated", np.uint8), ("base_truncated", np.uint8)):
            if inputs.get(name) is not None:
                setattr(io, name, put(np.asarray(inputs[name], dtype=kind)))
        if mask is not None:
            io.lane_mask = put(np.asarray(mask, dtype=np.uint8))
        for name in outputs:
            out[name] = torch.as_tensor(emu.new_output(name, plan, B, np.dtype(dtype), fill), device=self.device)
            setattr(io, name, out[name].data_ptr())
        training = inputs["training"] if training is None else training
        self.lib.check(self.lib.L.jm_block_compose(self.h, _abi.JM_F64 if np.dtype(dtype) == np.float64 else _abi.JM_F32, B, C.byref(io),
                                                   int(bool(training)), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        torch.cuda.synchronize(self.device)
        del held
        return out if as_tensors else {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_matches_the_reference(name, gpu_device):
    """Every fixture case through the C ABI at B = 64, both dtypes."""
    dev = DeviceCompose(_prebuilt(load_builtin("cartpole")), case(name)[0], gpu_device)
    try:
        check_against_the_fixture(name, lambda plan, inputs, dtype: dev.run(inputs, dtype), "device")
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nested", "terminations", "combined"])
def test_device_is_independent_of_the_batch_mates(name, gpu_device):
    """The 64 lanes launched alone and as the lanes 193 .. 256 of B = 257 (the second block then holds one lane; the lanes in
    front hold lanes of the case in another order): `torch.equal` on every output, in both dtypes."""
    import torch
    plan, inputs = case(name)[:2]
    dev = DeviceCompose(_prebuilt(load_builtin("cartpole")), plan, gpu_device)
    try:
        lanes = np.concatenate([np.random.default_rng(5).integers(0, 64, 193), np.arange(64)])
        big_inputs = {k: v if k == "training" else [np.ascontiguousarray(s[:, lanes]) for s in v] if k == "sources" else v[lanes]
                      for k, v in inputs.items()}
        for dtype in (np.float64, np.float32):
            small, big = dev.run(inputs, dtype, as_tensors=True), dev.run(big_inputs, dtype, as_tensors=True)
            for out in cn.OUTPUTS:
                assert big[out].shape[-1] == 257
                a, b = small[out], big[out][..., 193:]
                if a.is_floating_point():       # (NaN marks the nodes that were not evaluated: compare the bits)
                    a, b = a.contiguous().view(torch.int64 if dtype is np.float64 else torch.int32), \
                        b.contiguous().view(torch.int64 if dtype is np.float64 else torch.int32)
                assert torch.equal(a, b), (out, dtype)
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_null_outputs_and_lane_mask(gpu_device):
    """An output that is not asked for changes no other; with a mask the other lanes, whose inputs hold NaN and garbage, keep
    every row unwritten."""
    lib = _prebuilt(load_builtin("cartpole"))
    devs = {name: DeviceCompose(lib, case(name)[0], gpu_device) for name in ("combined", "terminations")}
    by_plan = {id(case(name)[0]): dev for name, dev in devs.items()}
    try:
        check_null_outputs_and_lane_mask(lambda plan, inputs, dtype, **kw: by_plan[id(plan)].run(inputs, dtype, **kw))
    finally:
        for dev in devs.values():
            dev.close()


# ------------------------------------------------------------------------------------------------------ the environment
def test_python_surface_refusals_on_the_host(monkeypatch):
    import torch

    from jiminy_amd import blocks
    from jiminy_amd.compositions import AdditiveMixtureReward as Add, RewardTerm, SurviveReward, Termination
    from jiminy_amd.envs import PDControlledWalkerVecEnv, VecJiminyEnv, WalkerVecEnv
    model = load_builtin("anymal")
    engine = SimpleNamespace(model=model, dtype=torch.float64, device=torch.device("cpu"), batch_size=4, _lib=SimpleNamespace(L=None, check=None))
    monkeypatch.setenv("JIMINY_AMD_TENSOR_BLOCKS", "1")
    with pytest.raises(NotImplementedError, match="the composition layer has no tensor-program form"):
        blocks.Composition(engine, SurviveReward())
    monkeypatch.delenv("JIMINY_AMD_TENSOR_BLOCKS")
    with pytest.raises(ValueError, match="expected one row"):
        blocks.Composition(engine, RewardTerm("r", torch.zeros(2, 4, dtype=torch.float64)))
    with pytest.raises(TypeError, match="expected a Termination"):
        blocks.Composition(engine, None, [("flying", (0.1, 0.0))])

    def bare_init(self, *args, **kw):
        self.model, self.num_envs, self.step_dt, self.dtype, self.device, self.engine = model, 4, 0.04, torch.float64, torch.device("cpu"), None
    monkeypatch.setattr(VecJiminyEnv, "__init__", bare_init)
    with pytest.raises(ValueError, match="reward= and reward_mixture= both describe the reward"):
        WalkerVecEnv(reward=SurviveReward(), reward_mixture={"survival": 1.0})
    with pytest.raises(ValueError, match="termination_conditions= and terminations= both describe the terminations"):
        WalkerVecEnv(termination_conditions=[], terminations={})
    with pytest.raises(ValueError, match="unknown reward term 'speed'"):
        WalkerVecEnv(reward=Add("total", ["speed", SurviveReward()]))
    with pytest.raises(ValueError, match="unknown reward term 'survival'"):         # (not block-backed: `SurviveReward()` is its node)
        WalkerVecEnv(reward=RewardTerm("survival"))
    with pytest.raises(TypeError, match="expects a description of jiminy_amd.compositions"):
        WalkerVecEnv(reward={"momentum": 1.0})
    with pytest.raises(ValueError, match="unknown terminations \\['speed'\\]"):
        WalkerVecEnv(termination_conditions=[("speed", (1.0, 0.0))])
    with pytest.raises(ValueError, match="the termination 'flying' is given twice"):
        WalkerVecEnv(termination_conditions=[("flying", (1.0, 0.0)), ("flying", (2.0, 0.0))])
    with pytest.raises(ValueError, match="unknown options of the termination 'flying'"):
        WalkerVecEnv(termination_conditions=[("flying", (1.0, 0.0), dict(grace_period=1.0))])
    with pytest.raises(ValueError, match="termination 'mine' has no rows"):
        WalkerVecEnv(termination_conditions=[Termination("mine", None, 0.0, 1.0)])
    with pytest.raises(TypeError, match="expects compositions.Termination or"):
        WalkerVecEnv(termination_conditions=["flying"])
    # a named entry requires its block with the words of the dictionaries
    with pytest.raises(ValueError, match="the momentum and friction reward terms read the locomotion quantities block"):
        WalkerVecEnv(reward=Add("total", ["momentum", SurviveReward()]))
    with pytest.raises(ValueError, match=r"reward_mixture\['momentum'\] needs locomotion_quantities\['momentum_cutoff'\]"):
        WalkerVecEnv(reward=Add("total", [RewardTerm("momentum")]), locomotion_quantities={})
    with pytest.raises(ValueError, match="the power reward term reads the actuated-joint quantities block"):
        WalkerVecEnv(reward=Add("total", ["power"]))
    with pytest.raises(ValueError, match="the robustness reward term reads the support polygon block"):
        WalkerVecEnv(reward=Add("total", [Add("inner", ["robustness"])]))
    with pytest.raises(ValueError, match="the flying and impact_force terminations read the locomotion quantities block"):
        WalkerVecEnv(termination_conditions=[("flying", (0.1, 0.0), dict(is_truncation=True))])
    with pytest.raises(ValueError, match="the mechanical_safety and power_consumption terminations read the actuated-joint"):
        WalkerVecEnv(termination_conditions=[("mechanical_safety", (0.0, 10.0, 0.0))])
    with pytest.raises(ValueError, match="the terminations read the frame kinematics block"):
        WalkerVecEnv(termination_conditions=[("base_roll_pitch", (-0.3, 0.3, 0.0))])
    with pytest.raises(ValueError, match="needs trajectory_tracking\\['foot_horizon'\\]"):
        WalkerVecEnv(termination_conditions=[("shift_foot_positions", (0.1, 0.0))], trajectory_tracking={})
    # the dictionaries the named entries stand for
    assert WalkerVecEnv._named_reward_terms(Add("t", ["momentum", Add("u", ["power", SurviveReward(), RewardTerm("x", torch.zeros(4))])])) == \
        ["momentum", "power"]
    assert WalkerVecEnv._named_terminations([("flying", (0.1, 0.5)), Termination("x", torch.zeros(4), 0, 1),
                                             ("mechanical_safety", (0.0, 9.0, 0.0), {})]) == {"flying": (0.1, 0.5), "mechanical_safety": (0.0, 9.0, 0.0)}
    assert len(WalkerVecEnv.COMPOSED_REWARD_TERMS) == 11
    # whole-step graphs refuse the block
    env = object.__new__(PDControlledWalkerVecEnv)
    env.engine = SimpleNamespace(_adaptive=None, _sensor_noise=None, _impulse_forces=None, _profile_forces=None, _process_forces=None)
    env._hip_blocks, env.auto_reset, env.std_ratio, env._ground_patch_extent = object(), True, {}, None
    env.frames = env.actuation = env.tracking = env.trajectory = env._mahony = None
    env.composition = object()
    with pytest.raises(NotImplementedError, match="whole-step graphs do not take the composition block"):
        env.enable_graph(True, whole_step=True)


def _anymal(device, monkeypatch, B=64, steps=5, **kw):
    """An ANYmal environment with constraint contacts under its PD controller (zero action), every lane at its own place and
    yaw; the lanes 1 mod 4 start 3 m above the ground and are in free fall for the steps of the test."""
    import torch

    from jiminy_amd.envs import VecJiminyEnv, make_anymal_env
    high = torch.arange(B, device=device) % 4 == 1
    sample = VecJiminyEnv._sample_state

    def lifted(self, n):
        q, v = sample(self, n)
        q = q.clone()
        q[2] += torch.where(high, 3.0, 0.0).to(q.dtype)
        lane = torch.arange(B, device=device).to(q.dtype)
        yaw = 0.1 * lane - 3.0
        s, c = torch.sin(0.5 * yaw), torch.cos(0.5 * yaw)
        x, y, z, w_ = q[3].clone(), q[4].clone(), q[5].clone(), q[6].clone()
        q[3], q[4], q[5], q[6] = c * x - s * y, c * y + s * x, c * z + s * w_, c * w_ - s * z
        q[0] += 0.05 * lane
        q[1] -= 0.03 * lane
        return q, v
    if sample.__name__ != "lifted":         # (once per test, however many environments it builds)
        monkeypatch.setattr(VecJiminyEnv, "_sample_state", lifted)
    env = make_anymal_env(B, device=device, contact_model="constraint", auto_reset=False, **kw)
    env.reset(seed=3)
    action = torch.zeros(B, env.model.nmotors, dtype=torch.float64, device=device)
    out = None
    for _ in range(steps):
        out = env.step(action)
    return env, out, high


def _block_case(env):
    """The plan and the inputs of the last launch of `env.composition`, read back (every source as `[rows][B]`)."""
    block, B = env.composition, env.num_envs
    plan = {k: np.asarray(v) for k, v in block.plan.arrays.items()}
    sources = []
    for t in block.plan.sources:
        base = t if t._base is None else t._base
        assert base.is_contiguous() and base.data_ptr() == t.untyped_storage().data_ptr()
        sources.append(base.reshape(-1, B).cpu().numpy())
    base_terminated, base_truncated = (f.cpu().numpy().astype(np.uint8) for f in env._composition_base)
    return plan, dict(sources=sources, time=env._composition_time.cpu().numpy(), base_terminated=base_terminated,
                      base_truncated=base_truncated, training=env.training)


@pytest.mark.gpu
def test_environment_reward_and_termination_conditions(gpu_device, monkeypatch):
    """ANYmal, 64 lanes each at its own yaw (every fourth in free fall), the PD pipeline, five steps.  `reward=` a nested mixture
    over `momentum`, `power`, `foot_positions` and survive, `termination_conditions=` `base_roll_pitch`, `flying` (a truncation)
    and `mechanical_safety`: the block's outputs against the numpy restatement on the tensors read back; an L^1 mixture with
    normalised weights against `reward_mixture` with the same weights on a second environment stepped identically, on the
    lanes that did not terminate; the keys and shapes of `info`."""
    import torch

    from jiminy_amd.compositions import AdditiveMixtureReward as Add, MultiplicativeMixtureReward as Mul, SurviveReward
    blocks_cfg = dict(locomotion_quantities=dict(momentum_cutoff=2.0), foot_poses=dict(position_cutoff=0.5),
                      actuated_joints=dict(power_cutoff=200.0, power_horizon=0.2))
    reward = Mul("total", [Add("effort", ["momentum", "power"], 2, (0.5, 0.5)),
                           Add("last_resort", ["foot_positions", SurviveReward()], "inf", (1.0, 0.25))])
    conditions = [("base_roll_pitch", (-0.4, 0.4, 0.0)), ("flying", (0.3, 0.04), dict(is_truncation=True)),
                  ("mechanical_safety", (0.0, 12.0, 0.0))]
    env, out, high = _anymal(gpu_device, monkeypatch, reward=reward, termination_conditions=conditions, **blocks_cfg)
    # the blocks the dictionaries would build
    want = dict(reward_mixture={"momentum": 1.0, "power": 1.0, "foot_positions": 1.0},
                terminations={"base_roll_pitch": (-0.4, 0.4, 0.0), "flying": (0.3, 0.04), "mechanical_safety": (0.0, 12.0, 0.0)})
    twin, _, _ = _anymal(gpu_device, monkeypatch, steps=1, **want, **blocks_cfg)
    assert env.frames.frame_names == twin.frames.frame_names and env.frames.rpy is not None and env.frames.average == twin.frames.average
    assert (env.actuation.position_margin, env.actuation.velocity_max) == (twin.actuation.position_margin, twin.actuation.velocity_max) == (0.0, 12.0)
    assert twin.composition is None and env.training is True
    block = env.composition
    assert block.node_names == ["total", "effort", "momentum", "power", "last_resort", "foot_positions", "reward_survive"]
    assert block.condition_names == ["base_roll_pitch", "flying", "mechanical_safety"]
    torch.cuda.synchronize(gpu_device)
    plan, inputs = _block_case(env)
    host = cn.quantities(plan, inputs)
    dev = {k: getattr(block, k).cpu().numpy() for k in cn.OUTPUTS}
    for k in FLAG_OUTPUTS:
        assert np.array_equal(dev[k], host[k]), k
    for k in cn.FLOAT_OUTPUTS:
        e = rel_error(dev[k], host[k])
        print(f"ANYmal, device against the numpy restatement, {k}: {e:.2e}")
        assert e <= TOL, (k, e)
    obs, rew, terminated, truncated, info = out
    high_ = high.cpu().numpy()
    assert (dev["truncated"][high_] == 1).all() and (dev["trigger"][high_] == 1).all()          # the lanes in free fall fly
    assert not dev["terminated"][~high_].any() and (dev["trigger"][~high_] == -1).all() and (dev["violations"] == 0).all()
    assert torch.equal(terminated, block.terminated.bool()) and torch.equal(truncated, block.truncated.bool())
    assert torch.equal(rew, torch.nan_to_num(block.reward, nan=0.0, posinf=0.0, neginf=0.0)) and float(rew[~high].min()) > 0.0
    assert sorted(info) == ["reward", "terminated", "truncated", "violations"]
    assert list(info["reward"]) == block.node_names and all(v.shape == (64,) for v in info["reward"].values())
    assert info["terminated"].dtype == torch.int32 and (info["terminated"] == -1).all()
    assert torch.equal(info["truncated"], torch.where(high, 1, -1).to(torch.int32)) and info["violations"].shape == (64,)
    # evaluation mode reaches the launch
    env.training = False
    env.step(torch.zeros(64, env.model.nmotors, dtype=torch.float64, device=gpu_device))
    assert _block_case(env)[1]["training"] is False
    # an L^1 mixture against the dictionary with the same weights
    weights = {"momentum": 0.5, "power": 0.3, "foot_positions": 0.2}
    a, out_a, _ = _anymal(gpu_device, monkeypatch, reward=Add("total", list(weights), 1, list(weights.values())), **blocks_cfg)
    b, out_b, _ = _anymal(gpu_device, monkeypatch, reward_mixture=weights, **blocks_cfg)
    assert a.composition.plan.arrays["node_normalized"][0] == 1 and b.composition is None
    assert torch.equal(out_a[2], out_b[2]) and torch.equal(out_a[3], out_b[3])
    live = ~out_a[2]
    assert bool(live.any())
    e = float(((out_a[1] - out_b[1]).abs() / out_b[1].abs().clamp_min(1.0))[live].max())
    print(f"ANYmal, L^1 mixture against reward_mixture on the live lanes: {e:.2e}")
    assert e <= TOL and float(out_b[1][live].min()) > 0.0
    for e_ in (env, twin, a, b):
        e_.close()
