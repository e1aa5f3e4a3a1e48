"""The launch policy of the C ABI library (jiminy_amd/csrc/jm_dispatch.h) on the host: `select_form`, the pure function
from the facts of a launch to the kernel form it takes, and `SplitHistory`, the state machine that picks the form of a
constraint step of robots with small solves from the device counters of earlier steps.

Every expected value below is written out from the rule as README.md ("What runs where", "one more switch is visible in
the timings") and the comments of jm_dispatch.h state it, not from running the code under test."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from jiminy_amd import codegen
from tests.hostemu import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = ("REFUSED", "LANE_BATCH", "LANE_BATCH_GEN", "LANE_CON", "LANE_CON_GEN", "QUAD", "QUAD_ONE_WAVE", "QUAD_GEN", "QCON",
         "QCON_INIT", "QCON_GEN", "QCON_GEN_INIT", "SPLIT_START", "SPLIT_STEP", "SPLIT_STEP_LANE", "DOPRI", "DOPRI_GEN",
         "DOPRI_STAGES")
MODES = {"step": 0, "start": 1, "dynamics": 2, "reset": 3, "refresh": 4}
LANE, QUAD = 0, 1
# the members of jm::dispatch::Facts in the order of their declaration, with the values of a default-configured process
FACTS = dict(mode=0, family=LANE, n_cus=256, B=65536, f64=1, constraint=0, con_rows=1, model_lane=0, ground=0, applied=0,
             friction=0, joint_locks=0, compact=0, capturing=0, torsion=0, split=1, split_start=1, split_capture=0, cooling=0)
# topologies: (quad, qcon_split, qcon_split_large, block_waves, lane_pgs)
ARM = (0, 0, 0, 1, 0)           # no branch-parallel kernels (arms, pendulums, cartpole)
ANYMAL = (1, 1, 0, 4, 1)        # small solves: one lane per robot, the history chooses the form of a step
ATLAS = (1, 1, 1, 2, 0)         # large solves: split start / reset / step
NOSPLIT = (1, 0, 0, 1, 0)       # branch-parallel, never split (more than five contact points, solves that stay on chip)

NEEDS_OWN = {"ground": "a height-map ground needs a float64 batch (and, on a branch-parallel topology, its own kernels)",
             "model_lane": "per-lane body parameters need a float64 batch (and, on a branch-parallel topology, its own kernels)",
             "applied": "applied wrenches need a float64 batch (and, on a branch-parallel topology, its own kernels)"}
QUAD_FRICTION_F32 = "per-lane friction on a branch-parallel topology needs a float64 batch"
CONSTRAINT_F32 = "contacts.model = 'constraint' needs a float64 batch"


@pytest.fixture(scope="module")
def lib() -> C.CDLL:
    src, hdr = os.path.join(_HERE, "hostemu", "dispatch.cpp"), os.path.join(codegen.CSRC, "jm_dispatch.h")
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_dispatch.so")
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, hdr)):
        subprocess.check_call(emu.host_compiler() + [src, "-o", out])
    L = C.CDLL(out)
    L.history_new.restype = C.c_void_p
    for name in ("history_free", "history_reset", "history_due", "history_allowed", "history_take_step", "history_slot",
                 "history_outstanding"):
        getattr(L, name).argtypes = [C.c_void_p]
    L.history_absorb.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.history_recorded.argtypes = [C.c_void_p, C.c_int]
    return L


def _args(traits, facts):
    assert set(facts) <= set(FACTS), set(facts) - set(FACTS)
    v = dict(FACTS, **facts)
    v["mode"] = MODES.get(v["mode"], v["mode"])
    return (C.c_int * 5)(*traits), (C.c_longlong * len(FACTS))(*[int(v[k]) for k in FACTS])


def select(L, traits, **facts):
    """(form, counters) or ("REFUSED", message)."""
    t, f = _args(traits, facts)
    counters, refusal = C.c_int(0), C.c_char_p()
    form = FORMS[L.dispatch_select(t, f, C.byref(counters), C.byref(refusal))]
    if form == "REFUSED":
        return form, refusal.value.decode()
    assert refusal.value is None
    return form, bool(counters.value)


# ---------------------------------------------------------------------------------------------------------- select_form
def test_spring_damper_forms_of_both_families(lib):
    """README rows "runge_kutta_4 / euler_explicit", "float32 batches", "spring_damper": `k_batch` for the lane family (a
    branch-parallel topology forced to it included), `k_quad` for the quad family, every mode, both dtypes."""
    for mode in MODES:
        for f64 in (1, 0):
            assert select(lib, ARM, mode=mode, f64=f64) == ("LANE_BATCH", False)
            assert select(lib, ANYMAL, mode=mode, f64=f64, family=LANE) == ("LANE_BATCH", False)
            for topo in (ANYMAL, ATLAS, NOSPLIT):
                assert select(lib, topo, mode=mode, f64=f64, family=QUAD) == ("QUAD", False)


def test_small_batches_run_one_wave_per_block(lib):
    """`grid < 2 n_cus` -> one-wave `k_quad`: with 4 waves per block a block holds 64 robots, so 256 CUs want 512 blocks:
    up to 511 * 64 robots take the one-wave form; a topology whose blocks hold one wave anyway has no such form."""
    assert select(lib, ANYMAL, family=QUAD, B=128) == ("QUAD_ONE_WAVE", False)
    assert select(lib, ANYMAL, family=QUAD, B=511 * 64) == ("QUAD_ONE_WAVE", False)
    assert select(lib, ANYMAL, family=QUAD, B=511 * 64 + 1) == ("QUAD", False)
    assert select(lib, ANYMAL, family=QUAD, B=511 * 64, n_cus=128) == ("QUAD", False)
    assert select(lib, ATLAS, family=QUAD, B=511 * 32) == ("QUAD_ONE_WAVE", False)      # (2 waves: 32 robots per block)
    assert select(lib, ATLAS, family=QUAD, B=511 * 32 + 1, f64=0) == ("QUAD", False)
    assert select(lib, NOSPLIT, family=QUAD, B=16) == ("QUAD", False)
    # (the variation kernel has one form)
    assert select(lib, ANYMAL, family=QUAD, B=128, friction=1) == ("QUAD_GEN", False)


@pytest.mark.parametrize("what", ["model_lane", "ground", "applied"])
def test_variation_inputs(lib, what):
    """README rows "per-lane body mass ...", "height-map ground", "impulse / profile forces": float64, the variation
    kernels of either family -- `k_quad_gen` / `k_quad_con_gen`, `k_batch<true>` / `k_constrained<true>` --; refused for
    float32 batches and for a branch-parallel topology forced to the lane kernels (it has no such instantiation)."""
    for mode in MODES:
        init = mode in ("start", "reset")
        assert select(lib, ARM, mode=mode, **{what: 1}) == ("LANE_BATCH_GEN", False)
        assert select(lib, ARM, mode=mode, constraint=1, **{what: 1}) == ("LANE_CON_GEN", False)
        for topo in (ANYMAL, ATLAS, NOSPLIT):
            assert select(lib, topo, mode=mode, family=QUAD, **{what: 1}) == ("QUAD_GEN", False)
            assert select(lib, topo, mode=mode, family=QUAD, constraint=1, **{what: 1}) == \
                ("QCON_GEN_INIT" if init else "QCON_GEN", False)
            assert select(lib, topo, mode=mode, family=LANE, **{what: 1}) == ("REFUSED", NEEDS_OWN[what])
            assert select(lib, topo, mode=mode, family=LANE, constraint=1, **{what: 1}) == ("REFUSED", NEEDS_OWN[what])
            assert select(lib, topo, mode=mode, family=QUAD, f64=0, **{what: 1}) == ("REFUSED", NEEDS_OWN[what])
        assert select(lib, ARM, mode=mode, f64=0, **{what: 1}) == ("REFUSED", NEEDS_OWN[what])
        # (the missing instantiation is named before the contact model)
        assert select(lib, ARM, mode=mode, f64=0, constraint=1, **{what: 1}) == ("REFUSED", NEEDS_OWN[what])


def test_refusals_name_the_first_missing_feature(lib):
    both = dict(f64=0, ground=1, model_lane=1, applied=1, friction=1)
    assert select(lib, ANYMAL, family=QUAD, **both) == ("REFUSED", NEEDS_OWN["ground"])
    assert select(lib, ANYMAL, family=QUAD, **dict(both, ground=0)) == ("REFUSED", NEEDS_OWN["model_lane"])
    assert select(lib, ANYMAL, family=QUAD, **dict(both, ground=0, model_lane=0)) == ("REFUSED", QUAD_FRICTION_F32)
    assert select(lib, ARM, **dict(both, ground=0, model_lane=0)) == ("REFUSED", NEEDS_OWN["applied"])


def test_per_lane_friction(lib):
    """README row "per-lane ground friction": both families, both contact models.  Spring-damper law of the quad family: its
    variation kernel, float64 only; the lane kernels read the field as it is, float32 included.  Constraint model: the solvers
    read their own pointer, the launch sees no friction (Facts::friction is "read by the contact law")."""
    for mode in MODES:
        assert select(lib, ANYMAL, mode=mode, family=QUAD, friction=1) == ("QUAD_GEN", False)
        assert select(lib, ANYMAL, mode=mode, family=QUAD, friction=1, f64=0) == ("REFUSED", QUAD_FRICTION_F32)
        for f64 in (1, 0):
            assert select(lib, ARM, mode=mode, friction=1, f64=f64) == ("LANE_BATCH", False)
            assert select(lib, ANYMAL, mode=mode, family=LANE, friction=1, f64=f64) == ("LANE_BATCH", False)
    assert select(lib, ARM, constraint=1, friction=1) == ("LANE_CON", False)


def test_constraint_model_needs_float64(lib):
    for mode in MODES:
        for topo, family in ((ARM, LANE), (ANYMAL, LANE), (ANYMAL, QUAD), (ATLAS, QUAD), (NOSPLIT, QUAD)):
            assert select(lib, topo, mode=mode, family=family, constraint=1, f64=0) == ("REFUSED", CONSTRAINT_F32)


def test_constraint_model_on_the_lane_family(lib):
    """`k_constrained`: every lane topology, a branch-parallel topology forced to the lane kernels, and a topology without
    constraint rows; user JointConstraints (bound-row form) run in the plain kernel."""
    for mode in MODES:
        assert select(lib, ARM, mode=mode, constraint=1) == ("LANE_CON", False)
        assert select(lib, ARM, mode=mode, constraint=1, joint_locks=1) == ("LANE_CON", False)
        assert select(lib, ANYMAL, mode=mode, family=LANE, constraint=1) == ("LANE_CON", False)
        assert select(lib, ATLAS, mode=mode, family=QUAD, constraint=1, con_rows=0) == ("LANE_CON", False)


def test_constraint_model_small_solves(lib):
    """README row `contacts.model = "constraint"`, robots with up to five contact points (ANYmal, bipeds): step launches as
    pre / solve / post with the one-lane-per-robot solve, which counts for the history; `start` / `reset` / `dynamics`
    (and `refresh`): the single kernel `k_quad_con`, `start` / `reset` in its INIT instantiation."""
    base = dict(family=QUAD, constraint=1, split_start=0)    # (jm_batch_create: split starts are for large solves)
    assert select(lib, ANYMAL, mode="step", **base) == ("SPLIT_STEP_LANE", True)
    assert select(lib, ANYMAL, mode="start", **base) == ("QCON_INIT", False)
    assert select(lib, ANYMAL, mode="reset", **base) == ("QCON_INIT", False)
    assert select(lib, ANYMAL, mode="dynamics", **base) == ("QCON", False)
    assert select(lib, ANYMAL, mode="refresh", **base) == ("QCON", False)
    # ... the single kernel for a step: batch not in whole waves of 16 robots, a captured stream, torsion rows, the history
    # cooling down, JIMINY_AMD_QCON_SPLIT=0, a compact batch
    for off in (dict(B=65536 + 8), dict(B=1), dict(capturing=1), dict(torsion=1), dict(cooling=1), dict(split=0), dict(compact=1)):
        assert select(lib, ANYMAL, mode="step", **base, **off) == ("QCON", False), off
    assert select(lib, ANYMAL, mode="step", B=16, **base) == ("SPLIT_STEP_LANE", True)
    # (a captured step may split when the environment says so at creation; it cannot count: no event to wait for in a graph)
    assert select(lib, ANYMAL, mode="step", capturing=1, split_capture=1, **base) == ("SPLIT_STEP_LANE", False)
    assert select(lib, ANYMAL, mode="step", capturing=1, split_capture=1, cooling=1, **base) == ("QCON", False)
    # compact batches of the adaptive stepper (dynamics launches) never split
    assert select(lib, ANYMAL, mode="dynamics", compact=1, B=4096, **base) == ("QCON", False)
    # JointConstraints: every kernel of a split topology is built with them
    assert select(lib, ANYMAL, mode="step", joint_locks=1, **base) == ("SPLIT_STEP_LANE", True)
    assert select(lib, ANYMAL, mode="dynamics", joint_locks=1, **base) == ("QCON", False)
    # JIMINY_AMD_QCON_SPLIT_START=1 forces the split start chain
    forced = dict(base, split_start=1)
    assert select(lib, ANYMAL, mode="start", **forced) == ("SPLIT_START", False)
    assert select(lib, ANYMAL, mode="reset", **forced) == ("SPLIT_START", False)
    assert select(lib, ANYMAL, mode="start", B=24, **forced) == ("QCON_INIT", False)


def test_constraint_model_large_solves(lib):
    """Atlas-sized solves: `start` / `reset` and step through the split kernels, whatever the history, the capture state or
    torsion say (those concern the one-lane-per-robot solve only); no counters."""
    base = dict(family=QUAD, constraint=1)
    for extra in (dict(), dict(cooling=1), dict(capturing=1), dict(torsion=1), dict(joint_locks=1)):
        assert select(lib, ATLAS, mode="step", **base, **extra) == ("SPLIT_STEP", False), extra
        assert select(lib, ATLAS, mode="start", **base, **extra) == ("SPLIT_START", False), extra
        assert select(lib, ATLAS, mode="reset", **base, **extra) == ("SPLIT_START", False), extra
        assert select(lib, ATLAS, mode="dynamics", **base, **extra) == ("QCON", False), extra
        assert select(lib, ATLAS, mode="refresh", **base, **extra) == ("QCON", False), extra
    for off in (dict(B=32768 + 4), dict(split=0), dict(compact=1)):
        assert select(lib, ATLAS, mode="step", **base, **off) == ("QCON", False), off
        assert select(lib, ATLAS, mode="start", **base, **off) == ("QCON_INIT", False), off
        assert select(lib, ATLAS, mode="reset", **base, **off) == ("QCON_INIT", False), off
    # JIMINY_AMD_QCON_SPLIT_START=0: only the start / reset launches go back to the single kernel
    assert select(lib, ATLAS, mode="start", split_start=0, **base) == ("QCON_INIT", False)
    assert select(lib, ATLAS, mode="step", split_start=0, **base) == ("SPLIT_STEP", False)
    # (a topology that has both a large solve and few contact points: the lane solve runs ahead, nothing is counted)
    assert select(lib, (1, 1, 1, 2, 1), mode="step", **base) == ("SPLIT_STEP_LANE", False)


def test_constraint_model_without_split_forms(lib):
    """A branch-parallel topology that never splits: the single kernel for every mode; `joint_locks` moves it to the
    variation kernels, the only ones of such a topology that are built with user JointConstraints."""
    base = dict(family=QUAD, constraint=1)
    for mode in MODES:
        init = mode in ("start", "reset")
        assert select(lib, NOSPLIT, mode=mode, **base) == ("QCON_INIT" if init else "QCON", False)
        assert select(lib, NOSPLIT, mode=mode, joint_locks=1, **base) == ("QCON_GEN_INIT" if init else "QCON_GEN", False)
        # (spring-damper contacts have no constraint rows to lock)
        assert select(lib, NOSPLIT, mode=mode, family=QUAD, joint_locks=1) == ("QUAD", False)


def test_needs_variation_is_one_predicate(lib):
    def gen(traits, **facts):
        return bool(lib.dispatch_needs_variation(*_args(traits, facts)))
    for topo, family in ((ARM, LANE), (ANYMAL, LANE), (ANYMAL, QUAD), (ATLAS, QUAD), (NOSPLIT, QUAD)):
        for constraint in (0, 1):
            assert not gen(topo, family=family, constraint=constraint)
            for what in ("model_lane", "ground", "applied"):
                assert gen(topo, family=family, constraint=constraint, **{what: 1})
            assert gen(topo, family=family, constraint=constraint, friction=1) == (family == QUAD and not constraint)
            assert gen(topo, family=family, constraint=constraint, joint_locks=1) == (topo == NOSPLIT and bool(constraint))
    assert [bool(lib.dispatch_lane_history((C.c_int * 5)(*t))) for t in (ARM, ANYMAL, ATLAS, NOSPLIT)] == [False, True, False, False]


def test_adaptive_stepper_forms(lib):
    """README row `runge_kutta_dopri`: quad family, spring-damper, float64 -> one persistent launch per interval, its variation
    form for per-lane inputs (friction alone included); everything else -> per-stage launches."""
    def form(traits, per_stage=0, **facts):
        return FORMS[lib.dispatch_adaptive(*_args(traits, facts), per_stage)]
    for topo in (ANYMAL, ATLAS, NOSPLIT):
        assert form(topo, family=QUAD) == "DOPRI"
        for what in ("model_lane", "ground", "applied", "friction"):
            assert form(topo, family=QUAD, **{what: 1}) == "DOPRI_GEN"
        assert form(topo, family=QUAD, joint_locks=1) == "DOPRI"
        assert form(topo, family=QUAD, per_stage=1) == "DOPRI_STAGES"
        assert form(topo, family=QUAD, f64=0) == "DOPRI_STAGES"
        assert form(topo, family=QUAD, constraint=1) == "DOPRI_STAGES"
        assert form(topo, family=LANE) == "DOPRI_STAGES"
    assert form(ARM) == "DOPRI_STAGES"
    assert form(ARM, ground=1) == "DOPRI_STAGES"


# --------------------------------------------------------------------------------------------------------- SplitHistory
MISFIT = (3, 4000, 64, 90)      # robots the one-lane solve could not take
SHORT = (0, 640, 64, 10)        # 10 sweeps on average, longest 10: 5.3 * 10 - 1.55 * 10 = 37.5 < 100
LONG = (0, 3840, 64, 80)        # 60 sweeps on average, longest 80: 5.3 * 60 - 1.55 * 80 = 194 >= 100


class History:
    """Drives a SplitHistory the way a step launch does: take in the counters that are due, ask for the form, and let a
    split step record `counters_of(step)` into its slot."""

    def __init__(self, L):
        self.L, self.h = L, C.c_void_p(L.history_new())
        self.slots, self.n = {}, 0

    def __del__(self):
        self.L.history_free(self.h)

    def reset(self):
        self.L.history_reset(self.h)
        self.slots, self.n = {}, 0

    def step(self, counters):
        """One step launch; `counters`: what the solve kernel would count if the step splits.  True: split form."""
        while True:
            k = self.L.history_due(self.h)
            if k < 0:
                break
            self.L.history_absorb(self.h, k, (C.c_int32 * 4)(*self.slots.pop(k)))
        allowed = bool(self.L.history_allowed(self.h))
        split = bool(self.L.history_take_step(self.h))
        assert split == allowed
        if split:
            k = self.L.history_slot(self.h)
            assert k not in self.slots, "a split step must find its slot drained"
            self.slots[k] = tuple(counters)
            self.L.history_recorded(self.h, k)
        assert self.L.history_outstanding(self.h) == len(self.slots)
        self.n += 1
        return split

    def run(self, n, counters_of):
        return [self.step(counters_of(self.n)) for _ in range(n)]


def model_forms(n, counters_of):
    """The rule restated in Python from README.md: the form of step i follows from the counters of split steps <= i - 2,
    each taken in once, oldest first; a misfit asks for 64 single-kernel steps, short solves for 256, the larger of what is
    asked and what is left holds; a step under a cool-down is single and records nothing."""
    forms, recorded, seen, cool = [], {}, set(), 0
    for i in range(n):
        for k in sorted(recorded):
            if k <= i - 2 and k not in seen:
                seen.add(k)
                miss, sweeps, waves, longest = recorded[k]
                ask = 64 if miss > 0 else (256 if waves > 0 and 5.3 * sweeps / waves - 1.55 * longest < 100.0 else 0)
                cool = max(cool, ask)
        split = cool == 0
        if not split:
            cool -= 1
        else:
            recorded[i] = counters_of(i)
        forms.append(split)
    return forms


def test_history_fresh_state_and_two_step_latency(lib):
    h = History(lib)
    assert lib.history_allowed(h.h) and lib.history_due(h.h) == -1 and lib.history_outstanding(h.h) == 0
    # misfits from the first step on: steps 0 and 1 still split -- counters recorded at step k are not consulted before k + 2
    assert h.step(MISFIT) is True
    assert lib.history_due(h.h) == -1
    assert h.step(MISFIT) is True
    assert lib.history_due(h.h) >= 0            # (step 0's slot is due for step 2)
    assert h.step(MISFIT) is False


def test_history_misfit_gives_64_single_steps(lib):
    h = History(lib)
    forms = h.run(80, lambda i: MISFIT if i == 0 else LONG)
    assert forms == [True, True] + [False] * 64 + [True] * 14


def test_history_short_solves_give_256_single_steps(lib):
    h = History(lib)
    forms = h.run(300, lambda i: SHORT if i == 0 else LONG)
    assert forms == [True, True] + [False] * 256 + [True] * 42


def test_history_larger_cooldown_wins(lib):
    # misfit at step 0 (taken in at step 2: 64), short solves at step 1 (taken in at step 3, 63 left: 256, not 63 + 256)
    forms = History(lib).run(330, lambda i: (MISFIT, SHORT)[i] if i < 2 else LONG)
    assert forms == [True, True] + [False] * (1 + 256) + [True] * 71
    # the other way round: 256 at step 2, the 64 asked at step 3 is less than the 255 left
    forms = History(lib).run(330, lambda i: (SHORT, MISFIT)[i] if i < 2 else LONG)
    assert forms == [True, True] + [False] * 256 + [True] * 72


def test_history_long_solves_and_empty_launches_keep_the_split_form(lib):
    assert all(History(lib).run(200, lambda i: LONG))
    # threshold 5.3 * sweeps / waves - 1.55 * longest >= 100: 30 sweeps on average -> 159; longest 38 -> 100.1, 39 -> 98.55
    assert all(History(lib).run(50, lambda i: (0, 30 * 64, 64, 38)))
    assert History(lib).run(5, lambda i: (0, 30 * 64, 64, 39)) == [True, True, False, False, False]
    # no wave ran the solve (st[2] == 0): nothing to judge
    assert all(History(lib).run(50, lambda i: (0, 5, 0, 1)))


def test_history_probes_after_a_cooldown(lib):
    """The cool-down of a misfit ends with step 65; step 66 probes in the split form.  Its counters may be read from step 68
    on (n - 2), so step 67 -- chosen before them -- is split as well, and the verdicts of both arrive at steps 68 and 69:
    short solves at the probe send the batch back for 256 steps from step 68, the second verdict (256 asked, 255 left)
    adds one."""
    counters = {0: MISFIT, 1: LONG, 66: SHORT, 67: SHORT}
    h = History(lib)
    forms = h.run(400, lambda i: counters.get(i, LONG))
    assert forms[:66] == [True, True] + [False] * 64
    assert forms[66:68] == [True, True]
    assert forms[68:68 + 257] == [False] * 257
    assert forms[325:] == [True] * 75
    # single-kernel steps record no counters: nothing is outstanding in the middle of a cool-down
    h2 = History(lib)
    h2.run(10, lambda i: MISFIT)
    assert lib.history_outstanding(h2.h) == 0 and lib.history_due(h2.h) == -1


def test_history_reset_returns_to_the_fresh_state(lib):
    h = History(lib)
    first = h.run(40, lambda i: SHORT)
    assert first == [True, True] + [False] * 38
    h.reset()
    assert lib.history_allowed(h.h) and lib.history_due(h.h) == -1 and lib.history_outstanding(h.h) == 0
    assert h.run(40, lambda i: SHORT) == first
    # ... also with counters outstanding
    h.reset()
    h.run(2, lambda i: MISFIT)
    assert lib.history_outstanding(h.h) == 2
    h.reset()
    assert lib.history_outstanding(h.h) == 0
    assert h.run(70, lambda i: LONG) == [True] * 70


def test_history_is_a_function_of_the_counters(lib):
    """1 000 steps driven twice from the same counters give the same forms -- and the forms of the rule as restated above."""
    rng = np.random.default_rng(7)
    kind = rng.choice(3, size=1000, p=[0.02, 0.03, 0.95])
    table = [MISFIT, SHORT, LONG]

    def counters_of(i):
        return table[kind[i]]
    a = History(lib).run(1000, counters_of)
    b = History(lib).run(1000, counters_of)
    assert a == b
    assert a == model_forms(1000, counters_of)
    assert 0 < sum(a) < 1000        # (both forms occur)
