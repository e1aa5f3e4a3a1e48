"""Helpers of tests/test_lane_failures.py: one scenario, three executors with the same few methods -- the CPU oracle, the
kernel code compiled for the host (tests/hostemu) and the device through `BatchedEngine` -- and the designed batches whose
lanes are made to carry a known status."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np

from jiminy_amd import _abi, codegen, load_builtin
from jiminy_amd.synthetic import joint_world_placements, sample_standing_states, sample_states
from oracle.oracle_py import OracleEngine, adaptive_state
from tests.helpers import ReferenceFixedStepLoop, alloc_constraint_state, alloc_soa, oracle_io, rel_err

NAN, OOB, OVERFLOW, STEPPER, SOLVER = (_abi.JM_LANE_NAN, _abi.JM_LANE_OUT_OF_BOUNDS, _abi.JM_LANE_FORCE_OVERFLOW,
                                       _abi.JM_LANE_STEPPER_FAILURE, _abi.JM_LANE_SOLVER_FAILURE)
FIELDS = ("q", "v", "a", "u_motor", "u", "imu", "force", "contact", "encoder", "effort", "energy", "contact_forces",
          "f_external", "joint_forces", "centroidal")
EXTRA = ("contact_forces", "energy", "f_external", "joint_forces", "centroidal")
BASE_HEIGHT = {"anymal": (0.45, 0.65), "atlas": (0.9, 1.1)}
# tolerances the PGS solver cannot meet: far below round-off (a robot with an active row runs into the iteration cap)
UNMEETABLE = dict(tol_abs=1e-300, tol_rel=1e-300)
TIGHT = dict(tol_abs=1e-11, tol_rel=1e-10)


@dataclasses.dataclass
class Setup:
    name: str
    B: int
    contact: str = "spring_damper"
    solver: str = "runge_kutta_4"
    dt: float = 1e-3
    family: str = "quad"                 # "lane": the one-robot-per-lane kernels
    split: bool = False                  # host: the pre | solve | post form of the constraint step
    copt: Optional[Dict[str, float]] = None
    ground: Optional[Tuple] = None       # (heights [ny][nx], x0, y0, dx, dy)
    gravity: Tuple[float, ...] = (0.0, 0.0, -9.81, 0.0, 0.0, 0.0)
    adaptive: Optional[Dict[str, float]] = None   # tol_rel, tol_abs, dt_max, successive_iter_failed_max

    @property
    def constrained(self) -> bool:
        return self.contact == "constraint"

    @property
    def constraint_options(self):
        return dict(self.copt or TIGHT) if self.constrained else None

    @property
    def fields(self):
        return FIELDS + (("con_data",) if self.constrained else ())


def model_of(name: str):
    return load_builtin(name)


def healthy_states(model, B: int, seed: int = 3, standing: bool = False) -> Dict[str, np.ndarray]:
    if standing:
        return sample_standing_states(model, B, seed=seed, out_of_bounds_fraction=0.0)
    return sample_states(model, B, seed=seed, base_height=BASE_HEIGHT.get(model.name, (0.45, 0.65)))


def bumpy_ground(seed: int = 5):
    rng = np.random.default_rng(seed)
    return (np.ascontiguousarray(rng.uniform(-0.03, 0.03, (9, 11))), -2.0, -1.5, 0.4, 0.4)


# ------------------------------------------------------------------ executors
class _Arrays:
    """Executors over SoA numpy arrays (oracle, host emulation)."""

    def __init__(self, setup: Setup, model) -> None:
        self.s, self.model = setup, model
        self.arr = alloc_soa(model, setup.B)
        if setup.constrained:
            alloc_constraint_state(model, self.arr, setup.B)
        self.loop = ReferenceFixedStepLoop(setup.dt)
        self.ad = None
        self.t = 0.0

    def get(self, k: str) -> np.ndarray:
        return self.arr[k][0].copy() if k == "status" else self.arr[k].copy()

    def poke(self, field: str, row: int, lane: int, value: float) -> None:
        self.arr[field][row, lane] = value

    def lane_time(self) -> np.ndarray:
        return np.array(self.ad["t"], dtype=np.float64)

    def set_command(self, command) -> None:
        self.arr["command"][:] = command

    def poke_status(self, lane: int, bits: int) -> None:
        self.arr["status"][0, lane] = bits

    def interval(self, t_next: float, new_step: bool) -> None:
        self._run_dopri(t_next, new_step)

    def start(self, q, v, command) -> None:
        for k, x in (("q", q), ("v", v), ("command", command)):
            self.arr[k][:] = x
        self.arr["a"][:] = 0.0
        self.loop = ReferenceFixedStepLoop(self.s.dt)
        self.t = 0.0
        if self.s.adaptive:
            self.ad = adaptive_state(self.s.B)
        self._run("start")

    def step(self) -> None:
        if self.s.adaptive:
            self.t += self.s.dt
            self._run_dopri(self.t)
            return
        changed = self.s.constrained      # (the engine refreshes a(t+) at every controller breakpoint of the constraint model)
        self.loop.advance(lambda dt, ch: self._run("step", dt=dt, command_changed=ch), self.s.dt, changed)
        self.t += self.s.dt

    def reset(self, mask: np.ndarray, q, v) -> None:
        raise NotImplementedError


class Oracle(_Arrays):
    def __init__(self, setup: Setup, model) -> None:
        super().__init__(setup, model)
        self.e = OracleEngine(model, gravity=setup.gravity)
        if setup.constrained:
            self.e.set_constraint_options(**setup.constraint_options)
            self.e.bind_constraints(self.arr["con_flags"], self.arr["con_data"])
        if setup.ground is not None:
            self.e.bind_ground(*setup.ground)

    def _run(self, mode: str, dt: float = 0.0, command_changed: bool = False) -> None:
        self.e.batch_run(mode, oracle_io(self.arr), solver=self.s.solver, dt=dt or self.s.dt, n_substeps=1,
                         command_changed=command_changed)

    def _run_dopri(self, t_next: float, new_step: bool = True) -> None:
        a = self.s.adaptive
        self.e.batch_run_dopri(oracle_io(self.arr), self.ad, t_next, new_step=new_step, command_changed=False, update_sensors=True,
                               tol_rel=a["tol_rel"], tol_abs=a["tol_abs"], dt_max=a["dt_max"],
                               successive_iter_failed_max=a["successive_iter_failed_max"])

    def reset(self, mask, q, v) -> None:
        # Engine::reset + Engine::start of the masked robots: a start of a copy, the masked lanes taken over
        sel = np.asarray(mask, dtype=bool)
        other = Oracle(dataclasses.replace(self.s, adaptive=None), self.model)
        other.start(q, v, self.arr["command"])
        for k, x in other.arr.items():
            self.arr[k][:, sel] = x[:, sel]
        if self.ad is not None:
            fresh = adaptive_state(self.s.B)
            for k in self.ad:
                self.ad[k][sel] = fresh[k][sel]
            self.ad["t"][sel] = self.t


class Host(_Arrays):
    """The kernel code on the host, one robot after the other."""

    def _kw(self):
        s = self.s
        return dict(options=_abi.make_options(gravity=s.gravity), solver=s.solver, variant=s.family,
                    constraint_options=s.constraint_options, ground=s.ground, split=s.split)

    def _run(self, mode: str, dt: float = 0.0, command_changed: bool = False) -> None:
        from tests.hostemu import emu
        emu.run(self.model, self.arr, mode, dt=dt or self.s.dt, n_substeps=1, command_changed=command_changed, **self._kw())

    def _run_dopri(self, t_next: float, new_step: bool = True) -> None:
        from tests.hostemu import emu
        a = self.s.adaptive
        left, _ = emu.run_dopri(self.model, self.arr, self.ad, t_next, tol_rel=a["tol_rel"], tol_abs=a["tol_abs"],
                                dt_max=a["dt_max"], successive_iter_failed_max=a["successive_iter_failed_max"], new_step=new_step,
                                options=_abi.make_options(gravity=self.s.gravity))
        assert left == 0
        # (the library's closing launch: extra terms and sensors at the breakpoint, status ORed in)
        emu.run(self.model, self.arr, "refresh", **self._kw())

    def reset(self, mask, q, v) -> None:
        self.arr["mask"] = np.ascontiguousarray(mask, dtype=np.uint8)
        self.arr["q_init"], self.arr["v_init"] = np.ascontiguousarray(q), np.ascontiguousarray(v)
        self._run("reset")
        if self.ad is not None:
            sel = np.asarray(mask, dtype=bool)
            fresh = adaptive_state(self.s.B)
            for k in self.ad:
                self.ad[k][sel] = fresh[k][sel]
            self.ad["t"][sel] = self.t


class Device:
    """The device build through `BatchedEngine`.  The environment switches that select a kernel form are read when the
    engine is created: the test sets them (monkeypatch) before it makes the executor."""

    def __init__(self, setup: Setup, model, device) -> None:
        import torch

        from jiminy_amd.engine import BatchedEngine
        self.s, self.model, self.torch = setup, model, torch
        s = setup
        self.eng = BatchedEngine(model, s.B, dtype=torch.float64, device=device, extra_outputs=EXTRA)
        stepper = {"odeSolver": s.solver, "dtMax": s.dt, "controllerUpdatePeriod": s.dt, "sensorsUpdatePeriod": s.dt}
        if s.constrained:
            stepper.update(tolAbs=s.constraint_options["tol_abs"], tolRel=s.constraint_options["tol_rel"])
        if s.adaptive:
            a = s.adaptive
            stepper.update(odeSolver="runge_kutta_dopri", tolRel=a["tol_rel"], tolAbs=a["tol_abs"], dtMax=a["dt_max"],
                           successiveIterFailedMax=a["successive_iter_failed_max"])
        self.eng.set_options({"world": {"gravity": list(s.gravity)}, "stepper": stepper, "contacts": {"model": s.contact}})
        if s.ground is not None:
            self.eng.set_ground_heightmap(*s.ground)

    def get(self, k: str) -> np.ndarray:
        self.torch.cuda.synchronize()
        if k == "status":
            return self.eng.status.cpu().numpy().reshape(-1).copy()
        return self.eng.field(k).cpu().numpy().copy()

    def poke(self, field: str, row: int, lane: int, value: float) -> None:
        self.eng.field(field)[row, lane] = value

    def set_command(self, command) -> None:
        self.eng.set_command(self.torch.from_numpy(np.ascontiguousarray(command)))

    def lane_time(self) -> np.ndarray:
        # (the engine has no accessor of the per-lane time: row `t` of the stepper state it lends to the library, jiminy_hip.h)
        from tests.hostemu.emu import _AD_F
        self.torch.cuda.synchronize()
        return self.eng._adaptive["f64"][_AD_F.index("t")].cpu().numpy().copy()

    def poke_status(self, lane: int, bits: int) -> None:
        self.eng.status[lane] = bits

    def interval(self, t_next: float, new_step: bool) -> None:
        """One `jm_batch_step_adaptive` call of the C ABI, as `BatchedEngine._step_adaptive` makes one per interval."""
        import ctypes as C
        eng, a = self.eng, self.s.adaptive
        o = _abi.AdaptiveOptions(a["tol_rel"], a["tol_abs"], a["dt_max"], 0.2, int(a["successive_iter_failed_max"]), eng._adaptive_form())
        attempts = C.c_int32(0)
        eng._lib.check(eng._L.jm_batch_step_adaptive(eng._batch_h, float(t_next), C.byref(o), int(new_step), 0, 1, 100000,
                                                     C.byref(attempts), eng._stream()))

    def start(self, q, v, command) -> None:
        t = self.torch
        self.eng.set_command(t.from_numpy(np.ascontiguousarray(command)))
        self.eng.start(t.from_numpy(np.ascontiguousarray(q)), t.from_numpy(np.ascontiguousarray(v)))

    def step(self) -> None:
        self.eng.step(self.s.dt)

    def reset(self, mask, q, v) -> None:
        t = self.torch
        self.eng.reset_lanes(t.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)), t.from_numpy(np.ascontiguousarray(q)),
                             t.from_numpy(np.ascontiguousarray(v)))


def snapshot(x, setup: Setup) -> Dict[str, np.ndarray]:
    out = {k: x.get(k) for k in setup.fields + ("status",)}
    if setup.constrained:
        out["con_flags"] = x.get("con_flags")
    return out


def assert_lanes_identical(a: Dict[str, np.ndarray], b: Dict[str, np.ndarray], lanes, what="") -> None:
    """Bit-identical on `lanes` in every field of the snapshots (NaN compares equal to NaN of the same lane and row)."""
    for k in a:
        x, y = a[k][..., lanes], b[k][..., lanes]
        assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (what, k, np.argwhere(~((x == y) | ((x != x) & (y != y))))[:4])


def assert_matches_oracle(got: Dict[str, np.ndarray], ref: Dict[str, np.ndarray], lanes, tol: float, setup: Setup, what="") -> None:
    for k in setup.fields:
        if ref[k].size:
            e = rel_err(got[k], ref[k], lanes)
            assert e < tol, (what, k, e)


# ------------------------------------------------------------------ designed batches
def limb_rows(model) -> Dict[str, List[Tuple[int, int]]]:
    """(q row, v row) of one bounded joint per limb lane k = 0..3 (the middle joint of the limb) and of the trunk joints."""
    qs = codegen.quad_structure(model)
    rows = lambda j: (int(model.idx_q[j]), int(model.idx_v[j]))     # noqa: E731
    return {"limb": [rows(c[len(c) // 2]) for c in qs["limbs"]], "trunk": [rows(j) for j in qs["trunk"][1:]]}


def contact_heights(model, q: np.ndarray) -> np.ndarray:
    """World height of every contact point, `[ncontacts][B]`."""
    Rs, ps = joint_world_placements(model, q)
    return np.stack([(ps[model.frames[c].parent_joint] + Rs[model.frames[c].parent_joint] @ model.frames[c].p)[:, 2]
                     for c in model.contacts])


def deep_state(model, k: int):
    """(q, v) of a robot whose limb k alone is past the force threshold of `start`: its lowest contact point 0.11 m under
    the ground (1.1e5 N at the default stiffness of 1e6 N/m, the threshold is 1e5 N), every contact point of the other limbs
    above -0.08 m (below 0.8e5 N).  Taken from a seeded pool of free-flight states."""
    qs = codegen.quad_structure(model)
    pool = sample_states(model, 512, seed=11, base_height=BASE_HEIGHT.get(model.name, (0.45, 0.65)), grounded_fraction=0.0)
    z = contact_heights(model, pool["q"])
    mine = np.zeros(z.shape[0], dtype=bool)
    mine[[c for c in qs["contact"][k] if c >= 0]] = True
    zk, zo = z[mine].min(axis=0), z[~mine].min(axis=0)
    lane = int(np.argmax(zo - zk))
    assert zo[lane] - zk[lane] > 0.03, (k, zo[lane] - zk[lane])
    q, v = pool["q"][:, lane].copy(), pool["v"][:, lane].copy()
    q[2] += -0.11 - zk[lane]
    return q, v


def designed_status_batch(model, B: int, nan: bool = True, overflow: bool = True):
    """Healthy seeded states with designed lanes written over them.  Returns (states, expected status after `start` [B],
    names of the designs per lane).  Every limb lane of the quad (k = 0..3), a base row and -- where the robot has them -- a
    trunk joint carry a NaN; one joint per limb lane and a trunk joint sit exactly at / one ulp beyond either bound."""
    st = healthy_states(model, B)
    q, v = st["q"], st["v"]
    rows = limb_rows(model)
    lo, hi = model.position_lower, model.position_upper
    designs = []
    if nan:
        designs += [("q_nan base z", "q", 2, np.nan, NAN), ("q_nan base quaternion", "q", 4, np.nan, NAN),
                    ("v_nan base", "v", 2, np.nan, NAN), ("v_inf base", "v", 0, np.inf, NAN)]
        for k, (iq, iv) in enumerate(rows["limb"]):
            designs.append((f"v_nan limb {k}", "v", iv, np.nan, NAN))
        designs.append(("q_nan limb 1", "q", rows["limb"][1][0], np.nan, NAN))
        designs.append(("v_inf limb 2", "v", rows["limb"][2][1], np.inf, NAN))
        for iq, iv in rows["trunk"][:1]:
            designs += [("q_nan trunk", "q", iq, np.nan, NAN), ("v_nan trunk", "v", iv, np.nan, NAN)]
    bounded = [(f"limb {k}", iq) for k, (iq, _) in enumerate(rows["limb"])] + [("trunk", iq) for iq, _ in rows["trunk"][:1]]
    for who, iq in bounded:
        designs += [(f"at upper {who}", "q", iq, hi[iq], 0), (f"at lower {who}", "q", iq, lo[iq], 0),
                    (f"above upper {who}", "q", iq, np.nextafter(hi[iq], np.inf), OOB),
                    (f"below lower {who}", "q", iq, np.nextafter(lo[iq], -np.inf), OOB)]
    if overflow:
        # the force check runs per limb lane and reaches the store through the OR of the quad: one deep robot per limb k
        for k in range(4):
            designs.append((f"deep in the ground, limb {k}", "state", k, None, OVERFLOW))
    assert len(designs) < B - 4, "the batch keeps clean lanes"
    lanes = np.random.default_rng(0).permutation(B)[:len(designs)]     # spread over the quads, waves and blocks
    expect = np.zeros(B, dtype=np.int32)
    names = ["clean"] * B
    for lane, (name, field, row, value, bits) in zip(lanes, designs):
        if field == "state":
            q[:, lane], v[:, lane] = deep_state(model, row)
        else:
            (q if field == "q" else v)[row, lane] = value
        expect[lane] = bits
        names[lane] = name
    return st, expect, names


def mixed_grounded_and_free_batch(model, B: int, seed: int = 7):
    """Constraint model: standing robots (active contact rows) on the even lanes, the same robots one metre up in free flight
    (no active row: joints inside their bounds) on the odd ones.  Returns (states, lanes in free flight [B] bool)."""
    st = healthy_states(model, B, seed=seed, standing=True)
    free = (np.arange(B) % 2) == 1
    st["q"][2, free] += 1.0
    return st, free


# ------------------------------------------------------------------ which form a launch takes (jm_dispatch.h on the host)
# `jm::dispatch::Traits` of the robots of `tests.robots.quad_topology_models()`, in the form of tests/test_dispatch_policy.py
# (quad, qcon_split, qcon_split_large, block_waves, lane_pgs).  Written out like ANYMAL / ATLAS there, so that a GPU test
# compiles nothing; tests/test_model_compiler.py holds every tuple to what the kernel headers state (hostemu.dispatch_traits).
QUAD_TOPOLOGY_TRAITS = {
    "hydra": (1, 1, 1, 4, 0),           # 25 bounded joints + 4 x 6 contact rows = 49 > 32: large solves (split start / step)
    "quadlet_bare": (1, 1, 0, 4, 1),    # 9 + 4 x 4 = 25 rows, 4 contact points: one lane per robot, history-driven
    "quadlet_jside": (1, 1, 0, 4, 1),
    "quadlet_free": (1, 0, 0, 4, 0),    # no contact point: 9 bound rows, never split
}


def expected_form(name: str, n_cus: int = 256, per_stage=None, **facts) -> str:
    """`select_form` (`select_adaptive_form` when `per_stage` is given) compiled for the host, as tests/test_dispatch_policy.py
    drives it, for the topology `name`."""
    import ctypes as C
    import os
    import subprocess

    from tests import test_dispatch_policy as dp
    from tests.hostemu import emu
    src, hdr = os.path.join(os.path.dirname(dp.__file__), "hostemu", "dispatch.cpp"), os.path.join(codegen.CSRC, "jm_dispatch.h")
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_dispatch.so")
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, hdr)):
        subprocess.check_call(emu.host_compiler() + [src, "-o", out])
    L, traits = C.CDLL(out), dict(QUAD_TOPOLOGY_TRAITS, anymal=dp.ANYMAL, atlas=dp.ATLAS)[name]
    if per_stage is not None:
        return dp.FORMS[L.dispatch_adaptive(*dp._args(traits, dict(facts, n_cus=n_cus)), int(per_stage))]
    return dp.select(L, traits, n_cus=n_cus, **facts)[0]
