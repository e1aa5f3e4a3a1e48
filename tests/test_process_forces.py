"""Process forces: wrench components `scale * process(lane time)` that the step kernels evaluate inside EVERY dynamics
evaluation, at the time of that evaluation -- the reference's continuous profile force (`Engine::computeExternalForces`,
core/src/engine/engine.cc:3482-3494; `WalkerJiminyEnv._setup`, gym_jiminy envs/locomotion.py:165-167, 326-359).

The yardstick.  The oracle has no time-dependent force; it has a batch `dynamics` mode, `integrate` and `bind_applied`.
`Composed` below builds RK4 (abstract_runge_kutta_stepper.cc:33-73: stages at t + dt/2, t + dt/2, t + dt, end-of-step
evaluation at t + dt) and explicit Euler (euler_explicit_stepper.cc:5-21) from those and rebinds the wrench before each
evaluation: that integrator IS the reference semantics.  `test_composed_integrator_reproduces_the_oracle_step` pins it to
the oracle's own `step` with a held wrench.  The spline values it binds come from `PeriodicGaussianProcess` on CPU tensors
(pinned by tests/test_processes.py)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from jiminy_amd import _abi, codegen, load_builtin
from jiminy_amd.processes import PeriodicFourierProcess, PeriodicGaussianProcess
from jiminy_amd.synthetic import sample_standing_states, sample_states
from oracle.oracle_py import OracleEngine
from tests import robots
from tests.helpers import ReferenceFixedStepLoop, alloc_constraint_state, alloc_soa, oracle_io, rel_err
from tests.hostemu import emu, force_process

TIGHT = dict(tol_abs=1e-11, tol_rel=1e-10)
SCALE = 50.0          # F_PROFILE_SCALE of the environments (envs/locomotion.py:56)


def env_processes(B, seed, device=None):
    """The environment's two processes (wavelength 0.2 and 1, period 1), one seeded realisation per lane."""
    p = [PeriodicGaussianProcess(0.2, 1.0, B, device=device), PeriodicGaussianProcess(1.0, 1.0, B, device=device)]
    g = torch.Generator().manual_seed(seed)
    for x in p:
        x.reset(g)
    return p


def device_twins(procs, device):
    """The same realisations on the device: the tables are COPIED (a realisation drawn there differs in the last bits: the
    products `L z` round differently), so that the kernels and the CPU yardstick read bit-identical knots."""
    out = []
    for p in procs:
        d = PeriodicGaussianProcess(p.wavelength, p.period, p.batch_size, device=device)
        d.values.copy_(p.values)
        d.grads.copy_(p.grads)
        out.append(d)
    return out


def wrench_of(procs, B, scale=SCALE):
    """`t` (a float, or one time per lane) -> `[6][B]`: the processes on force x and y."""
    def f(t):
        tt = torch.as_tensor(t, dtype=torch.float64).reshape(-1)
        w = np.zeros((6, B))
        for c, p in enumerate(procs):
            w[c] = scale * p(tt if tt.numel() > 1 else float(tt)).cpu().numpy()
        return w
    return f


class Composed:
    """RK4 / explicit Euler composed from the oracle's `dynamics` and `integrate`, the wrench rebound before every
    evaluation at the time of that evaluation.  `t` may be one time per lane."""

    def __init__(self, model, B, q, v, cmd, wrench_at, offsets, joints=None, copt=None, model_lane=None, ground=None,
                 ground_offset=None, **opt):
        self.B = B
        self.arr, self.d = alloc_soa(model, B), alloc_soa(model, B)
        self.e = OracleEngine(model, **opt)
        if copt is not None:
            alloc_constraint_state(model, self.arr, B)
            self.e.set_constraint_options(**copt)
            self.e.bind_constraints(self.arr["con_flags"], self.arr["con_data"])
        if model_lane is not None:
            self.e.bind_model_lane(model_lane)
        if ground is not None:
            self.e.bind_ground(*ground)
        if ground_offset is not None:
            self.e.bind_ground_offset(ground_offset)
        self.W = np.zeros((6 * len(offsets), B))
        self.e.bind_applied(self.W, np.asarray(offsets, dtype=np.float64), joints)
        self.wr = wrench_at
        for a in (self.arr, self.d):
            a["command"][:] = cmd
        self.arr["q"][:] = q
        self.arr["v"][:] = v
        self.io, self.dio = oracle_io(self.arr), oracle_io(self.d)
        self.t = np.zeros(B)
        self.W[:] = wrench_at(self.t)
        self.e.batch_run("start", self.io)

    def f(self, t, q, v, outputs=False):
        self.W[:] = self.wr(t)
        self.d["q"][:] = q
        self.d["v"][:] = v
        self.e.batch_run("dynamics", self.dio)
        return self.d["a"].copy()

    def integ(self, q, dv):
        return np.stack([self.e.integrate(np.ascontiguousarray(q[:, l]), np.ascontiguousarray(dv[:, l])) for l in range(self.B)], 1)

    def step(self, dt, solver="runge_kutta_4"):
        q, v, a, t = self.arr["q"].copy(), self.arr["v"].copy(), self.arr["a"].copy(), self.t
        if solver == "runge_kutta_4":
            k = [(v, a)]
            for A, c in ((.5, .5), (.5, .5), (1., 1.)):
                qi = self.integ(q, dt * A * k[-1][0])
                vi = v + dt * A * k[-1][1]
                k.append((vi, self.f(t + c * dt, qi, vi)))
            b = [1 / 6, 1 / 3, 1 / 3, 1 / 6]
            qn = self.integ(q, sum(dt * b[j] * k[j][0] for j in range(4)))
            vn = v + sum(dt * b[j] * k[j][1] for j in range(4))
        else:
            qn, vn = self.integ(q, dt * v), v + dt * a
        self.t = t + dt
        an = self.f(self.t, qn, vn)
        self.arr["q"][:], self.arr["v"][:], self.arr["a"][:] = qn, vn, an
        self.arr["f_external"][:] = self.d["f_external"]

    def reset_lanes(self, mask, q, v):
        """The masked lanes restart from (q, v) at lane time 0 (`start` of those lanes)."""
        self.t = np.where(mask, 0.0, self.t)
        a = self.f(self.t, np.where(mask[None], q, self.arr["q"]), np.where(mask[None], v, self.arr["v"]))
        for k, x in (("q", q), ("v", v), ("a", a), ("f_external", self.d["f_external"])):
            self.arr[k][:, mask] = x[:, mask]


def test_composed_integrator_reproduces_the_oracle_step():
    """Self-check of the yardstick: with a HELD wrench the composed RK4 / Euler is the oracle's own `step`, ANYmal with
    lanes in ground contact, 20 steps of 1e-3 (<= 1e-14; observed: 0)."""
    model = load_builtin("anymal")
    B = 16
    st = sample_states(model, B, 3)
    off = np.array([model.frame(next(n for n, f in model.frames.items() if f.parent_joint == 1)).p])
    held = np.array([30., -20., 10., 1., 2., -3.])[:, None] * np.linspace(0.5, 1.5, B)[None, :]
    for solver in ("runge_kutta_4", "euler_explicit"):
        a = Composed(model, B, st["q"], st["v"], st["command"], lambda t: held, off)
        b = Composed(model, B, st["q"], st["v"], st["command"], lambda t: held, off)
        worst, touched = 0.0, np.zeros(B, dtype=bool)
        for _ in range(20):
            a.step(1e-3, solver)
            b.e.batch_run("step", b.io, solver=solver, dt=1e-3, n_substeps=1, command_changed=False)
            touched |= np.abs(b.arr["contact_forces"]).sum(0) > 0
            for k in "qva":
                worst = max(worst, np.abs(a.arr[k] - b.arr[k]).max() / max(np.abs(b.arr[k]).max(), 1.0))
        print("composed", solver, "against the oracle's step:", worst)
        assert worst <= 1e-14
        assert touched.sum() >= 2


# ---------------------------------------------------------------------------------------------------------- 1. spline
def _emu_process(p, row=0, scale=1.0):
    return force_process.Process(row, p.dt, scale, p.values.cpu().numpy(), p.grads.cpu().numpy())


@pytest.mark.parametrize("wavelength", [0.2, 1.0])
def test_spline_of_the_kernel_code_matches_the_host_process(wavelength):
    """`process_force_value` (jm_kernels.h), compiled for the host, against `PeriodicGaussianProcess.__call__`: exact knots,
    the wrap at the period, several periods on, negative times.  Same formula in the same order: the bound is a few units
    in the last place of the largest intermediate, `1e-13 * (max|values| + h max|grads|)`."""
    model = robots.point_mass()
    B = 4
    p = PeriodicGaussianProcess(wavelength, 1.0, B)
    p.reset(torch.Generator().manual_seed(11))
    ep = _emu_process(p)
    rg = np.random.default_rng(5)
    n, h = p.num_times, p.dt
    times = np.concatenate([np.arange(n + 1) * h, [1.0, n * h, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 0.0, -0.0],
                            rg.uniform(0.0, 1.0, 150), rg.uniform(1.0, 7.5, 100), [3.0, 5.0 + 3 * h, -0.37, -1e-9, -2.25, -h],
                            rg.uniform(-3.0, 0.0, 40)])
    bound = 1e-13 * (float(p.values.abs().max()) + h * float(p.grads.abs().max()))
    worst = 0.0
    for lane in range(B):
        for t in times:
            want = float(p(float(t))[lane])
            worst = max(worst, abs(force_process.value(model, ep, lane, float(t)) - want))
    print("spline, wavelength", wavelength, ": worst", worst, "bound", bound, "times per lane", len(times))
    assert len(times) >= 300
    assert worst <= bound
    # the scale multiplies the value
    assert force_process.value(model, _emu_process(p, scale=SCALE), 1, 0.4321) == SCALE * force_process.value(model, ep, 1, 0.4321)


# ---------------------------------------------------------------------------------------------------------- 2. the law
def spline_integral(p, T):
    """Closed-form integral of the spline over [0, T], T a whole number of knot intervals: per interval
    h (yl + yr) / 2 + h^2 (gl - gr) / 12."""
    n = int(round(T / p.dt))
    assert abs(n * p.dt - T) < 1e-12
    y, g, N = p.values.cpu().numpy(), p.grads.cpu().numpy(), p.num_times
    s = 0.0
    for k in range(n):
        l, r = k % N, (k + 1) % N
        s = s + p.dt * (y[l] + y[r]) / 2 + p.dt ** 2 * (g[l] - g[r]) / 12
    return s


def _point_mass_scene(B):
    m = robots.point_mass()
    q0 = np.repeat(m.neutral()[:, None], B, 1)
    q0[2] = 5.0
    return m, float(np.sum(m.mass)), q0


@pytest.mark.parametrize("dt", [1e-3, 4e-3, 5e-3])
def test_impulse_momentum_law_on_the_host_emulated_lane_kernel(dt):
    """Point mass, no gravity, at rest 5 m up; the environment's two processes on force x and y, scale 50; RK4 for 1.2 s
    (past the period: the wrap is crossed).  Every dt divides both knot spacings (0.02, 0.1), so no step straddles a knot
    and RK4's quadrature is exact on each cubic piece: m v(T) = the closed-form integral of the spline, to rounding (1e-12
    relative; the composed oracle integrator reaches 6.6e-16, a force frozen over the step misses by 1e-3 or more)."""
    B, T = 8, 1.2
    m, mass, q0 = _point_mass_scene(B)
    procs = env_processes(B, 2)
    arr = alloc_soa(m, B)
    arr["q"][:] = q0
    lane_time = np.full((1, B), 123.0)    # (`start` has to zero it)
    ps = [_emu_process(p, row=c, scale=SCALE) for c, p in enumerate(procs)]
    kw = dict(processes=ps, frames=(np.zeros((1, 3)), [1]), options=_abi.make_options(gravity=(0.0,) * 6), variant="lane")
    force_process.run(m, arr, "start", lane_time, **kw)
    assert np.all(lane_time == 0.0)
    n = int(round(T / dt))
    done = 0
    while done < n:
        k = min(97, n - done)      # (sub-steps inside one launch, launches of uneven length)
        force_process.run(m, arr, "step", lane_time, solver="runge_kutta_4", dt=dt, n_substeps=k, **kw)
        done += k
    want = np.stack([SCALE * spline_integral(procs[0], T), SCALE * spline_integral(procs[1], T)])
    err = np.abs(mass * arr["v"][:2] - want).max() / np.abs(want).max()
    print("momentum law, dt", dt, ": relative error", err, "lane time error", np.abs(lane_time - n * dt).max())
    assert err <= 1e-12
    assert np.abs(lane_time - n * dt).max() <= 1e-12
    # the wrench of the closing evaluation is in the f_external output, at t = T
    fx = wrench_of(procs, B)(T)
    assert rel_err(arr["f_external"][6:8], fx[:2]) <= 1e-12


# ---------------------------------------------------------------------------------------------------------- 3. Euler
@pytest.mark.parametrize("dt", [1e-3, 5e-3])
def test_euler_on_the_host_emulated_lane_kernel_matches_the_composed_oracle(dt):
    """The scene of the law test under explicit Euler (one evaluation per step, at t + dt), against the test-side Euler
    built from the oracle; q, v, a to 1e-11 (`rel_err`): nothing is stiff, and one host-emulated evaluation sits 5e-12
    from the oracle (tests/test_hostemu_vs_oracle.py)."""
    B, n = 8, 240
    m, mass, q0 = _point_mass_scene(B)
    procs = env_processes(B, 4)
    ref = Composed(m, B, q0, np.zeros((m.nv, B)), 0.0, wrench_of(procs, B), np.zeros((1, 3)), gravity=(0.0,) * 6)
    arr = alloc_soa(m, B)
    arr["q"][:] = q0
    lane_time = np.zeros((1, B))
    ps = [_emu_process(p, row=c, scale=SCALE) for c, p in enumerate(procs)]
    kw = dict(processes=ps, frames=(np.zeros((1, 3)), [1]), options=_abi.make_options(gravity=(0.0,) * 6), variant="lane")
    force_process.run(m, arr, "start", lane_time, **kw)
    for k in "qva":
        assert rel_err(arr[k], ref.arr[k]) <= 1e-11, ("start", k)
    for i in range(n // 4):
        force_process.run(m, arr, "step", lane_time, solver="euler_explicit", dt=dt, n_substeps=4, **kw)
        for _ in range(4):
            ref.step(dt, "euler_explicit")
    errs = {k: rel_err(arr[k], ref.arr[k]) for k in "qva"}
    print("euler, dt", dt, errs)
    for k in "qva":
        assert errs[k] <= 1e-11, (k, errs)
    assert np.abs(arr["v"][:2]).max() > 1e-2      # (the force did act)


@pytest.mark.parametrize("name,constrained,solver", [("anymal", False, "runge_kutta_4"), ("anymal", False, "euler_explicit"),
                                                     ("anymal", True, "runge_kutta_4"), ("tree_arm_ff", False, "runge_kutta_4"),
                                                     ("tree_arm_ff", True, "euler_explicit")])
def test_host_emulated_kernels_with_process_forces_match_the_composed_oracle(name, constrained, solver):
    """Both kernel families and both contact models on the host, a time-varying process on top of a held wrench: `start`,
    launches of 4 sub-steps (sub-step time), a `reset` of a third of the lanes (their time restarts), more launches.
    Spring-damper: with ground contact.  Constraint model: states lifted clear of the ground, no row active, so the
    oracle's `dynamics` is stateless.  Bars: those of the host tests of tests/test_variation.py (1e-10 at `start`, 1e-8
    after steps), lanes the oracle blows up excluded."""
    quad = name == "anymal"
    model = load_builtin(name) if quad else robots.tree_arm(True)
    B, dt = 12, 5e-4
    st = sample_states(model, B, seed=7, grounded_fraction=0.0 if constrained else 0.75)
    q0 = st["q"].copy()
    if constrained:
        q0[2] += 1.0
    frame = next(n for n, f in model.frames.items() if f.parent_joint == 1)
    offs, joints = np.array([model.frame(frame).p]), np.array([1], dtype=np.int32)
    procs = env_processes(B, 21)
    held = np.random.default_rng(3).normal(0, 10.0, (6, B))
    wr = wrench_of(procs, B)
    copt = TIGHT if constrained else None
    ref = Composed(model, B, q0, st["v"], st["command"], lambda t: held + wr(t), offs, joints, copt=copt)
    got = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, got, B)
    for k, x in (("q", q0), ("v", st["v"]), ("command", st["command"])):
        got[k][:] = x
    lane_time = np.zeros((1, B))
    ps = [_emu_process(p, row=c, scale=SCALE) for c, p in enumerate(procs)]
    kw = dict(processes=ps, frames=(offs, joints), held=held, constraint_options=copt, variant="quad" if quad else "lane")
    force_process.run(model, got, "start", lane_time, **kw)
    for k in ("q", "v", "a", "f_external"):
        assert rel_err(got[k], ref.arr[k]) <= 1e-10, ("start", k)
    ok = np.ones(B, dtype=bool)

    def launches(count):
        nonlocal ok
        for _ in range(count):
            force_process.run(model, got, "step", lane_time, solver=solver, dt=dt, n_substeps=4, **kw)
            for _ in range(4):
                ref.step(dt, solver)
            ok &= np.isfinite(ref.arr["v"]).all(0) & (np.abs(ref.arr["v"]).max(axis=0) < 1e2) & (np.abs(ref.arr["a"]).max(axis=0) < 1e6)
    launches(2)
    mask = (np.arange(B) % 3) == 0
    got.update(mask=mask.astype(np.uint8), q_init=np.ascontiguousarray(q0), v_init=np.ascontiguousarray(st["v"]))
    force_process.run(model, got, "reset", lane_time, **kw)
    ref.reset_lanes(mask, q0, st["v"])
    launches(2)
    assert np.abs(lane_time[0] - ref.t).max() <= 1e-15
    assert lane_time[0, 0] < lane_time[0, 1]
    assert ok.sum() >= 0.8 * B
    errs = {k: rel_err(got[k], ref.arr[k], ok) for k in ("q", "v", "a", "f_external")}
    print(name, constrained, solver, errs, "lanes", int(ok.sum()))
    for k, e in errs.items():
        assert e <= 1e-8, (k, errs)


# ---------------------------------------------------------------------------------------------------------- 4. host logic
@pytest.mark.parametrize("cls", [PeriodicGaussianProcess, PeriodicFourierProcess])
def test_reset_refills_the_tables_in_place(cls):
    """The kernels hold pointers to `values` and `grads`: `reset` must not rebind them."""
    B = 6
    p = cls(0.2, 1.0, B)
    ptr = (p.values.data_ptr(), p.grads.data_ptr())
    g = torch.Generator().manual_seed(1)
    p.reset(g)
    assert (p.values.data_ptr(), p.grads.data_ptr()) == ptr
    v0, g0 = p.values.clone(), p.grads.clone()
    assert float(v0.abs().max()) > 0
    mask = torch.tensor([True, False, False, True, False, True])
    p.reset(g, lane_mask=mask)
    assert (p.values.data_ptr(), p.grads.data_ptr()) == ptr
    assert torch.equal(p.values[:, ~mask], v0[:, ~mask]) and torch.equal(p.grads[:, ~mask], g0[:, ~mask])
    assert bool((p.values[:, mask] != v0[:, mask]).any(0).all()) and bool((p.grads[:, mask] != g0[:, mask]).any(0).all())
    p.reset(g)
    assert (p.values.data_ptr(), p.grads.data_ptr()) == ptr
    assert bool((p.values != v0).any(0).all())


def test_process_forces_do_not_change_the_launch_plan():
    """With only process forces registered the launches of a step, and their `command_changed`, are those of a step
    without forces; a callable profile of update period 0 still cuts every launch to one step and refreshes a(t+)."""
    from jiminy_amd.engine import default_options, launch_pieces, plan_step, refresh_needed
    o = default_options()
    o["stepper"].update({"odeSolver": "euler_explicit", "dtMax": 1e-3, "controllerUpdatePeriod": 5e-3, "sensorsUpdatePeriod": 5e-3})
    launches, _, _ = plan_step(0.1, 0.0, 5e-3, o, ())

    def plan(profile, process, held_changed):
        out = []
        for dt, n, cmd_bp, sens in launches:
            for k, n_k in enumerate(launch_pieces(n, sens, False, profile, process)):
                out.append((dt, n_k, refresh_needed(cmd_bp, k, False, False, held_changed)))
        return out
    none = plan([], [], False)
    assert sum(n for _, n, _ in none) == 5 and len(none) == len(launches)
    assert not any(c for _, _, c in none)
    process = [{"frame": 0, "component": 0, "scale": 1.0, "process": None}] * 2
    assert plan([], process, False) == none
    cut = plan([{"period": 0.0}], [], True)
    assert [n for _, n, _ in cut] == [1] * 5 and all(c for _, _, c in cut)
    # a held profile (update period > 0) cuts nothing by itself; the constraint model refreshes at controller breakpoints only
    assert [n for _, n, _ in plan([{"period": 5e-3}], process, False)] == [n for _, n, _ in none]
    assert refresh_needed(True, 0, False, True, False) and not refresh_needed(True, 1, False, True, False)
    assert launch_pieces(5, True, True, [], process) == [1] * 5


def test_registration_errors_without_a_device():
    """The checks of `register_process_force` on an engine object that owns no library (the calls that reach the library
    are stubbed): `BadControlFlow` while running, `ValueError` for a fifth component or a process of another batch size or
    device, `NotImplementedError` naming the reason with the adaptive stepper; `remove_all_forces` clears the registry."""
    from jiminy_amd.engine import BatchedEngine, default_options
    from jiminy_amd._lib import BadControlFlow
    B = 5
    eng = object.__new__(BatchedEngine)
    eng._running, eng._options, eng._process_forces, eng.batch_size = False, default_options(), [], B
    eng.device, eng.dtype = torch.device("cpu"), torch.float64
    calls = []
    eng._force_frame_index = lambda name: 0
    eng._set_process_forces = lambda: calls.append(len(eng._process_forces))
    eng._options["stepper"]["odeSolver"] = "runge_kutta_4"
    p = PeriodicGaussianProcess(0.2, 1.0, B)
    with pytest.raises(ValueError, match="batch size"):
        eng.register_process_force("root", PeriodicGaussianProcess(0.2, 1.0, B + 1), 0)
    with pytest.raises(ValueError, match="lives on"):
        eng.register_process_force("root", PeriodicGaussianProcess(0.2, 1.0, B, device=torch.device("meta")), 0)
    with pytest.raises(ValueError, match="component"):
        eng.register_process_force("root", p, 6)
    for c in range(4):
        eng.register_process_force("root", p, c, scale=2.0)
    assert calls == [1, 2, 3, 4] and eng._process_forces[3] == {"frame": 0, "component": 3, "scale": 2.0, "process": p}
    with pytest.raises(ValueError, match="at most 4"):
        eng.register_process_force("root", p, 4)
    eng._running = True
    with pytest.raises(BadControlFlow):
        eng.register_process_force("root", p, 0)
    eng._running, eng._process_forces = False, []
    eng._options["stepper"]["odeSolver"] = "runge_kutta_dopri"
    with pytest.raises(NotImplementedError, match="adaptive stepper"):
        eng.register_process_force("root", p, 0)
    assert eng._process_forces == []


def test_abi_mirror_carries_the_lane_time_field_and_version_11():
    assert _abi.ABI_VERSION == 11
    assert _abi.FIELD_NAMES["lane_time"] == _abi.JM_F_LANE_TIME == 25 and _abi.JM_F_COUNT == 26
    hdr = open(os.path.join(os.path.dirname(codegen.CSRC.rstrip("/")), "..", "include", "jiminy_hip.h")).read()
    assert "JM_F_LANE_TIME = 25" in hdr and "JM_F_COUNT = 26" in hdr and "jm_batch_set_process_forces" in hdr
    assert "#define JM_ABI_VERSION 11" in open(os.path.join(codegen.CSRC, "jm_lib.cpp")).read()
    # jm_process_force: 2 x int32, 2 x double, 2 pointers
    assert C.sizeof(_abi.ProcessForce) == 40 and _abi.ProcessForce.values.offset == 24


FORMS = ("REFUSED", "LANE_BATCH", "LANE_BATCH_GEN", "LANE_CON", "LANE_CON_GEN", "QUAD", "QUAD_ONE_WAVE", "QUAD_GEN", "QCON",
         "QCON_INIT", "QCON_GEN", "QCON_GEN_INIT", "SPLIT_START", "SPLIT_STEP", "SPLIT_STEP_LANE", "DOPRI", "DOPRI_GEN",
         "DOPRI_STAGES")


def test_dispatch_of_process_forces():
    """Process forces alone select the variation kernels exactly as applied wrenches do -- `k_quad_gen`, `k_quad_con_gen`
    (its INIT form for `start` / `reset`), `k_batch<true>`, `k_constrained<true>` --, never a split form, and are refused
    on a float32 batch."""
    here = os.path.dirname(os.path.abspath(__file__))
    src, hdr = os.path.join(here, "hostemu", "dispatch_process.cpp"), os.path.join(codegen.CSRC, "jm_dispatch.h")
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_dispatch_process.so")
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, hdr)):
        subprocess.check_call(emu.host_compiler() + [src, "-o", out])
    L = C.CDLL(out)
    L.dispatch_process_select.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_char_p)]
    ARM, ANYMAL, ATLAS, NOSPLIT = (0, 0, 0, 1, 0), (1, 1, 0, 4, 1), (1, 1, 1, 2, 0), (1, 0, 0, 1, 0)
    LANE, QUAD = 0, 1

    def select(traits, mode, family, constraint, process=1, applied=0, f64=1, B=65536):
        why = C.c_char_p()
        form = FORMS[L.dispatch_process_select((C.c_int * 5)(*traits), mode, family, B, f64, constraint, applied, process, C.byref(why))]
        return (form, why.value.decode()) if form == "REFUSED" else form
    for mode in range(5):     # step, start, dynamics, reset, refresh
        init = mode in (1, 3)
        assert select(ARM, mode, LANE, 0) == "LANE_BATCH_GEN"
        assert select(ARM, mode, LANE, 1) == "LANE_CON_GEN"
        for topo in (ANYMAL, ATLAS, NOSPLIT):
            assert select(topo, mode, QUAD, 0) == "QUAD_GEN"
            assert select(topo, mode, QUAD, 1) == ("QCON_GEN_INIT" if init else "QCON_GEN")
            # the same as applied wrenches, alone or together
            assert select(topo, mode, QUAD, 1) == select(topo, mode, QUAD, 1, process=0, applied=1) == select(topo, mode, QUAD, 1, applied=1)
            # without them the constraint step of a splitting topology takes a split form: process forces keep it out
            if topo is not NOSPLIT and mode in (0, 1, 3):
                assert select(topo, mode, QUAD, 1, process=0).startswith("SPLIT")
            assert select(topo, mode, QUAD, 0, f64=0)[0] == "REFUSED"
        refused = select(ARM, mode, LANE, 0, f64=0)
        assert refused == ("REFUSED", "process forces need a float64 batch (and, on a branch-parallel topology, its own kernels)")
        # a branch-parallel topology forced to the lane kernels has no such instantiation
        assert select(ANYMAL, mode, LANE, 0)[0] == "REFUSED"
        assert select(ARM, mode, LANE, 0, process=0) == "LANE_BATCH"


# ================================================================================================== device (C ABI, float64)
def _constant_process(values_per_lane, device):
    """A process whose tables hold one value per lane and zero derivatives: the spline is that constant."""
    B = values_per_lane.shape[0]
    p = PeriodicGaussianProcess(0.5, 1.0, B, device=device)
    p.values.copy_(torch.as_tensor(values_per_lane, dtype=torch.float64)[None, :].expand(p.num_times, B))
    p.grads.zero_()
    return p


def _device_engine(model, B, device, solver, dt, constrained, period=None):
    from jiminy_amd.engine import BatchedEngine
    eng = BatchedEngine(model, B, dtype=torch.float64, device=device,
                        extra_outputs=("contact_forces", "f_external", "joint_forces", "energy", "centroidal"))
    period = dt if period is None else period
    stepper = {"odeSolver": solver, "dtMax": dt, "controllerUpdatePeriod": period, "sensorsUpdatePeriod": period}
    if constrained:
        stepper.update({"tolAbs": TIGHT["tol_abs"], "tolRel": TIGHT["tol_rel"]})
    eng.set_options({"stepper": stepper, "contacts": {"model": "constraint" if constrained else "spring_damper"}})
    return eng


QUAD_CASES = [("anymal", False), ("anymal", True), ("atlas", False), ("atlas", True)]
LANE_CASES = [("tree_arm_ff", False, "runge_kutta_4"), ("tree_arm_ff", True, "euler_explicit"), ("tree_arm_flex_ff", False, "runge_kutta_4")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,constrained", QUAD_CASES)
def test_gpu_constant_process_is_a_held_wrench_on_the_branch_parallel_kernels(gpu_device, name, constrained):
    """`k_quad_gen` / `k_quad_con_gen`: the scene, oracle, bars and lane-exclusion rule of `test_gpu_variation_matches_oracle`
    (tests/test_variation.py: per-lane models, bumpy ground, two wrenches on root-body frames; 1e-8 with the spring-damper
    model, 1e-9 with the constraint model at PGS tolerances TIGHT; lanes the oracle blows up leave, at most 20 %), four of
    the twelve wrench components supplied as constant process forces, the others as held values."""
    from tests.test_variation import OUTS, _oracle, _scene
    model = load_builtin(name)
    B, dt = (96, 5e-4) if name == "anymal" else (24, 2.5e-4)
    st, ml, ground, applied = _scene(model, B, 9, constrained)
    copt = TIGHT if constrained else None
    ref = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, ref, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    frames = [n for n, f in model.frames.items() if f.parent_joint == 1][:2]
    applied = (applied[0], np.array([model.frame(n).p for n in frames]))
    e = _oracle(model, ref, ml, ground, applied, copt)
    io = oracle_io(ref)
    eng = _device_engine(model, B, gpu_device, "runge_kutta_4", dt, constrained)
    eng.set_lane_model(torch.from_numpy(ml))
    eng.set_ground_heightmap(*ground)
    rows = (0, 1, 8, 9)            # force x, y of the first frame; force z, moment x of the second
    held = applied[0].copy()
    held[list(rows)] = 0.0
    for i, n in enumerate(frames):
        w = torch.from_numpy(held[6 * i:6 * i + 6].copy()).to(gpu_device)
        eng.register_profile_force(n, lambda t, q, v, w=w: w, update_period=1.0)
    procs = [_constant_process(applied[0][r] / 2.0, gpu_device) for r in rows]
    for r, p in zip(rows, procs):
        eng.register_process_force(frames[r // 6], p, r % 6, scale=2.0)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    assert float(eng.field("applied")[list(rows)].abs().max()) == 0.0
    e.batch_run("start", io)
    for k in OUTS:
        assert rel_err(eng.field(k).cpu().numpy(), ref[k]) < (1e-7 if constrained else 1e-10), ("start", k)
    loop = ReferenceFixedStepLoop(dt)
    ok = np.ones(B, dtype=bool)
    for _ in range(4):
        eng.step(dt)
        loop.advance(lambda h, first: e.batch_run("step", io, solver="runge_kutta_4", dt=h, n_substeps=1, command_changed=first),
                     dt, constrained)
        ok &= ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2) & (np.abs(ref["a"]).max(axis=0) < 1e6)
    assert ok.sum() >= 0.8 * B
    errs = {k: rel_err(eng.field(k).cpu().numpy(), ref[k], ok) for k in OUTS}
    print("constant process, quad family:", name, constrained, {k: float("%.1e" % v) for k, v in errs.items()}, "lanes", int(ok.sum()))
    for k in OUTS:
        assert errs[k] < (1e-9 if constrained else 1e-8), (k, errs)
    assert abs(float(eng.lane_time.max()) - 4 * dt) < 1e-12 and abs(float(eng.lane_time.min()) - 4 * dt) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name,constrained,solver", LANE_CASES)
def test_gpu_constant_process_is_a_held_wrench_on_the_one_robot_per_lane_kernels(gpu_device, name, constrained, solver):
    """`k_batch<true>` / `k_constrained<true>`: the scene, oracle, bars and exclusion rule of the fixed-step legs of
    `test_gpu_one_robot_per_lane_kernels_with_variation` (1e-8 spring-damper, 1e-7 constraint model, more than half of the
    lanes -- here the issue's cap: at most 20 % leave), the wrench on a frame of the last joint supplied as four constant
    process forces + two held components."""
    from jiminy_amd.randomization import sample_model_lane
    from tests.test_variation import OUTS, _lane_family_model, _oracle
    model = _lane_family_model(name)
    B, dt = 48, 5e-4
    rg = np.random.default_rng(41)
    st = sample_states(model, B, seed=41, base_height=(0.3, 0.6), grounded_fraction=0.6)
    ml = sample_model_lane(model, B, {"massBodiesBiasStd": 0.1, "inertiaBodiesBiasStd": 0.1,
                                      "centerOfMassPositionBodiesBiasStd": 0.05, "relativePositionBodiesBiasStd": 0.02},
                           torch.Generator().manual_seed(41)).numpy()
    frame = next(n for n, f in model.frames.items() if f.parent_joint == model.njoints - 1)
    wrench = rg.normal(0, 10.0, (6, B))
    copt = TIGHT if constrained else None
    ref = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, ref, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    ground = None if constrained else (0.02 * rg.standard_normal((7, 9)), -1.0, -0.8, 0.25, 0.3)
    offsets = np.ascontiguousarray(rg.uniform(-0.3, 0.3, (2, B)))
    e = _oracle(model, ref, ml, ground, (wrench, np.array([model.frame(frame).p]), np.array([model.njoints - 1], dtype=np.int32)), copt)
    if ground is not None:
        e.bind_ground_offset(offsets)
    io = oracle_io(ref)
    eng = _device_engine(model, B, gpu_device, solver, dt, constrained)
    eng.set_lane_model(torch.from_numpy(ml))
    if ground is not None:
        eng.set_ground_heightmap(*ground)
        eng.set_ground_offsets(torch.from_numpy(offsets.T.copy()))
    rows = (0, 2, 3, 5)
    held = wrench.copy()
    held[list(rows)] = 0.0
    w = torch.from_numpy(held).to(gpu_device)
    eng.register_profile_force(frame, lambda t, q, v, w=w: w, update_period=1.0)
    procs = [_constant_process(wrench[r], gpu_device) for r in rows]
    for r, p in zip(rows, procs):
        eng.register_process_force(frame, p, r)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
    for k in OUTS:
        assert rel_err(eng.field(k).cpu().numpy(), ref[k]) < (1e-7 if constrained else 1e-10), ("start", k)
    loop = ReferenceFixedStepLoop(dt)
    ok = np.ones(B, dtype=bool)
    for _ in range(3):
        eng.step(dt)
        loop.advance(lambda h, first: e.batch_run("step", io, solver=solver, dt=h, n_substeps=1, command_changed=first), dt, constrained)
        ok &= ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2)
    errs = {k: rel_err(eng.field(k).cpu().numpy(), ref[k], ok) for k in ("q", "v", "a", "contact_forces", "f_external")}
    print("constant process, lane family:", name, constrained, solver, {k: float("%.1e" % v) for k, v in errs.items()}, "lanes", int(ok.sum()))
    assert ok.sum() >= 0.8 * B
    for k, x in errs.items():
        assert x < (1e-7 if constrained else 1e-8), (k, errs)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["runge_kutta_4", "euler_explicit"])
@pytest.mark.parametrize("name,constrained", [("anymal", False), ("anymal", True), ("tree_arm_ff", False), ("tree_arm_ff", True)])
def test_gpu_time_varying_process_matches_the_composed_oracle_integrator(gpu_device, name, constrained, solver):
    """The environment's two processes, one seeded realisation per lane, through the C ABI against `Composed`: launches of
    4 integrator steps (the first opens with the reference's 1 us sub-step; the composed integrator takes the same sizes),
    two launches, `reset_lanes` on a third of the lanes (their time restarts at 0, the others go on), two more.
    Spring-damper model: the seeded states of the variation tests, with ground contact, per-lane models and a bumpy
    ground.  Constraint model: lifted clear of the ground and inside the joint bounds, no row active, so that the oracle's
    `dynamics` is stateless.  Bars on q, v, a, f_external, exclusion rule and cap: those of the constant-process tests above
    (quad family 1e-8 / 1e-9, lane family 1e-8 / 1e-7; at most 20 % of the lanes leave)."""
    from tests.test_variation import _lane_family_model, _scene
    quad = name == "anymal"
    model = load_builtin(name) if quad else _lane_family_model(name)
    B, dt = (96, 5e-4) if quad else (48, 5e-4)
    if constrained:
        st = sample_standing_states(model, B, seed=9) if quad else sample_states(model, B, seed=41, base_height=(0.3, 0.6), grounded_fraction=0.0)
        q0 = st["q"].copy()
        q0[2] += 1.0
        ml, ground = None, None
    else:
        if quad:
            st, ml, ground, _ = _scene(model, B, 9, False)
        else:
            from jiminy_amd.randomization import sample_model_lane
            st = sample_states(model, B, seed=41, base_height=(0.3, 0.6), grounded_fraction=0.6)
            ml = sample_model_lane(model, B, {"massBodiesBiasStd": 0.1, "inertiaBodiesBiasStd": 0.1}, torch.Generator().manual_seed(41)).numpy()
            ground = (0.02 * np.random.default_rng(41).standard_normal((7, 9)), -1.0, -0.8, 0.25, 0.3)
        q0 = st["q"].copy()
    lo, hi, mask_b = model.position_lower, model.position_upper, model.bounded_position_mask()
    if constrained:
        # (the standing sampler draws some hip joints a few hundredths of a radian past their bounds: bring every bounded joint
        # 0.1 rad inside, so that no bound row is active at the start nor reached within the 8 ms of the run)
        q0[mask_b] = np.clip(q0[mask_b], lo[mask_b][:, None] + 0.1, hi[mask_b][:, None] - 0.1)
        assert np.all((q0[mask_b] > lo[mask_b][:, None]) & (q0[mask_b] < hi[mask_b][:, None])), "states inside the joint bounds"
    joint = 1 if quad else model.njoints - 1
    frame = next(n for n, f in model.frames.items() if f.parent_joint == joint)
    offs, joints = np.array([model.frame(frame).p]), np.array([joint], dtype=np.int32)
    cpu = env_processes(B, 33)
    dev = device_twins(cpu, gpu_device)
    assert torch.equal(dev[0].values.cpu(), cpu[0].values) and torch.equal(dev[1].grads.cpu(), cpu[1].grads)
    copt = TIGHT if constrained else None
    ref = Composed(model, B, q0, st["v"], st["command"], wrench_of(cpu, B), offs, joints, copt=copt, model_lane=ml, ground=ground)
    eng = _device_engine(model, B, gpu_device, solver, dt, constrained, period=4 * dt)
    if ml is not None:
        eng.set_lane_model(torch.from_numpy(ml))
    if ground is not None:
        eng.set_ground_heightmap(*ground)
    for c, p in enumerate(dev):
        eng.register_process_force(frame, p, c, SCALE)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(q0), torch.from_numpy(st["v"]))
    for k in ("q", "v", "a", "f_external"):
        assert rel_err(eng.field(k).cpu().numpy(), ref.arr[k]) < (1e-7 if constrained else 1e-10), ("start", k)
    loop = ReferenceFixedStepLoop(dt)
    ok = np.ones(B, dtype=bool)

    def launches(count):
        nonlocal ok
        for _ in range(count):
            eng.step(4 * dt)
            for h in loop.sizes(4 * dt):
                ref.step(h, solver)
                ok &= np.isfinite(ref.arr["a"]).all(0) & (np.abs(ref.arr["v"]).max(axis=0) < 1e2) & (np.abs(ref.arr["a"]).max(axis=0) < 1e6)
    launches(2)
    mask = (np.arange(B) % 3) == 0
    eng.reset_lanes(torch.from_numpy(mask).to(gpu_device), torch.from_numpy(q0), torch.from_numpy(st["v"]))
    ref.reset_lanes(mask, q0, st["v"])
    launches(2)
    lt = eng.lane_time.cpu().numpy()
    assert np.abs(lt - ref.t).max() < 1e-12 and abs(lt[0] - 8 * dt) < 1e-12 and abs(lt[1] - 16 * dt) < 1e-12
    errs = {k: rel_err(eng.field(k).cpu().numpy(), ref.arr[k], ok) for k in ("q", "v", "a", "f_external")}
    print("time-varying process:", name, constrained, solver, {k: float("%.1e" % v) for k, v in errs.items()}, "lanes", int(ok.sum()))
    assert ok.sum() >= 0.8 * B
    tol = (1e-9 if constrained else 1e-8) if quad else (1e-7 if constrained else 1e-8)
    for k, x in errs.items():
        assert x < tol, (k, errs)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [1e-3, 4e-3, 5e-3])
def test_gpu_impulse_momentum_law(gpu_device, dt):
    """The law of `test_impulse_momentum_law_on_the_host_emulated_lane_kernel` on the device lane kernel, same bar (1e-12
    relative).  A controller breakpoint every dt keeps the integrator steps on the grid of dt: the opening 1 us sub-step of
    `BatchedEngine.step` adds one boundary at 1e-6 and moves none."""
    from jiminy_amd.engine import BatchedEngine
    B, T = 64, 1.2
    m, mass, q0 = _point_mass_scene(B)
    cpu = env_processes(B, 2)
    dev = device_twins(cpu, gpu_device)
    eng = BatchedEngine(m, B, dtype=torch.float64, device=gpu_device)
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt},
                     "world": {"gravity": [0.0] * 6}, "contacts": {"model": "spring_damper"}})
    frame = next(n for n, f in m.frames.items() if f.parent_joint == 1 and np.allclose(f.p, 0.0))
    for c, p in enumerate(dev):
        eng.register_process_force(frame, p, c, SCALE)
    eng.start(torch.from_numpy(q0), torch.zeros((m.nv, B), dtype=torch.float64))
    for _ in range(12):
        eng.step(0.1)
    want = np.stack([SCALE * spline_integral(cpu[0], T), SCALE * spline_integral(cpu[1], T)])
    v = eng.field("v").cpu().numpy()
    err = np.abs(mass * v[:2] - want).max() / np.abs(want).max()
    print("momentum law on the device, dt", dt, ": relative error", err, "lane time error", float((eng.lane_time - T).abs().max()))
    assert err <= 1e-12
    assert float((eng.lane_time - T).abs().max()) <= 1e-12


def _rot(q):
    x, y, z, s = q[3], q[4], q[5], q[6]
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)]),
                        torch.stack([2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)]),
                        torch.stack([2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)])])


@pytest.mark.gpu
def test_gpu_environment_disturbance_on_the_device(gpu_device):
    """`make_anymal_env(..., std_ratio={"disturbance": 0.3}, disturbance_on_device=True)`: the `applied` rows carry no process
    part; ANYmal's root body has no contact point, so the linear part of the root joint's `f_external` is the applied wrench
    alone: after reset and after each of 10 environment steps it is R(q)^T (50 * 0.3 * process(lane time)) with the
    environment's own q, the processes evaluated on the CPU and lane time k * step_dt counted here (1e-9 relative, the bar of
    tests/test_gpu_env.py for the callable path); after a masked `reset_lanes` those lanes use time 0 and a new realisation."""
    from jiminy_amd.envs import make_anymal_env
    B = 64
    env = make_anymal_env(B, device=gpu_device, std_ratio={"disturbance": 0.3}, disturbance_on_device=True,
                          disturbance_impulses=False, auto_reset=False)
    env.engine.enable_output("f_external")
    env.reset(seed=4)
    assert not env.engine._profile_forces and len(env.engine._process_forces) == 2
    action = torch.zeros((B, env.model.nmotors), dtype=torch.float64, device=gpu_device)
    t = np.zeros(B)

    def check(tag):
        assert float(env.engine.field("applied").abs().max()) == 0.0
        w = torch.zeros((3, B), dtype=torch.float64)
        for c, p in enumerate(env._f_xy_profile):
            host = PeriodicGaussianProcess(p.wavelength, p.period, B)
            host.values.copy_(p.values.cpu())
            host.grads.copy_(p.grads.cpu())
            w[c] = 50.0 * 0.3 * host(torch.from_numpy(t))
        want = torch.einsum("ijb,ib->jb", _rot(env.engine.field("q").cpu()), w)
        got = env.engine.field("f_external")[6:9].cpu()
        err = float((got - want).abs().max()) / float(want.abs().max())
        print("environment,", tag, ": relative error", err)
        assert err < 1e-9, tag
        assert float((env.engine.lane_time.cpu() - torch.from_numpy(t)).abs().max()) < 1e-9
    check("reset")
    for k in range(10):
        env.step(action)
        t = t + env.step_dt
        check(f"step {k}")
        if k == 5:
            mask = torch.zeros(B, dtype=torch.bool, device=gpu_device)
            mask[::3] = True
            before = env._f_xy_profile[0].values.clone()
            env.reset_lanes(mask)
            assert bool((env._f_xy_profile[0].values[:, mask] != before[:, mask]).any())
            assert torch.equal(env._f_xy_profile[0].values[:, ~mask], before[:, ~mask])
            t = np.where(mask.cpu().numpy(), 0.0, t)
            check("reset_lanes")
    # with the impulses kept, they stay on the host path and the process part stays out of the held rows
    env2 = make_anymal_env(8, device=gpu_device, std_ratio={"disturbance": 0.3}, disturbance_on_device=True)
    env2.reset(seed=1)
    assert env2._impulse_frame is not None and len(env2.engine._process_forces) == 2 and not env2.engine._profile_forces
    with pytest.raises(NotImplementedError):
        env2.enable_graph()


@pytest.mark.gpu
def test_gpu_graph_replay_with_process_forces_is_bit_identical(gpu_device):
    """`enable_graph()` under the continuous disturbance (`disturbance_impulses=False`): the replayed step equals the eager one
    bit for bit -- q, v, the PD state and the lane time -- over 50 environment steps."""
    from jiminy_amd.envs import make_anymal_env
    B = 256
    kw = dict(device=gpu_device, dt_max=1e-3, std_ratio={"disturbance": 0.3}, disturbance_on_device=True, disturbance_impulses=False)
    envs = [make_anymal_env(B, **kw) for _ in range(2)]
    envs[1].enable_graph()
    g = torch.Generator(device="cpu").manual_seed(0)
    for e in envs:
        e.reset(seed=5)
    for i in range(50):
        action = (0.3 * torch.randn(B, 12, generator=g, dtype=torch.float64)).to(gpu_device)
        outs = [e.step(action) for e in envs]
        for k in ("q", "v"):
            assert torch.equal(outs[0][0]["states"]["agent"][k], outs[1][0]["states"]["agent"][k]), (i, k)
        assert torch.equal(envs[0].command_state, envs[1].command_state), i
        assert torch.equal(envs[0].engine.lane_time, envs[1].engine.lane_time), i
    assert envs[1]._graph is not None
    assert float(envs[0].engine.lane_time.max()) > 0.0
    with pytest.raises(NotImplementedError):
        envs[1].enable_graph(whole_step=True)


@pytest.mark.gpu
def test_gpu_registration_errors(gpu_device):
    """`register_process_force`: refused while running, for a fifth component, for a process of another batch size or
    device, and with the adaptive stepper (which names the reason)."""
    from jiminy_amd.engine import BatchedEngine
    from jiminy_amd._lib import BadControlFlow
    m = robots.point_mass()
    B = 8
    eng = BatchedEngine(m, B, dtype=torch.float64, device=gpu_device)
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": 1e-3}, "contacts": {"model": "spring_damper"}})
    frame = next(n for n, f in m.frames.items() if f.parent_joint == 1)
    p = PeriodicGaussianProcess(0.2, 1.0, B, device=gpu_device)
    with pytest.raises(ValueError):
        eng.register_process_force(frame, PeriodicGaussianProcess(0.2, 1.0, B + 1, device=gpu_device), 0)
    with pytest.raises(ValueError):
        eng.register_process_force(frame, PeriodicGaussianProcess(0.2, 1.0, B), 0)      # a CPU process
    for c in range(4):
        eng.register_process_force(frame, p, c)
    with pytest.raises(ValueError):
        eng.register_process_force(frame, p, 4)
    eng.start(torch.from_numpy(np.repeat(m.neutral()[:, None], B, 1) + np.array([0, 0, 5.0, 0, 0, 0, 0])[:, None]),
              torch.zeros((m.nv, B), dtype=torch.float64))
    with pytest.raises(BadControlFlow):
        eng.register_process_force(frame, p, 0)
    eng.stop()
    eng.remove_all_forces()
    assert not eng._process_forces
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_dopri"}})
    with pytest.raises(NotImplementedError, match="adaptive stepper"):
        eng.register_process_force(frame, p, 0)
