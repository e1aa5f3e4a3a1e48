"""Process forces under the adaptive Dormand-Prince stepper: stage `i` of an attempt of size `dt` by a lane whose process
time is `tl` is evaluated at `tl + c_i dt` (c = 0, 1/5, 3/10, 4/5, 8/9, 1, 1: runge_kutta_dopri_stepper.h:21-23,
abstract_runge_kutta_stepper.cc:46), `tl` advances with every accepted step, in both forms of the stepper (the persistent
kernel of jm_qdopri.h and the per-stage launches of jm_adaptive.h).

The yardstick.  The oracle has no time-dependent force.  `ComposedDopri` builds the adaptive loop of `Engine::step`
(engine.cc:2021-2222) on top of `Composed` (tests/test_process_forces.py) from the oracle's own pieces: its batch `dynamics`
with the wrench rebound before every evaluation, `integrate`, the tableaux (`orc_leaf_tableaux`), the step-size selection
(`orc_leaf_substep`), the controller (`orc_leaf_dopri_adjust`) and the bookkeeping after a try (`orc_leaf_after_try`).  Only
`difference` (log6 on the free-flyer) and the max-norm of `computeError` are numpy here, after oracle.cpp's own lines.
`test_composed_adaptive_loop_reproduces_the_oracle` pins it to `OracleEngine.batch_run_dopri` with a held wrench."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from jiminy_amd import _abi, codegen, load_builtin
from jiminy_amd.processes import PeriodicGaussianProcess
from jiminy_amd.model import JT_FREEFLYER, JT_NQ, JT_RUBU, JT_RUBX
from jiminy_amd.synthetic import lowest_contact_height, sample_states
from oracle import oracle_py
from oracle.oracle_py import OracleEngine, adaptive_state
from tests import robots
from tests.helpers import alloc_soa, oracle_io, rel_err
from tests.hostemu import dopri_process, emu, force_process
from tests.test_process_forces import (SCALE, TIGHT, Composed, _constant_process, _emu_process, _point_mass_scene, device_twins,
                                       env_processes, spline_integral, wrench_of)

STEPPER_MIN_TIMESTEP = 1e-10
TOL = dict(tol_abs=1e-8, tol_rel=1e-7)
# bars of tests/test_variation.py:985-989 (same tolerances): 1e-7 on the lanes that follow the yardstick's accept / reject
# sequence, 1e-4 on all of them, at most 20 % of the lanes on another sequence
BAR_SAME, BAR_ALL, CAP = 1e-7, 1e-4, 0.2
pd = C.POINTER(C.c_double)
pi32 = C.POINTER(C.c_int32)
_HERE = os.path.dirname(os.path.abspath(__file__))


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def _leaves():
    L = oracle_py.lib()
    L.orc_leaf_tableaux.argtypes = [pd]
    L.orc_leaf_substep.argtypes = [C.c_int64, pd, pd, pd, pi32, pd]
    L.orc_leaf_dopri_adjust.argtypes = [C.c_int64, pd, pd, pi32, pd]
    L.orc_leaf_after_try.argtypes = [C.c_int64, pi32, pi32, C.c_double, C.c_double, pd, pd, pd, C.POINTER(C.c_int64)]
    return L


# ------------------------------------------------------------------------------------------ numpy: State::difference
def _quat_to_matrix(x, y, z, w):
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _log3(R):
    """Pinocchio v2.7.0 log3 (explog.hpp), as oracle.cpp restates it."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr >= 3.0:
        tr, theta = 3.0, 0.0
    elif tr <= -1.0:
        tr, theta = -1.0, math.pi
    else:
        theta = math.acos((tr - 1.0) / 2.0)
    if theta >= math.pi - 1e-2:
        cphi = -(tr - 1.0) / 2.0
        beta = theta * theta / (1.0 + cphi)
        t = [(R[i, i] + cphi) * beta for i in range(3)]
        sg = [1.0 if R[2, 1] > R[1, 2] else -1.0, 1.0 if R[0, 2] > R[2, 0] else -1.0, 1.0 if R[1, 0] > R[0, 1] else -1.0]
        return np.array([sg[i] * (math.sqrt(t[i]) if t[i] > 0 else 0.0) for i in range(3)])
    prec3 = np.finfo(np.float64).eps ** 0.25
    t = ((theta / math.sin(theta)) if theta > prec3 else 1.0) / 2.0
    return np.array([t * (R[2, 1] - R[1, 2]), t * (R[0, 2] - R[2, 0]), t * (R[1, 0] - R[0, 1])])


def _log6(R, p):
    w = _log3(R)
    t2 = float(w @ w)
    t = math.sqrt(t2)
    if t < np.finfo(np.float64).eps ** 0.25:
        alpha = 1.0 - t2 / 12.0 - t2 * t2 / 720.0
        beta = 1.0 / 12.0 + t2 / 720.0
    else:
        st, ct = math.sin(t), math.cos(t)
        alpha = t * st / (2.0 * (1.0 - ct))
        beta = 1.0 / t2 - st / (2.0 * t * (1.0 - ct))
    return np.concatenate([alpha * p - 0.5 * np.cross(w, p) + (beta * float(w @ p)) * w, w])


def difference(model, q0, q1):
    """`pinocchio::difference(model, q0, q1)`, `[nq][B]` -> `[nv][B]`: free-flyer and one-dof joints (what the robots of these
    tests are made of)."""
    out = np.zeros((model.nv, q0.shape[1]))
    for j in range(1, model.njoints):
        iq, iv = int(model.idx_q[j]), int(model.idx_v[j])
        if int(model.jtypes[j]) == JT_FREEFLYER:
            for l in range(q0.shape[1]):
                a, b = q0[iq:iq + 7, l], q1[iq:iq + 7, l]
                R0, R1 = _quat_to_matrix(*a[3:7]), _quat_to_matrix(*b[3:7])
                out[iv:iv + 6, l] = _log6(R0.T @ R1, R0.T @ (b[:3] - a[:3]))
        elif JT_RUBX <= int(model.jtypes[j]) <= JT_RUBU:
            # SO(2) from (cos, sin) pairs: the signed angle (liegroup/special-orthogonal.hpp), oracle.cpp's lines
            for l in range(q0.shape[1]):
                a, b = q0[iq:iq + 2, l], q1[iq:iq + 2, l]
                c, sn = a[0] * b[0] + a[1] * b[1], a[0] * b[1] - a[1] * b[0]
                tr = 2.0 * c
                if tr > 2.0:
                    th = 0.0
                elif tr < -2.0:
                    th = math.pi if sn >= 0.0 else -math.pi
                elif tr > 2.0 - 1e-2:
                    th = math.asin((sn - (-sn)) / 2.0)
                else:
                    th = math.acos(tr / 2.0) if sn >= 0.0 else -math.acos(tr / 2.0)
                out[iv, l] = th
        else:
            assert JT_NQ[int(model.jtypes[j])] == 1, "free-flyer, unbounded and one-dof joints only"
            out[iv] = q1[iq] - q0[iq]
    return out


# ------------------------------------------------------------------------------------------ the composed adaptive loop
class ComposedDopri:
    """`step_dopri` of the oracle (≙ engine.cc:2021-2222) for a whole batch, every dynamics evaluation through
    `Composed.f` at the time of its stage.  Stepper state: `self.ad` (oracle_py.adaptive_state); process time: `Composed.t`."""

    def __init__(self, comp: Composed, model, tol_rel, tol_abs, dt_max=0.02, restore=0.2, fail_max=1000):
        self.c, self.model, self.L = comp, model, _leaves()
        self.tol_rel, self.tol_abs, self.dt_max, self.restore, self.fail_max = tol_rel, tol_abs, dt_max, restore, fail_max
        self.ad = adaptive_state(comp.B)
        t = np.zeros(94)
        self.L.orc_leaf_tableaux(_p(t))
        self.A, self.cn, self.b, self.e = t[24:73].reshape(7, 7), t[73:80], t[80:87], t[87:94]
        self.stopped = np.zeros(comp.B, dtype=bool)
        self.vmax = np.zeros(comp.B)          # largest |v| of the accepted states, per lane (the law test's bound)

    def _weighted(self, h, w, k):
        """sum_j (h w_j) k_j, in the oracle's order, from a zero accumulator"""
        acc = np.zeros_like(k[0])
        for j in range(len(w)):
            acc += (h * w[j])[None, :] * k[j]
        return acc

    def interval(self, t_next, new_step=True, refresh=False):
        c, ad, L, B = self.c, self.ad, self.L, self.c.B
        if new_step:
            ad["succ_too_large"][:] = 0
            ad["succ_failed"][:] = 0
        if refresh:                            # a(t+): the FSAL fix when the dynamics changed at the breakpoint
            go = t_next - ad["t"] > STEPPER_MIN_TIMESTEP
            a = c.f(c.t, c.arr["q"], c.arr["v"])
            c.arr["a"][:, go] = a[:, go]
        while True:
            active = (t_next - ad["t"] > STEPPER_MIN_TIMESTEP) & ~self.stopped
            self.stopped |= active & (ad["dt"] < STEPPER_MIN_TIMESTEP)
            active &= ~self.stopped
            dt_new = np.zeros(B)
            L.orc_leaf_substep(B, _p(ad["dt"]), _p(ad["t"]), _p(np.full(B, float(t_next))),
                               _p(ad["succ_too_large"].astype(np.int32), C.c_int32), _p(dt_new))
            ad["dt"][active] = dt_new[active]
            self.stopped |= active & (ad["succ_failed"] > self.fail_max)
            active &= ~self.stopped
            if not active.any():
                return
            bp = (ad["dt_largest"] > ad["dt"]).astype(np.int32)
            h = np.where(active, ad["dt"], 0.0)
            q0, v0 = c.arr["q"].copy(), c.arr["v"].copy()
            kv, ka = [v0], [c.arr["a"].copy()]
            for i in range(1, 7):
                qs = c.integ(q0, self._weighted(h, self.A[i][:i], kv))
                vs = v0 + self._weighted(h, self.A[i][:i], ka)
                kv.append(vs)
                ka.append(c.f(c.t + self.cn[i] * h, qs, vs))
            qsol, vsol = c.integ(q0, self._weighted(h, self.b, kv)), v0 + self._weighted(h, self.b, ka)
            qoth, voth = c.integ(q0, self._weighted(h, self.e, kv)), v0 + self._weighted(h, self.e, ka)
            # computeError (runge_kutta_dopri_stepper.cc:58-87): scale = tolAbs + tolRel |x0 (-) 0|, max-norm
            sq = np.abs(difference(self.model, q0, np.zeros_like(q0))) * self.tol_rel + self.tol_abs
            sv = np.abs(0.0 - v0) * self.tol_rel + self.tol_abs
            with np.errstate(invalid="ignore"):
                eq, ev = np.abs(difference(self.model, qsol, qoth) / sq), np.abs((voth - vsol) / sv)
            error = np.where(np.isnan(eq).any(0) | np.isnan(ev).any(0), np.nan, np.fmax(eq, ev).max(0))
            code, dtl = np.zeros(B, dtype=np.int32), np.zeros(B)
            L.orc_leaf_dopri_adjust(B, _p(np.ascontiguousarray(error)), _p(np.ascontiguousarray(h)), _p(code, C.c_int32), _p(dtl))
            rc = np.where(code == 2, 2, np.where(code == 1, np.where(np.isnan(ka[6]).any(0), 2, 0), 1)).astype(np.int32)
            ok = active & (rc == 0)
            c.arr["q"][:, ok], c.arr["v"][:, ok], c.arr["a"][:, ok] = qsol[:, ok], vsol[:, ok], ka[6][:, ok]
            ad["t"][ok] += h[ok]
            c.t = np.where(ok, c.t + h, c.t)
            self.vmax = np.where(ok, np.maximum(self.vmax, np.abs(vsol).max(0)), self.vmax)
            dt, dtlp = ad["dt"].copy(), ad["dt_largest_prev"].copy()
            cnt = np.ascontiguousarray(np.stack([ad["succ_too_large"], ad["succ_failed"], ad["iter"], ad["iter_failed"]], 1).astype(np.int64))
            L.orc_leaf_after_try(B, _p(rc, C.c_int32), _p(bp, C.c_int32), self.restore, self.dt_max, _p(dt), _p(dtl), _p(dtlp),
                                 _p(cnt, C.c_int64))
            ad["dt"][active], ad["dt_largest"][active], ad["dt_largest_prev"][active] = dt[active], dtl[active], dtlp[active]
            for col, name in enumerate(("succ_too_large", "succ_failed", "iter", "iter_failed")):
                ad[name][active] = cnt[active, col]

    def reset_lanes(self, mask, q, v, t_engine):
        """`BatchedEngine.reset_lanes`: the lanes restart at process time 0 with a fresh stepper state at the engine's time."""
        self.c.reset_lanes(mask, q, v)
        for k in ("dt", "dt_largest", "dt_largest_prev"):
            self.ad[k][mask] = 1e-6
        self.ad["t"][mask] = t_engine
        for k in ("iter", "iter_failed", "succ_too_large", "succ_failed"):
            self.ad[k][mask] = 0
        self.stopped[mask] = False


def _root_frame(model):
    return next(n for n, f in model.frames.items() if f.parent_joint == 1)


def _compare(got_q, got_v, got_it, got_if, ref: ComposedDopri, what):
    """The two bars and the cap; prints what it measures."""
    same = (np.asarray(got_it) == ref.ad["iter"]) & (np.asarray(got_if) == ref.ad["iter_failed"])
    share = 1.0 - same.mean()
    e_same = {k: rel_err(x, ref.c.arr[k], same) for k, x in (("q", got_q), ("v", got_v))}
    e_all = {k: rel_err(x, ref.c.arr[k]) for k, x in (("q", got_q), ("v", got_v))}
    print(what, ": lanes on another accept / reject sequence", share, "; same-sequence lanes", e_same, "; all lanes", e_all,
          "; accepted steps", int(ref.ad["iter"].min()), "..", int(ref.ad["iter"].max()), "rejected", int(ref.ad["iter_failed"].sum()))
    assert share <= CAP, (got_it, ref.ad["iter"], got_if, ref.ad["iter_failed"])
    for k in ("q", "v"):
        assert e_same[k] <= BAR_SAME, (k, e_same)
        assert e_all[k] <= BAR_ALL, (k, e_all)
    return same


# ------------------------------------------------------------------------------------------ 0. the yardstick itself
def test_composed_adaptive_loop_reproduces_the_oracle():
    """Self-check of the yardstick: with a HELD wrench the composed loop is the oracle's own `batch_run_dopri`, ANYmal with
    lanes in ground contact (grounded_fraction 0.4), three breakpoint intervals of 4 ms: identical accept / reject counts on
    every lane; q, v, a and the per-lane step size to round-off (rel_err <= 1e-12)."""
    model = load_builtin("anymal")
    B = 16
    st = sample_states(model, B, seed=5, grounded_fraction=0.4)
    off = np.array([model.frame(_root_frame(model)).p])
    held = np.array([30., -20., 10., 1., 2., -3.])[:, None] * np.linspace(0.5, 1.5, B)[None, :]
    a = ComposedDopri(Composed(model, B, st["q"], st["v"], st["command"], lambda t: held, off), model, **_tol(TOL))
    b = Composed(model, B, st["q"], st["v"], st["command"], lambda t: held, off)
    bad = adaptive_state(B)
    touched = lowest_contact_height(model, st["q"]) < 0.0         # (lanes that start in ground contact)
    for i in range(3):
        a.interval(4e-3 * (i + 1))
        b.e.batch_run_dopri(b.io, bad, 4e-3 * (i + 1), tol_rel=TOL["tol_rel"], tol_abs=TOL["tol_abs"], new_step=True,
                            command_changed=False, update_sensors=True)
    assert np.array_equal(a.ad["iter"], bad["iter"]) and np.array_equal(a.ad["iter_failed"], bad["iter_failed"]), \
        (a.ad["iter"], bad["iter"], a.ad["iter_failed"], bad["iter_failed"])
    errs = {k: rel_err(a.c.arr[k], b.arr[k]) for k in "qva"}
    errs["dt"] = float(np.abs(a.ad["dt"] / bad["dt"] - 1.0).max())
    errs["t"] = float(np.abs(a.ad["t"] - bad["t"]).max())
    print("composed adaptive loop against the oracle's:", errs, "accepted", bad["iter"], "rejected", bad["iter_failed"])
    for k, e in errs.items():
        assert e <= 1e-12, (k, errs)
    assert touched.sum() >= 2 and np.all(bad["iter_failed"][touched] > 0)


def _tol(t):
    return dict(tol_rel=t["tol_rel"], tol_abs=t["tol_abs"])


def test_numpy_difference_is_the_inverse_of_the_oracle_integrate():
    """`difference(q, integrate(q, d)) == d` on ANYmal, rotations from tiny to near pi.  Bound per angle: 1e-12 relative plus
    the conditioning of the formulas themselves (shared with the oracle): log3's branch near pi, whose `1 + cos(theta)` ~
    (pi - theta)^2 / 2 cancels, 4 eps / (pi - theta)^2; and `1 - cos(theta)` in exp6 / log6 past the Taylor threshold,
    4 eps / (1 - cos(theta)) (1.8e-9 at theta = 1e-3; observed there: 4.7e-12)."""
    model = load_builtin("anymal")
    rg = np.random.default_rng(2)
    e = OracleEngine(model)
    q = sample_states(model, 12, seed=1)["q"]
    for l, ang in enumerate([0.0, 1e-9, 1e-5, 1e-3, 0.1, 0.5, 1.0, 2.0, 3.0, 3.13, 3.14, 3.1415]):
        d = rg.normal(0, 0.3, model.nv)
        ax = rg.normal(size=3)
        d[3:6] = ang * ax / np.linalg.norm(ax)
        q1 = e.integrate(q[:, l], d)
        got = difference(model, q[:, l:l + 1], q1[:, None])[:, 0]
        err = np.abs(got - d).max() / max(np.abs(d).max(), 1.0)
        eps = np.finfo(np.float64).eps
        bound = 1e-12 + 4.0 * eps / (math.pi - ang) ** 2
        if ang >= eps ** 0.25:      # past the Taylor branch exp6 and log6 divide by 1 - cos(theta), known to eps absolute
            bound += 4.0 * eps / (1.0 - math.cos(ang))
        print("difference o integrate - id: angle", ang, "error", err, "bound", bound)
        assert err <= bound, ang


# ------------------------------------------------------------------------------------------ 1. host-emulated persistent kernel
def _emu_scene(name, B, seed):
    model = load_builtin("anymal") if name == "anymal" else getattr(robots, name)()
    # (free flight over the three intervals: the accept / reject sequences of the emulated kernel and of the yardstick then
    # differ by round-off at a threshold only, which keeps the share of such lanes inside the cap on every host)
    st = sample_states(model, B, seed=seed, base_height=(1.0, 1.5), grounded_fraction=0.0)
    return model, st, np.zeros((1, 3)), np.array([1], dtype=np.int32)


def _emu_start(model, st, B, ps, frames, held=None):
    arr = alloc_soa(model, B)
    for k in ("q", "v", "command"):
        arr[k][:] = st[k]
    lane_time = np.full((1, B), 7.0)           # (`start` zeroes it)
    force_process.run(model, arr, "start", lane_time, processes=ps, frames=frames, held=held, variant="quad")
    assert np.all(lane_time == 0.0)
    return arr, lane_time


@pytest.mark.parametrize("name", ["anymal", "crane_walker"])
def test_host_emulated_persistent_kernel_matches_the_composed_loop(name):
    """`quad_dopri_run<..., GEN = true>` on the host with the environment's two processes (wavelength 0.2 and 1, period 1,
    scale 50) on force x and y of the root joint, tolAbs 1e-8, tolRel 1e-7, three intervals of 4 ms, against the composed
    loop: the two bars and the cap of the module header; lane time = stepper time."""
    B = 16
    model, st, offs, joints = _emu_scene(name, B, seed=9)
    procs = env_processes(B, 21)
    ref = ComposedDopri(Composed(model, B, st["q"], st["v"], st["command"], wrench_of(procs, B), offs, joints), model, **_tol(TOL))
    ps = [_emu_process(p, row=c, scale=SCALE) for c, p in enumerate(procs)]
    arr, lane_time = _emu_start(model, st, B, ps, (offs, joints))
    for k in "qva":
        assert rel_err(arr[k], ref.c.arr[k]) <= 1e-10, ("start", k)
    ad = adaptive_state(B)
    for i in range(3):
        left, _ = dopri_process.run(model, arr, ad, 4e-3 * (i + 1), lane_time, ps, (offs, joints), **TOL)
        assert left == 0
        ref.interval(4e-3 * (i + 1))
    assert int(arr["status"].sum()) == 0
    assert np.array_equal(lane_time[0], ad["t"]) and np.abs(ad["t"] - 0.012).max() <= 1e-12
    _compare(arr["q"], arr["v"], ad["iter"], ad["iter_failed"], ref, f"host-emulated persistent kernel, {name}")
    # the force did act: against the same run without it
    free = ComposedDopri(Composed(model, B, st["q"], st["v"], st["command"], lambda t: np.zeros((6, B)), offs, joints), model, **_tol(TOL))
    for i in range(3):
        free.interval(4e-3 * (i + 1))
    assert np.abs(free.c.arr["v"][:2] - ref.c.arr["v"][:2]).max() > 1e-4


def test_constant_process_equals_a_held_wrench_on_the_host():
    """Same-stage-time check: a process that is constant in time gives BIT-identical results to the same kernel stepping with
    that value as a held applied wrench (the spline of a constant is exact: y + r ((1 - r)(0) + 0))."""
    B = 8
    model, st, offs, joints = _emu_scene("anymal", B, seed=4)
    val = np.linspace(-1.0, 1.0, B)
    p = _constant_process(val, None)
    held = np.zeros((6, B))
    held[1] = SCALE * val
    runs = []
    for ps, hw in (([_emu_process(p, row=1, scale=SCALE)], None), ([], held)):
        arr = alloc_soa(model, B)
        for k in ("q", "v", "command"):
            arr[k][:] = st[k]
        lane_time = np.zeros((1, B))
        force_process.run(model, arr, "start", lane_time, processes=ps, frames=(offs, joints), held=hw, variant="quad")
        ad = adaptive_state(B)
        for i in range(3):
            dopri_process.run(model, arr, ad, 4e-3 * (i + 1), lane_time, ps, (offs, joints), held=hw, **TOL)
        runs.append((arr, ad))
    (a, ada), (b, adb) = runs
    for k in "qva":
        assert np.array_equal(a[k], b[k]), k
    for k in ("t", "dt", "iter", "iter_failed"):
        assert np.array_equal(ada[k], adb[k]), k
    assert ada["iter"].min() >= 3


# ------------------------------------------------------------------------------------------ 2. the law
def _law_bound(n_accepted, vmax, tol):
    """Sum of the per-step bounds of the error controller: each accepted step keeps its velocity error estimate below
    tolAbs + tolRel |v0| (computeError, max-norm < 1); nothing else is chosen."""
    return n_accepted * (tol["tol_abs"] + tol["tol_rel"] * vmax)


LAW_TOLS = (dict(tol_abs=1e-6, tol_rel=1e-5), dict(tol_abs=1e-8, tol_rel=1e-7))     # (a factor 100 apart)


@pytest.mark.parametrize("dt_max", [0.02, 0.15])
def test_impulse_momentum_law_of_the_composed_loop(dt_max):
    """Point mass (`_point_mass_scene`), no gravity, the environment's two processes on force x and y, DOPRI over 1.2 s (past
    the period) in intervals of 0.1 s: |m dv - int F dt| / m <= n_accepted (tolAbs + tolRel max|v|) per lane, `int F` the
    closed form of the spline.  Two tolerance pairs a factor 100 apart: the observed error shrinks.  dt_max = 0.15 exceeds
    both knot spacings (0.02, 0.1): steps cross knots.  The point mass has no branch-parallel decomposition, so the
    host-emulated persistent kernel cannot run it: on the CPU the law is held against the yardstick, on the device against
    the per-stage kernels (`test_gpu_impulse_momentum_law`)."""
    B, T = 8, 1.2
    m, mass, q0 = _point_mass_scene(B)
    procs = env_processes(B, 2)
    want = np.stack([SCALE * spline_integral(procs[0], T), SCALE * spline_integral(procs[1], T)])
    worst = []
    for tol in LAW_TOLS:
        ref = ComposedDopri(Composed(m, B, q0, np.zeros((m.nv, B)), 0.0, wrench_of(procs, B), np.zeros((1, 3)),
                                     gravity=(0.0,) * 6), m, dt_max=dt_max, **_tol(tol))
        for i in range(12):
            ref.interval(0.1 * (i + 1))
        err = np.abs(mass * ref.c.arr["v"][:2] - want).max(0) / mass
        bound = _law_bound(ref.ad["iter"], ref.vmax, tol)
        print("law, composed loop, dt_max", dt_max, tol, ": error", err.max(), "bound", bound.min(), "accepted", ref.ad["iter"],
              "largest step", float(ref.ad["dt_largest_prev"].max()))
        assert np.all(err <= bound), (err, bound)
        assert np.abs(ref.c.t - T).max() <= 1e-12
        worst.append(err.max())
    assert worst[1] < worst[0]


def test_dispatch_sends_process_forces_to_the_variation_form_of_the_stepper():
    """`select_adaptive_form` (jm_dispatch.h) with `Facts::process` set: the persistent kernel in its variation form
    (`k_quad_dopri_gen`) on a branch-parallel float64 batch with spring-damper contacts, the per-stage launches elsewhere
    (constraint model, float32, lane family, a forced per-stage form)."""
    from tests.test_dispatch_policy import ANYMAL, ARM, ATLAS, FORMS, LANE, NOSPLIT, QUAD
    src, hdr = os.path.join(_HERE, "hostemu", "dispatch_dopri_process.cpp"), os.path.join(codegen.CSRC, "jm_dispatch.h")
    os.makedirs(codegen.BUILD, exist_ok=True)
    out = os.path.join(codegen.BUILD, "libemu_dispatch_dopri_process.so")
    if (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, hdr)):
        subprocess.check_call(emu.host_compiler() + [src, "-o", out])
    L = C.CDLL(out)

    def form(traits, family, f64=1, constraint=0, process=1, per_stage=0):
        return FORMS[L.dispatch_dopri_process((C.c_int * 5)(*traits), family, f64, constraint, process, per_stage)]
    for topo in (ANYMAL, ATLAS, NOSPLIT):
        assert form(topo, QUAD) == "DOPRI_GEN" and form(topo, QUAD, process=0) == "DOPRI"
        assert form(topo, QUAD, per_stage=1) == "DOPRI_STAGES"
        assert form(topo, QUAD, constraint=1) == "DOPRI_STAGES"
        assert form(topo, QUAD, f64=0) == "DOPRI_STAGES"
        assert form(topo, LANE) == "DOPRI_STAGES"
    assert form(ARM, LANE) == "DOPRI_STAGES"


# ------------------------------------------------------------------------------------------ 3. the device
def _engine(model, B, device, constrained=False, extra=("f_external",), **stepper):
    from jiminy_amd.engine import BatchedEngine
    eng = BatchedEngine(model, B, dtype=torch.float64, device=device, extra_outputs=extra)
    st = {"odeSolver": "runge_kutta_dopri", "tolAbs": TOL["tol_abs"], "tolRel": TOL["tol_rel"], "controllerUpdatePeriod": 4e-3,
          "sensorsUpdatePeriod": 4e-3}
    st.update(stepper)
    eng.set_options({"stepper": st, "contacts": {"model": "constraint" if constrained else "spring_damper"}})
    return eng


def _gpu_scene(name, constrained, B, seed):
    model = load_builtin("anymal") if name == "anymal" else robots.tree_arm(True)
    # (free flight, as in tests/test_variation.py's adaptive profile-force test; the constraint model needs it anyway: no row
    # active, so the oracle's `dynamics` is stateless)
    st = sample_states(model, B, seed=seed, base_height=(1.0, 1.5), grounded_fraction=0.0)
    frame = _root_frame(model)
    return model, st, frame, np.array([model.frame(frame).p]), np.array([1], dtype=np.int32)


def _drive(eng, ref, constrained, n_steps=3, step=4e-3, t0=0.0, t_err0=0.0):
    """`n_steps` engine steps and the composed loop over the engine's own breakpoint schedule (a(t+) is refreshed at
    controller breakpoints under the constraint model, engine.py `_step_adaptive`)."""
    from jiminy_amd.engine import plan_breakpoints
    t, t_err = t0, t_err0
    for _ in range(n_steps):
        intervals, t_end, t_err = plan_breakpoints(t, t_err, step, eng.get_options())
        for i, (t_next, cmd_bp, sens) in enumerate(intervals):
            ref.interval(float(t_next), new_step=(i == 0), refresh=bool(cmd_bp and constrained))
        t = t_end
        eng.step(step)
    return t, t_err


GPU_CASES = [("anymal", False, "0"), ("anymal", False, "1"), ("anymal", True, "1"), ("tree_arm_ff", False, "1"),
             ("tree_arm_ff", True, "1")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,constrained,form", GPU_CASES)
def test_gpu_time_varying_processes_match_the_composed_loop(gpu_device, monkeypatch, name, constrained, form):
    """Both forms of the stepper (JIMINY_AMD_ADAPTIVE_FORM: 0 persistent kernel, 1 per-stage launches) and both kernel
    families and contact models, the environment's two processes on force x and y of a root frame, three steps of 4 ms:
    the two bars and the cap of the module header against the composed loop; status 0; lane time = stepper time."""
    monkeypatch.setenv("JIMINY_AMD_ADAPTIVE_FORM", form)
    B = 40
    model, st, frame, offs, joints = _gpu_scene(name, constrained, B, seed=9)
    procs = env_processes(B, 21)
    ref = ComposedDopri(Composed(model, B, st["q"], st["v"], st["command"], wrench_of(procs, B), offs, joints,
                                 copt=TIGHT if constrained else None), model, **_tol(TOL))
    eng = _engine(model, B, gpu_device, constrained)
    for c, p in enumerate(device_twins(procs, gpu_device)):
        eng.register_process_force(frame, p, c, scale=SCALE, adaptive=True)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    _drive(eng, ref, constrained)
    ss = eng.stepper_state
    assert int(eng.status.abs().sum()) == 0
    assert abs(ss.t - 0.012) < 1e-12
    lt = eng.lane_time.cpu().numpy()
    assert np.array_equal(lt, eng._adaptive["f64"][0].cpu().numpy()) and np.abs(lt - 0.012).max() <= 1e-12
    _compare(eng.field("q").cpu().numpy(), eng.field("v").cpu().numpy(), ss.iter_lanes.cpu().numpy(),
             ss.iter_failed_lanes.cpu().numpy(), ref, f"device, {name}, constraint model {constrained}, form {form}")


def _run_engine(gpu_device, model, st, frame, B, form, monkeypatch, procs=None, held=None, row=None, n_steps=3):
    monkeypatch.setenv("JIMINY_AMD_ADAPTIVE_FORM", form)
    eng = _engine(model, B, gpu_device)
    if procs is not None:
        for c, p in enumerate(procs):
            eng.register_process_force(frame, p, c if row is None else row, scale=SCALE, adaptive=True)
    if held is not None:
        w = torch.from_numpy(held.copy()).to(gpu_device)
        eng.register_profile_force(frame, lambda t, q, v, w=w: w, update_period=1.0)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    for _ in range(n_steps):
        eng.step(4e-3)
    ss = eng.stepper_state
    out = {k: eng.field(k).cpu().numpy().copy() for k in "qva"}
    out.update(iter=ss.iter_lanes.cpu().numpy().copy(), iter_failed=ss.iter_failed_lanes.cpu().numpy().copy(),
               status=eng.status.cpu().numpy().copy())
    eng.stop()
    return out


@pytest.mark.gpu
def test_gpu_persistent_and_per_stage_forms_agree(gpu_device, monkeypatch):
    """The same inputs through both forms: identical accept / reject counts on at least 80 % of the lanes, q and v of those
    lanes to 1e-7."""
    B = 40
    model, st, frame, offs, joints = _gpu_scene("anymal", False, B, seed=9)
    procs = device_twins(env_processes(B, 21), gpu_device)
    a = _run_engine(gpu_device, model, st, frame, B, "0", monkeypatch, procs)
    b = _run_engine(gpu_device, model, st, frame, B, "1", monkeypatch, procs)
    same = (a["iter"] == b["iter"]) & (a["iter_failed"] == b["iter_failed"])
    errs = {k: rel_err(a[k], b[k], same) for k in "qv"}
    print("persistent against per-stage: lanes on another sequence", 1.0 - same.mean(), errs)
    assert 1.0 - same.mean() <= CAP
    assert int(a["status"].sum()) == 0 and int(b["status"].sum()) == 0
    for k in "qv":
        assert errs[k] <= BAR_SAME, errs


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["0", "1"])
def test_gpu_constant_process_equals_a_held_wrench(gpu_device, monkeypatch, form):
    """A process that is constant in time against the same value as a held profile force, on the device, per form: bit
    identical states and accept / reject counts (the stage times cannot matter, everything else is the same code)."""
    B = 24
    model, st, frame, offs, joints = _gpu_scene("anymal", False, B, seed=4)
    val = np.linspace(-1.0, 1.0, B)
    p = [_constant_process(val, gpu_device)]
    held = np.zeros((6, B))
    held[1] = SCALE * val
    a = _run_engine(gpu_device, model, st, frame, B, form, monkeypatch, procs=p, row=1)
    b = _run_engine(gpu_device, model, st, frame, B, form, monkeypatch, held=held)
    for k in ("q", "v", "a", "iter", "iter_failed"):
        assert np.array_equal(a[k], b[k]), k
    assert a["iter"].min() >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["0", "1"])
def test_gpu_reset_lanes_in_the_middle_of_a_run(gpu_device, monkeypatch, form):
    """Two steps, `reset_lanes` of every third lane, two more steps: the reset lanes restart their process at lane time 0
    while the others continue; against the composed loop with the same reset."""
    monkeypatch.setenv("JIMINY_AMD_ADAPTIVE_FORM", form)
    B = 30
    model, st, frame, offs, joints = _gpu_scene("anymal", False, B, seed=13)
    procs = env_processes(B, 8)
    ref = ComposedDopri(Composed(model, B, st["q"], st["v"], st["command"], wrench_of(procs, B), offs, joints), model, **_tol(TOL))
    eng = _engine(model, B, gpu_device)
    for c, p in enumerate(device_twins(procs, gpu_device)):
        eng.register_process_force(frame, p, c, scale=SCALE, adaptive=True)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    t, t_err = _drive(eng, ref, False, n_steps=2)
    mask = (np.arange(B) % 3) == 0
    eng.reset_lanes(torch.from_numpy(mask), torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    ref.reset_lanes(mask, st["q"], st["v"], t)
    assert np.all(eng.lane_time.cpu().numpy()[mask] == 0.0)
    _drive(eng, ref, False, n_steps=2, t0=t, t_err0=t_err)
    lt = eng.lane_time.cpu().numpy()
    assert np.abs(lt - ref.c.t).max() <= 1e-12 and np.abs(lt - np.where(mask, 0.008, 0.016)).max() <= 1e-12
    assert int(eng.status.abs().sum()) == 0
    ss = eng.stepper_state
    _compare(eng.field("q").cpu().numpy(), eng.field("v").cpu().numpy(), ss.iter_lanes.cpu().numpy(),
             ss.iter_failed_lanes.cpu().numpy(), ref, f"device, reset_lanes, form {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt_max", [0.02])
def test_gpu_impulse_momentum_law(gpu_device, dt_max):
    """The law of `test_impulse_momentum_law_of_the_composed_loop` on the device (point mass: the one-robot-per-lane
    kernels, per-stage form), with the bound from the lanes' own accepted-step counts; the error shrinks with the tolerances.
    Controller period 0.1 s (12 steps of 0.1 s, dtMax 0.02: steps cross the knots of the short process)."""
    B, T = 8, 1.2
    m, mass, q0 = _point_mass_scene(B)
    procs = env_processes(B, 2)
    want = np.stack([SCALE * spline_integral(procs[0], T), SCALE * spline_integral(procs[1], T)])
    frame = _root_frame(m)
    worst = []
    for tol in LAW_TOLS:
        eng = _engine(m, B, gpu_device, extra=(), tolAbs=tol["tol_abs"], tolRel=tol["tol_rel"], dtMax=dt_max,
                      controllerUpdatePeriod=0.1, sensorsUpdatePeriod=0.1)
        eng.set_options({"world": {"gravity": [0.0] * 6}})
        for c, p in enumerate(device_twins(procs, gpu_device)):
            eng.register_process_force(frame, p, c, scale=SCALE, adaptive=True)
        eng.start(torch.from_numpy(q0), torch.zeros((m.nv, B), dtype=torch.float64))
        vmax = np.zeros(B)
        for _ in range(12):
            eng.step(0.1)
            vmax = np.maximum(vmax, eng.field("v").abs().max(0).values.cpu().numpy())
        assert int(eng.status.abs().sum()) == 0
        n_acc = eng.stepper_state.iter_lanes.cpu().numpy()
        err = np.abs(mass * eng.field("v").cpu().numpy()[:2] - want).max(0) / mass
        bound = _law_bound(n_acc, vmax, tol)
        print("law, device", tol, ": error", err.max(), "bound", bound.min(), "accepted", n_acc)
        assert np.all(err <= bound), (err, bound)
        assert np.abs(eng.lane_time.cpu().numpy() - T).max() <= 1e-9
        worst.append(err.max())
        eng.stop()
    assert worst[1] < worst[0]


@pytest.mark.gpu
def test_gpu_environment_with_the_default_solver_and_the_disturbance_on_the_device(gpu_device):
    """`make_anymal_env(..., ode_solver="runge_kutta_dopri", std_ratio={"disturbance": ...}, disturbance_on_device=True)`:
    a few environment steps, finite observations, `engine.lane_time` = the episode time of every environment (also after an
    auto-reset), a nonzero `f_external` on the root joint."""
    from jiminy_amd.envs import make_anymal_env
    B = 32
    env = make_anymal_env(B, device=gpu_device, ode_solver="runge_kutta_dopri", std_ratio={"disturbance": 0.3},
                          disturbance_on_device=True, disturbance_impulses=False, simulation_duration_max=0.1)
    env.engine.enable_output("f_external")
    obs, _ = env.reset(seed=3)
    assert len(env.engine._process_forces) == 2 and not env.engine._profile_forces
    action = torch.zeros((B, env.model.nmotors), dtype=torch.float64, device=gpu_device)
    reset_seen = False
    for k in range(8):
        obs, reward, terminated, truncated, info = env.step(action)
        for x in (obs["states"]["agent"]["q"], obs["states"]["agent"]["v"]):
            assert bool(torch.isfinite(x).all()), k
        lt, et = env.engine.lane_time, env._lane_time()
        assert float((lt - et).abs().max()) < 1e-9, (k, lt, et)
        reset_seen |= bool((et == 0.0).all()) and k > 0
        assert float(env.engine.field("f_external")[6:8].abs().max()) > 0.0
    assert reset_seen      # (simulation_duration_max = 0.1 s: every environment restarted once, at lane time 0)


@pytest.mark.gpu
def test_gpu_refusals_that_stay(gpu_device):
    """Process forces on a float32 batch, a registration under the adaptive solver that does not opt in, and `enable_graph`
    with the adaptive solver are still refused."""
    from jiminy_amd.engine import BatchedEngine
    from jiminy_amd.envs import make_anymal_env
    m = robots.point_mass()
    B = 8
    eng = BatchedEngine(m, B, dtype=torch.float32, device=gpu_device)
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_dopri"}, "contacts": {"model": "spring_damper"}})
    with pytest.raises(NotImplementedError, match="float64"):
        eng.register_process_force(_root_frame(m), PeriodicGaussianProcess(0.2, 1.0, B, device=gpu_device), 0, adaptive=True)
    # a registration that does not say `adaptive=True` is refused under the adaptive solver, as before
    e64 = BatchedEngine(m, B, dtype=torch.float64, device=gpu_device)
    e64.set_options({"stepper": {"odeSolver": "runge_kutta_dopri"}, "contacts": {"model": "spring_damper"}})
    with pytest.raises(NotImplementedError, match="adaptive stepper"):
        e64.register_process_force(_root_frame(m), PeriodicGaussianProcess(0.2, 1.0, B, device=gpu_device), 0)
    assert not e64._process_forces
    env = make_anymal_env(8, device=gpu_device, ode_solver="runge_kutta_dopri", std_ratio={"disturbance": 0.3},
                          disturbance_on_device=True, disturbance_impulses=False)
    env.reset(seed=1)
    with pytest.raises(NotImplementedError, match="fixed-step solver"):      # (its existing message)
        env.enable_graph()
