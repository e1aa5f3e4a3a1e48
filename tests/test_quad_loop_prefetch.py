"""Where the branch-parallel step kernels issue their loads: the launch prologue (state, commands and limb table loaded in
one batch ahead of the stage-buffer stores) and the evaluation loop behind it, on every path that shares the code.

The results must not depend on where a load is issued, so everything here is a parity check against the CPU oracle at
the bars tests/test_gpu_parity.py uses (`test_ragged_and_tiny_batches`: 1e-9 on the outputs and equal status words after
single-step launches; `test_multi_substep_launches_match_oracle`: 1e-8 on the outputs, `u`, the energies and fExternal
after launches of several integrator steps), over the launch shapes on which a misplaced read shows:

* robots: ANYmal (root + four equal limbs, the two-waves-per-SIMD kernel), `biped_torso` (a trunk tree, limbs of
  3 / 3 / 1 / 0 joints: padded and empty limbs) and Atlas (long limbs: velocities and commands re-read from the stage rows);
* batches of 1, 17 and 80 robots: a partial quad tile (16 robots per wave), a partial wave and a partial block;
* RK4 (rows read after an intermediate stage stored them) and explicit Euler (every evaluation commits);
* one and three integrator steps per launch, with and without the a(t+) evaluation of a changed command in front;
* the first launch after `start`, and the first launch after `reset_lanes` of a lane subset (the reset launch takes the
  early-exit path for the other lanes and stores the state it loaded back into the batch);
* the same robot in all 80 lanes: every lane must give the same bits (a read of a neighbour's stage row would not).
"""
import numpy as np
import pytest
import torch

from jiminy_amd import load_builtin
from jiminy_amd.engine import BatchedEngine
from jiminy_amd.synthetic import sample_states
from tests.helpers import ReferenceFixedStepLoop, alloc_soa, oracle_batch, oracle_engine_step, rel_err

OUTS = ("q", "v", "a", "u_motor", "imu", "force", "encoder", "effort", "contact_forces")
EXTRA = ("contact_forces", "energy", "f_external", "joint_forces", "centroidal")
# name: (sample_states arguments, dtMax)
ROBOTS = {
    "anymal": (dict(base_height=(0.45, 0.65)), 5e-4),
    "biped_torso": (dict(base_height=(0.55, 0.75), grounded_fraction=0.5), 2.5e-4),
    "atlas": (dict(base_height=(0.9, 1.1)), 2.5e-4),
}
BATCHES = (1, 17, 80)


def _model(name):
    if name == "biped_torso":
        from tests import robots
        return robots.biped(True)
    return load_builtin(name)


def _engine(model, B, solver, dt, n_sub):
    eng = BatchedEngine(model, B, dtype=torch.float64, extra_outputs=EXTRA)
    eng.set_options({"stepper": {"odeSolver": solver, "dtMax": dt, "controllerUpdatePeriod": n_sub * dt,
                                 "sensorsUpdatePeriod": n_sub * dt}, "contacts": {"model": "spring_damper"}})
    return eng


def _compare(eng, ref, n_sub, what):
    ok = (ref["status"][0] & 1) == 0
    assert ok.any(), what
    if n_sub == 1:   # the bar of test_ragged_and_tiny_batches
        for k in OUTS:
            e = rel_err(eng.field(k).cpu().numpy(), ref[k], ok)
            assert e < 1e-9, (what, k, e)
        assert np.array_equal(eng.status.cpu().numpy()[ok], ref["status"][0][ok]), what
    else:            # the bar of test_multi_substep_launches_match_oracle
        for k in OUTS + ("u", "energy", "f_external"):
            e = rel_err(eng.field(k).cpu().numpy(), ref[k], ok)
            assert e < 1e-8, (what, k, e)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["runge_kutta_4", "euler_explicit"])
@pytest.mark.parametrize("name", list(ROBOTS))
def test_first_launches_after_start_and_after_a_lane_reset_match_oracle(gpu_device, name, solver):
    model = _model(name)
    kw_states, dt = ROBOTS[name]
    rng = np.random.default_rng(5)
    for B in BATCHES:
        st = sample_states(model, B, seed=31 + B, **kw_states)
        st2 = sample_states(model, B, seed=47 + B, **kw_states)      # where the reset lanes restart
        mask = np.zeros(B, dtype=bool)
        mask[::3] = True                                              # (B = 1: the only lane)
        for n_sub in (1, 3):
            for changed in (False, True):
                what = f"{name} {solver} B={B} n_sub={n_sub} command_changed={changed}"
                ref = alloc_soa(model, B)
                for k in ("q", "v", "command"):
                    ref[k][:] = st[k]
                oracle_batch(model, ref, "start")
                loop = ReferenceFixedStepLoop(dt)
                eng = _engine(model, B, solver, dt, n_sub)
                eng.set_command(torch.from_numpy(st["command"]))
                eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))

                def step():
                    if changed:
                        cmd = ref["command"] * rng.uniform(0.5, 1.0)
                        ref["command"][:] = cmd
                        eng.set_command(torch.from_numpy(cmd))
                    oracle_engine_step(model, ref, loop, n_sub * dt, solver, command_changed=changed)
                    eng.step(n_sub * dt)

                # one launch after `start` (with the opening microsecond step of a simulation in front of it)
                step()
                _compare(eng, ref, n_sub, what + ": after start")
                # the masked lanes restart from another state, the others go on; one launch after that
                sub = alloc_soa(model, int(mask.sum()))
                sub["q"][:] = st2["q"][:, mask]
                sub["v"][:] = st2["v"][:, mask]
                sub["command"][:] = ref["command"][:, mask]
                oracle_batch(model, sub, "start")
                for k in ref:
                    ref[k][:, mask] = sub[k]
                eng.reset_lanes(torch.from_numpy(mask), torch.from_numpy(st2["q"]), torch.from_numpy(st2["v"]))
                step()
                _compare(eng, ref, n_sub, what + ": after reset_lanes")


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["runge_kutta_4", "euler_explicit"])
@pytest.mark.parametrize("name", list(ROBOTS))
def test_replicas_of_one_robot_give_the_same_bits_in_every_lane(gpu_device, name, solver):
    model = _model(name)
    kw_states, dt = ROBOTS[name]
    B, n_sub = 80, 3
    one = sample_states(model, 1, seed=7, **kw_states)
    eng = _engine(model, B, solver, dt, n_sub)
    eng.set_command(torch.from_numpy(np.repeat(one["command"], B, axis=1)))
    eng.start(torch.from_numpy(np.repeat(one["q"], B, axis=1)), torch.from_numpy(np.repeat(one["v"], B, axis=1)))
    eng.step(n_sub * dt)
    eng.mark_command_changed()
    eng.step(n_sub * dt)
    for k in OUTS + ("u", "energy", "f_external", "joint_forces", "centroidal"):
        x = eng.field(k).cpu().numpy()
        assert np.array_equal(x.view(np.uint8), np.repeat(x[:, :1], B, axis=1).view(np.uint8)), k
    s = eng.status.cpu().numpy()
    assert (s == s[0]).all()


@pytest.mark.parametrize("solver", ["runge_kutta_4", "euler_explicit"])
@pytest.mark.parametrize("name", ["anymal", "biped_torso"])
def test_host_emulation_of_the_same_launches(name, solver):
    """The kernel code on the host (one thread per quad lane), the same launch shapes: against the oracle at the bar of
    tests/test_hostemu_vs_oracle.py, and replicas bit for bit."""
    from tests.hostemu import emu
    model = _model(name)
    kw_states, dt = ROBOTS[name]
    B = 5
    st = sample_states(model, B, seed=31, **kw_states)
    st["q"][:, 3:] = st["q"][:, 2:3]          # lanes 2, 3, 4: one robot
    st["v"][:, 3:] = st["v"][:, 2:3]
    st["command"][:, 3:] = st["command"][:, 2:3]
    ref, got = alloc_soa(model, B), alloc_soa(model, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
        got[k][:] = st[k]
    oracle_batch(model, ref, "start")
    emu.run(model, got, "start", variant="quad")
    for n_sub, changed in ((1, False), (3, True), (3, False), (1, True)):
        kw = dict(solver=solver, dt=dt, n_substeps=n_sub, command_changed=changed)
        oracle_batch(model, ref, "step", **kw)
        emu.run(model, got, "step", variant="quad", **kw)
    ok = (ref["status"][0] & 1) == 0
    assert ok.any()
    for k in OUTS:
        e = rel_err(got[k], ref[k], ok)
        assert e < 1e-8, (k, e)
    assert np.array_equal(got["status"][0][ok], ref["status"][0][ok])
    for k in OUTS:
        assert np.array_equal(got[k][:, 3:].view(np.uint8), np.repeat(got[k][:, 2:3], 2, axis=1).view(np.uint8)), k
