"""Robots that exist for compile-time branches of the branch-parallel kernels (`robots.quad_topology_models()`).

The quad family (jm_quad.h, jm_qcon.h, jm_qtip.h, jm_qdopri.h) is compiled once per topology from the tables of
`codegen.quad_structure`, and a topology the suite has never compiled is guarded by the self-tests at first use alone.
`hydra` and the three `quadlet_*` are built for the branches the other quad robots of the suite (anymal, atlas,
crane_walker, biped, biped_torso) never instantiate; the structural test below keeps them there, the GPU tests of this file
run the spring-damper kernels on them, and the parametrisations they join elsewhere do the rest:

  tests/test_hostemu_vs_oracle.py   host twins of the step and of the persistent adaptive stepper
  tests/test_constraint_model.py    constraint model, single kernel and split form, host and device (`hydra+trunk_bounds`)
  tests/test_quad_output_pass.py    every output of every mode (`hydra`, `quadlet_jside`)
  tests/test_gpu_parity.py          float32 engines (`hydra`, `quadlet_bare`), persistent adaptive stepper (`hydra`)
  tests/test_variation.py           variation kernels, both contact models (`hydra`)
  tests/test_frame_kinematics.py, tests/test_centroidal_state.py    the topology-independent blocks on a branched tree
"""
import numpy as np
import pytest

from jiminy_amd import codegen
from jiminy_amd.synthetic import sample_states
from tests import lane_failures as lf
from tests import robots
from tests.helpers import ReferenceFixedStepLoop, alloc_soa, oracle_batch, oracle_engine_step, rel_err

# robot: (model, base height of the sampled states, step size).  Chosen with the oracle alone at B = 96, 20 steps: every
# lane stays clean and 10 lanes are in contact at `start` (`quadlet_free` has no contact point).
CASES = {
    "hydra": (robots.hydra, (0.9, 1.2), 2.5e-4),
    "quadlet_bare": (lambda: robots.quadlet("bare"), (0.25, 0.4), 2.5e-4),
    "quadlet_jside": (lambda: robots.quadlet("jside"), (0.25, 0.4), 2.5e-4),
    "quadlet_free": (lambda: robots.quadlet("free"), (0.25, 0.4), 2.5e-4),
}
FIELDS = ("q", "v", "a", "u_motor", "u", "imu", "force", "contact", "encoder", "effort", "contact_forces", "energy",
          "f_external", "joint_forces", "centroidal")
EXTRA = ("contact_forces", "energy", "f_external", "joint_forces", "centroidal")


def test_quad_topology_models_hit_the_branches_they_are_for():
    """The structural facts the four robots exist for, from `codegen.quad_structure` and the motor flags: a change of the
    compiler's joint ordering (or of the data files) cannot silently turn them back into chains.

    hydra -- trunk_parent [-1, 0, 1, 2, 3, 4, 1, 6], QT = 8, limbs of 5 / 5 / 4 / 4 joints attached at trunk joints 0 / 0 / 2 / 2:
      * jm_quad.h:508   the `else` of `trunk_fk_store`: the parent's placement read back from the quad-distributed
                        `TrunkStore` with `get_kin<tp>` (tail_a: its parent, the waist, is neither the root nor the joint before);
      * jm_quad.h:1309  the `qbcast` of `atst[slot<tp>]` in the forward acceleration pass;
      * `QInfo::child_after`, the accumulating arm of `first_contrib` and `fjT` at jm_quad.h:1505 with siblings: chest and
                        tail_a are both trunk children of the waist;
      * jm_qcon.h:108   the ancestry test of the constraint rows answers "not an ancestor" (tail_a / head_j, the state of
                        `hydra+trunk_bounds` in tests/test_constraint_model.py), jm_qcon.h:435-469 `trunk_column` with siblings;
      * `TrunkStore::SLOTS = (QT + 2) / 4 = 2`: `slot<t>() == 1`, and a fetch whose source lane and slot both differ from
                        the reader's (tail_a, entry 6, reads the waist, entry 1);
      * limbs of 4 and of 5 joints; a prismatic unaligned (`JT_PU`) trunk joint (tail_b).
    quadlet_bare  -- `QHAS_FORCE`, `QHAS_ENC`, `QHAS_EFF` all false; `limb_motor` / `trunk_motor` (jm_quad.h:263-279) without
                     the effort and without the velocity limit; a `JT_PU` trunk joint.
    quadlet_jside -- `QENC_SIDE == 1`: the `else` arms at jm_quad.h:821 and jm_quad.h:838; contact sensors on every contact
                     point; motors with the effort limit and friction, without the velocity limit.
    quadlet_free  -- no contact point: `NC = 0`, `QCL = 0` (`_arr` and `padc` pad the tables to length 1).

    Worst error of the device against the oracle as measured on an MI355X (`test_gpu_start_and_steps_match_oracle_fp64`, both
    solvers, B in {1, 65, 96}; worst field), next to the bar it is held to:

      robot            start (bar 1e-11)    20 steps (bar 1e-8)
      hydra            2.4e-12              1.2e-10
      quadlet_bare     4.0e-14              1.6e-12
      quadlet_jside    4.0e-14              1.4e-12
      quadlet_free     5.3e-15              5.4e-14

    and of the other phases on `hydra`: block-wave form (B = 32 705) 3.6e-14 / 5.4e-14; constraint model, single kernel and split
    form, with and without the trunk-bounds state, 1.3e-12 at worst (bars 1e-7 ... 1e-4 of the joined functions).
    """
    from tests.hostemu import emu
    models = {m.name: m for m in robots.quad_topology_models()}
    assert sorted(models) == sorted(CASES)
    assert len({m.topology_hash() for m in models.values()}) == 4            # each hardware file is a topology of its own
    qs = {n: codegen.quad_structure(m) for n, m in models.items()}
    assert all(q is not None for q in qs.values())
    flags = {n: {(x.enable_effort_limit, x.enable_velocity_limit, x.enable_friction) for x in m.motors} for n, m in models.items()}
    traits = lambda q: (q["has_force"], q["has_cs"], q["has_enc"], q["has_eff"], q["enc_side"], q["ncl"])  # noqa: E731

    # ---- hydra: a trunk TREE
    m, q = models["hydra"], qs["hydra"]
    tp, QT = q["trunk_parent"], len(q["trunk"])
    assert m.nv - 6 == 25 and m.njoints - 1 == 26 and QT == 8 and tp == [-1, 0, 1, 2, 3, 4, 1, 6]
    assert q["limb_len"] == [5, 5, 4, 4] and q["limb_attach"] == [0, 0, 2, 2] and q["imu_trunk"] == [0, 4]
    assert any(tp[t] not in (0, t - 1) for t in range(1, QT))                # a parent that is read back from the store
    assert max(tp.count(t) for t in range(1, QT)) >= 2                       # two trunk children of one (non-root) trunk joint
    assert (QT + 2) // 4 >= 2                                                # TrunkStore::SLOTS
    # TrunkStore (jm_quad.h): trunk entry t >= 1 lives in lane (t - 1) & 3, slot (t - 1) >> 2 (the root is not stored) -- a
    # fetched parent in another slot AND another lane than its reader
    lane, slot = (lambda t: (t - 1) & 3), (lambda t: (t - 1) >> 2)      # noqa: E731
    assert max(slot(t) for t in range(1, QT)) == 1
    assert any(tp[t] not in (0, t - 1) and slot(tp[t]) != slot(t) and lane(tp[t]) != lane(t) for t in range(1, QT))
    assert traits(q) == (True, False, True, True, 0, 2) and flags["hydra"] == {(True, True, False)}
    assert codegen.qcon_split(m) and m.ncontacts == 6
    from jiminy_amd.model import JT_PU
    assert int(m.jtypes[q["trunk"][7]]) == JT_PU and m.joint_names[q["trunk"][6]] == "tail_a" and m.joint_names[q["trunk"][4]] == "head_j"
    sa = m.signed_axes()
    assert (sa < 0).any() and (sa > 0).any() and any(sa[j] == 0 for j in range(2, m.njoints))   # aligned, negative, unaligned axes

    # ---- quadlet: one tree, three sets of traits
    for n in ("quadlet_bare", "quadlet_jside", "quadlet_free"):
        assert qs[n]["trunk_parent"] == [-1, 0] and qs[n]["limb_len"] == [2, 2, 2, 2] and qs[n]["limb_attach"] == [0, 0, 1, 1]
        assert int(models[n].jtypes[qs[n]["trunk"][1]]) == JT_PU
    assert traits(qs["quadlet_bare"]) == (False, False, False, False, 0, 1) and flags["quadlet_bare"] == {(False, False, False)}
    assert traits(qs["quadlet_jside"]) == (False, True, True, False, 1, 1) and flags["quadlet_jside"] == {(True, False, True)}
    assert traits(qs["quadlet_free"]) == (False, False, True, True, 0, 0) and flags["quadlet_free"] == {(True, True, False)}
    assert models["quadlet_free"].ncontacts == 0 and models["quadlet_bare"].ncontacts == 4
    assert len(models["quadlet_bare"].sensors.get("ImuSensor", [])) == 1

    # ---- the dispatch traits the GPU tests select the expected kernel form with are those of the kernel headers
    from tests import test_dispatch_policy as dp
    from jiminy_amd import load_builtin
    for n, mdl in models.items():
        assert emu.dispatch_traits(mdl) == lf.QUAD_TOPOLOGY_TRAITS[n], n
    # (... and the reading of the headers is held to the tuples known for the shipped robots.  `dp.ATLAS` states 2 block waves
    # as an example of the rule; the library's own value follows the LDS layout of the shipped Atlas: not compared)
    assert emu.dispatch_traits(load_builtin("anymal")) == dp.ANYMAL
    atlas = emu.dispatch_traits(load_builtin("atlas"))
    assert atlas[:3] + atlas[4:] == dp.ATLAS[:3] + dp.ATLAS[4:]


# ------------------------------------------------------------------------------------------------------ device
def _states(name, B, seed=3):
    model = CASES[name][0]()
    st = sample_states(model, B, seed=seed, base_height=CASES[name][1])
    return model, st


def _engine(model, B, solver, dt, device):
    import torch

    from jiminy_amd.engine import BatchedEngine
    eng = BatchedEngine(model, B, dtype=torch.float64, device=device, extra_outputs=EXTRA)
    eng.set_options({"stepper": {"odeSolver": solver, "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt},
                     "contacts": {"model": "spring_damper"}})
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 65, 96])
@pytest.mark.parametrize("solver", ["runge_kutta_4", "euler_explicit"])
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_start_and_steps_match_oracle_fp64(gpu_device, name, solver, B):
    """The body of tests/test_gpu_parity.py::test_start_and_steps_match_oracle_fp64 on the four robots, through the C ABI:
    every output 1e-11 after `start`, 1e-8 after 20 steps on the lanes the oracle leaves clean, status bit-equal.  Batches of
    a partial wave, of a partial second block and of six quad waves: all in the one-wave form (asserted)."""
    import torch
    from tests.test_lane_failures import _Q, _assert_forms
    _assert_forms(gpu_device, name, B, [(dict(_Q, mode="start"), "QUAD_ONE_WAVE"), (dict(_Q, mode="step"), "QUAD_ONE_WAVE")])
    model, st = _states(name, B)
    dt = CASES[name][2]
    ref = alloc_soa(model, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    oracle_batch(model, ref, "start")
    loop = ReferenceFixedStepLoop(dt)   # the reference's sub-step rule: opens with a 1 us step (engine.cc:1176)
    eng = _engine(model, B, solver, dt, gpu_device)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    torch.cuda.synchronize()
    errs = {k: rel_err(eng.field(k).cpu().numpy(), ref[k]) for k in FIELDS}
    print(f"[{name} {solver} B={B}] start: worst {max(errs.values()):.2e} | " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, e in errs.items():
        assert e < 1e-11, ("start", k, e)
    assert np.array_equal(eng.status.cpu().numpy(), ref["status"][0])
    if B >= 65 and model.ncontacts:
        assert (np.abs(ref["contact_forces"]).sum(axis=0) > 0).sum() >= 3      # the contact branch is exercised
    for i in range(20):
        oracle_engine_step(model, ref, loop, dt, solver, command_changed=(i == 0))
        if i == 0:
            eng.mark_command_changed()
        eng.step(dt)
    torch.cuda.synchronize()
    ok = (ref["status"][0] & 1) == 0
    assert ok.sum() > 0.5 * B
    errs = {k: rel_err(eng.field(k).cpu().numpy(), ref[k], ok) for k in FIELDS}
    print(f"[{name} {solver} B={B}] 20 steps: worst {max(errs.values()):.2e} | " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, e in errs.items():
        # fp64 tolerance: only operation order / FMA contraction differ from the oracle
        assert e < 1e-8, ("steps", k, e)
    assert np.array_equal(eng.status.cpu().numpy()[ok], ref["status"][0][ok])


@pytest.mark.gpu
def test_gpu_hydra_in_the_block_wave_form(gpu_device):
    """`k_quad` with the topology's block waves: the trunk table is staged once per block, and a table of 8 trunk joints is
    new for it.  The smallest batch `select_form` sends there (tests/test_lane_failures.py,
    `test_gpu_isolation_in_the_block_wave_form`): hydra's blocks hold 4 waves of 16 robots, so 64 (2 n_cus - 1) + 1 robots;
    one robot less runs one wave per block (asserted).  The batch repeats a pool of 128 seeded states; the oracle runs on the
    64 lanes around the first block boundary (63 | 64) and on the last robot, alone in its block.  `start` plus three steps."""
    import torch
    from tests.test_lane_failures import _Q, _assert_forms
    name, solver = "hydra", "runge_kutta_4"
    B = 64 * (2 * torch.cuda.get_device_properties(gpu_device).multi_processor_count - 1) + 1
    _assert_forms(gpu_device, name, B, [(dict(_Q, mode="start"), "QUAD"), (dict(_Q, mode="step"), "QUAD")])
    _assert_forms(gpu_device, name, B - 1, [(dict(_Q, mode="step"), "QUAD_ONE_WAVE")])
    model, pool = _states(name, 128, seed=5)
    dt = CASES[name][2]
    lanes = np.arange(B) % 128
    sample = np.concatenate([np.arange(32, 96), [B - 1]])
    ref = alloc_soa(model, len(sample))
    for k in ("q", "v", "command"):
        ref[k][:] = pool[k][:, lanes[sample]]
    oracle_batch(model, ref, "start")
    loop = ReferenceFixedStepLoop(dt)
    eng = _engine(model, B, solver, dt, gpu_device)
    eng.set_command(torch.from_numpy(np.ascontiguousarray(pool["command"][:, lanes])))
    eng.start(torch.from_numpy(np.ascontiguousarray(pool["q"][:, lanes])), torch.from_numpy(np.ascontiguousarray(pool["v"][:, lanes])))
    torch.cuda.synchronize()

    def fields():
        return {k: eng.field(k).cpu().numpy() for k in FIELDS}, eng.status.cpu().numpy()

    got, status = fields()
    errs = {k: rel_err(got[k][:, sample], ref[k]) for k in FIELDS}
    print(f"[hydra block waves B={B}] start: worst {max(errs.values()):.2e}")
    assert max(errs.values()) < 1e-11, errs
    assert np.array_equal(status[sample], ref["status"][0])
    for i in range(3):
        oracle_engine_step(model, ref, loop, dt, solver, command_changed=(i == 0))
        if i == 0:
            eng.mark_command_changed()
        eng.step(dt)
    torch.cuda.synchronize()
    got, status = fields()
    ok = (ref["status"][0] & 1) == 0
    assert ok.sum() > 0.5 * len(sample)
    errs = {k: rel_err(got[k][:, sample], ref[k], ok) for k in FIELDS}
    print(f"[hydra block waves B={B}] 3 steps: worst {max(errs.values()):.2e}")
    assert max(errs.values()) < 1e-8, errs
    assert np.array_equal(status[sample][ok], ref["status"][0][ok])
    # every robot of the batch repeats one of the pool: the same bits in every block, whichever wave of it the robot rides in
    first = {k: v[:, :128] for k, v in got.items()}
    for k in ("q", "v", "a", "imu", "centroidal"):
        assert np.array_equal(got[k], first[k][:, lanes], equal_nan=True), k
