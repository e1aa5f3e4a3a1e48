"""Per-environment variation: body-parameter biases per lane
(`Model::addBiasedToExtendedModel`, core/src/robot/model.cc:1166-1236), the ground profile as a height map
(`world.groundProfile`, engine.h:292-302, engine.cc:3138-3145) and impulse / profile forces on frames of any joint
(engine.cc:1838-2016).  Layers: the oracle on laws it must obey, the kernel sources on the host against the
oracle, and (`-m gpu`) the device build through the C ABI / BatchedEngine against the oracle."""
import math

import numpy as np
import pytest

from jiminy_amd import load_builtin
from jiminy_amd.engine import _breakpoint_intervals, default_options
from jiminy_amd.randomization import nominal_model_lane, sample_model_lane
from jiminy_amd.synthetic import sample_standing_states, sample_states
from oracle.oracle_py import OracleEngine
from tests.helpers import (ReferenceFixedStepLoop, alloc_constraint_state, alloc_soa, oracle_batch, oracle_engine_step, oracle_io,
                           rel_err)
from tests.hostemu import emu

OUTS = ("q", "v", "a", "u", "imu", "force", "energy", "contact_forces", "f_external", "joint_forces", "centroidal")
TIGHT = dict(tol_abs=1e-11, tol_rel=1e-10)


def _scene(model, B, seed, constrained):
    """Seeded states + a biased model per lane + a bumpy ground + two wrenches on root-body frames."""
    import torch
    rg = np.random.default_rng(seed)
    st = sample_standing_states(model, B, seed=seed) if constrained else sample_states(model, B, seed=seed, grounded_fraction=0.75)
    ml = sample_model_lane(model, B, {"massBodiesBiasStd": 0.1, "inertiaBodiesBiasStd": 0.1,
                                      "centerOfMassPositionBodiesBiasStd": 0.05, "relativePositionBodiesBiasStd": 0.02},
                           torch.Generator().manual_seed(seed)).numpy()
    heights = 0.02 * rg.standard_normal((7, 9))
    # (both contact models: with the constraint model the contact rows live in the local frame of the bumpy surface)
    ground = (0.25 * heights, -1.0, -0.8, 0.25, 0.3) if constrained else (heights, -1.0, -0.8, 0.25, 0.3)
    applied = (rg.normal(0, 30.0, (12, B)), np.array([[0.0, 0.0, 0.0], [0.1, -0.05, 0.02]]))
    return st, ml, ground, applied


def _oracle(model, arr, ml, ground, applied, copt):
    e = OracleEngine(model)
    if copt is not None:
        e.set_constraint_options(**copt)
        e.bind_constraints(arr["con_flags"], arr["con_data"])
    e.bind_model_lane(ml)
    if ground is not None:
        e.bind_ground(*ground)
    if applied is not None:
        e.bind_applied(*applied)
    return e


def _model(name):
    # (`biped_torso`: limbs of 3 / 3 / 1 / 0 joints -- the per-lane parameters of a decomposition with an empty limb)
    if name == "biped_torso":
        from tests import robots
        return robots.biped(True)
    # (`hydra`: the per-lane body parameters of the 7 movable trunk joints pass through `ma.rbi`, on both trunk branches)
    if name == "hydra":
        from tests import robots
        return robots.hydra()
    return load_builtin(name)


@pytest.mark.parametrize("name,constrained", [("anymal", False), ("anymal", True), ("atlas", False), ("atlas", True),
                                              ("biped_torso", False), ("biped_torso", True), ("hydra", False), ("hydra", True)])
def test_branch_parallel_code_with_variation_matches_oracle_on_the_host(name, constrained):
    model = _model(name)
    B = 16 if name == "anymal" else 4
    st, ml, ground, applied = _scene(model, B, 5 if name == "anymal" else 6, constrained)
    copt = TIGHT if constrained else None
    ref, got = alloc_soa(model, B), alloc_soa(model, B)
    for arr in (ref, got):
        if constrained:
            alloc_constraint_state(model, arr, B)
        for k in ("q", "v", "command"):
            arr[k][:] = st[k]
    e = _oracle(model, ref, ml, ground, applied, copt)
    io = oracle_io(ref)
    kw = dict(variant="quad", constraint_options=copt, model_lane=ml, ground=ground, applied=applied)
    e.batch_run("start", io)
    emu.run(model, got, "start", **kw)
    for k in OUTS:
        assert rel_err(got[k], ref[k]) < 1e-10, ("start", k)
    a_start = got["a"].copy()
    in_contact = np.abs(ref["contact_forces"]).sum(axis=0) > 0
    for solver in ("runge_kutta_4", "euler_explicit"):
        for _ in range(2):
            e.batch_run("step", io, solver=solver, dt=5e-4, n_substeps=2, command_changed=True)
            emu.run(model, got, "step", solver=solver, dt=5e-4, n_substeps=2, command_changed=True, **kw)
            in_contact |= np.abs(ref["contact_forces"]).sum(axis=0) > 0
        ok = (ref["status"][0] & 1) == 0
        assert ok.sum() >= B - 1
        for k in OUTS:
            assert rel_err(got[k], ref[k], ok) < 1e-8, (solver, k)
    assert in_contact.sum() >= 1
    # the variation is not a no-op: the nominal model on flat ground without wrenches gives another answer
    plain = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, plain, B)
    for k in ("q", "v", "command"):
        plain[k][:] = st[k]
    emu.run(model, plain, "start", variant="quad", constraint_options=copt)
    assert rel_err(plain["a"], a_start) > 1e-3


def _lane_family_model(name):
    from tests import robots
    return {"tree_arm_ff": lambda: robots.tree_arm(True), "tree_arm": lambda: robots.tree_arm(False),
            "tree_arm_flex_ff": lambda: robots.tree_arm_flexible(True), "arm7": robots.arm7}[name]()


@pytest.mark.parametrize("name,constrained", [("tree_arm_ff", False), ("tree_arm_ff", True), ("tree_arm_flex_ff", False),
                                              ("arm7", False), ("arm7", True)])
def test_one_robot_per_lane_code_with_variation_matches_oracle_on_the_host(name, constrained):
    """The variation instantiation of the one-robot-per-lane kernels (round 6, ABI 9): a biased model per lane
    (`Model::addBiasedToExtendedModel`: mass, centre of mass, inertia, relative body position) and wrenches on frames of two
    joints, both contact models, against the oracle's one-robot engine."""
    import torch
    model = _lane_family_model(name)
    B = 8
    rg = np.random.default_rng(31)
    st = sample_states(model, B, seed=31, base_height=(0.3, 0.6), grounded_fraction=0.6)
    ml = sample_model_lane(model, B, {"massBodiesBiasStd": 0.1, "inertiaBodiesBiasStd": 0.1,
                                      "centerOfMassPositionBodiesBiasStd": 0.05, "relativePositionBodiesBiasStd": 0.02},
                           torch.Generator().manual_seed(31)).numpy()
    joints = np.array([2, model.njoints - 1], dtype=np.int32)
    applied = (rg.normal(0, 20.0, (12, B)), np.array([[0.05, -0.02, 0.03], [0.0, 0.01, -0.04]]), joints)
    copt = TIGHT if constrained else None
    # (spring-damper law: a bumpy height map too, every lane on its own patch of it)
    ground = None if constrained else (0.03 * rg.standard_normal((7, 9)), -1.0, -0.8, 0.25, 0.3)
    offsets = None if constrained else np.ascontiguousarray(rg.uniform(-0.3, 0.3, (2, B)))
    for with_wrenches in (False, True):
        ref, got = alloc_soa(model, B), alloc_soa(model, B)
        for arr in (ref, got):
            if constrained:
                alloc_constraint_state(model, arr, B)
            for k in ("q", "v", "command"):
                arr[k][:] = st[k]
        e = _oracle(model, ref, ml, ground, applied if with_wrenches else None, copt)
        if offsets is not None:
            e.bind_ground_offset(offsets)
            got["ground_offset"] = offsets
        io = oracle_io(ref)
        kw = dict(variant="lane", constraint_options=copt, model_lane=ml, ground=ground, applied=applied if with_wrenches else None)
        e.batch_run("start", io)
        emu.run(model, got, "start", **kw)
        for k in OUTS:
            assert rel_err(got[k], ref[k]) < 1e-10, ("start", with_wrenches, k)
        a_start = got["a"].copy()
        for solver in ("runge_kutta_4", "euler_explicit"):
            e.batch_run("step", io, solver=solver, dt=5e-4, n_substeps=2, command_changed=True)
            emu.run(model, got, "step", solver=solver, dt=5e-4, n_substeps=2, command_changed=True, **kw)
            # (a robot dropped deep into a bump of the map leaves at 1e12 m/s on both sides: not a comparison)
            ok = ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2) & (np.abs(ref["a"]).max(axis=0) < 1e6)
            assert ok.sum() >= B // 2
            for k in OUTS:
                assert rel_err(got[k], ref[k], ok) < 1e-8, (solver, with_wrenches, k)
    # the biased models are not a no-op
    plain = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, plain, B)
    for k in ("q", "v", "command"):
        plain[k][:] = st[k]
    emu.run(model, plain, "start", variant="lane", constraint_options=copt, applied=applied)
    assert rel_err(plain["a"], a_start) > 1e-3


@pytest.mark.parametrize("name,constrained", [("anymal", False), ("anymal", True), ("atlas", False),
                                              ("tree_arm_ff", False), ("tree_arm_flex_ff", False)])
def test_applied_forces_on_frames_of_any_joint_on_the_host(name, constrained):
    """`Engine::registerImpulseForce / registerProfileForce` accept any frame (engine.cc:1838-1935); the wrench goes to the
    frame's parent joint (computeExternalForces, engine.cc:3481-3560).  Two frames: one on the first joint after the root
    (ANYmal: a hip, Atlas: the first back joint of the trunk tree), one on the last joint (a limb tip)."""
    from tests import robots
    lane_family = name not in ("anymal", "atlas")      # (round 6, ABI 9: the one-robot-per-lane kernels take the wrenches too)
    model = {"tree_arm_ff": lambda: robots.tree_arm(True), "tree_arm_flex_ff": lambda: robots.tree_arm_flexible(True),
             "arm7": robots.arm7}[name]() if lane_family else load_builtin(name)
    variant = "lane" if lane_family else "quad"
    B = 8 if name == "anymal" else 4
    rg = np.random.default_rng(21)
    if lane_family:
        st = sample_states(model, B, seed=21, base_height=(0.3, 0.6), grounded_fraction=0.6)
    else:
        st = sample_standing_states(model, B, seed=21) if constrained else sample_states(model, B, seed=21, grounded_fraction=0.5)
    joints = np.array([2 if model.njoints > 2 else 1, model.njoints - 1], dtype=np.int32)
    applied = (rg.normal(0, 40.0, (12, B)), np.array([[0.05, -0.02, 0.03], [0.0, 0.01, -0.04]]), joints)
    copt = TIGHT if constrained else None
    ref, got = alloc_soa(model, B), alloc_soa(model, B)
    for arr in (ref, got):
        if constrained:
            alloc_constraint_state(model, arr, B)
        for k in ("q", "v", "command"):
            arr[k][:] = st[k]
    e = OracleEngine(model)
    if copt is not None:
        e.set_constraint_options(**copt)
        e.bind_constraints(ref["con_flags"], ref["con_data"])
    e.bind_applied(*applied)
    io = oracle_io(ref)
    kw = dict(variant=variant, constraint_options=copt, applied=applied)
    e.batch_run("start", io)
    emu.run(model, got, "start", **kw)
    for k in OUTS:
        assert rel_err(got[k], ref[k]) < 1e-10, ("start", k)
    # RobotState::fExternal of the two parent joints carries the wrenches (joint frame)
    fe = ref["f_external"].reshape(model.njoints, 6, B)
    assert np.abs(fe[joints[0]]).max() > 1.0 and np.abs(fe[model.njoints - 1]).max() > 1.0
    for solver in ("runge_kutta_4", "euler_explicit"):
        e.batch_run("step", io, solver=solver, dt=5e-4, n_substeps=2, command_changed=True)
        emu.run(model, got, "step", solver=solver, dt=5e-4, n_substeps=2, command_changed=True, **kw)
        ok = (ref["status"][0] & 1) == 0
        for k in OUTS:
            assert rel_err(got[k], ref[k], ok) < 1e-8, (solver, k)
    # not a no-op, and not the same as the wrenches on the root body
    plain = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, plain, B)
    for k in ("q", "v", "command"):
        plain[k][:] = st[k]
    emu.run(model, plain, "start", variant=variant, constraint_options=copt, applied=applied[:2])
    assert rel_err(plain["a"], ref["a"]) > 1e-3


@pytest.mark.parametrize("constrained", [False, True])
def test_per_lane_ground_patches_on_the_host(constrained):
    """JM_F_GROUND_OFFSET: every lane samples the height map at its own (x, y) offset.  The kernel sources against the
    oracle, and the law that defines the feature: a lane with offset (ox, oy) behaves exactly like a lane WITHOUT offset
    whose robot stands at (x + ox, y + oy) on the same map."""
    model = load_builtin("anymal")
    B = 12
    st, _, ground, _ = _scene(model, B, 13, constrained)
    rg = np.random.default_rng(3)
    off = np.ascontiguousarray(rg.uniform(-0.6, 0.6, (2, B)))
    copt = TIGHT if constrained else None
    arrs = [alloc_soa(model, B) for _ in range(3)]   # oracle with offsets | emulation with offsets | emulation, robots moved
    for arr in arrs:
        if constrained:
            alloc_constraint_state(model, arr, B)
        for k in ("q", "v", "command"):
            arr[k][:] = st[k]
    ref, got, moved = arrs
    moved["q"][0:2] += off
    got["ground_offset"] = off
    e = OracleEngine(model)
    if copt is not None:
        e.set_constraint_options(**copt)
        e.bind_constraints(ref["con_flags"], ref["con_data"])
    e.bind_ground(*ground)
    e.bind_ground_offset(off)
    io = oracle_io(ref)
    kw = dict(variant="quad", constraint_options=copt, ground=ground)
    e.batch_run("start", io)
    emu.run(model, got, "start", **kw)
    emu.run(model, moved, "start", **kw)
    a_start = got["a"].copy()
    for _ in range(3):
        e.batch_run("step", io, solver="runge_kutta_4", dt=5e-4, n_substeps=1, command_changed=True)
        emu.run(model, got, "step", solver="runge_kutta_4", dt=5e-4, n_substeps=1, command_changed=True, **kw)
        emu.run(model, moved, "step", solver="runge_kutta_4", dt=5e-4, n_substeps=1, command_changed=True, **kw)
    ok = (ref["status"][0] & 1) == 0
    assert ok.sum() >= B - 1 and (np.abs(ref["contact_forces"]).sum(axis=0) > 0).sum() >= 2
    for k in OUTS:
        assert rel_err(got[k], ref[k], ok) < 1e-8, k
    back = moved["q"].copy()
    back[0:2] -= off
    assert rel_err(back, got["q"], ok) < 1e-12
    for k in ("v", "a", "contact_forces", "u"):
        assert rel_err(moved[k], got[k], ok) < 1e-9, k
    # ... and the offsets matter: the same lanes without them see another ground
    plain = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, plain, B)
    for k in ("q", "v", "command"):
        plain[k][:] = st[k]
    emu.run(model, plain, "start", **kw)
    assert rel_err(plain["a"], a_start) > 1e-6


def test_per_lane_friction_with_the_spring_damper_law_on_the_host():
    """`contacts.friction` per environment (envs/locomotion.py:257-262 randomises it whatever the contact model): the
    spring-damper law of the variation kernels reads the lane's own coefficient; sliding robots, kernel sources on the
    host against the oracle, and the tangential force scales with the lane's coefficient."""
    model = load_builtin("anymal")
    B = 16
    st = sample_states(model, B, seed=31, grounded_fraction=1.0)
    st["v"][:2] += 0.5         # sliding: the friction force is saturated at mu * fN
    mu = np.linspace(0.1, 1.6, B)
    ref, got = alloc_soa(model, B), alloc_soa(model, B)
    for arr in (ref, got):
        for k in ("q", "v", "command"):
            arr[k][:] = st[k]
        arr["friction"] = mu.copy()
    oracle_batch(model, ref, "start")
    emu.run(model, got, "start", variant="quad")
    for _ in range(3):
        kw = dict(solver="runge_kutta_4", dt=2.5e-4, n_substeps=1, command_changed=False)
        oracle_batch(model, ref, "step", **kw)
        emu.run(model, got, "step", variant="quad", **kw)
    ok = (ref["status"][0] & 1) == 0
    for k in ("q", "v", "a", "contact_forces", "f_external"):
        assert rel_err(got[k], ref[k], ok) < 1e-9, k
    # a lane of the per-lane run is the batch-wide option set to that lane's coefficient
    from oracle.oracle_py import OracleEngine
    touching = np.flatnonzero(np.abs(ref["contact_forces"]).sum(0) > 0)
    assert len(touching) >= 3
    for l0 in (touching[0], touching[-1]):
        other = touching[1]
        one = alloc_soa(model, B)
        for k in ("q", "v", "command"):
            one[k][:] = st[k]
        e = OracleEngine(model, friction=float(mu[l0]))
        e.batch_run("start", oracle_io(one))
        for _ in range(3):
            e.batch_run("step", oracle_io(one), solver="runge_kutta_4", dt=2.5e-4, n_substeps=1, command_changed=False)
        assert np.array_equal(one["a"][:, l0], ref["a"][:, l0]) and not np.array_equal(one["a"][:, other], ref["a"][:, other])


def test_oracle_ground_profile_laws():
    """A point mass dropped on an inclined plane z = s x feels a normal force along the plane's normal and rests
    at depth m g n_z / k along it (first-order projection, engine.cc:3138-3145); outside the grid the ground
    continues flat."""
    from tests import robots
    model = robots.point_mass()
    e = OracleEngine(model)
    slope = 0.2
    xs = np.arange(5) * 1.0 - 2.0
    heights = np.tile(slope * xs[None, :], (4, 1))
    e.bind_ground(heights, -2.0, -1.5, 1.0, 1.0)
    q = model.neutral()
    q[0], q[2] = 0.3, slope * 0.3 - 1e-4        # 0.1 mm below the plane
    e.start(q, np.zeros(model.nv))
    f = e.get("contact_forces")[:3]              # contact frame = world aligned for an upright point mass
    n = np.array([-slope, 0.0, 1.0]) / math.hypot(slope, 1.0)
    assert np.linalg.norm(f) > 0 and np.allclose(f / np.linalg.norm(f), n, atol=1e-9)
    # normal force magnitude k * depth with depth = dz * n_z, times the tanh blend of the reference's law
    depth = 1e-4 * n[2]
    assert np.linalg.norm(f) == pytest.approx(1.0e6 * depth * math.tanh(2.0 * depth / 1.0e-3), rel=1e-9)
    q[0] = 50.0                                  # far outside the grid: height of the last sample, zero slope
    q[2] = slope * 2.0 - 1e-4
    e.start(q, np.zeros(model.nv))
    f = e.get("contact_forces")[:3]
    assert abs(f[0]) < 1e-12 and f[2] > 0


def test_model_bias_sampler_follows_the_reference_laws():
    """`addBiasedToExtendedModel` (model.cc:1166-1236): multiplicative N(1, std) biases, mass floor, inertia biased
    through its principal axes / moments (stays positive definite), translations only for the relative position."""
    import torch
    m = load_builtin("anymal")
    B = 8192
    opts = {"massBodiesBiasStd": 0.1, "inertiaBodiesBiasStd": 0.05, "centerOfMassPositionBodiesBiasStd": 0.05,
            "relativePositionBodiesBiasStd": 0.02}
    ml = sample_model_lane(m, B, opts, torch.Generator().manual_seed(1)).view(m.njoints, 13, B)
    nom = nominal_model_lane(m, B).view(m.njoints, 13, B)
    j = 3
    r = ml[j, 0] / nom[j, 0]
    assert float(r.mean()) == pytest.approx(1.0, abs=5e-3) and float(r.std()) == pytest.approx(0.1, rel=5e-2)
    rc = ml[j, 1:4] / nom[j, 1:4]
    assert float(rc.std()) == pytest.approx(0.05, rel=5e-2)
    rp = ml[j, 10:13][nom[j, 10:13].abs() > 1e-9] / nom[j, 10:13][nom[j, 10:13].abs() > 1e-9]
    assert float(rp.std()) == pytest.approx(0.02, rel=1e-1)
    I = ml[j, 4:10]
    M = torch.stack([torch.stack([I[0], I[1], I[2]]), torch.stack([I[1], I[3], I[4]]), torch.stack([I[2], I[4], I[5]])]).permute(2, 0, 1)
    ev = torch.linalg.eigvalsh(M)
    ev0 = torch.linalg.eigvalsh(torch.as_tensor(m.inertia[j]))
    assert float(ev.min()) > 0.0
    assert torch.allclose(ev.mean(0), ev0, rtol=5e-2)
    # nothing drawn when every option is zero; only the masked lanes change on an episode-wise re-draw
    same = sample_model_lane(m, 16, {k: 0.0 for k in opts}, torch.Generator().manual_seed(2))
    assert torch.equal(same, nominal_model_lane(m, 16))
    mask = torch.zeros(B, dtype=torch.bool)
    mask[::2] = True
    again = sample_model_lane(m, B, opts, torch.Generator().manual_seed(3), lane_mask=mask, previous=ml.view(-1, B))
    assert torch.equal(again[:, ~mask], ml.view(-1, B)[:, ~mask]) and not torch.equal(again[:, mask], ml.view(-1, B)[:, mask])
    # a tiny mass keeps its floor: max(m * N(1, std), min(m, 1 g))
    light = load_builtin("anymal")
    light.mass[4] = 5.0e-4
    lm = sample_model_lane(light, 4096, {"massBodiesBiasStd": 0.5}, torch.Generator().manual_seed(4)).view(light.njoints, 13, -1)
    assert float(lm[4, 0].min()) >= 5.0e-4


def test_force_breakpoints_cut_the_launches():
    """Impulse starts / ends are breakpoints of `Engine::step` (engine.cc:1985-2016)."""
    o = default_options()
    o["stepper"].update({"controllerUpdatePeriod": 0.01, "sensorsUpdatePeriod": 0.01, "dtMax": 1e-3})
    iv, t_end, _ = _breakpoint_intervals(0.0, 0.0, 0.02, o, (0.0123, 0.0173))
    ends = [round(x[0], 10) for x in iv]
    assert ends == [0.01, 0.0123, 0.0173, 0.02]
    iv, _, _ = _breakpoint_intervals(0.0, 0.0, 0.02, o, ())
    assert [round(x[0], 10) for x in iv] == [0.01, 0.02]


# ------------------------------------------------------------------ device build
@pytest.mark.gpu
@pytest.mark.parametrize("name,constrained", [("anymal", False), ("anymal", True), ("atlas", False), ("atlas", True),
                                              ("biped_torso", False), ("biped_torso", True), ("hydra", False), ("hydra", True)])
def test_gpu_variation_matches_oracle(gpu_device, name, constrained):
    import torch

    from jiminy_amd.engine import BatchedEngine
    model = _model(name)
    B, dt = (96, 5e-4) if name == "anymal" else (24, 2.5e-4)
    st, ml, ground, applied = _scene(model, B, 9, constrained)
    copt = TIGHT if constrained else None
    if name == "hydra":
        from tests.test_lane_failures import _Q, _assert_forms
        gen = dict(_Q, model_lane=1, ground=1, applied=1, constraint=int(constrained))
        _assert_forms(gpu_device, "hydra", B, [(dict(gen, mode="start"), "QCON_GEN_INIT" if constrained else "QUAD_GEN"),
                                               (dict(gen, mode="step"), "QCON_GEN" if constrained else "QUAD_GEN")])
    ref = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, ref, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    e = _oracle(model, ref, ml, ground, applied, copt)
    io = oracle_io(ref)
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device,
                        extra_outputs=("contact_forces", "f_external", "joint_forces", "energy", "centroidal"))
    stepper = {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt}
    if constrained:
        stepper.update({"tolAbs": TIGHT["tol_abs"], "tolRel": TIGHT["tol_rel"]})
    eng.set_options({"stepper": stepper, "contacts": {"model": "constraint" if constrained else "spring_damper"}})
    eng.set_lane_model(torch.from_numpy(ml))
    if ground is not None:
        eng.set_ground_heightmap(*ground)
    # the two wrenches as profile forces on two frames of the root body (held values)
    frames = [n for n, f in model.frames.items() if f.parent_joint == 1][:2]
    offsets = np.array([model.frame(n).p for n in frames])
    applied = (applied[0], offsets)
    e.bind_applied(*applied)
    for i, n in enumerate(frames):
        w = torch.from_numpy(applied[0][6 * i:6 * i + 6].copy()).to(gpu_device)
        eng.register_profile_force(n, lambda t, q, v, w=w: w)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
    loop = ReferenceFixedStepLoop(dt)   # the reference's sub-step rule: opens with a 1 us step (engine.cc:1176)
    for k in OUTS:
        assert rel_err(eng.field(k).cpu().numpy(), ref[k]) < (1e-7 if constrained else 1e-10), ("start", k)
    ok = np.ones(B, dtype=bool)
    for _ in range(4):
        eng.step(dt)
        # (continuous profile forces -- update period 0 -- are re-evaluated at the start of EVERY integrator step and a(t+)
        # is recomputed with them, `BatchedEngine.step`: with the constraint model that refresh re-runs the warm-started
        # solve, so the oracle refreshes at every sub-step too, the opening microsecond step included)
        loop.advance(lambda h, first: e.batch_run("step", io, solver="runge_kutta_4", dt=h, n_substeps=1, command_changed=constrained), dt, constrained)
        # lanes that blow up numerically (light biased shanks landing on a bump: explicit RK4 on the stiff ground,
        # DESIGN.md section 5) leave the comparison, as in the teacher-forced test of test_gpu_parity.py
        ok &= ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2) & (np.abs(ref["a"]).max(axis=0) < 1e6)
    assert ok.sum() > 0.8 * B
    errs = {k: rel_err(eng.field(k).cpu().numpy(), ref[k], ok) for k in OUTS}
    print("variation on the device:", {k: float("%.1e" % v) for k, v in errs.items()})
    for k in OUTS:
        # (observed on the MI355X: <= 1.1e-13 with the constraint model, PGS tolerances 1e-11 -- the solves converge
        # to the same fixed point; the bar leaves room for one more PGS sweep on either side)
        assert errs[k] < (1e-9 if constrained else 1e-8), (k, errs)
    assert (np.abs(ref["contact_forces"]).sum(axis=0) > 0).sum() > B // 8


@pytest.mark.gpu
@pytest.mark.parametrize("name,constrained", [("anymal", False), ("anymal", True), ("atlas", False),
                                              ("tree_arm_ff", False), ("tree_arm_ff", True), ("tree_arm_flex_ff", False)])
def test_gpu_applied_forces_on_frames_of_any_joint(gpu_device, name, constrained):
    """`register_profile_force` on a frame of a limb and on a frame of the first joint after the root (engine.cc:1895-1935 accepts
    any frame): device against the oracle, through the engine's API."""
    import torch

    from jiminy_amd.engine import BatchedEngine
    from tests import robots
    lane_family = name not in ("anymal", "atlas")      # (round 6, ABI 9: the one-robot-per-lane kernels take the wrenches too)
    model = {"tree_arm_ff": lambda: robots.tree_arm(True),
             "tree_arm_flex_ff": lambda: robots.tree_arm_flexible(True)}[name]() if lane_family else load_builtin(name)
    B, dt = (64, 5e-4) if name == "anymal" else (24, 2.5e-4)
    rg = np.random.default_rng(22)
    if lane_family:
        st = sample_states(model, B, seed=22, base_height=(0.3, 0.6), grounded_fraction=0.6)
    else:
        st = sample_standing_states(model, B, seed=22) if constrained else sample_states(model, B, seed=22, grounded_fraction=0.5)
    frames = [next(n for n, f in model.frames.items() if f.parent_joint == j) for j in (2, model.njoints - 1)]
    joints = np.array([model.frame(n).parent_joint for n in frames], dtype=np.int32)
    offsets = np.array([model.frame(n).p for n in frames])
    wrenches = rg.normal(0, 40.0, (12, B))
    copt = TIGHT if constrained else None
    ref = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, ref, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    e = OracleEngine(model)
    if copt is not None:
        e.set_constraint_options(**copt)
        e.bind_constraints(ref["con_flags"], ref["con_data"])
    e.bind_applied(wrenches, offsets, joints)
    io = oracle_io(ref)
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device,
                        extra_outputs=("contact_forces", "f_external", "joint_forces", "energy", "centroidal"))
    stepper = {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt}
    if constrained:
        stepper.update({"tolAbs": TIGHT["tol_abs"], "tolRel": TIGHT["tol_rel"]})
    eng.set_options({"stepper": stepper, "contacts": {"model": "constraint" if constrained else "spring_damper"}})
    for i, n in enumerate(frames):
        w = torch.from_numpy(wrenches[6 * i:6 * i + 6].copy()).to(gpu_device)
        eng.register_profile_force(n, lambda t, q, v, w=w: w, update_period=1.0)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
    loop = ReferenceFixedStepLoop(dt)   # the reference's sub-step rule: opens with a 1 us step (engine.cc:1176)
    for k in OUTS:
        assert rel_err(eng.field(k).cpu().numpy(), ref[k]) < (1e-7 if constrained else 1e-10), ("start", k)
    ok = np.ones(B, dtype=bool)
    for _ in range(3):
        eng.step(dt)
        loop.advance(lambda h, first: e.batch_run("step", io, solver="runge_kutta_4", dt=h, n_substeps=1, command_changed=first), dt, constrained)
        ok &= ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2) & (np.abs(ref["a"]).max(axis=0) < 1e6)
    assert ok.sum() > 0.8 * B
    for k in OUTS:
        # (constraint model: the PGS fixed point at tolerance 1e-11 carries the round-off of the two builds, see
        # test_gpu_variation_matches_oracle)
        assert rel_err(eng.field(k).cpu().numpy(), ref[k], ok) < (1e-7 if constrained else 1e-8), k
    fe = ref["f_external"].reshape(model.njoints, 6, B)
    assert np.abs(fe[2]).max() > 1.0 and np.abs(fe[model.njoints - 1]).max() > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name,constrained", [("anymal", False), ("anymal", True), ("atlas", True)])
def test_gpu_per_lane_ground_patches(gpu_device, name, constrained):
    """`BatchedEngine.set_ground_offsets` (JM_F_GROUND_OFFSET) on the device against the oracle."""
    import torch

    from jiminy_amd.engine import BatchedEngine
    model = load_builtin(name)
    B, dt = (64, 5e-4) if name == "anymal" else (16, 2.5e-4)
    st, _, ground, _ = _scene(model, B, 17, constrained)
    off = np.ascontiguousarray(np.random.default_rng(4).uniform(-0.6, 0.6, (2, B)))
    copt = TIGHT if constrained else None
    ref = alloc_soa(model, B)
    if constrained:
        alloc_constraint_state(model, ref, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    e = OracleEngine(model)
    if copt is not None:
        e.set_constraint_options(**copt)
        e.bind_constraints(ref["con_flags"], ref["con_data"])
    e.bind_ground(*ground)
    e.bind_ground_offset(off)
    io = oracle_io(ref)
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device, extra_outputs=("contact_forces", "f_external", "energy"))
    stepper = {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt}
    if constrained:
        stepper.update({"tolAbs": TIGHT["tol_abs"], "tolRel": TIGHT["tol_rel"]})
    eng.set_options({"stepper": stepper, "contacts": {"model": "constraint" if constrained else "spring_damper"}})
    eng.set_ground_heightmap(*ground)
    eng.set_ground_offsets(torch.from_numpy(off.T.copy()))   # (B, 2)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
    loop = ReferenceFixedStepLoop(dt)   # the reference's sub-step rule: opens with a 1 us step (engine.cc:1176)
    ok = np.ones(B, dtype=bool)
    for _ in range(3):
        eng.step(dt)
        loop.advance(lambda h, first: e.batch_run("step", io, solver="runge_kutta_4", dt=h, n_substeps=1, command_changed=first), dt, constrained)
        ok &= ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2) & (np.abs(ref["a"]).max(axis=0) < 1e6)
    assert ok.sum() > 0.8 * B and (np.abs(ref["contact_forces"]).sum(axis=0) > 0).sum() >= B // 16
    for k in OUTS:
        if k in eng._fields and ref[k].size:
            assert rel_err(eng.field(k).cpu().numpy(), ref[k], ok) < 1e-8, k
    # the same engine without offsets sees another ground
    eng.stop()
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    a_off = eng.field("a").clone()
    eng.stop()
    eng.set_ground_offsets(None)
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    assert rel_err(eng.field("a").cpu().numpy(), a_off.cpu().numpy()) > 1e-6


@pytest.mark.gpu
def test_gpu_per_lane_friction_with_the_spring_damper_law(gpu_device):
    import torch

    from jiminy_amd.engine import BatchedEngine
    model = load_builtin("anymal")
    B, dt = 128, 2.5e-4
    st = sample_states(model, B, seed=32, grounded_fraction=1.0)
    st["v"][:2] += 0.5
    mu = np.linspace(0.1, 1.6, B)
    ref = alloc_soa(model, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    ref["friction"] = mu.copy()
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device, extra_outputs=("contact_forces", "f_external"))
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt},
                     "contacts": {"model": "spring_damper"}})
    eng.set_lane_friction(mu)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    oracle_batch(model, ref, "start")
    loop = ReferenceFixedStepLoop(dt)   # the reference's sub-step rule: opens with a 1 us step (engine.cc:1176)
    for _ in range(4):
        eng.step(dt)
        oracle_engine_step(model, ref, loop, dt, "runge_kutta_4", command_changed=False)
    ok = (ref["status"][0] & 1) == 0
    for k in ("q", "v", "a", "contact_forces", "f_external"):
        assert rel_err(eng.field(k).cpu().numpy(), ref[k], ok) < 1e-8, k
    # back to the batch-wide option
    eng.stop()
    eng.set_lane_friction(None)
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    plain = alloc_soa(model, B)
    for k in ("q", "v", "command"):
        plain[k][:] = st[k]
    oracle_batch(model, plain, "start")
    assert rel_err(eng.field("a").cpu().numpy(), plain["a"]) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["runge_kutta_4", "runge_kutta_dopri"])
def test_gpu_per_lane_friction_and_flexibility_on_the_one_robot_per_lane_kernels(gpu_device, solver):
    """The per-environment rows of the lane family (ABI 9): ground friction of every lane under the spring-damper law and the
    stiffness / damping of the flexibility joints of every lane (`WalkerJiminyEnv._setup`, envs/locomotion.py:257-262,
    288-296), fixed-step and adaptive (whose compact launches find the rows through `BatchArgs::lane_map`), against the
    oracle's one-robot engine with the lane's own values."""
    import torch

    from jiminy_amd.engine import BatchedEngine
    from tests import robots
    model = robots.tree_arm_flexible(True)
    B, dt = 48, 5e-4
    rng = np.random.default_rng(8)
    st = sample_states(model, B, seed=21, base_height=(0.3, 0.6), grounded_fraction=0.7)
    flex = model.flexibility_joint_indices
    k = np.stack([model.flex_stiffness[j][:, None] * rng.uniform(0.5, 1.5, (1, B)) for j in flex])
    d = np.stack([model.flex_damping[j][:, None] * rng.uniform(0.5, 1.5, (1, B)) for j in flex])
    mu = 10.0 ** rng.uniform(-0.7, 0.3, B)
    ref = alloc_soa(model, B)
    for key in ("q", "v", "command"):
        ref[key][:] = st[key]
    ref["friction"] = mu.copy()
    ref["flexibility"] = np.ascontiguousarray(np.concatenate([np.concatenate([k[i], d[i]]) for i in range(len(flex))]))
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device, extra_outputs=("contact_forces", "f_external"))
    eng.set_options({"stepper": {"odeSolver": solver, "dtMax": 0.02 if solver == "runge_kutta_dopri" else dt,
                                 "controllerUpdatePeriod": 2e-3 if solver == "runge_kutta_dopri" else dt,
                                 "sensorsUpdatePeriod": 2e-3 if solver == "runge_kutta_dopri" else dt},
                     "contacts": {"model": "spring_damper"}})
    eng.set_lane_friction(mu)
    eng.set_lane_flexibility(k, d)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    oracle_batch(model, ref, "start")
    assert rel_err(eng.field("a").cpu().numpy(), ref["a"]) < 1e-9
    plain = alloc_soa(model, B)
    for key in ("q", "v", "command"):
        plain[key][:] = st[key]
    oracle_batch(model, plain, "start")
    assert rel_err(plain["a"], ref["a"]) > 1e-3          # the rows matter on this batch
    if solver == "runge_kutta_4":
        loop = ReferenceFixedStepLoop(dt)
        for _ in range(6):
            eng.step(dt)
            oracle_engine_step(model, ref, loop, dt, "runge_kutta_4", command_changed=False)
        tol = 1e-8
    else:
        from jiminy_amd.engine import plan_breakpoints
        from oracle.oracle_py import OracleEngine, adaptive_state
        from tests.helpers import oracle_io
        orc = OracleEngine(model)
        orc.bind_friction(ref["friction"])
        orc.bind_flexibility(ref["flexibility"])
        io = oracle_io(ref)
        ad = adaptive_state(B)
        o = eng.get_options()["stepper"]
        t, t_err = 0.0, 0.0
        for _ in range(3):
            intervals, t_end, t_err = plan_breakpoints(t, t_err, 2e-3, eng.get_options())
            for i, (t_next, cmd, sens) in enumerate(intervals):
                orc.batch_run_dopri(io, ad, t_next, tol_rel=o["tolRel"], tol_abs=o["tolAbs"], dt_max=o["dtMax"],
                                    new_step=(i == 0), command_changed=False, update_sensors=sens)
            t = t_end
            eng.step(2e-3)
        # (accept / reject decisions are discontinuous in the error estimate: lanes that follow the oracle's step sequence)
        ss = eng.stepper_state
        same = (ss.iter_lanes.cpu().numpy() == ad["iter"]) & (ss.iter_failed_lanes.cpu().numpy() == ad["iter_failed"])
        assert same.mean() > 0.8
        ref["status"][0][~same] |= 1
        tol = 1e-7
    ok = (ref["status"][0] & 1) == 0
    assert ok.sum() > B // 2
    for key in ("q", "v", "a", "contact_forces", "f_external"):
        assert rel_err(eng.field(key).cpu().numpy(), ref[key], ok) < tol, key
    # back to the model's own values
    eng.stop()
    eng.set_lane_friction(None)
    eng.set_lane_flexibility(None)
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    assert rel_err(eng.field("a").cpu().numpy(), plain["a"]) < 1e-9
    with pytest.raises(LookupError):
        BatchedEngine(load_builtin("cartpole"), 4, dtype=torch.float64, device=gpu_device).set_lane_flexibility(np.ones((1, 3)), np.ones((1, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["persistent", "per_stage"])
def test_gpu_per_lane_friction_with_the_adaptive_stepper(gpu_device, monkeypatch, form):
    """Per-lane friction as the ONLY per-lane input, spring-damper law, `runge_kutta_dopri`: the persistent kernel must
    be the variation one (`k_quad_dopri_gen` -- the plain kernel never reads the friction field and would silently use
    the batch-wide coefficient).  Against the oracle's adaptive loop on sliding robots."""
    import torch

    from jiminy_amd.engine import BatchedEngine
    from oracle.oracle_py import OracleEngine, adaptive_state
    model = load_builtin("anymal")
    monkeypatch.setenv("JIMINY_AMD_ADAPTIVE_FORM", "1" if form == "per_stage" else "0")
    B, T = 32, 2e-3
    st = sample_states(model, B, seed=32, grounded_fraction=1.0)
    st["v"][:2] += 0.5
    mu = np.linspace(0.1, 1.6, B)
    ref = alloc_soa(model, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    ref["friction"] = mu.copy()
    tol = dict(tolAbs=1e-8, tolRel=1e-8)
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device, extra_outputs=("contact_forces",))
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_dopri", "controllerUpdatePeriod": T, "sensorsUpdatePeriod": T, **tol},
                     "contacts": {"model": "spring_damper"}})
    eng.set_lane_friction(mu)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    orc = OracleEngine(model)
    orc.bind_friction(ref["friction"])
    from tests.helpers import oracle_io
    orc.batch_run("start", oracle_io(ref))
    ad = adaptive_state(B)
    for i in range(3):
        eng.step(T)
        orc.batch_run_dopri(ref, ad, (i + 1) * T, tol_rel=1e-8, tol_abs=1e-8, new_step=True, command_changed=(i == 0))
    ok = (ref["status"][0] == 0) & (eng.status.cpu().numpy() == 0)
    assert ok.sum() >= B // 2
    for k in ("q", "v"):
        assert rel_err(eng.field(k).cpu().numpy(), ref[k], ok) < 1e-6, k
    # the coefficient matters: the same run with the batch-wide friction differs
    eng.stop()
    eng.set_lane_friction(None)
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    for i in range(3):
        eng.step(T)
    assert rel_err(eng.field("v").cpu().numpy(), ref["v"], ok) > 1e-4


@pytest.mark.gpu
def test_gpu_impulse_force_schedule_and_model_options(gpu_device):
    """`register_impulse_force` (engine.cc:1838-1893): the wrench acts exactly during [t, t + dt] -- the launches are
    cut at its breakpoints -- and pushes the base; `set_model_options` draws a biased model per lane at `start`."""
    import torch

    from jiminy_amd.engine import BatchedEngine
    model = load_builtin("anymal")
    B, dt = 64, 1e-3
    st = sample_states(model, B, seed=2, base_height=(2.0, 3.0), grounded_fraction=0.0)
    frame = next(n for n, f in model.frames.items() if f.parent_joint == 1)

    def run(push, std):
        eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device, extra_outputs=("f_external",))
        eng.set_options({"stepper": {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": 5 * dt,
                                     "sensorsUpdatePeriod": 5 * dt}, "contacts": {"model": "spring_damper"}})
        if std:
            eng.set_model_options({"dynamics": {"massBodiesBiasStd": std}})
            eng.seed_model(7)
        if push:
            eng.register_impulse_force(frame, 0.0032, 0.0041, np.array([400.0, 0.0, 0.0, 0.0, 0.0, 0.0]))
        eng.set_command(torch.from_numpy(st["command"]))
        eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
        fx = []
        for _ in range(3):
            eng.step(5 * dt)
            fx.append(float(eng.field("f_external")[6:9].abs().max()))
        return eng.field("v").clone(), fx, eng
    v0, fx0, _ = run(False, 0.0)
    v1, fx1, eng = run(True, 0.0)
    assert max(fx0) == 0.0
    assert fx1[0] > 0.0 and fx1[1] == 0.0 and fx1[2] == 0.0     # active at t = 5 ms (inside [3.2, 7.3] ms), over by 10 ms
    # impulse = F dt on a ~50 kg robot: the base gained about 400 * 0.0041 / 52 m/s along the push
    dv = (v1 - v0)[0:3].norm(dim=0)
    assert float(dv.median()) == pytest.approx(400.0 * 0.0041 / 52.1, rel=0.2)
    assert eng.impulse_forces[0]["frame_name"] == frame
    v2, _, eng2 = run(False, 0.1)
    ml = eng2.field("model_lane").view(model.njoints, 13, B)
    assert float((ml[2, 0] / model.mass[2]).std()) == pytest.approx(0.1, rel=0.5)
    assert float((ml[1, 0] / model.mass[1]).std()) == 0.0     # the free-flyer root is not a mechanical joint (model.cc:337-341)
    assert not torch.equal(v2, v0)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["persistent", "per_stage"])
def test_gpu_adaptive_stepper_with_per_lane_models_and_forces(gpu_device, monkeypatch, form):
    """The persistent adaptive stepper (jm_qdopri.h) keeps every robot in its lane, so per-lane body parameters and
    applied forces work with `runge_kutta_dopri` too (`k_quad_dopri_gen`); the per-stage form (JIMINY_AMD_ADAPTIVE_FORM=1)
    evaluates compact batches of the active lanes, whose per-lane optional inputs are read through the lane map of the
    compaction (`BatchArgs::lane_map`).  Both: (a) with the NOMINAL parameters bound per
    lane it follows the plain adaptive kernel step for step; (b) an impulse force acts during [t, t + dt] exactly --
    its start and end are breakpoints of the adaptive loop -- and changes the base velocity by F dt / m; (c) biased
    masses change the motion."""
    import torch

    from jiminy_amd.engine import BatchedEngine
    from jiminy_amd.randomization import nominal_model_lane
    model = load_builtin("anymal")
    B = 64
    monkeypatch.setenv("JIMINY_AMD_ADAPTIVE_FORM", "1" if form == "per_stage" else "0")
    st = sample_states(model, B, seed=6, base_height=(2.0, 3.0), grounded_fraction=0.0)
    frame = next(n for n, f in model.frames.items() if f.parent_joint == 1)

    def run(nominal=False, push=False, std=0.0):
        eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device, extra_outputs=("f_external",))
        eng.set_options({"stepper": {"odeSolver": "runge_kutta_dopri", "tolAbs": 1e-7, "tolRel": 1e-6, "controllerUpdatePeriod": 5e-3,
                                     "sensorsUpdatePeriod": 5e-3}, "contacts": {"model": "spring_damper"}})
        if nominal:
            eng.set_lane_model(nominal_model_lane(model, B, torch.float64, gpu_device))
        if std:
            eng.set_model_options({"dynamics": {"massBodiesBiasStd": std}})
            eng.seed_model(7)
        if push:
            eng.register_impulse_force(frame, 0.0032, 0.0041, np.array([400.0, 0.0, 0.0, 0.0, 0.0, 0.0]))
        eng.set_command(torch.from_numpy(st["command"]))
        eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
        fx = []
        for _ in range(3):
            eng.step(5e-3)
            fx.append(float(eng.field("f_external")[6:9].abs().max()))
        ss = eng.stepper_state
        assert abs(ss.t - 0.015) < 1e-12 and int(eng.status.abs().sum()) == 0
        return eng.field("q").clone(), eng.field("v").clone(), ss.iter_lanes.clone(), ss.iter_failed_lanes.clone(), fx
    q0, v0, it0, if0, fx0 = run()
    q1, v1, it1, if1, _ = run(nominal=True)
    assert torch.equal(it0, it1) and torch.equal(if0, if1)
    assert float((q1 - q0).abs().max()) < 1e-9 and float((v1 - v0).abs().max()) < 1e-8
    q2, v2, it2, _, fx2 = run(push=True)
    assert max(fx0) == 0.0 and fx2[0] > 0.0 and fx2[1] == 0.0 and fx2[2] == 0.0
    dv = (v2 - v0)[0:3].norm(dim=0)
    assert float(dv.median()) == pytest.approx(400.0 * 0.0041 / 52.1, rel=0.2)
    assert int(it2.min()) >= int(it0.min())       # the two extra breakpoints cost steps
    q3, v3, *_ = run(std=0.1)
    assert not torch.equal(v3, v0)


@pytest.mark.gpu
def test_gpu_per_stage_adaptive_stepper_with_the_constraint_model_and_variation(gpu_device):
    """The reference's two defaults together (`runge_kutta_dopri` + constraint contacts: per-stage launches over compact
    batches) with per-lane friction, body parameters and a terrain patch per lane: (a) nominal parameters / the batch-wide
    friction bound per lane / zero offsets reproduce the plain run step for step; (b) the varied inputs change the motion;
    (c) the lanes' step counts differ, i.e. the compact batches really re-order the lanes."""
    import torch

    from jiminy_amd.engine import BatchedEngine
    from jiminy_amd.randomization import nominal_model_lane
    model = load_builtin("anymal")
    B = 64
    st = sample_standing_states(model, B, seed=8)
    rg = np.random.default_rng(8)
    heights = 0.004 * rg.standard_normal((9, 9))

    def run(vary):
        eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device)
        eng.set_options({"stepper": {"odeSolver": "runge_kutta_dopri", "tolAbs": 1e-7, "tolRel": 1e-6, "controllerUpdatePeriod": 5e-3,
                                     "sensorsUpdatePeriod": 5e-3}, "contacts": {"model": "constraint", "friction": 0.8}})
        eng.set_ground_heightmap(heights, -1.0, -1.0, 0.25, 0.25)
        if vary is not None:
            eng.set_lane_model(nominal_model_lane(model, B, torch.float64, gpu_device))
            eng.set_lane_friction(torch.full((B,), 0.8, dtype=torch.float64) if not vary else torch.linspace(0.2, 1.4, B, dtype=torch.float64))
            eng.set_ground_offsets(torch.zeros(B, 2, dtype=torch.float64) if not vary else torch.from_numpy(rg.uniform(-0.5, 0.5, (B, 2))))
            if vary:
                eng.set_model_options({"dynamics": {"massBodiesBiasStd": 0.1}})
                eng.seed_model(3)
        eng.set_command(torch.from_numpy(st["command"]))
        eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
        for _ in range(3):
            eng.step(5e-3)
        ss = eng.stepper_state
        assert abs(ss.t - 0.015) < 1e-12
        return eng.field("q").clone(), eng.field("v").clone(), ss.iter_lanes.clone()
    q0, v0, it0 = run(None)
    q1, v1, it1 = run(False)
    assert torch.equal(it0, it1) and float((q1 - q0).abs().max()) < 1e-9 and float((v1 - v0).abs().max()) < 1e-7
    q2, v2, it2 = run(True)
    assert float((v2 - v0).abs().max()) > 1e-4
    assert int(it0.max()) > int(it0.min())


@pytest.mark.gpu
def test_gpu_impulse_force_launches_match_the_oracle_step_for_step(gpu_device):
    """The whole force path against the oracle: the engine cuts its launches at the start and the end of an impulse
    force (3.2 ms, 7.3 ms inside 5 ms controller periods), holds the wrench in between and recomputes a(t+) at the
    launch where it changes (`hasDynamicsChanged`, engine.cc:1860-1868, 2031-2042).  The oracle is driven with the
    same schedule (`plan_step` with the force breakpoints), the wrench bound launch by launch and the refresh flag set
    where the wrench changed: state and outputs agree to round-off after every `step`."""
    import torch

    from jiminy_amd.engine import BatchedEngine, plan_step
    model = load_builtin("anymal")
    B, dt = 48, 1e-3
    st = sample_states(model, B, seed=8, base_height=(1.0, 1.5), grounded_fraction=0.0)
    frame = next(n for n, f in model.frames.items() if f.parent_joint == 1)
    push = np.array([300.0, -150.0, 80.0, 5.0, -3.0, 2.0])
    t_on, t_len = 0.0032, 0.0041
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device,
                        extra_outputs=("contact_forces", "f_external", "joint_forces", "energy", "centroidal"))
    options = {"stepper": {"odeSolver": "runge_kutta_4", "dtMax": dt, "controllerUpdatePeriod": 5 * dt, "sensorsUpdatePeriod": 5 * dt},
               "contacts": {"model": "spring_damper"}}
    eng.set_options(options)
    eng.register_impulse_force(frame, t_on, t_len, push)
    eng.set_command(torch.from_numpy(st["command"]))
    ref = alloc_soa(model, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    e = OracleEngine(model)
    io = oracle_io(ref)
    wrench = np.zeros((6, B))
    e.bind_applied(wrench, np.array([model.frame(frame).p]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
    t, t_err, active = 0.0, 0.0, False
    breakpoints = (t_on, t_on + t_len)
    n_refresh = 0
    for k_step in range(3):
        # (the engine's own schedule, opening microsecond step of the simulation included: `substep_sizes`)
        launches, t_end, t_err = plan_step(t, t_err, 5 * dt, eng.get_options(), tuple(b for b in breakpoints if b > t + 1e-10),
                                           dt_first=1e-6 if k_step == 0 else None)
        for h, n, cmd_bp, sens in launches:
            now = t_on - 1e-10 <= t < t_on + t_len - 1e-10
            wrench[:] = push[:, None] if now else 0.0
            changed = now != active
            active = now
            n_refresh += int(changed)
            e.bind_applied(wrench, np.array([model.frame(frame).p]))
            e.batch_run("step", io, solver="runge_kutta_4", dt=h, n_substeps=n, command_changed=changed, update_sensors=sens)
            t += h * n
        t = t_end
        eng.step(5 * dt)
        for k in OUTS:
            assert rel_err(eng.field(k).cpu().numpy(), ref[k]) < 1e-9, (t, k)
    assert n_refresh == 2 and abs(eng.stepper_state.t - 0.015) < 1e-12
    assert float(np.abs(ref["v"][0:3] - st["v"][0:3]).max()) > 1e-3


@pytest.mark.gpu
def test_gpu_adaptive_stepper_with_a_periodic_profile_force_matches_the_oracle(gpu_device):
    """`register_profile_force(..., update_period)` under the adaptive solver: the force is re-evaluated every 2 ms, those
    times are breakpoints of the per-robot step-size loops, a(t+) is recomputed when the held value changes.  The oracle's
    adaptive loop is driven with the same schedule interval by interval; robots that follow the same accept / reject
    sequence (nearly all) agree to the integration tolerance."""
    import torch

    from jiminy_amd.engine import BatchedEngine, plan_breakpoints
    from oracle.oracle_py import adaptive_state
    model = load_builtin("anymal")
    B = 40
    st = sample_states(model, B, seed=9, base_height=(1.0, 1.5), grounded_fraction=0.0)
    frame = next(n for n, f in model.frames.items() if f.parent_joint == 1)
    period = 2e-3

    def wrench_at(t):
        return np.array([80.0 * math.sin(2 * math.pi * t / 0.01), 40.0 * math.cos(2 * math.pi * t / 0.01), 0.0, 0.0, 0.0, 3.0])
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device, extra_outputs=("f_external",))
    eng.set_options({"stepper": {"odeSolver": "runge_kutta_dopri", "tolAbs": 1e-8, "tolRel": 1e-7, "controllerUpdatePeriod": 4e-3,
                                 "sensorsUpdatePeriod": 4e-3}, "contacts": {"model": "spring_damper"}})
    eng.register_profile_force(frame, lambda t, q, v: torch.as_tensor(wrench_at(t), device=gpu_device), update_period=period)
    eng.set_command(torch.from_numpy(st["command"]))
    ref = alloc_soa(model, B)
    for k in ("q", "v", "command"):
        ref[k][:] = st[k]
    e = OracleEngine(model)
    io = oracle_io(ref)
    wrench = np.tile(wrench_at(0.0)[:, None], (1, B))
    e.bind_applied(wrench, np.array([model.frame(frame).p]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
    ad = adaptive_state(B)
    t, t_err, held_t = 0.0, 0.0, 0.0
    for _ in range(3):
        extra = tuple(period * k for k in range(1, 20) if period * k > t + 1e-10)
        intervals, t_end, t_err = plan_breakpoints(t, t_err, 4e-3, eng.get_options(), extra)
        for i, (t_next, cmd_bp, sens) in enumerate(intervals):
            refresh = False
            if t - held_t >= period - 1e-10:            # re-evaluated at this interval's start
                held_t = math.floor(t / period + 1e-9) * period
                wrench[:] = wrench_at(t)[:, None]
                refresh = True
            e.bind_applied(wrench, np.array([model.frame(frame).p]))
            e.batch_run_dopri(io, ad, t_next, tol_rel=1e-7, tol_abs=1e-8, new_step=(i == 0), command_changed=refresh, update_sensors=sens)
            t = t_next
        t = t_end
        eng.step(4e-3)
    ss = eng.stepper_state
    assert abs(ss.t - 0.012) < 1e-12 and int(eng.status.abs().sum()) == 0
    same = (ss.iter_lanes.cpu().numpy() == ad["iter"]) & (ss.iter_failed_lanes.cpu().numpy() == ad["iter_failed"])
    assert same.mean() > 0.8, (ss.iter_lanes.cpu().numpy(), ad["iter"])
    for k in ("q", "v"):
        assert rel_err(eng.field(k).cpu().numpy(), ref[k], same) < 1e-7, k
        assert rel_err(eng.field(k).cpu().numpy(), ref[k]) < 1e-4, k


@pytest.mark.gpu
@pytest.mark.parametrize("name,constrained,solver", [("tree_arm_ff", False, "runge_kutta_4"), ("tree_arm_ff", True, "euler_explicit"),
                                                     ("tree_arm_flex_ff", False, "runge_kutta_4"), ("arm7", False, "runge_kutta_4"),
                                                     ("tree_arm_ff", False, "runge_kutta_dopri")])
def test_gpu_one_robot_per_lane_kernels_with_variation(gpu_device, name, constrained, solver):
    """A biased model per lane (`set_lane_model`, ≙ `Model::addBiasedToExtendedModel` per environment) and a profile force on a
    frame, on robots of the one-robot-per-lane family (`k_batch<..., true>` / `k_constrained<..., true>`): device against the
    oracle through the engine's API; the adaptive solver reads the rows through the compact launches' lane map."""
    import torch

    from jiminy_amd.engine import BatchedEngine, plan_breakpoints
    from oracle.oracle_py import adaptive_state
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
    # (spring-damper law: a bumpy height map, every lane on its own patch of it)
    ground = None if constrained else (0.02 * rg.standard_normal((7, 9)), -1.0, -0.8, 0.25, 0.3)
    offsets = np.ascontiguousarray(rg.uniform(-0.3, 0.3, (2, B)))
    e = _oracle(model, ref, ml, ground, (wrench, np.array([model.frame(frame).p]), np.array([model.njoints - 1], dtype=np.int32)), copt)
    if ground is not None:
        e.bind_ground_offset(offsets)
    io = oracle_io(ref)
    eng = BatchedEngine(model, B, dtype=torch.float64, device=gpu_device,
                        extra_outputs=("contact_forces", "f_external", "joint_forces", "energy", "centroidal"))
    adaptive = solver == "runge_kutta_dopri"
    stepper = {"odeSolver": solver, "dtMax": 0.02 if adaptive else dt, "controllerUpdatePeriod": 2e-3 if adaptive else dt,
               "sensorsUpdatePeriod": 2e-3 if adaptive else dt}
    if constrained:
        stepper.update({"tolAbs": TIGHT["tol_abs"], "tolRel": TIGHT["tol_rel"]})
    eng.set_options({"stepper": stepper, "contacts": {"model": "constraint" if constrained else "spring_damper"}})
    eng.set_lane_model(torch.from_numpy(ml))
    if ground is not None:
        eng.set_ground_heightmap(*ground)
        eng.set_ground_offsets(torch.from_numpy(offsets.T.copy()))   # (B, 2)
    w = torch.from_numpy(wrench.copy()).to(gpu_device)
    eng.register_profile_force(frame, lambda t, q, v, w=w: w, update_period=1.0)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
    for k in OUTS:
        assert rel_err(eng.field(k).cpu().numpy(), ref[k]) < (1e-7 if constrained else 1e-10), ("start", k)
    if adaptive:
        ad = adaptive_state(B)
        o = eng.get_options()["stepper"]
        t, t_err = 0.0, 0.0
        for _ in range(3):
            intervals, t_end, t_err = plan_breakpoints(t, t_err, 2e-3, eng.get_options())
            for i, (t_next, cmd, sens) in enumerate(intervals):
                e.batch_run_dopri(io, ad, t_next, tol_rel=o["tolRel"], tol_abs=o["tolAbs"], dt_max=o["dtMax"],
                                  new_step=(i == 0), command_changed=False, update_sensors=sens)
            t = t_end
            eng.step(2e-3)
        ss = eng.stepper_state
        ok = (ss.iter_lanes.cpu().numpy() == ad["iter"]) & (ss.iter_failed_lanes.cpu().numpy() == ad["iter_failed"])
        assert ok.mean() > 0.8
        ok &= ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2)
        tol = 1e-7
    else:
        loop = ReferenceFixedStepLoop(dt)
        ok = np.ones(B, dtype=bool)
        for _ in range(3):
            eng.step(dt)
            loop.advance(lambda h, first: e.batch_run("step", io, solver=solver, dt=h, n_substeps=1, command_changed=first), dt, constrained)
            ok &= ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2)
        tol = 1e-7 if constrained else 1e-8
    assert ok.sum() > 0.5 * B
    for k in ("q", "v", "a", "contact_forces", "f_external"):
        assert rel_err(eng.field(k).cpu().numpy(), ref[k], ok) < tol, k
