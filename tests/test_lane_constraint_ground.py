"""Constraint contacts on a height-map ground for the one-robot-per-lane kernels (`k_constrained<double, Topo, true>`,
jm_constraint.h): the contact rows live in the local frame of the surface under every contact point, rotationLocal =
[t0 t1 n] from the ground normal (FrameConstraint::setNormal, frame_constraint.cc:62-68), with the first-order depth
(z - h) n_z (engine.cc:3133-3193).  Layers: the kernel sources on the host against the oracle, the oracle on the incline's
known answers, and (`-m gpu`) the device build through BatchedEngine against the oracle, against laws that need no oracle
(tilted ground = tilted gravity, the incline, a zero map = flat ground) and through the walker environment."""
import math

import numpy as np
import pytest

from jiminy_amd import _abi, codegen
from jiminy_amd.synthetic import joint_world_placements, sample_standing_states, sample_states
from oracle.oracle_py import OracleEngine
from tests.helpers import ReferenceFixedStepLoop, alloc_constraint_state, alloc_soa, oracle_io, rel_err

TIGHT = dict(tol_abs=1e-11, tol_rel=1e-10)
OUTS = ("q", "v", "a", "con_data", "u", "contact_forces", "f_external", "imu", "force", "contact")
BIAS = {"massBodiesBiasStd": 0.1, "inertiaBodiesBiasStd": 0.1, "centerOfMassPositionBodiesBiasStd": 0.05,
        "relativePositionBodiesBiasStd": 0.02}


def _robot(name):
    from tests import robots
    m = {"tree_arm_ff": lambda: robots.tree_arm(True), "tree_arm_flex_ff": lambda: robots.tree_arm_flexible(True),
         "anymal_held": robots.anymal_held, "point_mass": robots.point_mass}[name]()
    assert codegen.quad_structure(m) is None   # the one-robot-per-lane family
    return m


def _bumpy(seed):
    """The map shape of test_variation._scene under the constraint model."""
    rg = np.random.default_rng(seed)
    return (0.25 * 0.02 * rg.standard_normal((7, 9)), -1.0, -0.8, 0.25, 0.3)


def _setup(name, B, seed):
    """Model, states, constraint options, the SoA arrays (user constraints of anymal_held held on half of the lanes: the base
    frame on the even lanes, the rod on the odd ones), per-lane patch offsets, the held lanes."""
    model = _robot(name)
    rg = np.random.default_rng(seed)
    if name == "anymal_held":
        st = sample_standing_states(model, B, seed=seed)
        copt = dict(TIGHT, regularization=1e-3, user_stabilization_freq=10.0)
    else:
        st = sample_states(model, B, seed=seed, base_height=(0.3, 0.6), grounded_fraction=0.6)
        copt = dict(TIGHT)
    arr = alloc_soa(model, B)
    alloc_constraint_state(model, arr, B)
    held = np.arange(B) % 2 == 0
    if name == "anymal_held":
        rows = _abi.constraint_rows(model)
        f0 = rows["n_bounds"] + rows["n_contacts"]
        arr["con_flags"][f0, held] = 1
        arr["con_flags"][f0 + 1, ~held] = 1
    for k in ("q", "v", "command"):
        arr[k][:] = st[k]
    off = np.ascontiguousarray(rg.uniform(-0.3, 0.3, (2, B)))
    return model, st, copt, arr, off, held


def _oracle(model, arr, copt, ground, off, ml=None, **options):
    e = OracleEngine(model, **options)
    e.set_constraint_options(**copt)
    e.bind_constraints(arr["con_flags"], arr["con_data"])
    if ml is not None:
        e.bind_model_lane(ml)
    if ground is not None:
        e.bind_ground(*ground)
        if off is not None:
            e.bind_ground_offset(off)
    return e


def _sane(ref):
    # (a robot dropped deep into a bump leaves at huge speeds on both sides: not a comparison)
    return ((ref["status"][0] & 1) == 0) & (np.abs(ref["v"]).max(axis=0) < 1e2) & (np.abs(ref["a"]).max(axis=0) < 1e6)


def _contacts_active(model, arr):
    nb = _abi.constraint_rows(model)["n_bounds"]
    return int((arr["con_flags"][nb:nb + len(model.contacts)] & 1).sum())


# ---------------------------------------------------------------- host emulation of the kernel code

@pytest.mark.parametrize("name", ["tree_arm_ff", "anymal_held"])
def test_lane_constraint_kernel_on_a_height_map_matches_oracle_on_the_host(name):
    """The variation instantiation's code (jm_constraint.h) on the host, on a bumpy map with a patch per lane: switching,
    delassus rows, right-hand side and forces in the local frame of the surface, against the oracle's one-robot engine."""
    from tests.hostemu import lane_ground
    B = 8
    model, st, copt, ref, off, _ = _setup(name, B, 23)
    ground = _bumpy(23)
    got = {k: v.copy() for k, v in ref.items()}
    got["ground_offset"] = off
    e = _oracle(model, ref, copt, ground, off)
    io = oracle_io(ref)
    e.batch_run("start", io)
    lane_ground.run(model, got, "start", copt, ground=ground)
    assert np.array_equal(got["con_flags"], ref["con_flags"])
    for k in OUTS:
        if ref[k].size:
            assert rel_err(got[k], ref[k]) < 1e-9, ("start", k)
    a_start = got["a"].copy()
    assert _contacts_active(model, ref) >= 2
    for solver in ("euler_explicit", "runge_kutta_4"):
        for _ in range(3):
            e.batch_run("step", io, solver=solver, dt=5e-4, n_substeps=1, command_changed=True)
            lane_ground.run(model, got, "step", copt, ground=ground, solver=solver, dt=5e-4, n_substeps=1, command_changed=True)
        ok = _sane(ref)
        assert ok.sum() >= B // 2
        assert np.array_equal(got["con_flags"][:, ok], ref["con_flags"][:, ok]), solver
        for k in OUTS:
            if ref[k].size:
                assert rel_err(got[k], ref[k], ok) < 1e-8, (solver, k)
    # the map is not a no-op: the same lanes on flat ground (same instantiation) start with another acceleration
    _, _, _, flat, _, _ = _setup(name, B, 23)
    lane_ground.run(model, flat, "start", copt)
    assert rel_err(flat["a"], a_start) > 1e-3


# ---------------------------------------------------------------- incline: known answers

THETA, MASS = 0.3, 2.0
INCLINE_COPT = dict(regularization=1e-9, stabilization_freq=0.0)


def _incline(theta):
    """The plane z = -tan(theta) x (tilted by `theta` about y, downhill towards +x) as a height map around the origin."""
    xs = np.linspace(-4.0, 4.0, 9)
    return (np.tile(-math.tan(theta) * xs, (9, 1)), -4.0, -4.0, 1.0, 1.0)


def _incline_expected(mu, g=9.81):
    """(world linear acceleration, world contact force) of a point mass at rest on the incline at t = 0."""
    s, c = math.sin(THETA), math.cos(THETA)
    n, d = np.array([s, 0.0, c]), np.array([c, 0.0, -s])     # normal, downhill tangent (= t0)
    if mu >= math.tan(THETA):
        return np.zeros(3), np.array([0.0, 0.0, MASS * g])
    N = MASS * g * c
    return g * (s - mu * c) * d, N * n - mu * N * d


def _check_incline(a, v, cf, mu, t):
    """`a`, `v` (free-flyer, local = world: the base does not turn), `cf` (contact frame = world) of one lane at time t."""
    acc, f = _incline_expected(mu)
    scale = 9.81
    assert np.abs(a[:3] - acc).max() < 1e-8 * scale and np.abs(a[3:]).max() < 1e-8 * scale, (a, acc)
    assert np.abs(v[:3] - t * acc).max() < 1e-8 * max(1.0, scale * t) and np.abs(v[3:]).max() < 1e-8, (v, t * acc)
    assert np.abs(cf[:3] - f).max() < 1e-8 * MASS * scale, (cf, f)


@pytest.mark.parametrize("mu", [0.5, 0.1])
def test_incline_known_answers_on_the_oracle(mu):
    """CPU pin of the law the device follows: a point mass (contact point at its centre of mass) on a plane tilted by
    0.3 rad stays at rest under mu >= tan (contact force m g z) and slides with g (sin - mu cos) along the slope under
    mu < tan (normal force m g cos), at `start` and over 50 steps."""
    model = _robot("point_mass")
    arr = alloc_soa(model, 1)
    alloc_constraint_state(model, arr, 1)
    arr["q"][:, 0] = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    e = _oracle(model, arr, INCLINE_COPT, _incline(THETA), None, friction=mu)
    io = oracle_io(arr)
    e.batch_run("start", io)
    _check_incline(arr["a"][:, 0], arr["v"][:, 0], arr["contact_forces"][:, 0], mu, 0.0)
    dt = 1e-3
    for k in range(50):
        e.batch_run("step", io, solver="euler_explicit", dt=dt, n_substeps=1, command_changed=False)
    _check_incline(arr["a"][:, 0], arr["v"][:, 0], arr["contact_forces"][:, 0], mu, 50 * dt)


# ---------------------------------------------------------------- device

def _engine(model, B, dev, solver, dt, copt, contacts=None, extra=("contact_forces", "f_external")):
    import torch

    from jiminy_amd.engine import BatchedEngine
    eng = BatchedEngine(model, B, dtype=torch.float64, device=dev, extra_outputs=extra)
    stepper = {"odeSolver": solver, "dtMax": dt, "controllerUpdatePeriod": dt, "sensorsUpdatePeriod": dt,
               "tolAbs": copt["tol_abs"], "tolRel": copt["tol_rel"]}
    opts = {"stepper": stepper, "contacts": dict({"model": "constraint"}, **(contacts or {}))}
    if "regularization" in copt:
        opts["constraints"] = {"regularization": copt["regularization"]}
    if "stabilization_freq" in copt:
        opts["contacts"]["stabilizationFreq"] = copt["stabilization_freq"]
    eng.set_options(opts)
    return eng


def _add_held_constraints(eng, model, held, freq):
    import torch

    from jiminy_amd.engine import DistanceConstraint, FrameConstraint
    xs = model.constraint_frames
    eng.add_constraint("hold_base", FrameConstraint(xs[0]["frame"], tuple(bool((xs[0]["mask"] >> d) & 1) for d in range(6)),
                                                    baumgarte_freq=freq), lane_mask=torch.from_numpy(held))
    eng.add_constraint("rod", DistanceConstraint(xs[1]["frame"], xs[1]["frame2"], baumgarte_freq=freq),
                       lane_mask=torch.from_numpy(~held))


def _fields(eng, keys):
    import torch
    torch.cuda.synchronize()
    return {k: eng.field(k).cpu().numpy() for k in keys if k in eng._fields}


@pytest.mark.gpu
@pytest.mark.parametrize("name,solver,biased", [("tree_arm_ff", "euler_explicit", False), ("tree_arm_ff", "runge_kutta_4", True),
                                                ("tree_arm_flex_ff", "euler_explicit", True),
                                                ("anymal_held", "euler_explicit", False)])
def test_gpu_lane_constraint_contacts_on_a_height_map_match_oracle(gpu_device, name, solver, biased):
    """`set_ground_heightmap` + `set_ground_offsets` under `contacts.model = "constraint"` on robots of the one-robot-per-lane
    family (tree robots, a flexible one, ANYmal with user constraints on half of the lanes): device against the oracle."""
    import torch

    from jiminy_amd.randomization import sample_model_lane
    B, dt = 32, (1e-3 if name == "anymal_held" else 5e-4)
    model, st, copt, ref, off, held = _setup(name, B, 41)
    ground = _bumpy(41)
    ml = sample_model_lane(model, B, BIAS, torch.Generator().manual_seed(41)).numpy() if biased else None
    e = _oracle(model, ref, copt, ground, off, ml)
    io = oracle_io(ref)
    eng = _engine(model, B, gpu_device, solver, dt, copt)
    freq = copt.get("user_stabilization_freq")
    if name == "anymal_held":
        _add_held_constraints(eng, model, held, freq)
    if ml is not None:
        eng.set_lane_model(torch.from_numpy(ml))
    eng.set_ground_heightmap(*ground)
    eng.set_ground_offsets(torch.from_numpy(off.T.copy()))   # (B, 2)
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
    tol_start, tol = (1e-6, 1e-5) if name == "anymal_held" else (1e-7, 1e-7)

    def check(what, ok, tol):
        got = _fields(eng, ("con_flags",) + OUTS)
        assert np.array_equal(got["con_flags"][:, ok], ref["con_flags"][:, ok]), what
        for k in OUTS:
            if k in got and ref[k].size:
                assert rel_err(got[k], ref[k], ok) < tol, (what, k, rel_err(got[k], ref[k], ok))
    check("start", np.ones(B, dtype=bool), tol_start)
    assert _contacts_active(model, ref) >= 4
    loop = ReferenceFixedStepLoop(dt)
    ok = np.ones(B, dtype=bool)
    for _ in range(5):
        eng.step(dt)
        loop.advance(lambda h, first: e.batch_run("step", io, solver=solver, dt=h, n_substeps=1, command_changed=first), dt, True)
        ok &= _sane(ref)
    assert ok.sum() > 0.5 * B
    check(solver, ok, tol)


@pytest.mark.gpu
def test_gpu_adaptive_stepper_reads_the_patches_through_the_lane_map(gpu_device):
    """`runge_kutta_dopri` (per-stage launches over compact batches) on a bumpy map with a patch per lane, constraint
    contacts: against the oracle's adaptive stepper -- the offsets are read in batch order through the lane map."""
    import torch

    from jiminy_amd.engine import plan_breakpoints
    from oracle.oracle_py import adaptive_state
    B = 32
    model, st, copt, ref, off, _ = _setup("tree_arm_ff", B, 43)
    ground = _bumpy(43)
    e = _oracle(model, ref, copt, ground, off)
    io = oracle_io(ref)
    eng = _engine(model, B, gpu_device, "runge_kutta_dopri", 0.02, copt)
    eng.set_options({"stepper": {"controllerUpdatePeriod": 2e-3, "sensorsUpdatePeriod": 2e-3}})
    eng.set_ground_heightmap(*ground)
    eng.set_ground_offsets(torch.from_numpy(off.T.copy()))
    eng.set_command(torch.from_numpy(st["command"]))
    eng.start(torch.from_numpy(st["q"]), torch.from_numpy(st["v"]))
    e.batch_run("start", io)
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
    assert ok.mean() > 0.8 and int(ad["iter"].max()) > int(ad["iter"].min())   # (the compact batches re-order the lanes)
    ok &= _sane(ref)
    assert ok.sum() > 0.5 * B and _contacts_active(model, ref) >= 4
    got = _fields(eng, ("q", "v", "a", "contact_forces", "f_external"))
    for k, x in got.items():
        assert rel_err(x, ref[k], ok) < 1e-7, k


def _quat_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions, columns = lanes."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


@pytest.mark.gpu
def test_gpu_tilted_ground_is_tilted_gravity(gpu_device):
    """No oracle: a plane tilted by theta about y as a height map under standard gravity, the base posed R M, against flat
    ground under gravity R^T g with the base posed M (the validated flat path).  The local bases coincide (t0 = R e_x,
    t1 = R e_y, n = R e_z), so the joint positions, the local base velocity and every local output agree to round-off."""
    import torch

    from jiminy_amd.randomization import nominal_model_lane
    theta, B, dt = 0.25, 32, 5e-4
    s, c = math.sin(theta), math.cos(theta)
    Rm = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    model = _robot("tree_arm_ff")
    st = sample_states(model, B, seed=47, base_height=(0.3, 0.6), grounded_fraction=0.6)
    # no threshold ties: every contact point >= 1 mm inside the ground or >= 2 transitionEps above it
    Rs, ps = joint_world_placements(model, st["q"])
    z = np.stack([(ps[model.frames[n].parent_joint] + Rs[model.frames[n].parent_joint] @ model.frames[n].p)[:, 2]
                  for n in model.contacts])
    keep = np.all((z <= -1e-3) | (z >= 2e-3), axis=0)
    assert keep.sum() >= B // 2
    qB, vB = st["q"][:, keep], st["v"][:, keep]
    cmd = st["command"][:, keep]
    B = int(keep.sum())
    qA = qB.copy()
    qA[:3] = Rm @ qB[:3]
    qA[3:7] = _quat_mul(np.array([0.0, math.sin(theta / 2), 0.0, math.cos(theta / 2)])[:, None], qB[3:7])
    # (the plane z = -tan(theta) x; the map covers every contact point of the 20 steps)
    xs = np.linspace(-3.0, 3.0, 13)
    tilted = (np.tile(-math.tan(theta) * xs, (13, 1)), -3.0, -3.0, 0.5, 0.5)
    g = np.array([0.0, 0.0, -9.81])
    keys = ("q", "v", "a", "con_flags", "con_data", "contact_forces", "f_external", "imu")
    out = []
    for setup in ("A", "B"):
        eng = _engine(model, B, gpu_device, "euler_explicit", dt, TIGHT)
        if setup == "A":
            eng.set_ground_heightmap(*tilted)
            q0 = qA
        else:
            eng.set_options({"world": {"gravity": list(Rm.T @ g) + [0.0, 0.0, 0.0]}})
            q0 = qB
        # (both setups run the variation instantiation: nominal body parameters bound)
        eng.set_lane_model(nominal_model_lane(model, B, torch.float64, gpu_device))
        eng.set_command(torch.from_numpy(np.ascontiguousarray(cmd)))
        eng.start(torch.from_numpy(np.ascontiguousarray(q0)), torch.from_numpy(np.ascontiguousarray(vB)))
        for _ in range(20):
            eng.step(dt)
        out.append(_fields(eng, keys))
    A_, B_ = out
    assert np.array_equal(A_["con_flags"], B_["con_flags"])
    assert (A_["con_flags"][_abi.constraint_rows(model)["n_bounds"]:] & 1).sum() >= 4
    for k in ("v", "a", "con_data", "contact_forces", "f_external", "imu"):
        assert rel_err(A_[k], B_[k]) < 1e-9, (k, rel_err(A_[k], B_[k]))
    assert rel_err(A_["q"][7:], B_["q"][7:]) < 1e-9
    # ... and the base itself: A = R B
    assert rel_err(A_["q"][:3], Rm @ B_["q"][:3]) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("mu", [0.5, 0.1])
def test_gpu_incline_known_answers(gpu_device, mu):
    """The incline on the device (the variation instantiation with the map): at rest under mu >= tan theta, sliding with
    g (sin - mu cos) under mu < tan theta, at `start` and over 50 Euler steps."""
    import torch
    model = _robot("point_mass")
    B, dt = 4, 1e-3
    eng = _engine(model, B, gpu_device, "euler_explicit", dt, dict(TIGHT, **INCLINE_COPT), contacts={"friction": mu})
    eng.set_ground_heightmap(*_incline(THETA))
    q0 = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])[:, None], (1, B))
    q0[1] = np.linspace(-0.5, 0.5, B)   # (lanes across the slope: the same answer)
    eng.start(torch.from_numpy(q0), torch.zeros(6, B, dtype=torch.float64))

    def check(t):
        got = _fields(eng, ("a", "v", "contact_forces"))
        for lane in range(B):
            _check_incline(got["a"][:, lane], got["v"][:, lane], got["contact_forces"][:, lane], mu, t)
    check(0.0)
    for _ in range(50):
        eng.step(dt)
    check(50 * dt)


@pytest.mark.gpu
def test_gpu_zero_map_is_flat_ground(gpu_device):
    """An all-zero map, and a constant map c with the robots raised by c, reproduce the no-map run of the same variation
    instantiation (per-lane body parameters bound in all three) to round-off."""
    import torch

    from jiminy_amd.randomization import sample_model_lane
    B, dt, c = 32, 5e-4, 0.137
    model, st, copt, _, off, _ = _setup("tree_arm_ff", B, 53)
    ml = torch.from_numpy(sample_model_lane(model, B, BIAS, torch.Generator().manual_seed(53)).numpy())
    keys = ("q", "v", "a", "con_flags", "con_data", "u", "contact_forces", "f_external", "imu")
    out = []
    for heights, dz in ((None, 0.0), (np.zeros((7, 9)), 0.0), (np.full((7, 9), c), c)):
        eng = _engine(model, B, gpu_device, "euler_explicit", dt, copt)
        eng.set_lane_model(ml)
        if heights is not None:
            eng.set_ground_heightmap(heights, -1.0, -0.8, 0.25, 0.3)
            eng.set_ground_offsets(torch.from_numpy(off.T.copy()))
        q0 = st["q"].copy()
        q0[2] += dz
        eng.set_command(torch.from_numpy(st["command"]))
        eng.start(torch.from_numpy(q0), torch.from_numpy(st["v"]))
        for _ in range(10):
            eng.step(dt)
        got = _fields(eng, keys)
        got["q"][2] -= dz
        out.append(got)
    flat = out[0]
    assert (flat["con_flags"][_abi.constraint_rows(model)["n_bounds"]:] & 1).sum() >= 4
    for other in out[1:]:
        assert np.array_equal(other["con_flags"], flat["con_flags"])
        for k in keys[:2] + keys[3:]:
            if k in flat and k != "con_flags":
                # (con_data holds the reference positions of the bounded joints, not of the base: no shift there)
                assert rel_err(other[k], flat[k]) < 1e-12, (k, rel_err(other[k], flat[k]))


@pytest.mark.gpu
def test_gpu_lane_family_walker_env_on_random_tiles_with_constraint_contacts(gpu_device):
    """The env path (`ground_profile`, `ground_patch_extent`, `ground_height_around` at the resets) for a walker of the
    one-robot-per-lane family (ANYmal declaring user constraints) under the reference's default contact model."""
    import torch

    from jiminy_amd import envs
    from jiminy_amd.terrain import random_tile_ground
    B = 64
    model = _robot("anymal_held")
    terrain = (random_tile_ground((0.4, 0.4), 0.02, (0.05, 0.05), 2, 0.3, 17), (-3.0, 3.0), (-3.0, 3.0), 0.02)
    opts = {"stepper": {"odeSolver": "euler_explicit", "dtMax": 1e-3}, "contacts": {"model": "constraint"}}
    env = envs.PDControlledWalkerVecEnv(model, B, envs.ANYMAL_STEP_DT, envs.ANYMAL_CONTROL_DT, envs.ANYMAL_PD_KP,
                                        envs.ANYMAL_PD_KD, envs.ANYMAL_MAHONY_KP, envs.ANYMAL_MAHONY_KI,
                                        joint_velocity_limit=envs.ANYMAL_MOTOR_VELOCITY_MAX,
                                        joint_acceleration_limit=envs.ANYMAL_MOTOR_ACCELERATION_MAX, engine_options=opts,
                                        dtype=torch.float64, device=gpu_device, ground_profile=terrain,
                                        ground_patch_extent=(2.0, 2.0))
    obs, _ = env.reset(seed=5)
    assert env.engine._ground is not None and float(env.engine.field("ground_offset").abs().max()) > 0.0
    g = torch.Generator(device="cpu").manual_seed(7)
    bad = torch.zeros(B, dtype=torch.bool, device=gpu_device)
    for i in range(20):
        action = (0.5 * torch.randn(B, model.nmotors, generator=g, dtype=torch.float64)).to(gpu_device)
        obs, reward, terminated, truncated, info = env.step(action)
        q = obs["states"]["agent"]["q"]
        bad |= ~torch.isfinite(q).all(dim=1) | ~torch.isfinite(reward)
        if i == 10:
            mask = torch.zeros(B, dtype=torch.bool, device=gpu_device)
            mask[::5] = True
            env.reset_lanes(mask)
    assert int(bad.sum()) <= 0.01 * B
    nb = _abi.constraint_rows(model)["n_bounds"]
    assert int((env.engine.field("con_flags")[nb:nb + len(model.contacts)] & 1).sum()) >= B
