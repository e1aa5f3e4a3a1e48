"""The `tracking_rewards` keyword of `WalkerVecEnv`: the reference side (one frame kinematics block, `blocks.CentroidalState`,
`blocks.LocomotionQuantities(state=...)`) and `blocks.TrackingRewards` inside the environment, its refusals on the host and a
replay of the environment's own record on the device."""
from __future__ import annotations

import numpy as np
import pytest

from jiminy_amd import load_builtin, trajectory

CUTOFFS = dict(base_height_cutoff=0.1, odometry_velocity_cutoff=0.5, capture_point_cutoff=0.2, joint_positions_cutoff=0.5)
TERMS = ("base_height", "odometry_velocity", "capture_point", "joint_positions")


def test_environment_keywords_are_refused_on_the_host(monkeypatch):
    """Every refusal of the keyword, before any block is built (the base class is not run: it needs a device)."""
    import torch

    from jiminy_amd.envs import VecJiminyEnv, WalkerVecEnv
    model = load_builtin("anymal")

    def bare_init(self, *args, **kw):
        self.model, self.num_envs, self.step_dt, self.dtype, self.device, self.engine = model, 4, 0.04, torch.float64, torch.device("cpu"), None
    monkeypatch.setattr(VecJiminyEnv, "__init__", bare_init)
    t, q = [0.0, 0.5, 1.0], np.tile(model.neutral(), (3, 1))
    with_v = dict(dataset={"a": (trajectory.Trajectory(t, q, v=np.zeros((3, model.nv))), "wrap")})
    without_v = dict(dataset={"a": (trajectory.Trajectory(t, q), "wrap")})
    with pytest.raises(NotImplementedError, match=r"a recorded trajectory carries no constraint multipliers \(`State.lambda_c`\)"):
        WalkerVecEnv(reward_mixture={"foot_force_distribution": 1.0})
    for term in TERMS:
        with pytest.raises(ValueError, match="read the tracking rewards block: give tracking_rewards as well"):
            WalkerVecEnv(reward_mixture={term: 1.0})
        with pytest.raises(ValueError, match=rf"reward_mixture\['{term}'\] needs tracking_rewards\['{term}_cutoff'\]"):
            WalkerVecEnv(reward_mixture={term: 1.0}, tracking_rewards={f"{term}_cutoff": None}, trajectory_database=with_v)
    with pytest.raises(ValueError, match=r"unknown keys in tracking_rewards: \['cutoff'\]"):
        WalkerVecEnv(tracking_rewards=dict(cutoff=1.0), trajectory_database=with_v)
    with pytest.raises(ValueError, match="give trajectory_database as well"):
        WalkerVecEnv(tracking_rewards=dict(base_height_cutoff=0.1))
    for key in ("odometry_velocity_cutoff", "capture_point_cutoff"):
        with pytest.raises(ValueError, match="need a dataset with v"):
            WalkerVecEnv(tracking_rewards={key: 0.1}, trajectory_database=without_v, locomotion_quantities={})
    with pytest.raises(ValueError, match=r"\['joint_positions_cutoff'\] reads the actuated-joint quantities block: give actuated_joints"):
        WalkerVecEnv(tracking_rewards=dict(joint_positions_cutoff=0.1), trajectory_database=without_v)
    with pytest.raises(ValueError, match=r"\['capture_point_cutoff'\] reads the locomotion quantities block: give locomotion_quantities"):
        WalkerVecEnv(tracking_rewards=dict(capture_point_cutoff=0.1), trajectory_database=with_v)
    with pytest.raises(ValueError, match=r"locomotion_quantities\['dcm_reference_frame'\] must be 'LOCAL'"):
        WalkerVecEnv(tracking_rewards=dict(capture_point_cutoff=0.1), trajectory_database=with_v,
                     locomotion_quantities=dict(dcm_reference_frame="LOCAL_WORLD_ALIGNED"))


BLOCKS = dict(locomotion_quantities=dict(forces=False, momentum=False), foot_poses=dict(position_cutoff=0.1, orientation_cutoff=0.2),
              actuated_joints={})


@pytest.mark.gpu
def test_environment_replays_its_own_record_with_the_tracking_rewards(gpu_device):
    """`WalkerVecEnv` (ANYmal, 64 lanes, no randomisation): `q`, `v`, `a` at the reset and after each of 4 steps of a fixed
    action are recorded as one trajectory per lane, mode "wrap".  Replayed with all four terms from the recorded start under
    the recorded action, the even lanes track their own record: the height, the velocity and the joint positions of the two
    sides agree to the bit and every reward is 1 or within 1e-9 of it (the capture point of the reference side comes from
    `CentroidalState`, the true one from the physics kernels: they agree to round-off).  The odd lanes track their record
    from half of it on (`time_offset_ratio` 0.5) while the robot starts at its beginning -- a start perturbed by two steps of
    motion relative to the reference (every lane of this environment resets to the same state, so that a neighbour's record
    would be no perturbation): every reward is strictly below 1.  `value` and `reference` are the host composition of the
    tensors of the other blocks.

    `reset_lanes` on half the lanes: the other half keeps every bit; the reset half equals the snapshot taken right after
    `reset` -- a fresh environment, since every lane restarts from the same state on the same trajectory and offset -- in
    `value`, `reference`, `rewards` and in the pose, the centroidal rows and the capture point of the reference side, with
    rewards of 1 on the tracking lanes.  The odometry velocity rows are the exception: the step average of a frame kinematics
    block has no value at a restart, `FrameKinematics.reset` leaves `average_velocity` of the masked lanes as the last step
    wrote it (zeros in a fresh environment), and the rows are held to the host composition of those tensors instead.

    Graph capture: the whole-step graph of the environment refuses a trajectory database, and its per-step graph ends before
    `_after_step`, where these blocks run.  What is captured here is the `refresh` of the reference frame kinematics, the
    reference foot poses, `CentroidalState`, the reference `LocomotionQuantities` and `TrackingRewards`; the trajectory query
    (its time is a host-side subtraction), the step average (it advances `pose_prev`: a replay is not idempotent) and the
    physics step stay outside.  Every tensor those five launches write is poisoned before the replay and must come back to
    the bits of the eager launches.  Without the keyword the environment builds what it built before."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    B, steps = 64, 4
    common = dict(device=gpu_device, contact_model="constraint", auto_reset=False, **BLOCKS)
    gen = torch.Generator(device="cpu").manual_seed(3)
    action = (0.3 * (2.0 * torch.rand(B, 12, generator=gen, dtype=torch.float64) - 1.0)).to(gpu_device)
    lane = torch.arange(B, device=gpu_device)

    first = make_anymal_env(B, **common)
    assert first.tracking_rewards is None and first._reference_centroidal is None and first._reference_locomotion is None
    first.reset(seed=11)
    state = lambda env: tuple(env.engine.field(k).cpu().numpy().copy() for k in ("q", "v", "a"))      # noqa: E731
    times, record = [float(first._lane_time()[0])], [state(first)]
    rewards_plain = []
    for _ in range(steps):
        rewards_plain.append(first.step(action)[1].clone())
        times.append(float(first._lane_time()[0]))
        record.append(state(first))
    first.close()
    database = {f"lane{b}": (trajectory.Trajectory(times, *[np.stack([r[i][:, b] for r in record]) for i in (0, 1)],
                                                   a=np.stack([r[2][:, b] for r in record])), "wrap") for b in range(B)}
    assert np.abs(record[2][0] - record[0][0]).max() > 1e-3, "two steps move the robot"

    # without the keyword: the blocks and the reward of before
    plain = make_anymal_env(B, trajectory_database=dict(dataset=database), **common)
    plain.select_trajectory(lane)
    plain.reset(seed=11)
    assert plain.tracking_rewards is None and plain._reference_centroidal is None and plain._reference_locomotion is None
    assert plain._reference_frames.frame_names == list(plain.foot_poses.foot_frame_names) and not plain._reference_frames.average
    assert plain.trajectory.a is not None
    assert torch.equal(plain.step(action)[1], rewards_plain[0])
    plain.close()

    mixture = {"survival": 1.0, **{term: 1.0 for term in TERMS}}
    env = make_anymal_env(B, trajectory_database=dict(dataset=database), tracking_rewards=CUTOFFS, reward_mixture=mixture, **common)
    own = lane % 2 == 0
    env.select_trajectory(lane, None, torch.where(own, 0.0, 0.5).to(torch.float64))
    env.reset(seed=11)
    tr, ref_frames = env.tracking_rewards, env._reference_frames
    names = ["root_joint"] + list(env.model.contacts)
    assert ref_frames.frame_names[:5] == names and set(env.foot_poses.foot_frame_names) <= set(ref_frames.frame_names)
    assert ref_frames.average and env.frames.average and env._reference_foot_poses._frames is ref_frames
    assert env._reference_locomotion.zmp is not None and env._reference_centroidal.has_acceleration
    tensors = {k: getattr(tr, k) for k in ("value", "reference", "rewards")}
    written = dict(tensors, pose=ref_frames.pose, rows=env._reference_centroidal.centroidal, dcm=env._reference_locomotion.dcm,
                   com=env._reference_locomotion.com, relative=env._reference_foot_poses.relative_pose)
    torch.cuda.synchronize(gpu_device)
    fresh = {k: t.clone() for k, t in written.items()}
    assert (fresh["rewards"][:, own] == 1).all() and (fresh["rewards"][[0, 2, 3]][:, ~own] < 1).all()

    def composition():
        z, zr = env.frames.pose[2], ref_frames.pose[2]
        col = [env.frames.index(n) for n in names]
        assert torch.equal(tr.value[0], z[col[0]] - z[col[1:]].min(0).values)
        assert torch.equal(tr.reference[0], zr[0] - zr[1:5].min(0).values)
        assert torch.equal(tr.value[4:6], env.locomotion.dcm) and torch.equal(tr.reference[4:6], env._reference_locomotion.dcm)
        assert torch.equal(tr.value[6:], env.actuation.position) and torch.equal(tr.reference[6:], env.trajectory.position)
        for side, blk, root in ((tr.value, env.frames, col[0]), (tr.reference, ref_frames, 0)):
            x, y, zq, w = blk.quat_no_yaw[:, root]
            R = torch.stack([torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * w), 2 * (x * zq + y * w)]),
                             torch.stack([2 * (x * y + zq * w), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * w)]),
                             torch.stack([2 * (x * zq - y * w), 2 * (y * zq + x * w), 1 - 2 * (x * x + y * y)])])
            v = blk.average_velocity[:, root]
            lin, ang = torch.einsum("ijb,jb->ib", R, v[:3]), torch.einsum("ijb,jb->ib", R, v[3:])
            # (a rotation of vectors below 10 m/s and rad/s: a few dozen float64 roundings)
            assert (side[1:4] - torch.stack([lin[0], lin[1], ang[2]])).abs().max() < 1e-13
        e = tr.value - tr.reference
        sq = torch.stack([(e[0:1] ** 2).sum(0), (e[1:4] ** 2).sum(0), (e[4:6] ** 2).sum(0), (e[6:] ** 2).sum(0)])
        cutoff = torch.tensor(list(CUTOFFS.values()), dtype=torch.float64, device=gpu_device)[:, None]
        assert (tr.rewards - torch.pow(torch.tensor(0.01, dtype=torch.float64, device=gpu_device), sq / cutoff ** 2)).abs().max() < 1e-12

    out = env.step(action)
    torch.cuda.synchronize(gpu_device)
    composition()
    assert torch.equal(env.trajectory.q[:, own], torch.as_tensor(record[1][0], device=gpu_device)[:, own])
    for rows in (slice(0, 4), slice(6, None)):
        assert torch.equal(tr.value[rows][:, own], tr.reference[rows][:, own]), "the same kernels on the same numbers"
    print("rewards of the tracking lanes, min per term:", tr.rewards[:, own].min(1).values.tolist())
    print("rewards of the perturbed lanes, max per term:", tr.rewards[:, ~own].max(1).values.tolist())
    assert (tr.rewards[[0, 1, 3]][:, own] == 1).all() and (tr.rewards[2, own] > 1 - 1e-9).all() and (tr.rewards[:, own] <= 1).all()
    assert (tr.rewards[:, ~own] < 1).all()
    assert torch.equal(out[1], 1.0 + tr.rewards[0] + tr.rewards[1] + tr.rewards[2] + tr.rewards[3])
    assert all(getattr(tr, k) is t for k, t in tensors.items())

    # a captured graph of the reference side and the rewards (docstring: what is captured and what is not)
    blocks_ = (ref_frames, env._reference_foot_poses, env._reference_centroidal, env._reference_locomotion, tr)
    eager = {k: t.clone() for k, t in written.items()}
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.graph(graph):
        for blk in blocks_:
            blk.refresh()
    for t in written.values():
        t.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize(gpu_device)
    for k, t in written.items():
        assert torch.equal(t, eager[k]), k

    # reset_lanes on half the lanes
    half = lane < B // 2
    held = {k: t.clone() for k, t in written.items()}
    held["prev"] = ref_frames.pose_prev.clone()
    env.reset_lanes(half)
    torch.cuda.synchronize(gpu_device)
    for k, t in dict(written, prev=ref_frames.pose_prev).items():
        assert torch.equal(t[..., ~half], held[k][..., ~half]), k
    assert torch.equal(env.trajectory.q[:, half & own], torch.as_tensor(record[0][0], device=gpu_device)[:, half & own])
    assert torch.equal(ref_frames.pose[..., half], ref_frames.pose_prev[..., half])
    other = torch.ones(tr.value.shape[0], dtype=torch.bool, device=gpu_device)
    other[1:4] = False      # (the odometry velocity rows: docstring)
    for k, t in written.items():
        if k in ("value", "reference"):
            assert torch.equal(t[other][:, half], fresh[k][other][:, half]), k
        elif k == "rewards":
            assert torch.equal(t[[0, 2, 3]][:, half], fresh[k][[0, 2, 3]][:, half]), k
        else:
            assert torch.equal(t[..., half], fresh[k][..., half]), k
    assert (tr.rewards[[0, 2, 3]][:, half & own] == 1).all()
    assert not torch.equal(held["rows"][:, half], fresh["rows"][:, half]), "the step had moved the reference side"
    composition()
    env.close()


@pytest.mark.gpu
def test_environment_builds_only_the_blocks_a_term_reads(gpu_device):
    """With the joint positions alone the reference side is what it was without the keyword; with the base height alone there
    is the merged frame kinematics block (no step average) and no centroidal or locomotion block."""
    import torch

    from jiminy_amd.envs import make_anymal_env
    model = load_builtin("anymal")
    t, q = [0.0, 0.5, 1.0], np.tile(model.neutral(), (3, 1))
    dataset = {"a": (trajectory.Trajectory(t, q, v=np.zeros((3, model.nv))), "wrap")}
    common = dict(device=gpu_device, contact_model="constraint", auto_reset=False, trajectory_database=dict(dataset=dataset), **BLOCKS)
    env = make_anymal_env(8, tracking_rewards=dict(joint_positions_cutoff=0.5), reward_mixture={"joint_positions": 1.0}, **common)
    assert env._reference_centroidal is None and env._reference_locomotion is None
    assert env._reference_frames.frame_names == list(env.foot_poses.foot_frame_names) and not env._reference_frames.average
    env.reset(seed=1)
    reward = env.step(torch.zeros(8, 12, dtype=torch.float64, device=gpu_device))[1]
    assert torch.equal(reward, env.tracking_rewards.reward("joint_positions")) and (env.tracking_rewards.rewards[:3] == 0).all()
    env.close()
    env = make_anymal_env(8, tracking_rewards=dict(base_height_cutoff=0.1), **common)
    assert env._reference_centroidal is None and env._reference_locomotion is None
    assert env._reference_frames.frame_names[:5] == ["root_joint"] + list(model.contacts) and not env._reference_frames.average
    env.close()
