"""Vectorised environments on top of BatchedEngine: the gym_jiminy reset / step / observe surface
for B lanes at once, every array a device tensor.

Restates, for the hot-path subset, `BaseJiminyEnv` (reference
python/gym_jiminy/common/gym_jiminy/common/envs/generic.py: reset :521, step :761,
`_sample_state` :1300, `has_terminated` :1434, observation layout :1247-1270) and
`WalkerJiminyEnv` (envs/locomotion.py: fall detection :361-385, survival / energy reward :387-431),
plus the ANYmal pipeline of `gym_jiminy/envs/anymal.py:82-127` (PD controller + Mahony filter) as
device-resident blocks.  Differences that come with batching are explicit: numerical failures are
per lane (`truncated`), and finished lanes are re-initialised in place (`jm_batch_reset_lanes`)
instead of raising for the whole batch.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, blocks
from .engine import BatchedEngine
from .model import CompiledModel, JT_FREEFLYER, load_builtin
from .synthetic import lowest_contact_height

ObsType = Dict[str, Any]


class VecJiminyEnv:
    """B independent single-robot environments stepped by one kernel launch.

    `action` is the motor command `[B][nmotors]` unless a controller block is configured.
    Observations follow the reference layout with a leading batch axis:
    `{'t': (B,), 'states': {'agent': {'q': (B, nq), 'v': (B, nv)}},
      'measurements': {SensorType: (B, n_fields, n_sensors)}}` -- zero-copy views of the
    engine's `[rows][B]` storage.
    """

    def __init__(self, model: CompiledModel, num_envs: int, step_dt: float,
                 engine_options: Optional[Dict[str, Dict[str, Any]]] = None,
                 dtype: torch.dtype = torch.float64, device: Optional[torch.device] = None,
                 simulation_duration_max: float = 86400.0, auto_reset: bool = True,
                 std_ratio: Optional[Dict[str, float]] = None,
                 model_options: Optional[Dict[str, Dict[str, float]]] = None,
                 ground_profile: Optional[Tuple[Any, Tuple[float, float], Tuple[float, float], float]] = None,
                 ground_patch_extent: Optional[Tuple[float, float]] = None,
                 disturbance_on_device: bool = False, disturbance_impulses: bool = True) -> None:
        self.model = model
        # the continuous disturbance force (std_ratio['disturbance']) as PROCESS FORCES: the step kernels evaluate the two
        # Gaussian processes inside every dynamics evaluation, at its own time, like the reference's profile force
        # (`BatchedEngine.register_process_force`) -- instead of a callable the host re-evaluates at the start of every
        # integrator step.  `disturbance_impulses=False` keeps only that continuous part: nothing is scheduled on the
        # host any more, and the step can be replayed as a graph (`enable_graph`).
        self._disturbance_on_device = bool(disturbance_on_device)
        self._disturbance_impulses = bool(disturbance_impulses)
        # every environment its own patch of the ground profile: at every (lane) reset a new (x, y) offset of its
        # height-map queries, uniform in +- extent (`BatchedEngine.set_ground_offsets`) -- the batched form of a new random
        # `groundProfile` per environment instance and episode
        if ground_patch_extent is not None and ground_profile is None:
            raise ValueError("ground_patch_extent needs a ground_profile to take the patches from")
        self._ground_patch_extent = ground_patch_extent
        # ≙ `engine_options["world"]["groundProfile"]`: `(heightmap(x, y), x_range, y_range, resolution)`, e.g. a
        # `jiminy_amd.terrain.random_tile_ground` generator; sampled on the device at every `reset()`, shared by the batch
        self._ground_profile = ground_profile
        # ≙ `WalkerJiminyEnv(std_ratio=...)` (envs/locomotion.py:100-135): scale of the episode-wise
        # randomisation.  Supported keys: 'ground' (friction coefficient of every environment, constraint
        # contact model) and 'sensors' (white noise, bias, delay and jitter of every sensor type, drawn once per
        # `reset()` for the whole batch: the sensor options are lane-uniform kernel parameters) and 'disturbance'
        # (impulse forces on the root body, envs/locomotion.py:298-331: one random horizontal push per environment
        # every F_IMPULSE_PERIOD seconds of ENGINE time).  `model_options` ≙ `robot.set_model_options`: standard
        # deviations of the body mass / centre of mass / inertia / relative position biases
        # (`{"dynamics": {"massBodiesBiasStd": ...}}`, model.h:147-158); every environment gets its own biased model,
        # drawn again whenever it is reset
        self.std_ratio = dict(std_ratio or {})
        self._model_options = model_options
        self.num_envs = int(num_envs)
        self.step_dt = float(step_dt)
        self.engine = BatchedEngine(model, num_envs, dtype=dtype, device=device)
        self.device, self.dtype = self.engine.device, dtype
        if engine_options:
            self.engine.set_options(engine_options)
        if model_options:
            self.engine.set_model_options(model_options)
        self.simulation_duration_max = float(simulation_duration_max)
        self.auto_reset = auto_reset
        self._generator = torch.Generator(device="cpu")
        self.num_steps = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        self._t0 = torch.zeros(self.num_envs, dtype=self.dtype, device=self.device)
        # engine time on the device (set from the host clock around every step, never read back): episode times,
        # truncation and the reset bookkeeping are tensor programs that a captured graph can replay
        self._clock = torch.zeros((), dtype=self.dtype, device=self.device)
        self._state_cache: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._q0 = None
        self._v0 = None
        q_neutral, _ = self._sample_state_numpy()
        self._height_neutral = float(q_neutral[2]) if model.has_freeflyer else 0.0

    # ------------------------------------------------------------------ overridable hooks
    def _sample_state_numpy(self) -> Tuple[np.ndarray, np.ndarray]:
        """≙ `BaseJiminyEnv._sample_state` (generic.py:1300-1334): neutral configuration clipped
        to the bounds, free-flyer placed so that the lowest contact point touches the ground."""
        m = self.model
        q = m.neutral()
        mask = m.bounded_position_mask()
        q[mask] = np.clip(q[mask], m.position_lower[mask], m.position_upper[mask])
        if m.has_freeflyer and m.ncontacts:
            q[2] -= float(lowest_contact_height(m, q)[0])
        return q, np.zeros(m.nv)

    def _sample_state(self, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Initial state for `n` lanes, `[nq][n]` and `[nv][n]`. Default: the neutral state."""
        q, v = self._sample_state_numpy()
        qt = torch.as_tensor(q, dtype=self.dtype, device=self.device)[:, None].expand(-1, n)
        vt = torch.as_tensor(v, dtype=self.dtype, device=self.device)[:, None].expand(-1, n)
        return qt.contiguous(), vt.contiguous()

    def compute_command(self, action: torch.Tensor) -> torch.Tensor:
        """≙ `BaseJiminyEnv.compute_command` (generic.py:1140-1160): the action IS the command.
        `action` is `[B][nmotors]`; returns `[nmotors][B]`."""
        return action.to(self.dtype).T

    def has_terminated(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(terminated, truncated) per lane: truncation on numerical failure / out-of-bounds
        state (generic.py:1434-1470) or on the maximum simulated duration."""
        # a PGS solve that hit its iteration cap is not fatal (the reference only counts it,
        # engine.cc:3755-3768)
        status = self.engine.status & ~_abi.JM_LANE_SOLVER_FAILURE
        # (a state that turned non-finite in the last integrator step of the launch is flagged by the kernel at the NEXT
        # launch: look at it directly, so that the lane restarts now and no NaN reaches the observation)
        # (the acceleration of the end state stands for the state: a non-finite q or v makes it non-finite; one column sum)
        finite = torch.isfinite(self.engine.robot_state.a.sum(0) + self._pipeline_sum())
        truncated = (status != 0) | ~finite | (self._lane_time() >= self.simulation_duration_max)
        return torch.zeros_like(truncated), truncated

    def _pipeline_sum(self) -> Any:
        """Per-lane sum of the controller / observer state (hook of the pipeline environments): non-finite where that
        state is."""
        return 0.0

    def compute_reward(self, terminated: torch.Tensor) -> torch.Tensor:
        return torch.zeros(self.num_envs, dtype=self.dtype, device=self.device)

    def _on_reset(self, lane_mask: Optional[torch.Tensor]) -> None:
        """Hook for controller/observer state (called with the mask of the lanes being reset)."""

    # ------------------------------------------------------------------ gym surface
    def _lane_time(self) -> torch.Tensor:
        return self._clock - self._t0

    def observation(self) -> ObsType:
        rs = self.engine.robot_state
        return {
            "t": self._lane_time(),
            "states": {"agent": {"q": rs.q.T, "v": rs.v.T}},
            "measurements": {k: v.permute(2, 0, 1) for k, v in self.engine.sensor_measurements.items()},
        }

    def reset(self, seed: Optional[int] = None, options: Optional[Dict[str, Any]] = None
              ) -> Tuple[ObsType, Dict[str, Any]]:
        """≙ `BaseJiminyEnv.reset(seed, options)` for the whole batch."""
        if seed is not None:
            self._generator.manual_seed(int(seed))
        # the device-side stream (terrain-patch offsets, spawn heights, masked re-draws) is re-seeded from the host
        # generator at its next use: `reset(seed=s)` reproduces all of them, whatever the disturbance settings
        self._dev_gen = None
        # cached reset states / PD targets of a previous graph capture do not outlive the episode batch
        self._state_cache = None
        self._target_cache = None
        self.engine.stop()
        q, v = self._sample_state(self.num_envs)
        self._q0, self._v0 = q, v
        self.engine.field("command").zero_()
        self._on_reset(None)
        if self._ground_profile is not None:
            self.engine.set_ground_profile(*self._ground_profile)
        self._randomise_ground(None)
        self._randomise_flexibility(None)
        if self._spawn_dz is not None:
            q = q.clone()
            q[2] += self._spawn_dz.to(q.dtype).to(q.device)
        self._randomise_sensors()
        self._schedule_disturbances()
        if self._model_options:
            self.engine.seed_model(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=self._generator)))
        self.engine.start(q, v)
        self.num_steps.zero_()
        self._t0.zero_()
        self._clock.zero_()
        return self.observation(), {}

    def step(self, action: torch.Tensor
             ) -> Tuple[ObsType, torch.Tensor, torch.Tensor, torch.Tensor, Dict[str, Any]]:
        """≙ `BaseJiminyEnv.step(action)` (generic.py:761-880)."""
        if not self.engine.is_simulation_running:
            raise RuntimeError("No simulation running. Please call `reset` before `step`.")
        if tuple(action.shape) != (self.num_envs, self.model.nmotors):
            raise ValueError(f"action must have shape ({self.num_envs}, {self.model.nmotors})")
        self._step_engine(action)
        self._clock.fill_(float(self.engine._t))
        reward, terminated, truncated, done = self._after_step()
        info: Dict[str, Any] = {}
        if self.auto_reset and bool(done.any()):
            # gymnasium "next-step" autoreset would cost a launch per step; lanes are reset in
            # place here and the final observation of the finished lanes is not returned
            info["reset_mask"] = done
            self.reset_lanes(done)
        return self.observation(), reward, terminated, truncated, info

    def _after_step(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Episode bookkeeping after the engine advanced (tensor programs only, no host read-back)."""
        self.num_steps += 1
        terminated, truncated = self.has_terminated()
        reward = torch.nan_to_num(self.compute_reward(terminated), nan=0.0, posinf=0.0, neginf=0.0)   # (numerically failed lanes)
        return reward, terminated, truncated, terminated | truncated

    def _step_engine(self, action: torch.Tensor) -> None:
        self.engine.set_command(self.compute_command(action))
        self._refill_impulses(self.step_dt)
        self.engine.step(self.step_dt)

    def _refill_impulses(self, horizon: float) -> None:
        """Keep the pushes that start within the next `horizon` seconds of engine time registered (see
        `_schedule_disturbances`); a push is drawn once, when it enters the horizon."""
        if getattr(self, "_impulse_frame", None) is None:
            return
        scale = float(self.std_ratio.get("disturbance", 0.0))
        g, B = self._generator, self.num_envs
        t_now = float(self.engine._t)    # (host-side clock: no device synchronisation)
        while True:
            t_ref = self._impulse_index * self.F_IMPULSE_PERIOD
            if t_ref - self.F_IMPULSE_DELTA > t_now + horizon + self.F_IMPULSE_DT:
                break
            t = t_ref + self.F_IMPULSE_DELTA * float(torch.rand(1, generator=g) * 2.0 - 1.0)
            t = max(t, t_now, self._impulse_end)
            d = torch.randn(2, B, generator=g, dtype=torch.float64)
            d = d / d.norm(dim=0, keepdim=True)
            mag = torch.rand(B, generator=g, dtype=torch.float64) * scale * self.F_IMPULSE_SCALE
            f = torch.zeros(6, B, dtype=torch.float64)
            f[:2] = d * mag
            f = f.to(self.device)
            # environments whose episode is younger than the first push of the reference's schedule are spared
            young = (t - self._t0) < (self.F_IMPULSE_PERIOD - self.F_IMPULSE_DELTA)
            f = torch.where(young[None, :], torch.zeros_like(f), f)
            self.engine._schedule_impulse_force(self._impulse_frame, t, self.F_IMPULSE_DT, f)
            self._impulse_end = t + self.F_IMPULSE_DT
            self._impulse_index += 1

    def reset_lanes(self, lane_mask: torch.Tensor) -> None:
        q, v = self._state_cache if self._state_cache is not None else self._sample_state(self.num_envs)
        self._on_reset(lane_mask)
        self._randomise_ground(lane_mask)
        self._randomise_flexibility(lane_mask)
        if self._spawn_dz is not None:
            q = q.clone()
            q[2] += self._spawn_dz.to(q.dtype).to(q.device)
        # a fresh episode starts from a zero command like `reset()` (for the PD pipeline it IS the controller's
        # output at the reset state: target = measured position, zero velocity), not from the last command of the
        # finished episode.  With sensor noise / delay configured the first observation of the re-initialised lanes
        # is the raw measurement (their generators and histories restart at the next sensor refresh).
        cmd = self.engine.field("command")
        cmd.copy_(torch.where(lane_mask[None, :], torch.zeros_like(cmd), cmd))
        if self._model_options and "model_lane" in self.engine._fields:
            self.engine.sample_model_biases(lane_mask)     # a new biased model for the new episode (Model::reset)
        if self._f_xy_profile is not None and float(self.std_ratio.get("disturbance", 0.0)) > 0.0:
            for proc in self._f_xy_profile:
                # `func.reset(self.np_random)` of the new episode; drawn by the device generator (all lanes, the masked
                # ones keep the draw): no host normals, no host -> device copy on the auto-reset path
                proc.reset(self._device_generator(), lane_mask=lane_mask)
        self.engine.reset_lanes(lane_mask, q, v)
        self.num_steps.masked_fill_(lane_mask, 0)
        self._t0.copy_(torch.where(lane_mask, self._clock.expand_as(self._t0), self._t0))

    def _device_generator(self) -> torch.Generator:
        g = getattr(self, "_dev_gen", None)
        if g is None:
            g = self._dev_gen = torch.Generator(device=self.device)
            g.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=self._generator)))
        return g

    GROUND_FOOTPRINT_RADIUS = 0.6
    _spawn_dz: Optional[torch.Tensor] = None

    def _randomise_ground(self, lane_mask: Optional[torch.Tensor]) -> None:
        """Ground friction of the environments being reset, ≙ `sample(*GROUND_FRICTION_RANGE,
        scale=std_ratio['ground'], enable_log_scale=True)` (envs/locomotion.py:28, 257-262 with
        utils/misc.py:178-219: 10 ** (mean + dev * U(-1, 1)), mean = 1.1, dev = 0.9 * scale)."""
        if self._ground_patch_extent is not None and self._ground_profile is not None:
            ext = torch.tensor(self._ground_patch_extent, dtype=torch.float64, device=self.device)[:, None]
            off = (torch.rand((2, self.num_envs), generator=self._device_generator(), dtype=torch.float64, device=self.device) * 2.0 - 1.0) * ext
            if lane_mask is not None and "ground_offset" in self.engine._fields:
                off = torch.where(lane_mask[None, :], off, self.engine.field("ground_offset").to(torch.float64))
            self.engine.set_ground_offsets(off)
            # put the robots down ON their patch: base height raised by the highest ground under the footprint
            self._spawn_dz = self.engine.ground_height_around(self._q0[0:2].to(self.device) + off, self.GROUND_FOOTPRINT_RADIUS)
        scale = float(self.std_ratio.get("ground", 0.0))
        if scale <= 0.0:
            return
        lo, hi = 0.2, 2.0
        u = torch.rand(self.num_envs, generator=self._generator, dtype=torch.float64) * 2.0 - 1.0
        mu = (10.0 ** (0.5 * (lo + hi) + 0.5 * scale * (hi - lo) * u)).to(self.dtype).to(self.device)
        if lane_mask is not None and "friction" in self.engine._fields:
            mu = torch.where(lane_mask, mu, self.engine.field("friction")[0])
        self.engine.set_lane_friction(mu)

    FLEX_STIFFNESS_SCALE, FLEX_DAMPING_SCALE = 1000.0, 10.0    # envs/locomotion.py:37-38

    def _randomise_flexibility(self, lane_mask: Optional[torch.Tensor]) -> None:
        """Flexibility parameters of the environments being reset, ≙ `flexibility['stiffness'] += FLEX_STIFFNESS_SCALE *
        sample(scale=std_ratio['model'])`, `flexibility['damping'] += FLEX_DAMPING_SCALE * sample(...)` for every entry of
        `flexibilityConfig` (envs/locomotion.py:288-296; utils/misc.py:178-212: `sample(scale=s)` = U(-s, s)): one draw per
        flexibility joint and environment, added to the three axes alike, around the model's own values (the reference
        starts every episode from the robot options it was built with).  Values are kept non-negative."""
        scale = float(self.std_ratio.get("model", 0.0))
        flex = self.model.flexibility_joint_indices
        if scale <= 0.0 or not flex or self.model.flex_stiffness is None:
            return
        n, B = len(flex), self.num_envs
        k0 = torch.tensor(np.asarray(self.model.flex_stiffness)[flex], dtype=torch.float64)[:, :, None]
        d0 = torch.tensor(np.asarray(self.model.flex_damping)[flex], dtype=torch.float64)[:, :, None]
        u = torch.rand((2, n, 1, B), generator=self._generator, dtype=torch.float64) * 2.0 - 1.0
        k = (k0 + self.FLEX_STIFFNESS_SCALE * scale * u[0]).clamp_min(0.0).to(self.dtype).to(self.device)
        d = (d0 + self.FLEX_DAMPING_SCALE * scale * u[1]).clamp_min(0.0).to(self.dtype).to(self.device)
        if lane_mask is not None and "flexibility" in self.engine._fields:
            old = self.engine.field("flexibility").reshape(n, 2, 3, B)
            k = torch.where(lane_mask[None, None, :], k, old[:, 0])
            d = torch.where(lane_mask[None, None, :], d, old[:, 1])
        self.engine.set_lane_flexibility(k, d)

    # envs/locomotion.py:30-36
    F_IMPULSE_DT, F_IMPULSE_PERIOD, F_IMPULSE_DELTA, F_IMPULSE_SCALE = 10.0e-3, 2.0, 0.25, 1000.0
    F_PROFILE_SCALE, F_PROFILE_WAVELENGTH, F_PROFILE_PERIOD = 50.0, 0.2, 1.0
    _f_xy_profile = None

    def _schedule_disturbances(self) -> None:
        """≙ the disturbance part of `WalkerJiminyEnv._setup` (envs/locomotion.py:298-326): every F_IMPULSE_PERIOD
        seconds (+- F_IMPULSE_DELTA) a horizontal push of random direction and magnitude
        U(0, std_ratio['disturbance'] * F_IMPULSE_SCALE) on the root body, one draw per environment, plus the
        continuous Gaussian-process force of :327-359 (below).

        The reference draws the pushes of a whole episode in episode time at every `_setup`.  Here the environments
        of a batch share the engine clock and its breakpoints while their episodes start at different times
        (auto-reset), so the schedule is periodic in ENGINE time and generated lazily -- only the next push is
        registered (`_refill_impulses`, called before every engine step), whatever `simulation_duration_max` -- and an
        environment is spared by the pushes of the first F_IMPULSE_PERIOD - F_IMPULSE_DELTA seconds of its own
        episode, in which the reference schedules none."""
        scale = float(self.std_ratio.get("disturbance", 0.0))
        self.engine.remove_all_forces()
        self._impulse_frame = None
        if scale <= 0.0 or not self.model.has_freeflyer:
            return
        frame = next(n for n, f in self.model.frames.items() if f.parent_joint == 1)
        g = self._generator
        B = self.num_envs
        self.engine._force_frame_index(frame)    # binds the `applied` field while no simulation is running
        self._impulse_frame = frame if self._disturbance_impulses else None
        self._impulse_index = 1                  # the push of period k starts at k * F_IMPULSE_PERIOD +- delta
        self._impulse_end = 0.0
        # the continuous part (envs/locomotion.py:165-167, 327-359): two periodic Gaussian processes, one realisation
        # per environment, drive the x / y force on the root body: F_PROFILE_SCALE * std_ratio * process(episode time)
        from .processes import PeriodicGaussianProcess
        if self._f_xy_profile is None:
            self._f_xy_profile = [PeriodicGaussianProcess(self.F_PROFILE_WAVELENGTH, self.F_PROFILE_PERIOD, B, self.dtype, self.device),
                                  PeriodicGaussianProcess(self.F_PROFILE_PERIOD, self.F_PROFILE_PERIOD, B, self.dtype, self.device)]
        self._dev_gen = None          # re-seeded from the (just re-seeded) host generator at its next use
        for proc in self._f_xy_profile:
            proc.reset(g)
        if self._disturbance_on_device:
            # lane time (0 at `start` and for the lanes of `reset_lanes`) is the episode time of every environment
            for component, proc in enumerate(self._f_xy_profile):
                # (`adaptive=True`: under `runge_kutta_dopri` the kernels evaluate it at the time of every stage)
                self.engine.register_process_force(frame, proc, component, self.F_PROFILE_SCALE * scale, adaptive=True)
            return

        def profile(t: float, q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
            w = torch.zeros((6, B), dtype=self.dtype, device=self.device)
            tl = t - self._t0
            w[0] = self.F_PROFILE_SCALE * scale * self._f_xy_profile[0](tl)
            w[1] = self.F_PROFILE_SCALE * scale * self._f_xy_profile[1](tl)
            return w
        self.engine.register_profile_force(frame, profile)

    # scales of envs/locomotion.py:40-61 (delay [s]; noise and bias per field)
    SENSOR_DELAY_SCALE = {"EncoderSensor": 3.0e-3, "EffortSensor": 0.0, "ContactSensor": 0.0, "ForceSensor": 0.0,
                          "ImuSensor": 0.0}
    SENSOR_NOISE_SCALE = {"EncoderSensor": (0.0, 0.02), "EffortSensor": (10.0,), "ContactSensor": (2.0, 2.0, 2.0),
                          "ForceSensor": (2.0, 2.0, 2.0, 10.0, 10.0, 10.0),
                          "ImuSensor": (0.0, 0.0, 0.0, 0.01, 0.01, 0.01, 0.2, 0.2, 0.2)}

    def _randomise_sensors(self) -> None:
        """Sensor noise, bias, delay and jitter, ≙ envs/locomotion.py:264-288: for every sensor
        `delay, jitter ~ U(0, s * SENSOR_DELAY_SCALE)`, `bias, noiseStd ~ s * SENSOR_NOISE_SCALE * U(-1, 1)`
        (the reference scales both with the *noise* table; a negative standard deviation is its own business:
        the magnitude is used here).  Called by `reset()` while no simulation is running."""
        scale = float(self.std_ratio.get("sensors", 0.0))
        if scale <= 0.0:
            return
        rg = np.random.default_rng(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=self._generator)))
        any_rng = False
        for stype, table in self.SENSOR_NOISE_SCALE.items():
            n = len(self.model.sensors.get(stype, []))
            if n == 0:
                continue
            sc = scale * np.asarray(table)
            nf = self.engine._SENSOR_FIELDS[stype][1]
            nb = 9 if stype == "ImuSensor" else nf
            bias = rg.uniform(-1.0, 1.0, (n, len(sc))) * sc
            std = np.abs(rg.uniform(-1.0, 1.0, (n, len(sc))) * sc)
            if stype == "ImuSensor":
                # 9 bias entries (rotation, gyro, accel) but 6 measured fields: noise on the last 6
                std = std[:, 3:]
            else:
                bias, std = bias[:, :nb], std[:, :nf]
            dmax = scale * self.SENSOR_DELAY_SCALE[stype]
            delay, jitter = rg.uniform(0.0, dmax, n), rg.uniform(0.0, dmax, n)
            self.engine.set_sensor_options(stype, noise_std=std, bias=bias, delay=delay, jitter=jitter)
            any_rng = True
        if any_rng:
            self.engine.seed_sensors(int(rg.integers(0, 2 ** 31 - 1)))

    def close(self) -> None:
        self.engine.stop()


class WalkerVecEnv(VecJiminyEnv):
    """≙ `WalkerJiminyEnv` (envs/locomotion.py): legged robot with a free-flyer, fall detection
    at half the neutral height and the 'survival' / 'energy' / 'failure' / 'direction' reward mixture.
    `std_ratio['model']` randomises the flexibility stiffness / damping of every environment per episode
    (locomotion.py:288-296, `VecJiminyEnv._randomise_flexibility`)."""

    def __init__(self, *args: Any, reward_mixture: Optional[Dict[str, float]] = None,
                 frame_kinematics: Optional[Dict[str, Any]] = None, terminations: Optional[Dict[str, Any]] = None,
                 locomotion_quantities: Optional[Dict[str, Any]] = None, actuated_joints: Optional[Dict[str, Any]] = None,
                 foot_poses: Optional[Dict[str, Any]] = None, trajectory_tracking: Optional[Dict[str, Any]] = None,
                 trajectory_database: Optional[Dict[str, Any]] = None, tracking_rewards: Optional[Dict[str, Any]] = None,
                 support_polygon: Optional[Dict[str, Any]] = None, reward: Any = None,
                 termination_conditions: Optional[Sequence[Any]] = None, **kw: Any) -> None:
        super().__init__(*args, **kw)
        # the composition layer ≙ `ComposedJiminyEnv(reward=..., terminations=[...])` as ONE launch (`blocks.Composition`, exposed
        # as `composition`) in place of the tensor programs of `has_terminated` / `compute_reward`:
        #   reward=                  a description of `jiminy_amd.compositions`: mixtures over `SurviveReward()`, `RewardTerm`s on
        #                            rows of the caller's own, and the names of the eleven block-backed keys of `reward_mixture`
        #                            (a string, or `RewardTerm(name)`), which require and configure their blocks as the dictionary
        #                            does; exclusive with `reward_mixture`
        #   termination_conditions=  a list, in evaluation order, of `compositions.Termination`s on rows of the caller's own and
        #                            of `(key, spec)` / `(key, spec, dict(is_truncation=..., training_only=...))` with the keys
        #                            and tuples of `terminations`, same bounds and grace periods; exclusive with `terminations`
        # `training` (default True) is the mode `training_only` conditions look at.  The base flags are computed as without the
        # keywords (numerical failure, duration, half the neutral height, `trajectory.out_of_range`, and the dictionary
        # `terminations` where those are given next to `reward=`); a lane they stop evaluates no condition.  `step` adds
        # `info["reward"]` (name -> row of every node, NaN where it was not evaluated), `info["terminated"]` /
        # `info["truncated"]` (the index of the condition that set the flag, -1 elsewhere) and `info["violations"]`.
        self.training = True
        self.composition = None
        if reward is not None and reward_mixture is not None:
            raise ValueError("reward= and reward_mixture= both describe the reward: give one of them")
        if termination_conditions is not None and terminations is not None:
            raise ValueError("termination_conditions= and terminations= both describe the terminations: give one of them")
        self._composed = (reward, None if termination_conditions is None else list(termination_conditions))
        if reward is not None:
            # (the named leaves as the dictionary that requires and configures the same blocks below)
            reward_mixture = {name: 1.0 for name in self._named_reward_terms(reward)}
        if termination_conditions is not None:
            terminations = self._named_terminations(self._composed[1])
        self.reward_mixture = dict(reward_mixture if reward is not None else reward_mixture or {"survival": 1.0})
        # optional `blocks.FrameKinematics` (its constructor's keywords, `frame_names` included), refreshed once per
        # environment step behind the physics and exposed as `frames`; and the first two terminations that read it, or-ed
        # into `has_terminated`:
        #   base_roll_pitch=(low, high, grace_period)  ≙ `BaseRollPitchTermination` (compositions/locomotion.py:318-355)
        #   min_base_height=(value, grace_period)      ≙ `FallingTermination` (:358-398) on `base_relative_height()`
        # a lane terminates when its episode time has reached the grace period and the value has left [low, high]
        # (bases/compositions.py:560-571, 647-663).  With both None nothing of this exists.
        # optional `blocks.LocomotionQuantities` (its constructor's keywords), refreshed behind the frames block, reset with
        # it and exposed as `locomotion`; the terminations and reward terms that read it:
        #   flying=(max_height, grace_period)          ≙ `FlyingTermination` (compositions/locomotion.py:543-579)
        #   impact_force=(max_force_rel, grace_period) ≙ `ImpactForceTermination` (:582-620)
        #   reward_mixture['momentum'] / ['friction']  ≙ `MinimizeAngularMomentumReward` / `MinimizeFrictionReward` (:257-315),
        #                                              weights on the reward rows of the block's `momentum_cutoff` / `friction_cutoff`
        # with an environment-level `ground_profile` pass `locomotion_quantities=dict(ground_profile=True, ...)`: the block then
        # reads the height map and the lanes' patch offsets at every launch (the map is bound in `reset()`, after the block is
        # built); without it the block evaluates the flat formulas on that ground without a word
        # optional `blocks.ActuatedJointQuantities` (its constructor's keywords; `step_dt` is the environment's), reset with the
        # other two blocks, refreshed once per environment step and exposed as `actuation`; what reads it:
        #   mechanical_safety=(position_margin, velocity_max, grace_period)  ≙ `MechanicalSafetyTermination`
        #                                              (compositions/generic.py:505-595): the block's safety count is not zero
        #   power_consumption=(max_power, grace_period) ≙ `MechanicalPowerConsumptionTermination` (:598-661): the average power
        #                                              of the block's `power_horizon`, the instantaneous power without one
        #   reward_mixture['power']                    ≙ `MinimizeMechanicalPowerConsumption` (:153-191), weight on the reward row
        #                                              of the block's `power_cutoff` and `power_horizon`
        # one window per block: the reward and the termination share the block's horizon.
        # optional `blocks.FootPoseQuantities` (its constructor's keywords), reset and refreshed behind the frames block like
        # `locomotion` and exposed as `foot_poses`; the reference of its relative poses is the block's tensor, which the caller
        # fills (`set_reference_from_current`); what reads it:
        #   reward_mixture['foot_positions'] / ['foot_orientations']  ≙ `TrackingFootPositionsReward` /
        #                                              `TrackingFootOrientationsReward` (compositions/locomotion.py:146-214), weights
        #                                              on the reward rows of the block's `position_cutoff` / `orientation_cutoff`
        # optional `blocks.TrackingWindows` (its constructor's keywords but the source blocks, which are the environment's own,
        # and `step_dt`, the environment's), reset and refreshed behind the other four blocks and exposed as `tracking`.  Just
        # before each of its launches the environment calls `_update_tracking_reference(lane_mask)`, where a subclass writes
        # the reference tensors; what reads the block:
        #   drift_odom_position / drift_odom_orientation=(threshold, grace_period)
        #                                              ≙ `DriftTrackingBaseOdometryPositionTermination` / `...OrientationTermination`
        #                                              (compositions/locomotion.py:623-736)
        #   shift_foot_positions / shift_foot_orientations / shift_motor_positions=(threshold, grace_period)
        #                                              ≙ `ShiftTrackingFootOdometryPositionsTermination` / `...OrientationsTermination`
        #                                              (:739-867), `ShiftTrackingMotorPositionsTermination` (compositions/generic.py:
        #                                              664-716); their grace period is max(grace_period, horizon) (:451)
        #   reward_mixture['odom_pose']                ≙ `DriftTrackingBaseOdometryPoseReward` (compositions/locomotion.py:85-120),
        #                                              weight on the reward row of the block's `odometry_cutoff`
        # optional `blocks.ReferenceTrajectory`: `trajectory_database={"dataset": {name: (Trajectory, mode)}, "name": ...,
        # "time_offset_ratio": 0.0}` (≙ `DatasetTrajectoryQuantity`, bases/quantities.py:870-1210; "name": the trajectory every lane
        # starts on, default the first), exposed as `trajectory`.  It is queried at the lanes' episode times at `reset`,
        # `reset_lanes` and after every step, before the foot pose quantities and the tracking windows, and is the source of
        # their references: `tracking.reference_odom_pose` / `reference_position` are written by the query itself, and with
        # `foot_poses` a second frame kinematics block over the foot frames and a second foot pose quantities block evaluate the
        # trajectory's state (on the nominal model) into `foot_poses.reference_relative_pose`.  A lane whose query time leaves a
        # trajectory of mode "raise" is truncated.  `_update_tracking_reference` is still called where it was: a subclass can
        # overwrite what the database wrote.
        # optional `blocks.TrackingRewards`: `tracking_rewards={"base_height_cutoff": ..., "odometry_velocity_cutoff": ...,
        # "capture_point_cutoff": ..., "joint_positions_cutoff": ...}` (each or None), exposed as `tracking_rewards`; needs
        # `trajectory_database`.  With it the reference side is evaluated on the trajectory's state, on the nominal model: one
        # frame kinematics block over the root joint, the contact frames and (with `foot_poses`) the feet where a term reads
        # one, and for the capture point a `blocks.CentroidalState` and a `blocks.LocomotionQuantities(state=...)`, refreshed
        # behind every query.  What reads it:
        #   reward_mixture['base_height'] / ['odometry_velocity'] / ['capture_point'] / ['joint_positions']
        #                                              ≙ `TrackingBaseHeightReward`, `TrackingBaseOdometryVelocityReward`,
        #                                              `TrackingCapturePointReward` (compositions/locomotion.py:33-143),
        #                                              `TrackingActuatedJointPositionsReward` (compositions/generic.py:125-150),
        #                                              weights on the reward rows of the block
        #   reward_mixture['foot_force_distribution'] is refused: a recorded trajectory carries no constraint multipliers.
        # optional `blocks.SupportPolygon` (its constructor's keywords: `cutoff_inner`, `cutoff_outer`, `reference_frame`), reset
        # and refreshed directly behind `locomotion`, which it needs, and exposed as `support`; what reads it:
        #   reward_mixture['robustness']               ≙ `MaximizeRobustness` (toolbox/compositions/locomotion.py:51-115), weight on
        #                                              the reward row of the block's `cutoff_inner` and `cutoff_outer`
        self.frames = self.locomotion = self.actuation = self.foot_poses = self.tracking = None
        self.trajectory = self._reference_frames = self._reference_foot_poses = None
        self.tracking_rewards = self._reference_centroidal = self._reference_locomotion = None
        self.support = None
        self._terminations = dict(terminations or {})
        tracking_terms = {"drift_odom_position": "odometry_horizon", "drift_odom_orientation": "odometry_horizon",
                          "shift_foot_positions": "foot_horizon", "shift_foot_orientations": "foot_horizon",
                          "shift_motor_positions": "motor_horizon"}
        known = ("base_roll_pitch", "min_base_height", "flying", "impact_force", "mechanical_safety", "power_consumption",
                 *tracking_terms)
        unknown = set(self._terminations) - set(known)
        if unknown:
            raise ValueError(f"unknown terminations {sorted(unknown)} ({', '.join(known)})")
        if {"flying", "impact_force"} & set(self._terminations) and locomotion_quantities is None:
            raise ValueError("the flying and impact_force terminations read the locomotion quantities block: give "
                             "locomotion_quantities as well")
        if locomotion_quantities is not None:
            frame_kinematics = {} if frame_kinematics is None else frame_kinematics
            for term, cutoff in (("momentum", "momentum_cutoff"), ("friction", "friction_cutoff")):
                if term in self.reward_mixture and locomotion_quantities.get(cutoff) is None:
                    raise ValueError(f"reward_mixture['{term}'] needs locomotion_quantities['{cutoff}']")
        elif {"momentum", "friction"} & set(self.reward_mixture):
            raise ValueError("the momentum and friction reward terms read the locomotion quantities block: give "
                             "locomotion_quantities as well")
        if support_polygon is not None:
            if locomotion_quantities is None:
                raise ValueError("the support polygon reads the locomotion quantities block: give locomotion_quantities as well")
            if "robustness" in self.reward_mixture and (support_polygon.get("cutoff_inner") is None or
                                                        support_polygon.get("cutoff_outer") is None):
                raise ValueError("reward_mixture['robustness'] needs support_polygon['cutoff_inner'] and "
                                 "support_polygon['cutoff_outer']")
        elif "robustness" in self.reward_mixture:
            raise ValueError("the robustness reward term reads the support polygon block: give support_polygon as well")
        if {"mechanical_safety", "power_consumption"} & set(self._terminations) and actuated_joints is None:
            raise ValueError("the mechanical_safety and power_consumption terminations read the actuated-joint quantities "
                             "block: give actuated_joints as well")
        if actuated_joints is not None:
            actuated_joints = dict(actuated_joints)
            if "power" in self.reward_mixture and (actuated_joints.get("power_cutoff") is None or
                                                   actuated_joints.get("power_horizon") is None):
                raise ValueError("reward_mixture['power'] needs actuated_joints['power_cutoff'] and actuated_joints['power_horizon']")
            if "mechanical_safety" in self._terminations:
                margin, velocity_max, _ = self._terminations["mechanical_safety"]
                given = (actuated_joints.setdefault("position_margin", margin), actuated_joints.setdefault("velocity_max", velocity_max))
                if given != (margin, velocity_max):
                    raise ValueError("the mechanical_safety termination and actuated_joints give different position_margin / "
                                     "velocity_max: the block evaluates one pair")
        elif "power" in self.reward_mixture:
            raise ValueError("the power reward term reads the actuated-joint quantities block: give actuated_joints as well")
        if foot_poses is not None:
            frame_kinematics = {} if frame_kinematics is None else frame_kinematics
            for term, cutoff in (("foot_positions", "position_cutoff"), ("foot_orientations", "orientation_cutoff")):
                if term in self.reward_mixture and foot_poses.get(cutoff) is None:
                    raise ValueError(f"reward_mixture['{term}'] needs foot_poses['{cutoff}']")
        elif {"foot_positions", "foot_orientations"} & set(self.reward_mixture):
            raise ValueError("the foot_positions and foot_orientations reward terms read the foot pose quantities block: give "
                             "foot_poses as well")
        if set(tracking_terms) & set(self._terminations) and trajectory_tracking is None:
            raise ValueError("the drift_odom_* and shift_* terminations read the tracking windows block: give "
                             "trajectory_tracking as well")
        if trajectory_tracking is not None:
            trajectory_tracking = dict(trajectory_tracking)
            for source in ("locomotion", "foot_poses", "actuation", "step_dt"):
                if source in trajectory_tracking:
                    raise ValueError(f"trajectory_tracking takes no '{source}': the source blocks and the step are the environment's")
            for term, horizon in tracking_terms.items():
                if term in self._terminations and trajectory_tracking.get(horizon) is None:
                    raise ValueError(f"the {term} termination needs trajectory_tracking['{horizon}']")
            if "odom_pose" in self.reward_mixture and trajectory_tracking.get("odometry_cutoff") is None:
                raise ValueError("reward_mixture['odom_pose'] needs trajectory_tracking['odometry_cutoff']")
            for horizon, given, keyword in (("odometry_horizon", locomotion_quantities, "locomotion_quantities"),
                                            ("foot_horizon", foot_poses, "foot_poses"),
                                            ("motor_horizon", actuated_joints, "actuated_joints")):
                if trajectory_tracking.get(horizon) is not None and given is None:
                    raise ValueError(f"trajectory_tracking['{horizon}'] reads the block of {keyword}: give {keyword} as well")
        elif "odom_pose" in self.reward_mixture:
            raise ValueError("the odom_pose reward term reads the tracking windows block: give trajectory_tracking as well")
        if "foot_force_distribution" in self.reward_mixture:
            raise NotImplementedError("reward_mixture['foot_force_distribution'] (`TrackingFootForceDistributionReward`): a "
                                      "recorded trajectory carries no constraint multipliers (`State.lambda_c`)")
        reward_terms = ("base_height", "odometry_velocity", "capture_point", "joint_positions")
        if tracking_rewards is not None:
            tracking_rewards = dict(tracking_rewards)
            unknown = set(tracking_rewards) - {f"{term}_cutoff" for term in reward_terms}
            if unknown:
                raise ValueError(f"unknown keys in tracking_rewards: {sorted(unknown)} "
                                 f"({', '.join(f'{term}_cutoff' for term in reward_terms)})")
            for term in reward_terms:
                if term in self.reward_mixture and tracking_rewards.get(f"{term}_cutoff") is None:
                    raise ValueError(f"reward_mixture['{term}'] needs tracking_rewards['{term}_cutoff']")
            if trajectory_database is None or "dataset" not in trajectory_database:
                raise ValueError("tracking_rewards compares with a reference trajectory: give trajectory_database as well")
            on = {term for term in reward_terms if tracking_rewards.get(f"{term}_cutoff") is not None}
            if {"odometry_velocity", "capture_point"} & on and any(
                    getattr(pair[0], "v", None) is None for pair in trajectory_database["dataset"].values() if isinstance(pair, tuple)):
                raise ValueError("tracking_rewards['odometry_velocity_cutoff'] and ['capture_point_cutoff'] need a dataset with v")
            if "joint_positions" in on and actuated_joints is None:
                raise ValueError("tracking_rewards['joint_positions_cutoff'] reads the actuated-joint quantities block: give "
                                 "actuated_joints as well")
            if "capture_point" in on:
                if locomotion_quantities is None:
                    raise ValueError("tracking_rewards['capture_point_cutoff'] reads the locomotion quantities block: give "
                                     "locomotion_quantities as well")
                if locomotion_quantities.get("dcm_reference_frame", "LOCAL") not in ("LOCAL", 0):
                    raise ValueError("tracking_rewards['capture_point_cutoff'] tracks the capture point in the odometry frame: "
                                     "locomotion_quantities['dcm_reference_frame'] must be 'LOCAL'")
            if {"base_height", "odometry_velocity"} & on:
                # (the true side reads the root joint and the contact frames, the velocity their step average)
                frame_kinematics = dict(frame_kinematics or {})
                if "odometry_velocity" in on:
                    frame_kinematics["average"] = True
            self._tracking_rewards_on = on
        elif set(reward_terms) & set(self.reward_mixture):
            raise ValueError("the base_height, odometry_velocity, capture_point and joint_positions reward terms read the "
                             "tracking rewards block: give tracking_rewards as well")
        no_frames = {"mechanical_safety", "power_consumption", *tracking_terms}
        if set(self._terminations) - no_frames and frame_kinematics is None:
            raise ValueError("the terminations read the frame kinematics block: give frame_kinematics as well")
        if frame_kinematics is not None:
            reading = {k: v for k, v in self._terminations.items() if k not in no_frames}
            if foot_poses is None:
                names, modes, cfg = self.frame_kinematics_config(self.model, frame_kinematics, reading, locomotion_quantities)
            else:
                names, modes, cfg = self.frame_kinematics_config(self.model, frame_kinematics, reading, locomotion_quantities, foot_poses)
            if tracking_rewards is not None and {"base_height", "odometry_velocity"} & self._tracking_rewards_on:
                for name in ["root_joint"] + list(self.model.contacts):
                    if name not in names:
                        names.append(name)
                        if modes is not None:
                            modes.append("LOCAL")
            self.frames = blocks.FrameKinematics(self.engine, names, reference_frames=modes, **cfg)
            if foot_poses is not None:
                self.foot_poses = blocks.FootPoseQuantities(self.engine, self.frames, **foot_poses)
            if locomotion_quantities is not None:
                self.engine.enable_output("centroidal")
                self.locomotion = blocks.LocomotionQuantities(self.engine, self.frames, **locomotion_quantities)
                if support_polygon is not None:
                    self.support = blocks.SupportPolygon(self.engine, self.frames, self.locomotion, **support_polygon)
            if set(self._terminations) - no_frames:
                self._frame_root = self.frames.index("root_joint")
                self._frame_contacts = torch.tensor([self.frames.index(n) for n in self.model.contacts], dtype=torch.long, device=self.device)
                if "base_roll_pitch" in self._terminations:
                    # (a bound is one number for both angles or one per angle)
                    low, high, grace = self._terminations["base_roll_pitch"]
                    bound = lambda x: torch.as_tensor(x, dtype=self.dtype, device=self.device).reshape(-1, 1)     # noqa: E731
                    self._roll_pitch_bounds = (bound(low), bound(high), float(grace))
                if "min_base_height" in self._terminations and not self.model.contacts:
                    raise ValueError("min_base_height needs a model with contact frames")
        if actuated_joints is not None:
            self.actuation = blocks.ActuatedJointQuantities(self.engine, step_dt=self.step_dt, **actuated_joints)
        if trajectory_tracking is not None:
            self.tracking = blocks.TrackingWindows(self.engine, locomotion=self.locomotion, foot_poses=self.foot_poses,
                                                   actuation=self.actuation, step_dt=self.step_dt, **trajectory_tracking)
        if trajectory_database is not None:
            cfg = dict(trajectory_database)
            if "dataset" not in cfg:
                raise ValueError("trajectory_database needs 'dataset': {name: (Trajectory, mode)}")
            dataset, name, ratio = cfg.pop("dataset"), cfg.pop("name", None), cfg.pop("time_offset_ratio", 0.0)
            if cfg:
                raise ValueError(f"unknown keys in trajectory_database: {sorted(cfg)} (dataset, name, time_offset_ratio)")
            self.trajectory = blocks.ReferenceTrajectory(self.engine, dataset, actuation=self.actuation)
            self.trajectory.select(self.trajectory.names[0] if name is None else name, None, ratio)
            if self.tracking is not None:
                self.trajectory.bind_references(self.tracking)
            self._trajectory_time = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
            self._trajectory_time_own = None if self.dtype == torch.float64 else torch.zeros_like(self._t0)
            feet = [] if self.foot_poses is None else list(self.foot_poses.foot_frame_names)
            on = self._tracking_rewards_on if tracking_rewards is not None else set()
            if {"base_height", "odometry_velocity", "capture_point"} & on:
                # the reference side: ONE frame kinematics block over the root joint, the contact frames and the feet, and
                # for the capture point the centroidal rows and the locomotion quantities of the trajectory's state; each
                # block exists only where a term reads it
                names = ["root_joint"] + list(self.model.contacts)
                names += [name for name in feet if name not in names]
                self._reference_frames = blocks.FrameKinematics(self.engine, names, compute_velocity=False,
                                                                average="odometry_velocity" in on,
                                                                state=(self.trajectory.q, self.trajectory.v))
                if "capture_point" in on:
                    traj = self.trajectory
                    self._reference_centroidal = blocks.CentroidalState(self.engine, state=(traj.q, traj.v, traj.a))
                    cfg = {k: locomotion_quantities[k] for k in ("foot_frame_names", "zmp_reference_frame", "dcm_reference_frame")
                           if k in locomotion_quantities}
                    self._reference_locomotion = blocks.LocomotionQuantities(
                        self.engine, self._reference_frames, state=(traj.q, self._reference_centroidal), forces=False,
                        momentum=False, **cfg)
            elif self.foot_poses is not None:
                self._reference_frames = blocks.FrameKinematics(self.engine, feet, compute_velocity=False,
                                                                state=(self.trajectory.q, self.trajectory.v))
            if self.foot_poses is not None:
                self._reference_foot_poses = blocks.FootPoseQuantities(self.engine, self._reference_frames, foot_frame_names=feet)
                # (its relative poses ARE the reference of the true side: no copy)
                self._reference_foot_poses.relative_pose = self.foot_poses.reference_relative_pose
            if tracking_rewards is not None:
                reads_frames = bool({"base_height", "odometry_velocity"} & on)
                self.tracking_rewards = blocks.TrackingRewards(
                    self.engine, frames=self.frames if reads_frames else None,
                    reference_frames=self._reference_frames if reads_frames else None,
                    locomotion=self.locomotion if "capture_point" in on else None,
                    reference_locomotion=self._reference_locomotion if "capture_point" in on else None,
                    actuation=self.actuation if "joint_positions" in on else None,
                    trajectory=self.trajectory if "joint_positions" in on else None, **tracking_rewards)
        if reward is not None or termination_conditions is not None:
            self._build_composition()
        m = self.model
        lim = torch.tensor([mo.effort_limit * mo.velocity_limit for mo in m.motors], dtype=self.dtype)
        self._power_consumption_max = float(lim.sum())  # locomotion.py:230-236
        # encoder of every motor (the reference indexes the encoder data through `encoder_to_motor_map`)
        enc_of = {e.get("motor_index", -1): i for i, e in enumerate(m.sensors.get("EncoderSensor", []))}
        self._motor_enc_idx = (torch.tensor([enc_of[i] for i in range(m.nmotors)], device=self.device)
                               if all(i in enc_of for i in range(m.nmotors)) and m.nmotors else None)

        # 'direction' (locomotion.py:419-424): mean of the logged free-flyer Y position over the episode, per environment.
        # The reference's log holds one row per integrator step; here the position is sampled once per environment step
        # (what a launch makes visible) plus the initial state, accumulated on the device.
        self._dir_sum = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
        self._dir_n = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)

    # the block-backed keys of `reward_mixture`, and the keys of `terminations`
    COMPOSED_REWARD_TERMS = ("momentum", "friction", "power", "foot_positions", "foot_orientations", "odom_pose", "base_height",
                             "odometry_velocity", "capture_point", "joint_positions", "robustness")

    @classmethod
    def _named_reward_terms(cls, reward: Any) -> list:
        """The names of the leaves of a reward description that stand for a reward row of the environment."""
        from . import compositions
        names: list = []

        def walk(c: Any) -> None:
            if isinstance(c, compositions.RewardTerm):
                if c.row is None:
                    if c.name not in cls.COMPOSED_REWARD_TERMS:
                        raise ValueError(f"unknown reward term '{c.name}' ({', '.join(cls.COMPOSED_REWARD_TERMS)}): a term of "
                                         "the caller's own is a RewardTerm on a row")
                    names.append(c.name)
            elif hasattr(c, "components"):
                for component in c.components:
                    walk(component)
            elif not isinstance(c, compositions.SurviveReward):
                raise TypeError(f"reward= expects a description of jiminy_amd.compositions, got {type(c).__name__}")
        walk(reward)
        return names

    @staticmethod
    def _named_terminations(conditions: list) -> Dict[str, Any]:
        """The named entries of `termination_conditions` as the dictionary `terminations` would be."""
        from . import compositions
        named: Dict[str, Any] = {}
        for entry in conditions:
            if isinstance(entry, compositions.Termination):
                if entry.rows is None:
                    raise ValueError(f"termination '{entry.name}' has no rows: a condition of the environment is given as "
                                     "(key, spec), with the tuple `terminations` takes")
                continue
            if not isinstance(entry, tuple) or len(entry) not in (2, 3) or not isinstance(entry[0], str):
                raise TypeError("termination_conditions expects compositions.Termination or (key, spec[, options]) entries")
            if len(entry) == 3 and set(entry[2]) - {"is_truncation", "training_only"}:
                raise ValueError(f"unknown options of the termination '{entry[0]}': {sorted(entry[2])} (is_truncation, training_only)")
            if entry[0] in named:
                raise ValueError(f"the termination '{entry[0]}' is given twice")
            named[entry[0]] = entry[1]
        return named

    def _build_composition(self) -> None:
        """`blocks.Composition` over the rows the named entries stand for and the caller's own."""
        import copy

        from . import compositions
        reward, conditions = self._composed

        def resolve(c: Any) -> Any:
            if isinstance(c, compositions.RewardTerm) and c.row is None:
                rows = dict(momentum=lambda: self.locomotion.reward_momentum, friction=lambda: self.locomotion.reward_friction,
                            power=lambda: self.actuation.reward_power, foot_positions=lambda: self.foot_poses.reward_foot_positions,
                            foot_orientations=lambda: self.foot_poses.reward_foot_orientations,
                            odom_pose=lambda: self.tracking.reward_odom_pose, robustness=lambda: self.support.reward_robustness)
                row = rows[c.name]() if c.name in rows else self.tracking_rewards.reward(c.name)
                return compositions.RewardTerm(c.name, row, is_normalized=c.is_normalized, is_terminal=c.is_terminal)
            if hasattr(c, "components"):
                c = copy.copy(c)
                c.components = tuple(resolve(component) for component in c.components)
            return c

        terminations = []
        for entry in conditions or ():
            if isinstance(entry, compositions.Termination):
                terminations.append(entry)
                continue
            key, spec, options = entry[0], self._terminations[entry[0]], dict(entry[2]) if len(entry) == 3 else {}
            grace, low, high = float(spec[-1]), None, None
            if key == "base_roll_pitch":
                rows, low, high = self.frames.rpy[:2, self._frame_root], self._roll_pitch_bounds[0].reshape(-1), self._roll_pitch_bounds[1].reshape(-1)
            elif key == "min_base_height":
                # (a value of the environment's own: written in front of every launch)
                self._base_height = torch.zeros(self.num_envs, dtype=self.dtype, device=self.device)
                rows, low = self._base_height, spec[0]
            elif key == "flying":
                rows, high = self.locomotion.ground_distance_min, spec[0]
            elif key == "impact_force":
                rows, high = self.locomotion.force_vertical_max, spec[0]
            elif key == "mechanical_safety":
                rows, high = self.actuation.safety, 0
            elif key == "power_consumption":
                act = self.actuation
                rows, high = act.power_average if act.plan.has_horizon else act.power, spec[0]      # (compositions/generic.py:640-650)
            else:
                rows, high = getattr(self.tracking, key), spec[0]
                if key.startswith("shift_"):
                    horizon = "motor_horizon" if key == "shift_motor_positions" else "foot_horizon"
                    grace = max(grace, getattr(self.tracking, horizon))       # (compositions/generic.py:451)
            terminations.append(compositions.Termination(key, rows, low, high, grace, **options))
        self._composition_time = torch.zeros(self.num_envs, dtype=self.dtype, device=self.device)
        self.composition = blocks.Composition(self.engine, None if reward is None else resolve(reward), terminations)

    @staticmethod
    def frame_kinematics_config(model: CompiledModel, frame_kinematics: Dict[str, Any], terminations: Dict[str, Any],
                                locomotion_quantities: Optional[Dict[str, Any]] = None,
                                foot_poses: Optional[Dict[str, Any]] = None) -> Tuple[list, Optional[list], Dict[str, Any]]:
        """Frame names, reference frames and remaining keywords of the `blocks.FrameKinematics` of an environment: the
        user's, plus what the terminations and the locomotion quantities read where it is missing -- the root joint and
        every contact frame (LOCAL), the Euler angles for `base_roll_pitch` and the step average for the angular momentum; with
        `foot_poses` (the keywords of the foot pose quantities block) the foot frames (LOCAL) as well."""
        cfg = dict(frame_kinematics)
        names = list(cfg.pop("frame_names", ()))
        modes = cfg.pop("reference_frames", None)
        modes = None if modes is None else list(modes)
        if modes is not None and len(modes) != len(names):
            raise ValueError(f"expected one reference frame per frame ({len(names)}), got {len(modes)}")
        if terminations or locomotion_quantities is not None:
            for name in ["root_joint"] + list(model.contacts):
                if name not in names:
                    names.append(name)
                    if modes is not None:
                        modes.append("LOCAL")
            if "base_roll_pitch" in terminations:
                cfg["compute_rpy"] = True
            if locomotion_quantities is not None and locomotion_quantities.get("momentum", True):
                cfg["average"] = True
        if foot_poses is not None:
            from .locomotion import sanitize_foot_frame_names
            for name in sanitize_foot_frame_names(model, foot_poses.get("foot_frame_names", "auto")):
                if name not in names:
                    names.append(name)
                    if modes is not None:
                        modes.append("LOCAL")
        return names, modes, cfg

    def _direction_restart(self, lane_mask: Optional[torch.Tensor]) -> None:
        y0 = self.engine.robot_state.q[1].to(torch.float64)
        if lane_mask is None:
            self._dir_sum.copy_(y0)
            self._dir_n.fill_(1.0)
        else:
            self._dir_sum.copy_(torch.where(lane_mask, y0, self._dir_sum))
            self._dir_n.copy_(torch.where(lane_mask, torch.ones_like(self._dir_n), self._dir_n))

    def _update_tracking_reference(self, lane_mask: Optional[torch.Tensor]) -> None:
        """Called just before every launch of the tracking windows block: with the mask of `reset_lanes` before a restart of
        those lanes, with None before the restart of every lane (`reset`) and before the push of a step.  The place where a
        subclass writes the reference tensors of `tracking` (and of `foot_poses`), for instance gathered from a trajectory
        by the step count of every lane.  Nothing by default: the references stay what the caller wrote."""

    def select_trajectory(self, name_or_indices, lane_mask: Optional[torch.Tensor] = None, time_offset_ratio=0.0) -> None:
        """≙ `DatasetTrajectoryQuantity.select`: forwards to `trajectory.select`; the next query reads the selection."""
        if self.trajectory is None:
            raise RuntimeError("select_trajectory needs trajectory_database")
        self.trajectory.select(name_or_indices, lane_mask, time_offset_ratio)

    def _query_trajectory(self, lane_mask: Optional[torch.Tensor], step: bool = False) -> None:
        """The reference state of the (masked) lanes at their episode time, and what the reference-side blocks make of it.
        `step`: the query behind an environment step, which the step average of the reference frames advances over; any other
        query restarts it."""
        if self._trajectory_time_own is None:
            torch.sub(self._clock, self._t0, out=self._trajectory_time)
        else:
            torch.sub(self._clock, self._t0, out=self._trajectory_time_own)
            self._trajectory_time.copy_(self._trajectory_time_own)
        self.trajectory.query(self._trajectory_time, lane_mask)
        if self._reference_frames is not None:
            averaged = self._reference_frames.average
            if lane_mask is None and (step or not averaged):
                self._reference_frames.refresh()
                if averaged:
                    self._reference_frames.refresh_average(self.step_dt)
            else:
                self._reference_frames.reset(lane_mask)
            if self._reference_foot_poses is not None:
                if lane_mask is None:
                    self._reference_foot_poses.refresh()
                else:
                    self._reference_foot_poses.reset(lane_mask)
        if self._reference_centroidal is not None:
            for blk in (self._reference_centroidal, self._reference_locomotion):
                if lane_mask is None:
                    blk.refresh()
                else:
                    blk.reset(lane_mask)

    def reset(self, seed: Optional[int] = None, options: Optional[Dict[str, Any]] = None):
        out = super().reset(seed, options)
        self._direction_restart(None)
        if self.frames is not None:
            self.frames.reset(None)
        if self.locomotion is not None:
            self.locomotion.reset(None)
        if self.support is not None:
            self.support.reset(None)
        if self.trajectory is not None:
            self._query_trajectory(None)
        if self.foot_poses is not None:
            self.foot_poses.reset(None)
        if self.actuation is not None:
            self.actuation.reset(None)
        if self.tracking is not None:
            self._update_tracking_reference(None)
            self.tracking.reset(None)
        if self.tracking_rewards is not None:
            self.tracking_rewards.reset(None)
        return out

    def reset_lanes(self, lane_mask: torch.Tensor) -> None:
        super().reset_lanes(lane_mask)
        self._direction_restart(lane_mask)
        if self.frames is not None:
            self.frames.reset(lane_mask)
        if self.locomotion is not None:
            self.locomotion.reset(lane_mask)
        if self.support is not None:
            self.support.reset(lane_mask)
        if self.trajectory is not None:
            self._query_trajectory(lane_mask)
        if self.foot_poses is not None:
            self.foot_poses.reset(lane_mask)
        if self.actuation is not None:
            self.actuation.reset(lane_mask)
        if self.tracking is not None:
            self._update_tracking_reference(lane_mask)
            self.tracking.reset(lane_mask)
        if self.tracking_rewards is not None:
            self.tracking_rewards.reset(lane_mask)

    def _after_step(self):
        self._dir_sum += self.engine.robot_state.q[1].to(torch.float64)
        self._dir_n += 1.0
        if self.frames is not None:
            self.frames.refresh()
            if self.frames.average:
                self.frames.refresh_average(self.step_dt)
        if self.locomotion is not None:
            self.locomotion.refresh()
        if self.support is not None:
            self.support.refresh()
        if self.trajectory is not None:
            self._query_trajectory(None, step=True)
        if self.foot_poses is not None:
            self.foot_poses.refresh()
        if self.actuation is not None:
            self.actuation.refresh()
        if self.tracking is not None:
            self._update_tracking_reference(None)
            self.tracking.refresh()
        if self.tracking_rewards is not None:
            self.tracking_rewards.refresh()
        return super()._after_step()

    def base_relative_height(self) -> torch.Tensor:
        """≙ `BaseRelativeHeight` (quantities/locomotion.py:88-97, 153-154): height of the root joint over the lowest contact
        frame, per lane, from the poses of the frame kinematics block."""
        if self.frames is None or not self._terminations:
            raise RuntimeError("base_relative_height needs frame_kinematics and terminations")
        z = self.frames.pose[2]
        return z[self._frame_root] - z[self._frame_contacts].min(0).values

    def has_terminated(self) -> Tuple[torch.Tensor, torch.Tensor]:
        terminated, truncated = super().has_terminated()
        z = self.engine.robot_state.q[2]
        terminated = terminated | (z < 0.5 * self._height_neutral)  # locomotion.py:381-383
        if self.trajectory is not None:
            truncated = truncated | self.trajectory.out_of_range        # (the reference raises "Query time out-of-range.")
        if self._terminations and self._composed[1] is None:
            t = self._lane_time()
            if "base_roll_pitch" in self._terminations:
                low, high, grace = self._roll_pitch_bounds
                rp = self.frames.rpy[:2, self._frame_root]
                terminated = terminated | ((t >= grace) & ((rp < low) | (rp > high)).any(0))
            if "min_base_height" in self._terminations:
                value, grace = self._terminations["min_base_height"]
                terminated = terminated | ((t >= grace) & (self.base_relative_height() < value))
            if "flying" in self._terminations:
                max_height, grace = self._terminations["flying"]
                terminated = terminated | ((t >= grace) & (self.locomotion.ground_distance_min > max_height))
            if "impact_force" in self._terminations:
                max_force_rel, grace = self._terminations["impact_force"]
                terminated = terminated | ((t >= grace) & (self.locomotion.force_vertical_max > max_force_rel))
            if "mechanical_safety" in self._terminations:
                grace = self._terminations["mechanical_safety"][2]
                terminated = terminated | ((t >= grace) & (self.actuation.safety > 0))
            if "power_consumption" in self._terminations:
                max_power, grace = self._terminations["power_consumption"]
                act = self.actuation
                value = act.power_average if act.plan.has_horizon else act.power      # (compositions/generic.py:640-650)
                terminated = terminated | ((t >= grace) & (value > max_power))
            for term in ("drift_odom_position", "drift_odom_orientation"):
                if term in self._terminations:
                    threshold, grace = self._terminations[term]
                    terminated = terminated | ((t >= grace) & (getattr(self.tracking, term) > threshold))
            for term, horizon in (("shift_foot_positions", "foot_horizon"), ("shift_foot_orientations", "foot_horizon"),
                                  ("shift_motor_positions", "motor_horizon")):
                if term in self._terminations:
                    threshold, grace = self._terminations[term]
                    grace = max(grace, getattr(self.tracking, horizon))       # (compositions/generic.py:451)
                    terminated = terminated | ((t >= grace) & (getattr(self.tracking, term) > threshold))
        if self.composition is not None:
            # the flags so far are those of the environment below; one launch gives the composed flags and the reward
            if getattr(self, "_base_height", None) is not None:
                torch.sub(self.frames.pose[2, self._frame_root], self.frames.pose[2, self._frame_contacts].min(0).values, out=self._base_height)
            torch.sub(self._clock, self._t0, out=self._composition_time)
            block = self.composition
            self._composition_base = (terminated.contiguous(), truncated.contiguous())       # (what the launch reads)
            block.refresh(self._composition_time, *self._composition_base, training=self.training)
            terminated, truncated = block.terminated.bool(), block.truncated.bool()
        return terminated, truncated

    def step(self, action: torch.Tensor):
        obs, reward, terminated, truncated, info = super().step(action)
        block = self.composition
        if block is not None:
            none = torch.full_like(block.trigger, -1)
            info["reward"] = block.info()
            info["terminated"] = torch.where(block.terminated.bool(), block.trigger, none)
            info["truncated"] = torch.where(block.truncated.bool(), block.trigger, none)
            info["violations"] = block.violations
        return obs, reward, terminated, truncated, info

    def compute_reward(self, terminated: torch.Tensor) -> torch.Tensor:
        if self._composed[0] is not None:
            return self.composition.reward
        total = torch.zeros(self.num_envs, dtype=self.dtype, device=self.device)
        if "survival" in self.reward_mixture:
            total += self.reward_mixture["survival"]
        if "energy" in self.reward_mixture:
            if self._motor_enc_idx is None:
                raise RuntimeError("the 'energy' reward needs one motor-side encoder per motor")
            enc = self.engine.sensor_measurements["EncoderSensor"]  # (2, n_enc, B), encoder order
            power = torch.clamp_min(self.engine.command * enc[1][self._motor_enc_idx], 0.0).sum(0)
            total -= self.reward_mixture["energy"] * power / self._power_consumption_max
        if "failure" in self.reward_mixture:
            total -= self.reward_mixture["failure"] * terminated.to(self.dtype)
        if "direction" in self.reward_mixture:
            # at termination only: minus the absolute mean lateral position of the episode (locomotion.py:419-424)
            drift = (self._dir_sum / torch.clamp_min(self._dir_n, 1.0)).abs().to(self.dtype)
            total -= self.reward_mixture["direction"] * drift * terminated.to(self.dtype)
        if "momentum" in self.reward_mixture:
            total += self.reward_mixture["momentum"] * self.locomotion.reward_momentum
        if "friction" in self.reward_mixture:
            total += self.reward_mixture["friction"] * self.locomotion.reward_friction
        if "power" in self.reward_mixture:
            total += self.reward_mixture["power"] * self.actuation.reward_power
        if "foot_positions" in self.reward_mixture:
            total += self.reward_mixture["foot_positions"] * self.foot_poses.reward_foot_positions
        if "foot_orientations" in self.reward_mixture:
            total += self.reward_mixture["foot_orientations"] * self.foot_poses.reward_foot_orientations
        if "odom_pose" in self.reward_mixture:
            total += self.reward_mixture["odom_pose"] * self.tracking.reward_odom_pose
        for term in ("base_height", "odometry_velocity", "capture_point", "joint_positions"):
            if term in self.reward_mixture:
                total += self.reward_mixture[term] * self.tracking_rewards.reward(term)
        if "robustness" in self.reward_mixture:
            total += self.reward_mixture["robustness"] * self.support.reward_robustness
        return total


class PDControlledWalkerVecEnv(WalkerVecEnv):
    """Walker with the reference's low-level pipeline on device (gym_jiminy/envs/anymal.py:82-127):
    `PDAdapter` (order 1: the action is the target motor velocity) -> `PDController` (ZOH command
    integrator + PD law, run at the controller period) and a `MahonyFilter` observer per IMU.

    The engine advances one controller period per launch; the command is refreshed between
    launches from the encoder rows written by the previous launch, like the reference's
    `_controller_handle` called from `Engine::step` at each controller breakpoint.
    """

    def __init__(self, model: CompiledModel, num_envs: int, step_dt: float, control_dt: float,
                 kp: Any, kd: Any, mahony_kp: float = 1.0, mahony_ki: float = 0.1,
                 joint_position_margin: float = 0.0, joint_velocity_limit: float = float("inf"),
                 joint_acceleration_limit: Optional[float] = None,
                 safety_limit: Optional[Dict[str, float]] = None,
                 deformation_estimator: Optional[Dict[str, Any]] = None,
                 mahony_filter: Optional[Dict[str, Any]] = None, body_observer: Optional[Dict[str, Any]] = None,
                 **kw: Any) -> None:
        opts = kw.pop("engine_options", None) or {}
        st = dict(opts.get("stepper", {}))
        st.setdefault("controllerUpdatePeriod", control_dt)
        st.setdefault("sensorsUpdatePeriod", control_dt)
        opts = dict(opts, stepper=st)
        super().__init__(model, num_envs, step_dt, engine_options=opts, **kw)
        self.control_dt = float(control_dt)
        self._n_ctrl = int(round(step_dt / control_dt))
        if abs(self._n_ctrl * control_dt - step_dt) > 1e-9:
            raise ValueError("step_dt must be a multiple of the controller period")
        M, B, dev, dt_ = model.nmotors, self.num_envs, self.device, self.dtype
        # encoders in motor order
        enc_of = {e["motor_index"]: i for i, e in enumerate(model.sensors["EncoderSensor"])
                  if e["motor_index"] >= 0}
        if sorted(enc_of) != list(range(M)):
            raise ValueError("the PD pipeline needs one motor-side encoder per motor")
        self._enc_idx = torch.tensor([enc_of[i] for i in range(M)], device=dev)
        self.kp = torch.as_tensor(kp, dtype=dt_, device=dev)
        self.kd = torch.as_tensor(kd, dtype=dt_, device=dev)
        self.effort_limit = torch.tensor([m.effort_limit for m in model.motors], dtype=dt_, device=dev)
        # command-state bounds of `PDController.__init__` (proportional_derivative_controller.py:405-437):
        # motor-side position limits shrunk by the margin, velocity min(motor limit, reduction * joint limit),
        # acceleration reduction * joint limit -- or, without one, the largest that still allows bang-bang control
        red = np.array([m.reduction for m in model.motors])
        p_lo = np.array([model.position_lower[m.idx_q] * m.reduction for m in model.motors]) + red * joint_position_margin
        p_hi = np.array([model.position_upper[m.idx_q] * m.reduction for m in model.motors]) - red * joint_position_margin
        v_lim = np.minimum(np.array([m.velocity_limit for m in model.motors]), red * joint_velocity_limit)
        if joint_acceleration_limit is None:
            kp_, kd_ = np.broadcast_to(np.asarray(kp, dtype=float), (M,)), np.broadcast_to(np.asarray(kd, dtype=float), (M,))
            eff = np.array([m.effort_limit for m in model.motors])
            a_lim = np.minimum(2.0 * v_lim / step_dt, eff / (kp_ * step_dt * np.maximum(step_dt, kd_)))
        else:
            a_lim = red * float(joint_acceleration_limit)
        lo = torch.tensor(np.stack([p_lo, -v_lim, -a_lim]), dtype=dt_, device=dev)
        hi = torch.tensor(np.stack([p_hi, v_lim, a_lim]), dtype=dt_, device=dev)
        self.command_state_lower, self.command_state_upper = lo, hi
        self.command_state = torch.zeros((3, M, B), dtype=dt_, device=dev)
        self._accel = torch.zeros((M, B), dtype=dt_, device=dev)
        self._torque = torch.zeros((M, B), dtype=dt_, device=dev)
        n_imu = len(model.sensors["ImuSensor"])
        self.mahony_kp, self.mahony_ki = float(mahony_kp), float(mahony_ki)
        self.imu_quat = torch.zeros((4, n_imu, B), dtype=dt_, device=dev)
        self.imu_quat[3] = 1.0
        self._bias = torch.zeros((3, n_imu, B), dtype=dt_, device=dev)
        self._omega = torch.zeros_like(self._bias)
        self._cf = torch.zeros_like(self._bias)
        # per-tick blocks as single HIP launches (JIMINY_AMD_TENSOR_BLOCKS=1 selects the tensor
        # programs of blocks.py instead: A/B measurements and debugging only)
        import os
        self._hip_blocks = None
        if os.environ.get("JIMINY_AMD_TENSOR_BLOCKS", "0") != "1":
            self._hip_blocks = blocks.HipBlocks(self.engine, self._enc_idx, lo, hi, self.kp, self.kd,
                                                self.effort_limit)
        # optional `MotorSafetyLimit` between the PD controller and the motors (gym_jiminy blocks/motor_safety_limit.py:
        # 81-175; Atlas: kp = 1 / MOTOR_POSITION_MARGIN, kd = MOTOR_VELOCITY_SAFE_GAIN): motor-side soft bounds
        self._safety = None
        if safety_limit is not None:
            if self._hip_blocks is None:
                raise NotImplementedError("the motor safety limit runs as a HIP block")
            margin = float(safety_limit.get("soft_position_margin", 0.0))
            vmax = float(safety_limit["soft_velocity_max"])
            if margin < 0.0 or vmax < 0.0:
                raise ValueError("Soft position margin and soft maximum velocity must be positive.")
            self._safety = dict(
                kp=np.full(M, float(safety_limit["kp"])), kd=np.full(M, float(safety_limit["kd"])),
                lo=np.array([model.position_lower[m.idx_q] * m.reduction for m in model.motors]) + red * margin,
                hi=np.array([model.position_upper[m.idx_q] * m.reduction for m in model.motors]) - red * margin,
                vlim=np.minimum(np.array([m.velocity_limit for m in model.motors]), red * vmax))

        # optional full `MahonyFilter` block (gym_jiminy blocks/mahony_filter.py:104-393) in place of the bare filter function:
        # `dict(ignore_twist=False, exact_init=True, kp=mahony_kp, ki=mahony_ki, compute_rpy=False, update_ratio=1 | -1)`, and
        # behind it the optional `BodyObserver` (blocks/body_orientation_observer.py): `dict(twist_time_constant=None,
        # compute_rpy=True, update_ratio=1 | -1)`.  Their state replaces `imu_quat` / `_bias` / `_omega` / `_cf`, so that
        # whatever reads the attitude estimates (the deformation estimator, `_pipeline_sum`) reads the same tensors as before.
        self._mahony = self._body = None
        if body_observer is not None and mahony_filter is None:
            raise ValueError("body_observer reads the estimates of the MahonyFilter block: give mahony_filter as well")
        if mahony_filter is not None:
            if self._hip_blocks is None:
                raise NotImplementedError("the MahonyFilter / BodyObserver blocks run as HIP blocks")

            def block_config(name: str, given: Dict[str, Any]) -> Tuple[Dict[str, Any], bool]:
                cfg = dict(given)
                ratio = int(cfg.pop("update_ratio", 1))
                if ratio not in (1, -1):
                    raise NotImplementedError(f"{name}: update_ratio must be 1 (every controller tick) or -1 "
                                              "(every environment step)")
                return cfg, ratio == 1
            cfg, self._mahony_every_tick = block_config("mahony_filter", mahony_filter)
            cfg.setdefault("kp", self.mahony_kp)
            cfg.setdefault("ki", self.mahony_ki)
            self._mahony = blocks.MahonyFilter(self.engine, **cfg)
            self.imu_quat, self._bias = self._mahony.quat, self._mahony.bias
            self._omega, self._cf = self._mahony.omega, self._mahony._cf
            if body_observer is not None:
                cfg, self._body_every_tick = block_config("body_observer", body_observer)
                self._body = blocks.BodyObserver(self.engine, self._mahony, **cfg)

        # optional `DeformationEstimator` observer behind the Mahony filter (gym_jiminy blocks/deformation_estimator.py):
        # `dict(imu_frame_names=..., flex_frame_names=..., ignore_twist=True, compute_rpy=True, update_ratio=1 | -1)`; it reads
        # `imu_quat` after the filter of every controller tick (`update_ratio` 1) or once per environment step (-1)
        self._deform = None
        if deformation_estimator is not None:
            if self._hip_blocks is None:
                raise NotImplementedError("the deformation estimator runs as a HIP block")
            cfg = dict(deformation_estimator)
            ratio = int(cfg.pop("update_ratio", 1))
            if ratio not in (1, -1):
                raise NotImplementedError("deformation_estimator: update_ratio must be 1 (every controller tick) or -1 "
                                          "(every environment step)")
            self._deform = blocks.DeformationEstimator(self.engine, **cfg)
            self._deform_every_tick = ratio == 1

    def _encoders(self) -> torch.Tensor:
        enc = self.engine.sensor_measurements["EncoderSensor"]   # (2, n_enc, B)
        return enc[:, self._enc_idx]

    def _pipeline_sum(self) -> Any:
        # (an infinite IMU sample of a lane that is about to fail poisons its attitude estimate one step before its state)
        return self.imu_quat.sum((0, 1))

    def _on_reset(self, lane_mask: Optional[torch.Tensor]) -> None:
        q0, _ = self._state_cache if self._state_cache is not None else self._sample_state(self.num_envs)
        if lane_mask is None or getattr(self, "_target_cache", None) is None:
            self._target_cache = torch.stack([q0[m.idx_q] * m.reduction for m in self.model.motors])
        target = self._target_cache
        if lane_mask is None:
            self._graph = None      # a full reset restarts the engine: the step graph is captured again
            self.command_state.zero_()
            self.command_state[0] = target
            self.imu_quat.zero_(); self.imu_quat[3] = 1.0
            self._bias.zero_()
        else:
            # by selection, never by arithmetic: a lane truncated for JM_LANE_NAN carries NaN in its controller /
            # observer state, and NaN * 0 stays NaN
            m = lane_mask[None, None, :]
            fresh = torch.zeros_like(self.command_state)
            fresh[0] = target
            self.command_state.copy_(torch.where(m, fresh, self.command_state))
            unit = torch.zeros_like(self.imu_quat)
            unit[3] = 1.0
            self.imu_quat.copy_(torch.where(m, unit, self.imu_quat))
            for t in (self._bias, self._omega, self._cf):
                t.copy_(torch.where(m, torch.zeros_like(t), t))
            for t in (self._accel, self._torque):
                t.copy_(torch.where(lane_mask[None, :], torch.zeros_like(t), t))
        if self._deform is not None:
            self._deform.reset(lane_mask)

    def _init_observers(self, lane_mask: Optional[torch.Tensor]) -> None:
        """The first refresh of an episode (mahony_filter.py:340-374), from the state and the IMU rows the engine's `start` /
        `reset_lanes` just wrote."""
        if self._mahony is not None:
            self._mahony.reset(lane_mask)
            if self._body is not None:
                self._body.reset(lane_mask)

    # (not in `_on_reset`: that hook runs before the engine's `start` / `reset_lanes`, and the initialisation reads the `q`
    # and IMU rows they write.  The auto-reset of `step` goes through `self.reset_lanes`, so it is covered as well.)
    def reset(self, seed: Optional[int] = None, options: Optional[Dict[str, Any]] = None):
        out = super().reset(seed, options)
        if self._mahony is None:
            return out
        self._init_observers(None)
        return self.observation(), out[1]

    def reset_lanes(self, lane_mask: torch.Tensor) -> None:
        super().reset_lanes(lane_mask)
        self._init_observers(lane_mask)

    # ------------------------------------------------------------------ HIP-graph replay of one environment step
    def enable_graph(self, enable: bool = True, whole_step: bool = False) -> None:
        """Replay the launches of one environment step -- PD adapter, then per controller tick PD controller -> physics
        launch -> Mahony filter: 26 launches for ANYmal -- as ONE captured HIP graph instead of issuing them from
        Python.  For small batches per GPU (a sharded config 4 / 5: a few thousand environments) the step is bound by
        the host's launch rate, not by the kernels; at B = 65 536 it makes no difference.  Needs the HIP blocks, a
        fixed-step solver, no sensor noise / delay and no applied forces whose schedule runs on the host between the
        launches: impulses and callable profiles.  Process forces (`disturbance_on_device=True` with
        `disturbance_impulses=False`) are part of the captured kernels -- they read the lane time and the process tables
        from device memory -- and replay like the rest.  The graph is captured at the next `step` and dropped by `reset`.

        `whole_step=True` captures the WHOLE `env.step`: the physics chain, the episode clock, termination / truncation,
        the reward and an unconditional masked auto-reset (`reset_lanes` with the `done` mask: lanes that are not done
        leave its launches at once) -- no host read-back at all (`bool(done.any())` of the eager step is the one
        synchronisation per environment step).  `step` then returns static tensors (`reward`, `terminated`, `truncated`,
        `info["reset_mask"]`) that the next `step` overwrites.  Additionally needs `auto_reset`, no ground-friction
        randomisation and the deterministic default state sampler (model biases are fine: drawn on the device)."""
        if enable:
            eng = self.engine
            if self._hip_blocks is None or eng._adaptive is not None or eng._sensor_noise or eng._impulse_forces or eng._profile_forces \
                    or getattr(self, "_impulse_frame", None) is not None:
                raise NotImplementedError("enable_graph needs the HIP blocks, a fixed-step solver, noiseless sensors and "
                                          "no applied forces but process forces (disturbance_on_device=True, "
                                          "disturbance_impulses=False)")
            if whole_step and (not self.auto_reset or float(self.std_ratio.get("ground", 0.0)) > 0.0 or
                               self._ground_patch_extent is not None):
                raise NotImplementedError("whole-step graphs need auto_reset and no ground-friction / terrain-patch randomisation")
            if whole_step and self.frames is not None:
                raise NotImplementedError("whole-step graphs do not take the frame kinematics block: its reset is not part "
                                          "of the captured step")
            if whole_step and self.actuation is not None:
                raise NotImplementedError("whole-step graphs do not take the actuated-joint quantities block: the restart of "
                                          "its windows at reset is not part of the captured step")
            if whole_step and self.tracking is not None:
                raise NotImplementedError("whole-step graphs do not take the tracking windows block: the restart of "
                                          "its windows at reset is not part of the captured step")
            if whole_step and self.trajectory is not None:
                raise NotImplementedError("whole-step graphs do not take the reference trajectories block: its query at "
                                          "reset is not part of the captured step")
            if whole_step and self.composition is not None:
                raise NotImplementedError("whole-step graphs do not take the composition block: its `info` entries are not "
                                          "part of the captured step")
            if whole_step and self._mahony is not None:
                raise NotImplementedError("whole-step graphs do not take the MahonyFilter / BodyObserver blocks: their "
                                          "initialisation at reset is not part of the captured step")
            if whole_step and (eng._process_forces or float(self.std_ratio.get("disturbance", 0.0)) > 0.0):
                raise NotImplementedError("whole-step graphs take no disturbance: their reset draws new realisations")
        self._graph_enabled = bool(enable)
        self._graph_whole = bool(enable and whole_step)
        self._graph = None
        self._state_cache = None
        self._target_cache = None

    def _graph_preconditions(self) -> None:
        """Checked again when the graph is captured: `reset()` may have registered disturbance forces (or the user sensor
        noise) after `enable_graph` was called, and their host-side schedules do not run inside a replay."""
        eng = self.engine
        if eng._adaptive is not None or eng._sensor_noise or eng._impulse_forces or eng._profile_forces \
                or getattr(self, "_impulse_frame", None) is not None:
            raise NotImplementedError("enable_graph needs a fixed-step solver, noiseless sensors and no applied forces "
                                      "but process forces (std_ratio['disturbance'] registers forces at reset(): "
                                      "disturbance_on_device=True, disturbance_impulses=False keeps them on the device)")
        if self._graph_whole and eng._process_forces:
            raise NotImplementedError("whole-step graphs take no disturbance: their reset draws new realisations")
        if self._graph_whole:
            a, b = self._sample_state(self.num_envs), self._sample_state(self.num_envs)
            if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
                raise NotImplementedError("whole-step graphs need a deterministic reset-state sampler")

    def _step_engine_graphed(self, action: torch.Tensor) -> None:
        eng = self.engine
        if self._graph is None:
            self._graph_preconditions()
            # the launches carry no time: the breakpoint plan of a step must be the same at every step
            plan = _plan_signature(eng, self.control_dt, self._n_ctrl)
            self._g_action = torch.zeros((self.model.nmotors, self.num_envs), dtype=self.dtype, device=self.device)
            host = (eng._t, eng._t_prev, eng._t_error, eng._iter, eng._dt, eng._command_dirty)
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize(self.device)
            if self._graph_whole:
                self._state_cache = self._sample_state(self.num_envs)    # (host -> device copies are not capturable)
            with torch.cuda.graph(g):
                self._issue_step(self._g_action)          # recorded, not executed
                if self._graph_whole:
                    reward, terminated, truncated, done = self._after_step()
                    self._g_out = (reward, terminated, truncated, done)
                    self.reset_lanes(done)
            after = (eng._t, eng._iter, eng._dt)
            eng._t, eng._t_prev, eng._t_error, eng._iter, eng._dt, eng._command_dirty = host
            self._graph = (g, plan, after[0] - host[0], after[1] - host[3], after[2])
            self._graph_replays = 0
        g, plan, dt_total, d_iter, dt_last = self._graph
        self._graph_replays += 1
        if self._graph_replays % 64 == 0 and _plan_signature(eng, self.control_dt, self._n_ctrl) != plan:
            self._graph = None                            # (never seen: the plan is periodic; re-capture if it is not)
            return self._step_engine_graphed(action)
        self._g_action.copy_(action.to(self.dtype).T)
        # host-side bookkeeping of the `n_ctrl` engine steps the graph stands for (Kahan-compensated like engine.step);
        # the device clock gets the end time before the replay: the captured episode bookkeeping reads it
        for _ in range(self._n_ctrl):
            corrected = self.control_dt - eng._t_error
            t_end = eng._t + corrected
            eng._t_error = (t_end - eng._t) - corrected
            eng._t_prev, eng._t = eng._t, t_end
        self._clock.fill_(float(eng._t))
        g.replay()
        eng._iter += d_iter
        eng._dt = dt_last
        eng._command_dirty = False

    def step(self, action: torch.Tensor):
        # (the first step of a simulation carries the reference's opening microsecond step -- `engine.substep_sizes` --:
        # it is issued eagerly, the periodic plan is captured from the second step on)
        if not getattr(self, "_graph_whole", False):
            return super().step(action)
        if self.engine._opening_step:
            obs, reward, terminated, truncated, info = super().step(action)
            info.setdefault("reset_mask", terminated | truncated)
            return obs, reward, terminated, truncated, info
        if not self.engine.is_simulation_running:
            raise RuntimeError("No simulation running. Please call `reset` before `step`.")
        if tuple(action.shape) != (self.num_envs, self.model.nmotors):
            raise ValueError(f"action must have shape ({self.num_envs}, {self.model.nmotors})")
        self._step_engine_graphed(action)
        reward, terminated, truncated, done = self._g_out
        return self.observation(), reward, terminated, truncated, {"reset_mask": done}

    def _step_engine(self, action: torch.Tensor) -> None:
        if getattr(self, "_graph_enabled", False) and not self.engine._opening_step:
            self._step_engine_graphed(action)
        else:
            self._refill_impulses(self.step_dt)
            self._issue_step(action.to(self.dtype).T)

    def _issue_step(self, a: torch.Tensor) -> None:
        hb = self._hip_blocks
        if hb is not None:
            hb.pd_adapter(a.contiguous(), 1, self.command_state, False, None, self.step_dt, self._accel)
        else:
            blocks.pd_adapter(a, 1, self.command_state, self.command_state_lower, self.command_state_upper,
                              False, None, self.step_dt, self._accel)
        self.command_state[2].copy_(self._accel)
        for _ in range(self._n_ctrl):
            if hb is not None:
                # torques go straight into the engine's command rows
                hb.pd_controller(self.command_state, self.control_dt, self.engine.field("command"))
                if self._safety is not None:
                    sf = self._safety
                    cmd = self.engine.field("command")
                    hb.motor_safety_limit(cmd, sf["kp"], sf["kd"], sf["lo"], sf["hi"], sf["vlim"], cmd)
                self.engine.mark_command_changed()
            else:
                blocks.pd_controller(self._encoders(), self.command_state, self.command_state_lower,
                                     self.command_state_upper, self.kp, self.kd, self.effort_limit,
                                     self.control_dt, self._torque)
                self.engine.set_command(self._torque)
            self.engine.step(self.control_dt)
            if self._mahony is not None:
                if self._mahony_every_tick:
                    self._mahony.refresh(self.control_dt)
                    if self._body is not None and self._body_every_tick:
                        self._body.refresh(self.control_dt)
                if self._deform is not None and self._deform_every_tick:
                    self._deform.refresh(self.imu_quat)
            elif hb is not None:
                hb.mahony_filter(self.imu_quat, self._omega, self._cf, self._bias,
                                 self.mahony_kp, self.mahony_ki, self.control_dt)
                if self._deform is not None and self._deform_every_tick:
                    self._deform.refresh(self.imu_quat)
            else:
                imu = self.engine.sensor_measurements["ImuSensor"]     # (6, n_imu, B)
                blocks.mahony_filter(self.imu_quat, self._omega, self._cf, imu[:3], imu[3:], self._bias,
                                     self.mahony_kp, self.mahony_ki, self.control_dt)
        if self._mahony is not None and not self._mahony_every_tick:
            self._mahony.refresh(self.step_dt)
        if self._body is not None and not (self._mahony_every_tick and self._body_every_tick):
            self._body.refresh(self.step_dt)
        if self._deform is not None and not self._deform_every_tick:
            self._deform.refresh(self.imu_quat)

    @staticmethod
    def _observer_features(block: Any) -> Dict[str, torch.Tensor]:
        out = {"quat": block.quat.permute(2, 0, 1), "omega": block.omega.permute(2, 0, 1)}
        if block.rpy is not None:
            out["rpy"] = block.rpy.permute(2, 0, 1)
        return out

    def observation(self) -> ObsType:
        obs = super().observation()
        obs["features"] = {"mahony_filter": self.imu_quat.permute(2, 0, 1)}
        if self._mahony is not None:
            obs["features"]["mahony_filter"] = self._observer_features(self._mahony)
        if self._body is not None:
            obs["features"]["body_observer"] = self._observer_features(self._body)
        if self._deform is not None:
            est = {"quat": self._deform.quat.permute(2, 0, 1)}
            if self._deform.rpy is not None:
                est["rpy"] = self._deform.rpy.permute(2, 0, 1)
            obs["features"]["deformation_estimator"] = est
        obs["actions"] = {"pd_controller": self.command_state[:2].permute(2, 0, 1)}
        return obs


def _plan_signature(eng: Any, control_dt: float, n_ctrl: int) -> tuple:
    """The launches `n_ctrl` engine steps of `control_dt` would issue from the engine's current time."""
    from .engine import plan_step
    t, t_err, out = eng._t, eng._t_error, []
    for _ in range(n_ctrl):
        launches, t, t_err = plan_step(t, t_err, control_dt, eng._options)
        out.append(tuple((round(dt / 1e-12), n, bool(c), bool(sn)) for dt, n, c, sn in launches))
    return tuple(out)


# constants of the reference ANYmal environment (python/gym_jiminy/envs/gym_jiminy/envs/anymal.py:17-35)
ANYMAL_STEP_DT = 0.04
ANYMAL_CONTROL_DT = 0.005
ANYMAL_PD_KP = (1500.0,) * 12
ANYMAL_PD_KD = (0.01,) * 12
ANYMAL_MAHONY_KP, ANYMAL_MAHONY_KI = 1.0, 0.1
ANYMAL_MOTOR_VELOCITY_MAX = 4.0
ANYMAL_MOTOR_ACCELERATION_MAX = 30.0
ANYMAL_SIMULATION_DURATION = 20.0


def make_anymal_env(num_envs: int, dtype: torch.dtype = torch.float64,
                    device: Optional[torch.device] = None, pd_pipeline: bool = True,
                    ode_solver: str = "euler_explicit", dt_max: float = 1e-3,
                    contact_model: str = "spring_damper", **kw: Any) -> VecJiminyEnv:
    """ANYmal with the reference's env constants. `contact_model="constraint"` selects what the
    shipped option file selects (anymal_options.toml:24: joint bounds and contact points as
    constraints, PGS); the default stays the spring-damper model of the north-star configuration."""
    model = load_builtin("anymal")
    opts = {"stepper": {"odeSolver": ode_solver, "dtMax": dt_max,
                        "controllerUpdatePeriod": ANYMAL_CONTROL_DT,
                        "sensorsUpdatePeriod": ANYMAL_CONTROL_DT},
            "contacts": {"model": contact_model}}
    kw.setdefault("simulation_duration_max", ANYMAL_SIMULATION_DURATION)
    if pd_pipeline:
        return PDControlledWalkerVecEnv(model, num_envs, ANYMAL_STEP_DT, ANYMAL_CONTROL_DT,
                                        ANYMAL_PD_KP, ANYMAL_PD_KD, ANYMAL_MAHONY_KP, ANYMAL_MAHONY_KI,
                                        joint_position_margin=0.0,
                                        joint_velocity_limit=ANYMAL_MOTOR_VELOCITY_MAX,
                                        joint_acceleration_limit=ANYMAL_MOTOR_ACCELERATION_MAX,
                                        engine_options=opts, dtype=dtype, device=device, **kw)
    return WalkerVecEnv(model, num_envs, ANYMAL_STEP_DT, engine_options=opts, dtype=dtype,
                        device=device, **kw)


# constants of the reference Atlas environment (python/gym_jiminy/envs/gym_jiminy/envs/atlas.py:24-80, atlas_options.toml)
ATLAS_STEP_DT = 0.04
ATLAS_CONTROL_DT = 0.005
ATLAS_SIMULATION_DURATION = 20.0
ATLAS_NEUTRAL_SAGITTAL_HIP_ANGLE = 0.2
ATLAS_MOTOR_POSITION_MARGIN = 0.02
ATLAS_MOTOR_VELOCITY_SAFE_GAIN = 0.15
ATLAS_MOTOR_VELOCITY_MAX = 4.0
ATLAS_MOTOR_ACCELERATION_MAX = 30.0
ATLAS_PD_REDUCED_KP = (5000.0, 5000.0, 8000.0, 4000.0, 8000.0, 5000.0) * 2      # legs: HpZ, HpX, HpY, KnY, AkY, AkX
ATLAS_PD_REDUCED_KD = (0.01, 0.02, 0.02, 0.01, 0.025, 0.01) * 2
ATLAS_PD_FULL_KP = ((5000.0, 8000.0, 5000.0)                                      # back: Z, Y, X
                    + (500.0, 100.0, 200.0, 500.0, 10.0, 100.0, 10.0)             # left arm
                    + (100.0,)                                                    # neck
                    + (500.0, 100.0, 200.0, 500.0, 10.0, 100.0, 10.0)             # right arm
                    + ATLAS_PD_REDUCED_KP)
ATLAS_PD_FULL_KD = ((0.01, 0.015, 0.02) + (0.01, 0.01, 0.01, 0.02, 0.01, 0.02, 0.02) + (0.01,)
                    + (0.01, 0.01, 0.01, 0.02, 0.01, 0.02, 0.02) + ATLAS_PD_REDUCED_KD)
ATLAS_MAHONY_KP, ATLAS_MAHONY_KI = 0.75, 0.057
# `AtlasJiminyEnv._neutral` (atlas.py:147-164): the arms folded along the body, a slight forward lean of the back
ATLAS_NEUTRAL_JOINTS = {"back_bky": 0.2, "l_arm_elx": 0.2, "l_arm_shx": -math.pi / 2.0, "l_arm_shz": math.pi / 4.0,
                        "l_arm_ely": math.pi / 4.0 + math.pi / 2.0, "r_arm_elx": -0.2, "r_arm_shx": math.pi / 2.0,
                        "r_arm_shz": -math.pi / 4.0, "r_arm_ely": math.pi / 4.0 + math.pi / 2.0}


class AtlasPDControlVecEnv(PDControlledWalkerVecEnv):
    """≙ `AtlasPDControlJiminyEnv` (atlas.py:254-309): MotorSafetyLimit -> PDController -> PDAdapter (order 1) ->
    MahonyFilter around `AtlasJiminyEnv`, whose neutral configuration folds the arms."""

    def _sample_state_numpy(self) -> Tuple[np.ndarray, np.ndarray]:
        m = self.model
        q = m.neutral()
        for name, value in ATLAS_NEUTRAL_JOINTS.items():
            q[int(m.idx_q[m.joint_names.index(name)])] = value
        mask = m.bounded_position_mask()
        q[mask] = np.clip(q[mask], m.position_lower[mask], m.position_upper[mask])
        q[2] -= float(lowest_contact_height(m, q)[0])
        return q, np.zeros(m.nv)


def make_atlas_env(num_envs: int, dtype: torch.dtype = torch.float64, device: Optional[torch.device] = None,
                   ode_solver: str = "euler_explicit", dt_max: float = 1e-3, contact_model: str = "constraint",
                   **kw: Any) -> AtlasPDControlVecEnv:
    """Atlas with the reference's environment constants (atlas.py, atlas_options.toml: explicit Euler at 1 ms, 5 ms
    controller / sensor period, constraint contact model).  All 32 box-vertex contact points of the compiled model are
    kept (the reference environment prunes the ones off the bottom convex hull of each foot, atlas.py:99-115: they never
    touch a flat ground)."""
    model = load_builtin("atlas")
    opts = {"stepper": {"odeSolver": ode_solver, "dtMax": dt_max, "controllerUpdatePeriod": ATLAS_CONTROL_DT,
                        "sensorsUpdatePeriod": ATLAS_CONTROL_DT},
            "contacts": {"model": contact_model}}
    kw.setdefault("simulation_duration_max", ATLAS_SIMULATION_DURATION)
    return AtlasPDControlVecEnv(
        model, num_envs, ATLAS_STEP_DT, ATLAS_CONTROL_DT, ATLAS_PD_FULL_KP, ATLAS_PD_FULL_KD, ATLAS_MAHONY_KP, ATLAS_MAHONY_KI,
        joint_position_margin=0.0, joint_velocity_limit=ATLAS_MOTOR_VELOCITY_MAX,
        joint_acceleration_limit=ATLAS_MOTOR_ACCELERATION_MAX,
        safety_limit={"kp": 1.0 / ATLAS_MOTOR_POSITION_MARGIN, "kd": ATLAS_MOTOR_VELOCITY_SAFE_GAIN,
                      "soft_position_margin": 0.0, "soft_velocity_max": ATLAS_MOTOR_VELOCITY_MAX},
        engine_options=opts, dtype=dtype, device=device, **kw)
