"""Batched replacement of [UPSTREAM] gym_pybullet_drones.envs.BaseAviary.

The reference drives this class through ``CtrlAviary(...)`` (PIDEnv.py:106-116,
simulations/EnvGeometric.py:89-100), ``env.step(action)`` (EnvGeometric.py:469),
``env.render()`` (:475), ``env.close()`` (:481) and the attribute census of SURVEY.md
section 3.4.  Here every drone of every env is stepped by one HIP kernel launch
(``mds_step`` / ``mds_step_geometric`` in include/mds.h); Bullet is not involved.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import torch

from .. import _capi as capi
from .._device import DTYPE_BY_NAME, TORCH_DTYPE, default_device_index, forget_env_device, note_env_device, require_gpu, stream_ptr, to_device
from ..utils.enums import DroneModel, Physics

__all__ = ["BaseAviary", "DroneModel", "Physics"]

_PHYSICS_MAP = {Physics.DYN: capi.MDS_PHYSICS_DYN, Physics.PYB: capi.MDS_PHYSICS_DYN,
                Physics.PYB_DRAG: capi.MDS_PHYSICS_DYN_DRAG, Physics.PYB_GND: capi.MDS_PHYSICS_DYN_GND,
                Physics.PYB_DW: capi.MDS_PHYSICS_DYN_DW, Physics.PYB_GND_DRAG_DW: capi.MDS_PHYSICS_DYN_GND_DRAG_DW}
_MODEL_MAP = {DroneModel.CF2X: capi.MDS_CF2X, DroneModel.CF2P: capi.MDS_CF2P}
_PYB_SUBSTITUTED = (Physics.PYB, Physics.PYB_DRAG, Physics.PYB_GND, Physics.PYB_DW, Physics.PYB_GND_DRAG_DW)
_CONSTANT_KEYS = {"M": 1, "L": 1, "KF": 1, "KM": 1, "J": 3, "G": 1, "thrust2weight": 1, "drag_coeff": 3}   # MdsConfig field -> length


def apply_constants(cfg, constants):
    """Overwrite the urdf constants of an ``MdsConfig`` (mds_default_config's, which include/mds.h documents as caller-settable) with the
    entries of ``constants``: M, L, KF, KM, G, thrust2weight (scalars), J, drag_coeff (3 values each).  Any other key is a ValueError."""
    for key, val in (constants or {}).items():
        if key not in _CONSTANT_KEYS:
            raise ValueError(f"constants: unknown key {key!r} (allowed: {', '.join(_CONSTANT_KEYS)})")
        if _CONSTANT_KEYS[key] == 1:
            setattr(cfg, key, float(val))
        else:
            v = np.asarray(val, dtype=np.float64).reshape(-1)
            if v.shape != (3,):
                raise ValueError(f"constants[{key!r}] needs 3 values, got {v.size}")
            setattr(cfg, key, (C.c_double * 3)(*v))
    return cfg


class BaseAviary:
    """Gym-style multi-drone env, batched over ``num_envs`` independent copies.

    Shapes follow the reference when ``num_envs == 1`` and NumPy goes in: ``step(action[D,4])
    -> obs[D,20]``.  With a torch tensor in (any ``num_envs``) everything stays on the GPU:
    ``step(action[E,D,4]) -> obs[E,D,20]``.  obs layout ([UPSTREAM] _getDroneStateVector):
    pos3 | quat4 xyzw | rpy3 | vel3 | ang_v3 (world) | last clipped RPM4.

    ``constants`` (keyword only) replaces urdf constants of the built-in model before the handle is created: a dict with any of
    ``M, L, KF, KM, J`` (3 values), ``G, thrust2weight, drag_coeff`` (3 values).

    ``Physics.PYB`` (the reference's default, PIDEnv.py:19) is served by the explicit
    ``Physics.DYN`` rigid-body model -- there is no Bullet here; ``PYB_DRAG`` adds upstream's
    ``_drag`` term; ``PYB_GND`` / ``PYB_DW`` / ``PYB_GND_DRAG_DW`` add upstream's ``_groundEffect`` / ``_downwash`` as extra
    terms of that model (``env.step(action)`` only: explicit Euler, f32 / f64; spec-level).  The first env
    created with a ``PYB*`` mode says so once (RuntimeWarning).
    """

    _warned_pyb = False

    def __init__(self, drone_model: DroneModel = DroneModel.CF2X, num_drones: int = 1, neighbourhood_radius: float = np.inf,
                 initial_xyzs=None, initial_rpys=None, physics: Physics = Physics.PYB, pyb_freq: int = 240,
                 ctrl_freq: int = 240, gui=False, record=False, obstacles=False, user_debug_gui=True,
                 output_folder="results", *, num_envs: int = 1, dtype="float32", integrator: str = "euler",
                 device: int | None = None, track_last_rpm: bool | None = None, constants: dict | None = None):
        lib = capi.load_library()
        if isinstance(drone_model, str):
            drone_model = DroneModel(drone_model)
        if isinstance(physics, str):
            physics = Physics(physics)
        if drone_model not in _MODEL_MAP:
            raise NotImplementedError(f"drone model {drone_model} (only CF2X / CF2P urdf constants are built in)")
        if physics not in _PHYSICS_MAP:
            raise NotImplementedError(f"physics {physics}")
        if pyb_freq % ctrl_freq != 0:
            raise ValueError("pyb_freq is not divisible by env_freq.")  # [UPSTREAM] BaseAviary.__init__
        if physics in _PYB_SUBSTITUTED and not BaseAviary._warned_pyb:
            import warnings
            BaseAviary._warned_pyb = True
            warnings.warn(f"Physics.{physics.name}: there is no Bullet here -- served by the explicit-Euler Physics.DYN rigid-body model "
                          "(no ground plane, no btMultiBody semi-implicit step); trajectories differ from the reference's PyBullet "
                          "runs from the first step (the reference starts on the floor at z = 0). Pass Physics.DYN to select it knowingly.",
                          RuntimeWarning, stacklevel=3)
        if device is None:
            device = default_device_index()
        else:
            note_env_device(id(self), device.index if isinstance(device, torch.device) else int(device))
        self.device = require_gpu(device)
        self._lib = lib
        self.DRONE_MODEL, self.PHYSICS = drone_model, physics
        self.NUM_DRONES, self.NUM_ENVS = int(num_drones), int(num_envs)
        self.NEIGHBOURHOOD_RADIUS = neighbourhood_radius
        self.PYB_FREQ, self.CTRL_FREQ = int(pyb_freq), int(ctrl_freq)
        self.PYB_STEPS_PER_CTRL = self.PYB_FREQ // self.CTRL_FREQ
        self.CTRL_TIMESTEP, self.PYB_TIMESTEP = 1.0 / self.CTRL_FREQ, 1.0 / self.PYB_FREQ
        self.GUI, self.RECORD, self.OBSTACLES, self.USER_DEBUG = gui, record, obstacles, user_debug_gui
        self.OUTPUT_FOLDER = output_folder
        self._dtype_code = DTYPE_BY_NAME[dtype]
        self.dtype = TORCH_DTYPE[self._dtype_code]

        cfg = capi.MdsConfig()
        capi.check(lib.mds_default_config(_MODEL_MAP[drone_model], C.byref(cfg)), "mds_default_config")
        cfg.num_envs, cfg.num_drones = self.NUM_ENVS, self.NUM_DRONES
        cfg.dtype = self._dtype_code
        cfg.physics = _PHYSICS_MAP[physics]
        cfg.integrator = {"euler": capi.MDS_INTEGRATOR_EULER, "rk4": capi.MDS_INTEGRATOR_RK4}[integrator]
        cfg.pyb_freq, cfg.ctrl_freq = self.PYB_FREQ, self.CTRL_FREQ
        cfg.device = self.device.index
        # _computeObs()[..., 16:20] after a step: kept by the library when the env is used the reference's way (one env);
        # batched envs read the last clipped RPM from the obs step() returns and skip the extra 16 B per drone-step
        cfg.track_last_rpm = int(self.NUM_ENVS == 1 if track_last_rpm is None else track_last_rpm)
        apply_constants(cfg, constants)      # the caller's own drone: every kernel's constant block and the mirrors below see it
        self._cfg = cfg
        # urdf constants ([UPSTREAM] _parseURDFParameters) + derived attributes the reference reads off env
        self.M, self.L, self.KF, self.KM = cfg.M, cfg.L, cfg.KF, cfg.KM
        self.THRUST2WEIGHT_RATIO = cfg.thrust2weight
        self.J = np.diag([cfg.J[0], cfg.J[1], cfg.J[2]])
        self.J_INV = np.linalg.inv(self.J)
        self.G = cfg.G
        self.DRAG_COEFF = np.array([cfg.drag_coeff[0], cfg.drag_coeff[1], cfg.drag_coeff[2]])
        h = C.c_void_p()
        capi.check(lib.mds_create(C.byref(cfg), C.byref(h)), "mds_create")
        self._h = h
        d = (C.c_double * 8)()
        capi.check(lib.mds_get_derived(self._h, d), "mds_get_derived")
        (self.GRAVITY, self.HOVER_RPM, self.MAX_RPM, self.MAX_THRUST, self.MAX_XY_TORQUE, self.MAX_Z_TORQUE) = list(d)[:6]
        self.n = self.NUM_ENVS * self.NUM_DRONES
        self.DRONE_IDS = np.arange(1, self.NUM_DRONES + 1)
        self.CLIENT = -1
        # initial poses ([UPSTREAM] defaults: a line of drones 4L apart, just above the floor)
        if initial_xyzs is None:
            initial_xyzs = np.vstack([np.array([x * 4 * self.L for x in range(self.NUM_DRONES)]),
                                      np.array([y * 4 * self.L for y in range(self.NUM_DRONES)]),
                                      np.ones(self.NUM_DRONES) * 0.1125]).T
        if initial_rpys is None:
            initial_rpys = np.zeros((self.NUM_DRONES, 3))
        self.INIT_XYZS = self._broadcast_init(initial_xyzs)
        self.INIT_RPYS = self._broadcast_init(initial_rpys)
        self._obs = torch.zeros((self.NUM_ENVS, self.NUM_DRONES, capi.OBS_DIM), dtype=self.dtype, device=self.device)
        self._act = torch.zeros((self.NUM_ENVS, self.NUM_DRONES, capi.ACT_DIM), dtype=self.dtype, device=self.device)
        self._has_traj = False
        self.step_counter = 0
        self.RESET_TIME = time.time()
        self._housekeeping()

    # ------------------------------------------------------------------ helpers
    def _broadcast_init(self, a):
        a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
        if a.shape == (self.NUM_DRONES, 3):
            a = np.broadcast_to(a, (self.NUM_ENVS, self.NUM_DRONES, 3))
        if a.shape != (self.NUM_ENVS, self.NUM_DRONES, 3):
            raise ValueError(f"initial_xyzs/initial_rpys must be ({self.NUM_DRONES},3) or "
                             f"({self.NUM_ENVS},{self.NUM_DRONES},3), got {a.shape}")
        return np.ascontiguousarray(a)

    def _stream(self):
        return C.c_void_p(stream_ptr(self.device))

    def _require_open(self):
        if self._h is None:
            raise capi.MdsError(capi.MDS_OK - 5, "BaseAviary", "environment is closed")

    def _housekeeping(self):
        """[UPSTREAM] _housekeeping: poses from INIT_XYZS / INIT_RPYS, zero velocity and action."""
        self._require_open()
        xyz = self.INIT_XYZS.reshape(-1, 3)
        rpy = self.INIT_RPYS.reshape(-1, 3)
        capi.check(self._lib.mds_reset(self._h, capi.as_double_ptr(xyz), capi.as_double_ptr(rpy), self._stream()), "mds_reset")
        self.step_counter = 0

    def _out(self, obs: torch.Tensor, numpy_out: bool):
        if not numpy_out:
            return obs
        o = obs.detach().to("cpu", torch.float64).numpy()
        return o[0] if self.NUM_ENVS == 1 else o

    # ------------------------------------------------------------------ gym API
    def reset(self, seed: int = None, options: dict = None):
        """gymnasium ``reset() -> (obs, info)``.  (The reference never calls it -- SURVEY.md 3.3.)"""
        self._housekeeping()
        obs = self._computeObs()
        return self._out(obs, True) if not getattr(self, "_tensor_mode", False) else obs, self._computeInfo()

    def step(self, action):
        """[UPSTREAM] BaseAviary.step: clip RPM, PYB_FREQ//CTRL_FREQ physics substeps, 20-float obs.
        Returns ``(obs, reward, terminated, truncated, info)`` exactly like CtrlAviary."""
        self._require_open()
        numpy_in = not isinstance(action, torch.Tensor)
        self._tensor_mode = not numpy_in
        act = to_device(action, self.device, self.dtype)
        if act.numel() != self.n * capi.ACT_DIM:
            raise ValueError(f"action must hold {self.NUM_ENVS}x{self.NUM_DRONES}x4 RPMs, got shape {tuple(act.shape)}")
        capi.check(self._lib.mds_step(self._h, C.c_void_p(act.data_ptr()), C.c_void_p(self._obs.data_ptr()), self._stream()),
                   "mds_step")
        self.step_counter += self.PYB_STEPS_PER_CTRL
        return (self._out(self._obs, numpy_in), self._computeReward(), self._computeTerminated(),
                self._computeTruncated(), self._computeInfo())

    def render(self, mode="human", close=False):
        """[UPSTREAM] BaseAviary.render: text dump of every drone of env 0 (EnvGeometric.py:475)."""
        o = self._computeObs().detach().to("cpu", torch.float64).numpy()[0]
        print("\n[INFO] BaseAviary.render() ——— it {:04d}".format(self.step_counter),
              "——— wall-clock time {:.1f}s,".format(time.time() - self.RESET_TIME),
              "simulation time {:.1f}s@{:d}Hz ({:.2f}x)".format(self.step_counter * self.PYB_TIMESTEP, self.PYB_FREQ,
                                                               (self.step_counter * self.PYB_TIMESTEP) / max(time.time() - self.RESET_TIME, 1e-9)))
        for i in range(self.NUM_DRONES):
            print("[INFO] BaseAviary.render() ——— drone {:d}".format(i),
                  "——— x {:+06.2f}, y {:+06.2f}, z {:+06.2f}".format(o[i, 0], o[i, 1], o[i, 2]),
                  "——— velocity {:+06.2f}, {:+06.2f}, {:+06.2f}".format(o[i, 10], o[i, 11], o[i, 12]),
                  "——— roll {:+06.2f}, pitch {:+06.2f}, yaw {:+06.2f}".format(*(o[i, 7:10] * 180 / np.pi)),
                  "——— angular velocity {:+06.4f}, {:+06.4f}, {:+06.4f} ——— ".format(o[i, 13], o[i, 14], o[i, 15]))

    def close(self):
        forget_env_device(id(self))
        if getattr(self, "_h", None) is not None:
            self._lib.mds_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def getPyBulletClient(self):
        return self.CLIENT

    def getDroneIds(self):
        return self.DRONE_IDS

    def _showDroneLocalAxes(self, nth_drone):
        pass  # Bullet GUI helper; nothing to draw here

    # ------------------------------------------------------------------ obs / state
    def _computeObs(self) -> torch.Tensor:
        self._require_open()
        capi.check(self._lib.mds_get_obs(self._h, C.c_void_p(self._obs.data_ptr()), self._stream()), "mds_get_obs")
        return self._obs

    def _getDroneStateVector(self, nth_drone, env: int = 0):
        return self._obs[env, nth_drone].detach().to("cpu", torch.float64).numpy()

    def get_state(self) -> np.ndarray:
        """World-frame 13-float state [E, D, 13] (pos3 | quat4 xyzw | vel3 | body rates3), float64 copy."""
        self._require_open()
        out = np.zeros((self.n, capi.STATE_DIM))
        capi.check(self._lib.mds_get_state(self._h, capi.as_double_ptr(out), self._stream()), "mds_get_state")
        return out.reshape(self.NUM_ENVS, self.NUM_DRONES, capi.STATE_DIM)

    def state_views(self):
        """Zero-copy torch views of the library-owned state (mds_state_ptrs): a dict with 13 strided ``[n]`` tensors
        ``comp[k]`` in the storage dtype (positions relative to ``origin``) and the three ``origin`` planes."""
        self._require_open()
        comp, stride, org = (C.c_void_p * 13)(), (C.c_size_t * 13)(), (C.c_void_p * 3)()
        capi.check(self._lib.mds_state_ptrs(self._h, comp, stride, org), "mds_state_ptrs")

        class _Raw:                      # the CUDA array interface is how torch adopts a foreign device pointer
            def __init__(self, ptr, n, stride, dt):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": dt, "data": (int(ptr), False), "version": 2,
                                                 "strides": (stride,)}

        ts = {torch.float16: "<f2", torch.float32: "<f4", torch.float64: "<f8"}
        es = {torch.float16: 2, torch.float32: 4, torch.float64: 8}[self.dtype]
        cdt = torch.float64 if self.dtype == torch.float64 else torch.float32
        return {"comp": [torch.as_tensor(_Raw(comp[k], self.n, int(stride[k]) * es, ts[self.dtype]), device=self.device) for k in range(13)],
                "origin": [torch.as_tensor(_Raw(org[k], self.n, es if cdt == self.dtype else 4, ts[cdt]), device=self.device) for k in range(3)]}

    def set_state(self, state):
        self._require_open()
        s = np.ascontiguousarray(np.asarray(state, dtype=np.float64).reshape(self.n, capi.STATE_DIM))
        capi.check(self._lib.mds_set_state(self._h, capi.as_double_ptr(s), self._stream()), "mds_set_state")

    def _kin(self, lo, hi):
        s = self.get_state()
        return s[0, :, lo:hi] if self.NUM_ENVS == 1 else s[:, :, lo:hi]

    pos = property(lambda self: self._kin(0, 3))
    quat = property(lambda self: self._kin(3, 7))
    vel = property(lambda self: self._kin(7, 10))
    rpy_rates = property(lambda self: self._kin(10, 13))

    @property
    def rpy(self):
        o = self._computeObs().detach().to("cpu", torch.float64).numpy()[..., 7:10]
        return o[0] if self.NUM_ENVS == 1 else o

    @property
    def ang_v(self):
        o = self._computeObs().detach().to("cpu", torch.float64).numpy()[..., 13:16]
        return o[0] if self.NUM_ENVS == 1 else o

    # ------------------------------------------------------------------ fused on-GPU control loop
    def set_trajectories(self, trajs):
        """Attach one trajectory per drone for ``step_geometric``: a list of D (shared by every env) or
        E*D trajectory objects, or an [E,D,7]/[D,7] Lemniscate parameter array (a, omega, centre3, yaw_rate,
        phase_shift).  All-Lemniscate sets use the fused fp32 kernel; anything else (Circle, Line, Wait,
        Compound, Rotate) is flattened into segment tables for the general kernel."""
        self._require_open()
        from ..trajectories.Lemniscate import Lemniscate
        from ..trajectories.base import upload_segments
        if isinstance(trajs, (list, tuple)):
            trajs = list(trajs)
            if len(trajs) == self.NUM_DRONES and self.NUM_ENVS > 1:
                trajs = trajs * self.NUM_ENVS
            if len(trajs) != self.n:
                raise ValueError(f"need {self.NUM_DRONES} or {self.n} trajectories, got {len(trajs)}")
            if not all(type(t) is Lemniscate for t in trajs):
                upload_segments(self._lib, self._h, trajs, self.device)
                self._has_traj = True
                return
            P = np.array([t.params() for t in trajs], dtype=np.float64)
        else:
            P = np.asarray(trajs, dtype=np.float64)
        if P.shape == (self.NUM_DRONES, capi.LEM_DIM):
            P = np.broadcast_to(P, (self.NUM_ENVS, self.NUM_DRONES, capi.LEM_DIM))
        P = np.ascontiguousarray(P.reshape(self.n, capi.LEM_DIM))
        capi.check(self._lib.mds_set_lemniscate(self._h, capi.as_double_ptr(P), self._stream()), "mds_set_lemniscate")
        self._has_traj = True

    def traj_eval(self, t: float) -> torch.Tensor:
        """The attached trajectories sampled at ``t`` for every drone (mds_traj_eval): ``[E, D, 11]`` in the env's dtype,
        pos3 | vel3 | acc3 | yaw | yaw_rate, world frame."""
        self._require_open()
        des = torch.empty((self.NUM_ENVS, self.NUM_DRONES, capi.DES_DIM), dtype=self.dtype, device=self.device)
        capi.check(self._lib.mds_traj_eval(self._h, C.c_double(float(t)), C.c_void_p(des.data_ptr()), self._stream()), "mds_traj_eval")
        return des

    def set_wind(self, force_world):
        """Constant world-frame force [N] on every drone each physics substep -- the reference's
        ``p.applyExternalForce(..., [wind_force, 0, 0], WORLD_FRAME)`` (EnvGeometric.py:463-467)."""
        f = np.ascontiguousarray(np.asarray(force_world, dtype=np.float64).reshape(3))
        capi.check(self._lib.mds_set_wind(self._h, capi.as_double_ptr(f)), "mds_set_wind")

    def set_geometric_gains(self, Kp=None, Kv=None, KR=None, Kw=None, g=None, max_tilt_angle=None):
        gains = capi.MdsGeometricGains()
        capi.check(self._lib.mds_default_geometric_gains(C.byref(gains)), "mds_default_geometric_gains")
        for name, val in (("Kp", Kp), ("Kv", Kv), ("KR", KR), ("Kw", Kw)):
            if val is not None:
                v = np.broadcast_to(np.asarray(val, dtype=np.float64), (3,))
                setattr(gains, name, (C.c_double * 3)(*v))
        if g is not None:
            gains.g = float(g)
        if max_tilt_angle is not None:
            gains.max_tilt_angle = float(max_tilt_angle)
        capi.check(self._lib.mds_set_geometric_gains(self._h, C.byref(gains)), "mds_set_geometric_gains")

    def step_geometric(self, t: float, return_action: bool = False):
        """One fused control step of simulations/EnvGeometric.py:434-469 for every drone:
        trajectory sample -> GeometricControl.compute -> input_to_action -> env.step."""
        self._require_open()
        act_ptr = C.c_void_p(self._act.data_ptr()) if return_action else C.c_void_p(None)
        capi.check(self._lib.mds_step_geometric(self._h, C.c_double(t), C.c_void_p(self._obs.data_ptr()), act_ptr,
                                                self._stream()), "mds_step_geometric")
        self.step_counter += self.PYB_STEPS_PER_CTRL
        return (self._obs, self._act) if return_action else self._obs

    def step_lqr(self, t: float, return_action: bool = False):
        """The same control step with the reference's 12-state LQRController (needs one constructed on this env): the default
        'lqr' branch of simulations/EnvGeometric.py do_control, fused for every drone."""
        self._require_open()
        act_ptr = C.c_void_p(self._act.data_ptr()) if return_action else C.c_void_p(None)
        capi.check(self._lib.mds_step_lqr(self._h, C.c_double(t), C.c_void_p(self._obs.data_ptr()), act_ptr, self._stream()), "mds_step_lqr")
        self.step_counter += self.PYB_STEPS_PER_CTRL
        return (self._obs, self._act) if return_action else self._obs

    def rollout_geometric(self, t0: float, n_steps: int, want_obs: bool = True, obs_every_step: bool = False):
        """``n_steps`` fused control steps enqueued from C; returns the last observation.
        ``obs_every_step`` materialises the [E,D,20] observation on every step (as env.step does)."""
        self._require_open()
        obs_ptr = C.c_void_p(self._obs.data_ptr()) if want_obs else C.c_void_p(None)
        capi.check(self._lib.mds_rollout_geometric(self._h, C.c_double(t0), C.c_int(n_steps), obs_ptr,
                                                   C.c_int(1 if obs_every_step else 0), self._stream()),
                   "mds_rollout_geometric")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return self._obs if want_obs else None

    def rollout_step(self, actions: torch.Tensor, first_step: int, n_steps: int, obs_log: torch.Tensor | None = None,
                     episode_len: int = 0, steps_per_launch: int = 1):
        """``n_steps`` plain ``env.step`` calls issued from C with a replayed action table: step j applies ``actions[j % A]``
        ([A,E,D,4] device tensor of this env's dtype) and writes its observation into ``obs_log[j % T]`` ([T,E,D,20]).
        ``episode_len`` > 0 puts the drones back to their initial poses before every step j > 0 with j % episode_len == 0.
        ``steps_per_launch`` > 1 runs that many steps per kernel launch with the state in registers (mds_rollout_step_fused).
        Returns the log (or None)."""
        self._require_open()
        if actions.dtype != self.dtype or not actions.is_contiguous() or actions.numel() % (self.n * capi.ACT_DIM):
            raise ValueError("actions must be a contiguous [A,E,D,4] tensor of the env's dtype")
        if obs_log is not None and (obs_log.dtype != self.dtype or not obs_log.is_contiguous() or obs_log.numel() % (self.n * 20)):
            raise ValueError("obs_log must be a contiguous [T,E,D,20] tensor of the env's dtype")
        A = actions.numel() // (self.n * capi.ACT_DIM)
        T = obs_log.numel() // (self.n * 20) if obs_log is not None else 0
        if steps_per_launch > 1:
            capi.check(self._lib.mds_rollout_step_fused(self._h, C.c_void_p(actions.data_ptr()), C.c_int(A), C.c_int(first_step), C.c_int(n_steps),
                                                        C.c_void_p(obs_log.data_ptr() if obs_log is not None else None), C.c_int(T),
                                                        C.c_int(int(episode_len)), C.c_int(int(steps_per_launch)), self._stream()),
                       "mds_rollout_step_fused")
            self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
            return obs_log
        capi.check(self._lib.mds_rollout_step(self._h, C.c_void_p(actions.data_ptr()), C.c_int(A), C.c_int(first_step), C.c_int(n_steps),
                                              C.c_void_p(obs_log.data_ptr() if obs_log is not None else None), C.c_int(T), C.c_int(int(episode_len)),
                                              self._stream()),
                   "mds_rollout_step")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return obs_log

    # ------------------------------------------------------------------ per-env episodes on the device
    def set_episodes(self, max_steps: int = 0, z_min=None, z_max=None, max_dist=None, max_tilt=None, max_speed=None, max_rate=None,
                     reward_r0: float = 2.0, term_penalty: float = 0.0, target=None, enabled: bool = True):
        """Per-env episodes decided and restarted inside the rollout kernel (mds_set_episodes).  A drone terminates its env when a
        state component is not finite, its world z leaves [``z_min``, ``z_max``], it is more than ``max_dist`` from its reset position,
        its body z axis is more than ``max_tilt`` rad off vertical, or it is faster than ``max_speed`` / spins faster than ``max_rate``
        (``None``: test off); an env is truncated after ``max_steps`` control steps (0: never).  A done env has all its drones put
        back to their initial poses.  Reward per env: sum over drones of ``max(0, reward_r0 - |p - target|^4)``, less ``term_penalty``
        when terminated; ``target`` [E,D,3] / [D,3] world frame (default: the initial positions).  ``enabled=False`` switches it off."""
        self._require_open()
        if not enabled:
            capi.check(self._lib.mds_set_episodes(self._h, None, None, self._stream()), "mds_set_episodes")
            return
        p = capi.MdsEpisodeParams()
        capi.check(self._lib.mds_default_episode_params(C.byref(p)), "mds_default_episode_params")
        p.max_steps = int(max_steps)
        for name, val in (("z_min", z_min), ("z_max", z_max), ("max_dist", max_dist), ("max_tilt", max_tilt), ("max_speed", max_speed),
                          ("max_rate", max_rate)):
            if val is not None:
                setattr(p, name, float(val))
        p.reward_r0, p.term_penalty = float(reward_r0), float(term_penalty)
        tgt = None
        if target is not None:
            tgt = np.ascontiguousarray(self._broadcast_init(target).reshape(self.n, 3))
        capi.check(self._lib.mds_set_episodes(self._h, C.byref(p), capi.as_double_ptr(tgt) if tgt is not None else None, self._stream()),
                   "mds_set_episodes")

    def _episode_dtype(self):
        return torch.float64 if self.dtype == torch.float64 else torch.float32

    def step_episodes(self, action: torch.Tensor, final_obs: torch.Tensor | None = None):
        """One control step with the episode rule (mds_step_episodes): ``(obs, reward[E], terminated[E], truncated[E], info)``, device
        tensors.  ``obs`` is what a policy acts on next: the rows of a done env are its post-reset observation; ``final_obs``
        (optional [E,D,20] tensor) receives the transition's own rows.  ``info["flags"]``: the int32 flags word per env (bit 0
        terminated, bit 1 truncated, bits 8..13 the causes; with ``set_episode_safety`` bit 14: two drones of the env inside the pair
        safety set, bit 15: a drone inside an obstacle's).  The returned tensors are reused by the next call."""
        self._require_open()
        act = to_device(action, self.device, self.dtype)
        if act.numel() != self.n * capi.ACT_DIM or not act.is_contiguous():
            raise ValueError(f"action must be a contiguous tensor of {self.NUM_ENVS}x{self.NUM_DRONES}x4 RPMs, got shape {tuple(act.shape)}")
        if final_obs is not None and (final_obs.dtype != self.dtype or not final_obs.is_contiguous() or final_obs.numel() != self.n * capi.OBS_DIM):
            raise ValueError("final_obs must be a contiguous [E,D,20] tensor of the env's dtype")
        if getattr(self, "_ep_reward", None) is None:
            self._ep_reward = torch.zeros((self.NUM_ENVS,), dtype=self._episode_dtype(), device=self.device)
            self._ep_flags = torch.zeros((self.NUM_ENVS,), dtype=torch.int32, device=self.device)
        capi.check(self._lib.mds_step_episodes(self._h, C.c_void_p(act.data_ptr()), C.c_void_p(self._obs.data_ptr()),
                                               C.c_void_p(final_obs.data_ptr() if final_obs is not None else None),
                                               C.c_void_p(self._ep_reward.data_ptr()), C.c_void_p(self._ep_flags.data_ptr()), self._stream()),
                   "mds_step_episodes")
        self.step_counter += self.PYB_STEPS_PER_CTRL
        return self._obs, self._ep_reward, (self._ep_flags & 1) != 0, (self._ep_flags & 2) != 0, {"flags": self._ep_flags}

    def rollout_episodes(self, actions: torch.Tensor, first_step: int, n_steps: int, obs_log: torch.Tensor | None = None,
                         reward_log: torch.Tensor | None = None, flags_log: torch.Tensor | None = None, steps_per_launch: int = 1):
        """``n_steps`` control steps of the replayed action table ``actions`` [A,E,D,4] with the episode rule, ``steps_per_launch`` per
        kernel launch (mds_rollout_episodes).  Step j writes slot ``j % T`` of each log given: ``obs_log`` [T,E,D,20] (the transition's
        rows, before any reset), ``reward_log`` [T,E] (float32; float64 on a float64 env), ``flags_log`` [T,E] int32; the logs share T.
        Returns the current observation [E,D,20] (post-reset rows where an env was done in the last step)."""
        self._require_open()
        if actions.dtype != self.dtype or not actions.is_contiguous() or actions.numel() % (self.n * capi.ACT_DIM):
            raise ValueError("actions must be a contiguous [A,E,D,4] tensor of the env's dtype")
        slots = set()
        for name, log, dt, per in (("obs_log", obs_log, self.dtype, self.n * capi.OBS_DIM), ("reward_log", reward_log, self._episode_dtype(), self.NUM_ENVS),
                                   ("flags_log", flags_log, torch.int32, self.NUM_ENVS)):
            if log is None:
                continue
            if log.dtype != dt or not log.is_contiguous() or log.numel() == 0 or log.numel() % per:
                raise ValueError(f"{name} must be a contiguous tensor of dtype {dt} with {per} values per step")
            slots.add(log.numel() // per)
        if len(slots) > 1:
            raise ValueError("obs_log, reward_log and flags_log must hold the same number of steps")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)   # noqa: E731
        capi.check(self._lib.mds_rollout_episodes(self._h, ptr(actions), C.c_int(actions.numel() // (self.n * capi.ACT_DIM)), C.c_int(int(first_step)),
                                                  C.c_int(int(n_steps)), ptr(obs_log), C.c_int(slots.pop() if slots else 0), ptr(reward_log),
                                                  ptr(flags_log), C.c_int(int(steps_per_launch)), ptr(self._obs), self._stream()),
                   "mds_rollout_episodes")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return self._obs

    def episode_counters(self):
        """Zero-copy torch views [E] of the per-env episode counters (mds_episode_ptrs): ``length`` (int32) and ``ret`` of the running
        episode; ``count`` (int32), ``sum_return`` and ``sum_length`` (int32) of the completed ones.  No atomics: reduce them yourself."""
        self._require_open()
        ptrs = (C.c_void_p * 5)()
        capi.check(self._lib.mds_episode_ptrs(self._h, ptrs), "mds_episode_ptrs")

        class _Raw:
            def __init__(self, ptr, n, dt):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": dt, "data": (int(ptr), False), "version": 2}

        ft = "<f8" if self.dtype == torch.float64 else "<f4"
        names = (("length", "<i4"), ("ret", ft), ("count", "<i4"), ("sum_return", ft), ("sum_length", "<i4"))
        return {k: torch.as_tensor(_Raw(ptrs[j], self.NUM_ENVS, dt), device=self.device) for j, (k, dt) in enumerate(names)}

    def set_episode_safety(self, safety_radius: float = 0.0, zscale: float = 2.0, obstacles=None, enabled: bool = True):
        """Collision causes of the per-env episodes (mds_set_episode_safety; needs ``set_episodes`` first): after every control step
        each drone is tested against the other drones of its env (``Ds = 2 safety_radius``) and against the sphere ``obstacles``
        [n_obs,4] = centre xyz in the world frame, radius (``Ds = safety_radius + radius``; at most 16, one list for all envs) on the
        CBF filter's zeroth-order barrier ``h = (ex^2 + ey^2)^2 + (ez / zscale)^4 - Ds^4``; ``h < 0`` terminates the env with flags bit
        14 (pair) or 15 (obstacle).  ``enabled=False`` switches the tests off; so does ``set_episodes(enabled=False)``."""
        self._require_open()
        if not enabled:
            capi.check(self._lib.mds_set_episode_safety(self._h, None, None, self._stream()), "mds_set_episode_safety")
            return
        obs = None
        if obstacles is not None and np.size(obstacles):
            obs = np.ascontiguousarray(np.asarray(obstacles, dtype=np.float64).reshape(-1, 4))
        p = capi.MdsEpisodeSafety(float(safety_radius), float(zscale), 0 if obs is None else obs.shape[0], 0)
        capi.check(self._lib.mds_set_episode_safety(self._h, C.byref(p), capi.as_double_ptr(obs) if obs is not None else None, self._stream()),
                   "mds_set_episode_safety")

    def episode_safety(self):
        """Zero-copy torch views [E] of the safety signal (mds_episode_safety_ptrs), in the compute type: ``h_min_step``, the env's
        smallest ``h`` over all its pairs and obstacles in the last step of the most recent call (pre-reset; ``+inf`` with nothing to
        test), and ``h_min_episode``, the running minimum over the env's current episode (``+inf`` again when it restarts)."""
        self._require_open()
        ptrs = (C.c_void_p * 2)()
        capi.check(self._lib.mds_episode_safety_ptrs(self._h, ptrs), "mds_episode_safety_ptrs")

        class _Raw:
            def __init__(self, ptr, n, dt):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": dt, "data": (int(ptr), False), "version": 2}

        ft = "<f8" if self.dtype == torch.float64 else "<f4"
        return {k: torch.as_tensor(_Raw(ptrs[j], self.NUM_ENVS, ft), device=self.device) for j, k in enumerate(("h_min_step", "h_min_episode"))}

    def set_episode_randomisation(self, seed: int = 0, pos=0.0, rpy=0.0, vel=0.0, rate=0.0, first_env: int = 0, enabled: bool = True):
        """Randomised episode starts (mds_set_episode_randomisation; needs ``set_episodes`` first): a done env's drones restart at their
        reset position ± ``pos`` (m), initial attitude ± ``rpy`` (rad), world velocity ± ``vel`` (m/s) and body rates ± ``rate`` (rad/s),
        each a scalar or a 3-vector of half-widths, drawn uniformly by a counter-based generator on the device.  A start is a pure
        function of (``seed``, the drone's global index ``first_env * D + i``, the env's ``count`` of completed episodes, the number of
        ``reset_episodes`` calls): it does not depend on ``steps_per_launch`` or on how the envs are sharded -- give every shard the same
        seed and the global index of its first env.  ``enabled=False`` switches it off; so does ``set_episodes(enabled=False)``."""
        self._require_open()
        if not enabled:
            capi.check(self._lib.mds_set_episode_randomisation(self._h, None, self._stream()), "mds_set_episode_randomisation")
            return
        p = capi.MdsEpisodeRandomisation()
        p.seed, p.first_env = int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_env)
        for name, val in (("pos", pos), ("rpy", rpy), ("vel", vel), ("rate", rate)):
            setattr(p, name, (C.c_double * 3)(*np.broadcast_to(np.asarray(val, dtype=np.float64), (3,))))
        capi.check(self._lib.mds_set_episode_randomisation(self._h, C.byref(p), self._stream()), "mds_set_episode_randomisation")

    def reset_episodes(self):
        """Every drone to a freshly drawn start and every env's running episode restarted (mds_reset_episodes; the completed episodes'
        statistics stay).  Returns the observation tensor [E,D,20]; it is reused by the next call."""
        self._require_open()
        capi.check(self._lib.mds_reset_episodes(self._h, C.c_void_p(self._obs.data_ptr()), self._stream()), "mds_reset_episodes")
        return self._obs

    # ------------------------------------------------------------------ an MLP policy inside the episode rollout kernel
    def set_episode_policy(self, weights, n_hidden: int, width: int, activation: str = "tanh", rpm_base=None, rpm_scale=None,
                           enabled: bool = True):
        """An MLP policy evaluated inside the episode rollout kernel (mds_set_episode_policy; needs ``set_episodes`` first): 12 features
        per drone (position - target | roll, pitch, yaw | world velocity | world angular velocity), ``n_hidden`` (1 or 2) hidden layers
        of ``width`` (1..64) neurons with ``activation`` ``"tanh"`` or ``"relu"``, a linear output of 4, and
        ``rpm = rpm_base + rpm_scale * clamp(y, -1, 1)`` (defaults: ``HOVER_RPM`` and ``0.05 HOVER_RPM``).  ``weights``: the flat
        vector ``torch.cat([p.detach().flatten() for p in net.parameters()])`` of an ``nn.Sequential`` of ``Linear`` layers (tensor or
        array).  ``enabled=False`` switches it off; so does ``set_episodes(enabled=False)``."""
        self._require_open()
        if not enabled:
            capi.check(self._lib.mds_set_episode_policy(self._h, None, None, self._stream()), "mds_set_episode_policy")
            return
        acts = {"tanh": 0, "relu": 1}
        if activation not in acts:
            raise ValueError(f"activation must be 'tanh' or 'relu', got {activation!r}")
        n_hidden, width = int(n_hidden), int(width)
        if n_hidden not in (1, 2) or not 1 <= width <= capi.POLICY_MAX_WIDTH:
            raise ValueError(f"n_hidden must be 1 or 2 and width in 1..{capi.POLICY_MAX_WIDTH}, got {n_hidden} and {width}")
        if isinstance(weights, torch.Tensor):
            weights = weights.detach().double().cpu().numpy()
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        want = (capi.POLICY_IN + 1) * width + (n_hidden - 1) * (width + 1) * width + (width + 1) * capi.POLICY_OUT
        if w.size != want:
            raise ValueError(f"a policy of {n_hidden} hidden layer(s) of width {width} has {want} weights, got {w.size}")
        p = capi.MdsEpisodePolicy(n_hidden, width, acts[activation], 0, float("nan") if rpm_base is None else float(rpm_base),
                                  float("nan") if rpm_scale is None else float(rpm_scale))
        capi.check(self._lib.mds_set_episode_policy(self._h, C.byref(p), capi.as_double_ptr(w), self._stream()), "mds_set_episode_policy")

    @staticmethod
    def _episode_policy_from_torch(module):
        """``(weights float64 [n], n_hidden, width, activation)`` of an ``nn.Sequential`` of the supported shape: ``Linear(12, w)``, act,
        [``Linear(w, w)``, the same act,] ``Linear(w, 4)`` with act ``Tanh`` or ``ReLU`` and w in 1..64.  ``ValueError`` on anything else."""
        nn = torch.nn
        if not isinstance(module, nn.Sequential):
            raise ValueError("the policy must be an nn.Sequential of Linear / Tanh / ReLU layers")
        layers = list(module)
        if len(layers) not in (3, 5):
            raise ValueError(f"the policy must have 1 or 2 hidden layers (3 or 5 modules), got {len(layers)} modules")
        lin, act = layers[0::2], layers[1::2]
        if not all(isinstance(m, nn.Linear) for m in lin) or not all(isinstance(m, (nn.Tanh, nn.ReLU)) for m in act):
            raise ValueError("the policy must alternate Linear layers with Tanh or ReLU")
        if len({type(m) for m in act}) != 1:
            raise ValueError("the hidden layers must share one activation")
        if any(m.bias is None for m in lin):
            raise ValueError("every Linear layer needs its bias")
        width = lin[0].out_features
        if not 1 <= width <= capi.POLICY_MAX_WIDTH:
            raise ValueError(f"the hidden width must be in 1..{capi.POLICY_MAX_WIDTH}, got {width}")
        dims = [(m.in_features, m.out_features) for m in lin]
        if dims != [(capi.POLICY_IN, width)] + [(width, width)] * (len(lin) - 2) + [(width, capi.POLICY_OUT)]:
            raise ValueError(f"the layers must be {capi.POLICY_IN} -> width [-> width] -> {capi.POLICY_OUT} with one common width, got {dims}")
        w = torch.cat([t.detach().double().flatten().cpu() for m in lin for t in (m.weight, m.bias)]).numpy()
        return w, len(lin) - 1, width, "tanh" if isinstance(act[0], nn.Tanh) else "relu"

    def set_episode_policy_from_torch(self, module, rpm_base=None, rpm_scale=None):
        """``set_episode_policy`` from an ``nn.Sequential`` of ``Linear`` / ``Tanh`` / ``ReLU`` (stable-baselines3:
        ``nn.Sequential(*model.policy.mlp_extractor.policy_net, model.policy.action_net)``).  ``ValueError`` on any other shape."""
        w, n_hidden, width, activation = self._episode_policy_from_torch(module)
        self.set_episode_policy(w, n_hidden, width, activation, rpm_base, rpm_scale)

    def episode_policy_compute(self, obs: torch.Tensor):
        """The policy alone on observation rows ``obs`` [E,D,20] (mds_episode_policy_compute): the commanded RPM [E,D,4], a new tensor.
        Followed by ``step_episodes`` this is the policy-in-the-loop form of ``rollout_episodes_policy``."""
        self._require_open()
        if obs.dtype != self.dtype or not obs.is_contiguous() or obs.numel() != self.n * capi.OBS_DIM or obs.device != self._obs.device:
            raise ValueError("obs must be a contiguous [E,D,20] device tensor of the env's dtype")
        rpm = torch.empty((self.NUM_ENVS, self.NUM_DRONES, capi.ACT_DIM), dtype=self.dtype, device=self._obs.device)
        capi.check(self._lib.mds_episode_policy_compute(self._h, C.c_void_p(obs.data_ptr()), C.c_void_p(rpm.data_ptr()), self._stream()),
                   "mds_episode_policy_compute")
        return rpm

    def rollout_episodes_policy(self, first_step: int, n_steps: int, obs_log: torch.Tensor | None = None, action_log: torch.Tensor | None = None,
                                reward_log: torch.Tensor | None = None, flags_log: torch.Tensor | None = None, steps_per_launch: int = 1):
        """``n_steps`` control steps of the configured policy in closed loop with the episode rule, ``steps_per_launch`` per kernel
        launch (mds_rollout_episodes_policy): every drone acts on its current state, post-reset where its env was just done.  Step j
        writes slot ``j % T`` of each log given: ``obs_log`` [T,E,D,20], ``action_log`` [T,E,D,4] (the commanded RPM), ``reward_log``
        [T,E], ``flags_log`` [T,E] int32, as in ``rollout_episodes``.  Returns the current observation [E,D,20]."""
        self._require_open()
        slots = set()
        for name, log, dt, per in (("obs_log", obs_log, self.dtype, self.n * capi.OBS_DIM), ("action_log", action_log, self.dtype, self.n * capi.ACT_DIM),
                                   ("reward_log", reward_log, self._episode_dtype(), self.NUM_ENVS), ("flags_log", flags_log, torch.int32, self.NUM_ENVS)):
            if log is None:
                continue
            if log.dtype != dt or not log.is_contiguous() or log.numel() == 0 or log.numel() % per:
                raise ValueError(f"{name} must be a contiguous tensor of dtype {dt} with {per} values per step")
            slots.add(log.numel() // per)
        if len(slots) > 1:
            raise ValueError("obs_log, action_log, reward_log and flags_log must hold the same number of steps")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)   # noqa: E731
        capi.check(self._lib.mds_rollout_episodes_policy(self._h, C.c_int(int(first_step)), C.c_int(int(n_steps)), ptr(obs_log),
                                                         C.c_int(slots.pop() if slots else 0), ptr(action_log), ptr(reward_log), ptr(flags_log),
                                                         C.c_int(int(steps_per_launch)), ptr(self._obs), self._stream()),
                   "mds_rollout_episodes_policy")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return self._obs

    # ------------------------------------------------------------------ Gaussian actions drawn in the rollout kernel
    def set_episode_policy_noise(self, log_std, seed: int = 0, first_env: int = 0, enabled: bool = True):
        """Gaussian exploration noise of the policy's actions (mds_set_episode_policy_noise; needs ``set_episode_policy`` first):
        ``rollout_episodes_sampled`` and ``episode_policy_sample`` command ``clip(a)`` with ``a ~ N(y, diag(exp(log_std))^2)``, ``y`` the
        network's output and ``log_std`` the state-independent vector of stable-baselines3's ``DiagGaussianDistribution`` (a scalar or
        4 values).  A draw is a pure function of (``seed``, the drone's global index ``first_env * D + i``, the env's ``count`` of
        completed episodes, the running episode's ``length``, the number of resets of all envs since this call): it does not depend on
        ``steps_per_launch`` or on how the envs are sharded.  ``rollout_episodes_policy`` stays the deterministic rollout.
        ``enabled=False`` switches the noise off; so does switching off the policy or the episodes."""
        self._require_open()
        if not enabled:
            capi.check(self._lib.mds_set_episode_policy_noise(self._h, None, self._stream()), "mds_set_episode_policy_noise")
            return
        if isinstance(log_std, torch.Tensor):
            log_std = log_std.detach().double().cpu().numpy()
        p = capi.MdsEpisodePolicyNoise()
        p.seed, p.first_env = int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_env)
        p.log_std = (C.c_double * 4)(*np.broadcast_to(np.asarray(log_std, dtype=np.float64).reshape(-1), (4,)))
        capi.check(self._lib.mds_set_episode_policy_noise(self._h, C.byref(p), self._stream()), "mds_set_episode_policy_noise")

    def episode_policy_sample(self, obs: torch.Tensor):
        """The policy and one draw on observation rows ``obs`` [E,D,20] (mds_episode_policy_sample): ``(rpm [E,D,4], sample [E,D,4],
        logp [E,D])``, new tensors -- the commanded RPM, the sample before the clamp and its log-probability (float32; float64 on a
        float64 env).  The draw is the one of each env's current ``count`` and ``length``: on the current observation and followed by
        ``step_episodes`` this is the policy-in-the-loop form of ``rollout_episodes_sampled``."""
        self._require_open()
        if obs.dtype != self.dtype or not obs.is_contiguous() or obs.numel() != self.n * capi.OBS_DIM or obs.device != self._obs.device:
            raise ValueError("obs must be a contiguous [E,D,20] device tensor of the env's dtype")
        rpm = torch.empty((self.NUM_ENVS, self.NUM_DRONES, capi.ACT_DIM), dtype=self.dtype, device=self._obs.device)
        sample = torch.empty_like(rpm)
        logp = torch.empty((self.NUM_ENVS, self.NUM_DRONES), dtype=self._episode_dtype(), device=self._obs.device)
        capi.check(self._lib.mds_episode_policy_sample(self._h, C.c_void_p(obs.data_ptr()), C.c_void_p(rpm.data_ptr()), C.c_void_p(sample.data_ptr()),
                                                       C.c_void_p(logp.data_ptr()), self._stream()),
                   "mds_episode_policy_sample")
        return rpm, sample, logp

    def rollout_episodes_sampled(self, first_step: int, n_steps: int, acted_obs_log: torch.Tensor | None = None, obs_log: torch.Tensor | None = None,
                                 action_log: torch.Tensor | None = None, sample_log: torch.Tensor | None = None, logp_log: torch.Tensor | None = None,
                                 reward_log: torch.Tensor | None = None, flags_log: torch.Tensor | None = None, steps_per_launch: int = 1):
        """``n_steps`` control steps of the configured policy with actions drawn in the kernel (mds_rollout_episodes_sampled), as
        ``rollout_episodes_policy`` otherwise.  Step j writes slot ``j % T`` of each log given: ``acted_obs_log`` [T,E,D,20] (the rows
        the action was drawn on: post-reset where the env was just done), ``obs_log`` [T,E,D,20] (the transition's rows, before any
        reset), ``action_log`` [T,E,D,4] (the commanded RPM), ``sample_log`` [T,E,D,4] (the sample before the clamp), ``logp_log``
        [T,E,D] (float32; float64 on a float64 env), ``reward_log`` [T,E], ``flags_log`` [T,E] int32.  Returns the current observation."""
        self._require_open()
        slots = set()
        n, E, rdt = self.n, self.NUM_ENVS, self._episode_dtype()
        logs = (("acted_obs_log", acted_obs_log, self.dtype, n * capi.OBS_DIM), ("obs_log", obs_log, self.dtype, n * capi.OBS_DIM),
                ("action_log", action_log, self.dtype, n * capi.ACT_DIM), ("sample_log", sample_log, self.dtype, n * capi.ACT_DIM),
                ("logp_log", logp_log, rdt, n), ("reward_log", reward_log, rdt, E), ("flags_log", flags_log, torch.int32, E))
        for name, log, dt, per in logs:
            if log is None:
                continue
            if log.dtype != dt or not log.is_contiguous() or log.numel() == 0 or log.numel() % per:
                raise ValueError(f"{name} must be a contiguous tensor of dtype {dt} with {per} values per step")
            slots.add(log.numel() // per)
        if len(slots) > 1:
            raise ValueError("the logs must hold the same number of steps")
        rings = capi.MdsEpisodeSampleRings(*(log.data_ptr() if log is not None else None for _, log, _, _ in logs))
        capi.check(self._lib.mds_rollout_episodes_sampled(self._h, C.c_int(int(first_step)), C.c_int(int(n_steps)), C.byref(rings),
                                                          C.c_int(slots.pop() if slots else 0), C.c_int(int(steps_per_launch)),
                                                          C.c_void_p(self._obs.data_ptr()), self._stream()),
                   "mds_rollout_episodes_sampled")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return self._obs

    def set_rollout_streams(self, n_streams: int = 0):
        """How rollout_geometric issues its steps: 0 auto, 1 the current stream only, 2 the two halves of the shard on two
        internal streams (mds_set_rollout_streams).  Same results either way."""
        self._require_open()
        capi.check(self._lib.mds_set_rollout_streams(self._h, C.c_int(int(n_streams))), "mds_set_rollout_streams")

    def last_rollout_streams(self) -> int:
        """1 or 2: how the most recent rollout_* call of this env was issued (0: none yet)."""
        self._require_open()
        return int(self._lib.mds_get_last_rollout_streams(self._h))

    def rollout_streams_for(self, n_steps: int, cbf: bool = False) -> int:
        """1 or 2: how a rollout of ``n_steps`` would be issued under the current ``set_rollout_streams`` setting."""
        self._require_open()
        return int(self._lib.mds_rollout_streams_for(self._h, C.c_int(1 if cbf else 0), C.c_int(int(n_steps))))

    def set_rollout_form(self, form: int = 0, steps_per_launch: int = 0):
        """How rollout_geometric launches its steps (mds_set_rollout_form): 0 auto (form 2 from 8 192 drones and 8 steps on), 1 one launch per control step
        (bit-identical to step_geometric calls at every shard size), 2 the whole-rollout kernel in launches of
        ``steps_per_launch`` control steps (state in registers; results equal to rounding)."""
        self._require_open()
        capi.check(self._lib.mds_set_rollout_form(self._h, C.c_int(int(form)), C.c_int(int(steps_per_launch))), "mds_set_rollout_form")

    def traj_yaw_free(self) -> bool:
        """True when every Lemniscate of the last ``set_trajectories`` has ``yaw_rate == 0`` (mds_traj_yaw_free): the fused geometric step and
        rollout then run the yaw-free kernels (results ``==`` the general ones'; only the sign of an exact zero may differ)."""
        self._require_open()
        return bool(self._lib.mds_traj_yaw_free(self._h))

    def set_traj_specialisation(self, on: bool = True):
        """``False`` keeps this env on the general kernels whatever its trajectories (mds_set_traj_specialisation; default on)."""
        self._require_open()
        capi.check(self._lib.mds_set_traj_specialisation(self._h, C.c_int(1 if on else 0)), "mds_set_traj_specialisation")

    def traj_phase_periodic(self) -> bool:
        """True when ``omega`` and ``phase_shift`` of the last ``set_trajectories`` repeat every 64 drones (mds_traj_phase_periodic): on a
        yaw-free env the whole-rollout kernel then reads sin / cos of the phase from the env's table (the same bits as computing them)."""
        self._require_open()
        return bool(self._lib.mds_traj_phase_periodic(self._h))

    def set_traj_phase_table(self, on: bool = True):
        """``False`` keeps the whole-rollout kernel computing the phase per drone and step (mds_set_traj_phase_table; default on)."""
        self._require_open()
        capi.check(self._lib.mds_set_traj_phase_table(self._h, C.c_int(1 if on else 0)), "mds_set_traj_phase_table")

    def last_rollout_phase_table(self) -> bool:
        """Whether the last whole-rollout launch read the phase table (mds_get_last_rollout_phase_table)."""
        self._require_open()
        return bool(self._lib.mds_get_last_rollout_phase_table(self._h))

    def traj_desired_periodic(self) -> bool:
        """True when ``a`` repeats every 64 drones as well as ``omega`` and ``phase_shift`` (mds_traj_desired_periodic): the env's table then
        holds what the controller reads of the desired state, not only sin / cos of the phase (the same bits as computing it)."""
        self._require_open()
        return bool(self._lib.mds_traj_desired_periodic(self._h))

    def set_traj_desired_table(self, on: bool = True):
        """``False`` falls back to the table of sin / cos pairs (mds_set_traj_desired_table; default on)."""
        self._require_open()
        capi.check(self._lib.mds_set_traj_desired_table(self._h, C.c_int(1 if on else 0)), "mds_set_traj_desired_table")

    def last_rollout_desired_table(self) -> bool:
        """Whether the last whole-rollout launch read the desired-state rows (mds_get_last_rollout_desired_table)."""
        self._require_open()
        return bool(self._lib.mds_get_last_rollout_desired_table(self._h))

    def rollout_form_for(self, n_steps: int) -> int:
        self._require_open()
        return int(self._lib.mds_rollout_form_for(self._h, C.c_int(int(n_steps))))

    def last_rollout_form(self) -> int:
        self._require_open()
        return int(self._lib.mds_get_last_rollout_form(self._h))

    def rollout_geometric_fused(self, t0: float, n_steps: int, log: bool = False, log_out: torch.Tensor | None = None,
                                controller: str = "geometric"):
        """``n_steps`` fused control steps in ONE kernel launch (state stays in registers).  With
        ``log`` every step's observation goes to a [T,E,D,20] tensor (the reference's
        ``observations.append(obs)``, EnvGeometric.py:471); returns (last obs, log or None).  ``controller="lqr"`` runs the
        12-state LQRController (constructed on this env) instead of GeometricControl.  Every step's slot of the log must start
        16-byte aligned: a log of more than one step on a ``float16`` env with an odd number of drones is refused (MDS_EALIGN)."""
        self._require_open()
        if log and log_out is None:
            log_out = torch.empty((n_steps, self.NUM_ENVS, self.NUM_DRONES, capi.OBS_DIM), dtype=self.dtype, device=self.device)
        fn = {"lqr": self._lib.mds_rollout_lqr_fused, "geometric": self._lib.mds_rollout_geometric_fused,
              "nominal": self._lib.mds_rollout_nominal_fused}[controller]   # "nominal": the LQR + low level chosen with set_cbf_nominal
        capi.check(fn(self._h, C.c_double(t0), C.c_int(n_steps), C.c_void_p(log_out.data_ptr() if log_out is not None else None),
                      C.c_void_p(self._obs.data_ptr()), self._stream()), "mds_rollout_*_fused")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return self._obs, log_out

    def set_dslpid_gains(self, ctrl):
        """Push the P/I/D_COEFF_FOR/TOR arrays of a DSLPIDControl object to this env (PIDEnv.py:124-134)."""
        from ..control.DSLPIDControl import gains_struct
        capi.check(self._lib.mds_set_dslpid_gains(self._h, C.byref(gains_struct(ctrl))), "mds_set_dslpid_gains")

    def step_dslpid(self, target_pos, target_rpy, return_action: bool = False):
        """MultiDroneEnv.sim_step (PIDEnv.py:161-176) for every drone: DSLPID towards target_pos / target_rpy
        ([E,D,3] or [D,3]), fused with env.step."""
        self._require_open()
        def prep(a):
            if not isinstance(a, torch.Tensor):
                a = np.asarray(a, dtype=np.float64)
                if a.shape == (self.NUM_DRONES, 3):
                    a = np.broadcast_to(a, (self.NUM_ENVS, self.NUM_DRONES, 3))
            return to_device(a, self.device, self.dtype).reshape(self.n, 3)
        tp, tr = prep(target_pos), prep(target_rpy)
        act_ptr = C.c_void_p(self._act.data_ptr()) if return_action else C.c_void_p(None)
        capi.check(self._lib.mds_step_dslpid(self._h, C.c_void_p(tp.data_ptr()), C.c_void_p(tr.data_ptr()), C.c_void_p(self._obs.data_ptr()),
                                             act_ptr, self._stream()), "mds_step_dslpid")
        self.step_counter += self.PYB_STEPS_PER_CTRL
        return (self._obs, self._act) if return_action else self._obs

    def dslpid_compute(self, obs, target_pos, target_rpy):
        """DSLPIDControl.computeControlFromState for every drone on the observations given ([E,D,20]; targets [E,D,3] or [D,3]):
        the controller of ``step_dslpid`` alone (``mds_dslpid_compute``).  It advances this env's PID memory and leaves the state
        untouched.  Returns the RPM [E,D,4] in a tensor of its own."""
        self._require_open()
        def prep(a, w):
            if not isinstance(a, torch.Tensor):
                a = np.asarray(a, dtype=np.float64)
                if a.shape == (self.NUM_DRONES, w):
                    a = np.broadcast_to(a, (self.NUM_ENVS, self.NUM_DRONES, w))
            return to_device(a, self.device, self.dtype).reshape(self.n, w)
        ob, tp, tr = prep(obs, capi.OBS_DIM), prep(target_pos, 3), prep(target_rpy, 3)
        rpm = torch.empty((self.NUM_ENVS, self.NUM_DRONES, capi.ACT_DIM), dtype=self.dtype, device=self.device)
        capi.check(self._lib.mds_dslpid_compute(self._h, C.c_void_p(ob.data_ptr()), C.c_void_p(tp.data_ptr()), C.c_void_p(tr.data_ptr()),
                                                C.c_void_p(rpm.data_ptr()), self._stream()), "mds_dslpid_compute")
        return rpm

    def rollout_dslpid(self, target_pos, target_rpy, n_steps: int, first_step: int = 0, obs_every_step: bool = False):
        """``for i in range(n_steps): env.sim_step()`` of PIDEnv.py:201-207 as one C call (``mds_rollout_dslpid``).  Targets:
        [D,3] / [E,D,3] (fixed, PIDEnv's TARGET_POSITIONS) or a waypoint table [W,E,D,3] used cyclically from ``first_step``.
        Returns the last observation."""
        self._require_open()
        def prep(a):
            if not isinstance(a, torch.Tensor):
                a = np.asarray(a, dtype=np.float64)
                if a.shape == (self.NUM_DRONES, 3):
                    a = np.broadcast_to(a, (self.NUM_ENVS, self.NUM_DRONES, 3))
            a = to_device(a, self.device, self.dtype)
            return a.reshape(-1, self.n, 3).contiguous()
        tp, tr = prep(target_pos), prep(target_rpy)
        if tp.shape != tr.shape:
            raise ValueError(f"target_pos {tuple(tp.shape)} and target_rpy {tuple(tr.shape)} must hold the same number of sets")
        capi.check(self._lib.mds_rollout_dslpid(self._h, C.c_void_p(tp.data_ptr()), C.c_void_p(tr.data_ptr()), C.c_int(tp.shape[0]),
                                                C.c_int(first_step), C.c_int(n_steps), C.c_void_p(self._obs.data_ptr()),
                                                C.c_int(1 if obs_every_step else 0), self._stream()), "mds_rollout_dslpid")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return self._obs

    def set_cbf_nominal(self, which: str):
        """Nominal controller of ``step_cbf_geometric``: "geometric" (GeometricControl return_omegas),
        "lqr_omega" (LQROmegaController), "lqr_yank_omega" (LQRYankOmegaController, the order-3 loop of
        simulations/CBFTestOrd3.py) or "dlqr_omega" (DecentralizedLQROmega, coupled over the drones of an env; order 2, the step loop
        only); the LQR ones need a controller constructed on this env first, "dlqr_omega" an uploaded gain."""
        capi.check(self._lib.mds_cbf_set_nominal(self._h, {"geometric": 0, "lqr_omega": 1, "lqr_yank_omega": 2, "dlqr_omega": 3}[which]),
                   "mds_cbf_set_nominal")

    def set_cbf_step_kernel(self, one_launch):
        """How the CBF-filtered step is issued (mds_cbf_set_step_kernel): False / 0 (default) the QP launch + the low-level launch,
        True / 1 one launch per control step where it applies (the faster of the two when few envs need active-set iterations),
        2 or "persistent" one launch of the several-steps-per-launch kernel per step (the fastest per-step form where it applies;
        ``rollout_cbf_geometric`` then runs 25 steps per launch)."""
        mode = 2 if one_launch == "persistent" else int(one_launch)
        capi.check(self._lib.mds_cbf_set_step_kernel(self._h, C.c_int(mode)), "mds_cbf_set_step_kernel")

    def cbf_step_inputs(self):
        """(u_hat, u_safe) [E, D, 4] of the last ``step_cbf_geometric``: the nominal input as the filter saw it and the filter's
        output, both without the hover force (mds_cbf_get_step_inputs; the QP launch + low-level launch form only)."""
        self._require_open()
        u = torch.empty((2, self.NUM_ENVS, self.NUM_DRONES, 4), dtype=self.dtype, device=self.device)
        capi.check(self._lib.mds_cbf_get_step_inputs(self._h, C.c_void_p(u[0].data_ptr()), C.c_void_p(u[1].data_ptr()), self._stream()),
                   "mds_cbf_get_step_inputs")
        return u[0], u[1]

    def cbf_last_step_kernel(self) -> int:
        """2: the most recent CBF-filtered step ran in the several-steps-per-launch kernel, 1: as one launch, 0: as QP launch +
        low-level launch, -1: none yet."""
        return int(self._lib.mds_cbf_last_step_kernel(self._h))

    def step_cbf_geometric(self, t: float, tracker, x_obs=None, obs_r_list=None, return_action: bool = False):
        """One CBF-filtered control step of simulations/CBFTest.py:303-350 for every env: nominal
        (force - M G, w_des) -> ``tracker`` (DroneQPTracker) ECBF QP -> ThrustOmega low level -> env.step; with an
        order-3 ``tracker.cbf`` the loop of simulations/CBFTestOrd3.py:306-352 (yank-omega LQR nominal, YankOmega low
        level).  Uses and updates the env's current observation; returns (obs, status[E])."""
        self._require_open()
        tracker.cbf.configure(x_obs, obs_r_list)
        if getattr(self, "_cbf_status", None) is None:
            self._cbf_status = torch.zeros((self.NUM_ENVS,), dtype=torch.int32, device=self.device)
        act_ptr = C.c_void_p(self._act.data_ptr()) if return_action else C.c_void_p(None)
        capi.check(self._lib.mds_step_cbf_geometric(self._h, C.c_double(t), C.c_void_p(self._obs.data_ptr()),
                                                    C.c_void_p(self._cbf_status.data_ptr()), act_ptr, self._stream()),
                   "mds_step_cbf_geometric")
        self.step_counter += self.PYB_STEPS_PER_CTRL
        return (self._obs, self._cbf_status, self._act) if return_action else (self._obs, self._cbf_status)

    def rollout_cbf_geometric(self, t0: float, n_steps: int, tracker, x_obs=None, obs_r_list=None):
        """``n_steps`` of ``step_cbf_geometric`` enqueued from C (mds_rollout_cbf_geometric); returns (obs, status) of the last step.
        Large batches run as two env halves on two internal streams (``set_rollout_streams``)."""
        self._require_open()
        tracker.cbf.configure(x_obs, obs_r_list)
        if getattr(self, "_cbf_status", None) is None:
            self._cbf_status = torch.zeros((self.NUM_ENVS,), dtype=torch.int32, device=self.device)
        capi.check(self._lib.mds_rollout_cbf_geometric(self._h, C.c_double(t0), C.c_int(n_steps), C.c_void_p(self._obs.data_ptr()),
                                                       C.c_void_p(self._cbf_status.data_ptr()), self._stream()),
                   "mds_rollout_cbf_geometric")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return self._obs, self._cbf_status

    def rollout_cbf_geometric_fused(self, t0: float, n_steps: int, tracker, x_obs=None, obs_r_list=None, steps_per_launch: int = 20,
                                    obs_log: torch.Tensor | None = None, first_slot: int = 0, status_log: torch.Tensor | None = None):
        """``n_steps`` of ``step_cbf_geometric`` with ``steps_per_launch`` control steps per launch (mds_rollout_cbf_geometric_fused: the
        persistent kernel -- state, nominal input and QP results stay on the chip between steps).  ``obs_log``: optional ring
        ``[slots, E, D, 20]``, step k writes slot ``(first_slot + k) % slots``; ``status_log``: optional int32 ``[n_steps, E]``.
        Returns (obs, status) of the last step."""
        self._require_open()
        tracker.cbf.configure(x_obs, obs_r_list)
        if getattr(self, "_cbf_status", None) is None:
            self._cbf_status = torch.zeros((self.NUM_ENVS,), dtype=torch.int32, device=self.device)
        slots = 0
        if obs_log is not None:
            if obs_log.dtype != self.dtype or obs_log.device != self.device or not obs_log.is_contiguous() or obs_log[0].numel() != self.n * capi.OBS_DIM:
                raise ValueError("obs_log must be a contiguous [slots, E, D, 20] tensor of the env's dtype on its device")
            slots = int(obs_log.shape[0])
        if status_log is not None and (status_log.dtype != torch.int32 or status_log.device != self.device or not status_log.is_contiguous()
                                       or status_log.numel() < n_steps * self.NUM_ENVS):
            raise ValueError("status_log must be a contiguous int32 [n_steps, E] tensor on the env's device")
        capi.check(self._lib.mds_rollout_cbf_geometric_fused(
            self._h, C.c_double(t0), C.c_int(n_steps), C.c_int(steps_per_launch),
            C.c_void_p(obs_log.data_ptr() if obs_log is not None else None), C.c_int(slots), C.c_int(first_slot),
            C.c_void_p(self._obs.data_ptr()), C.c_void_p(self._cbf_status.data_ptr()),
            C.c_void_p(status_log.data_ptr() if status_log is not None else None), self._stream()), "mds_rollout_cbf_geometric_fused")
        self.step_counter += n_steps * self.PYB_STEPS_PER_CTRL
        return self._obs, self._cbf_status

    def step_nominal(self, t: float, return_action: bool = False):
        """``ctrl[j].compute(obs[j])`` + ``env.step(action)`` of simulations/EnvGeometricOmega.py / EnvGeometricYankOmega.py for every
        drone: the LQR selected with ``set_cbf_nominal`` ("lqr_omega" | "lqr_yank_omega"), its low-level controller, the physics step.
        No safety filter.  Uses and updates the env's current observation."""
        self._require_open()
        act_ptr = C.c_void_p(self._act.data_ptr()) if return_action else C.c_void_p(None)
        capi.check(self._lib.mds_step_nominal(self._h, C.c_double(t), C.c_void_p(self._obs.data_ptr()), act_ptr, self._stream()),
                   "mds_step_nominal")
        self.step_counter += self.PYB_STEPS_PER_CTRL
        return (self._obs, self._act) if return_action else self._obs

    # ------------------------------------------------------------------ gym hooks (CtrlAviary fills them)
    def _computeReward(self):
        raise NotImplementedError

    def _computeTerminated(self):
        raise NotImplementedError

    def _computeTruncated(self):
        raise NotImplementedError

    def _computeInfo(self):
        raise NotImplementedError
