"""Randomizer — observation / action noise domain randomization (reference:
utils/domain_randomization/randomize.py:38-306, applied from envs/vec_env_rlgames.py:59-60,70-71).

Same configuration surface — the task YAML's ``domain_randomization`` block::

    domain_randomization:
      randomize: True
      randomization_params:
        observations: {on_reset: {operation, distribution, distribution_parameters},
                       on_interval: {frequency_interval, operation, distribution, distribution_parameters}}
        actions: {...same...}

with the same validation errors, flags (``task.randomize_observations`` / ``randomize_actions``)
and apply methods. The noise itself runs in HIP (include/mi_dr.h): inside the fused env-step
launch when VecEnvRLGames takes the fused path, or as one kernel per apply call
(``mi_dr_apply_actions`` / ``mi_dr_apply_observations``) on the method-by-method path.

Physics-parameter randomization (``simulation``, ``rigid_prim_views``, ``articulation_views``:
randomize.py:308-430) drives omni.replicator over PhysX views in the reference. Here the GPU
pipeline models four per-env parameters (include/mi_sim.h mi_set_env_params) and schedules them
in one HIP kernel per step (include/mi_dr_phys.h, mi_dr_phys_step)::

    simulation.gravity                                   -> gravity        (dim 3)
    articulation_views.<robot view>.damping              -> joint damping  (dim num_dof)
    articulation_views.<robot view>.joint_armatures      -> joint armature (dim num_dof)
    articulation_views.<robot view>.material_properties  -> friction       (dim num_bodies x 3)
    rigid_prim_views.<robot view>.material_properties    -> friction       (dim 3)

Deviations: one material per env (the dynamic-friction column drives the env's single friction
coefficient; a schedule that changes the static-friction or restitution column is refused); all
on_interval schedules share one frequency_interval; every other attribute the reference knows is
refused with NotImplementedError naming it. On the CPU pipeline the whole physics half stays
refused.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import native as N

_OPS = {"additive": N.MI_DR_OP_ADDITIVE, "scaling": N.MI_DR_OP_SCALING}
_DISTS = {"gaussian": N.MI_DR_DIST_GAUSSIAN, "normal": N.MI_DR_DIST_GAUSSIAN,
          "uniform": N.MI_DR_DIST_UNIFORM, "loguniform": N.MI_DR_DIST_LOGUNIFORM,
          "log_uniform": N.MI_DR_DIST_LOGUNIFORM}
_PHYSICS_GROUPS = ("simulation", "rigid_prim_views", "articulation_views")


_PHYS_OPS = {"additive": N.MI_DR_OP_ADDITIVE, "scaling": N.MI_DR_OP_SCALING, "direct": N.MI_DR_OP_DIRECT}
# omni.replicator.isaac's attribute lists (docs/domain_randomization.md:178-231)
SIMULATION_CONTEXT_ATTRIBUTES = ("gravity",)
RIGID_PRIM_ATTRIBUTES = ("position", "orientation", "linear_velocity", "angular_velocity", "velocity", "force",
                         "mass", "inertia", "material_properties", "contact_offset", "rest_offset", "scale",
                         "density")
ARTICULATION_ATTRIBUTES = ("position", "orientation", "linear_velocity", "angular_velocity", "velocity",
                           "stiffness", "damping", "joint_friction", "joint_positions", "joint_velocities",
                           "lower_dof_limits", "upper_dof_limits", "max_efforts", "joint_armatures",
                           "joint_max_velocities", "joint_efforts", "body_masses", "body_inertias",
                           "material_properties", "tendon_stiffnesses", "tendon_dampings",
                           "tendon_limit_stiffnesses", "tendon_lower_limits", "tendon_upper_limits",
                           "tendon_rest_lengths", "tendon_offsets", "scale")
_MATERIAL_COLUMNS = ("static friction", "dynamic friction", "restitution")


def sanitize_distribution_parameters(view_name, attribute, dimension, params):
    """randomize.py:445-458: [a, b] broadcast to `dimension`, [[...], [...]] of exactly that
    dimension, or one body's 3 material columns repeated over the bodies."""
    dp = np.array(params, dtype=np.float64)
    if dp.shape == (2,):
        return np.repeat(dp[:, None], dimension, axis=1)
    if dp.shape == (2, dimension):
        return dp
    if attribute in ("material_properties", "body_inertias") and dp.shape == (2, 3):
        return np.tile(dp, (1, dimension // 3))
    raise ValueError(f"The provided distribution_parameters for {view_name} {attribute} is invalid due to "
                     f"incorrect dimensions.")


def _neutral(op: str, dist: str, p0: float, p1: float) -> bool:
    """A schedule that leaves its operand unchanged whatever it draws."""
    one = 0.0 if op == "additive" else 1.0 if op == "scaling" else None
    if one is None:
        return False
    if dist in ("gaussian", "normal"):
        return p0 == one and p1 == 0.0
    return p0 == one and p1 == one


class PhysicsSchedule:
    """One on_reset / on_interval schedule of one attribute, in the reference's dimension
    (`params`, [2, ref_dim]) and in the native one (`native()`, two float32 [dim])."""

    def __init__(self, path, attr, when, view_name, attribute, ref_dim, cfg):
        self.path, self.attr, self.when = path, attr, when
        self.view_name, self.attribute, self.ref_dim = view_name, attribute, ref_dim
        self.operation, self.distribution = cfg["operation"], cfg["distribution"]
        if self.operation not in _PHYS_OPS:
            raise ValueError(f"The specified {self.operation} operation type is not supported.")
        if self.distribution not in _DISTS:
            raise ValueError(f"The provided distribution for {view_name} {attribute} is not supported. "
                             "Options: uniform, gaussian/normal, loguniform/log_uniform")
        self.frequency_interval = int(cfg.get("frequency_interval", 1))
        self.initial = np.array(cfg["distribution_parameters"])   # as given (randomize.py:317)
        self.set_params(cfg["distribution_parameters"])

    def set_params(self, distribution_parameters) -> None:
        dp = sanitize_distribution_parameters(self.view_name, self.attribute, self.ref_dim, distribution_parameters)
        if self.attribute == "material_properties":
            cols = dp.reshape(2, -1, 3)
            if not (cols == cols[:, :1, :]).all():
                raise NotImplementedError(f"{self.view_name} material_properties: per-body materials are not "
                                          f"modelled (one material per env)")
            for c in (0, 2):
                if self.operation == "direct":
                    raise NotImplementedError(
                        f"{self.view_name} material_properties: a direct schedule sets the "
                        f"{_MATERIAL_COLUMNS[c]} column too, which is not modelled (use additive or scaling "
                        f"with a neutral {_MATERIAL_COLUMNS[c]} column)")
                if not _neutral(self.operation, self.distribution, cols[0, 0, c], cols[1, 0, c]):
                    raise NotImplementedError(
                        f"{self.view_name} material_properties: randomizing the {_MATERIAL_COLUMNS[c]} column "
                        f"is not modelled (only the dynamic friction column drives the env's friction)")
        self.params = dp

    def native(self):
        dp = self.params
        if self.attribute == "material_properties":
            dp = dp[:, 1:2]
        return np.ascontiguousarray(dp[0], np.float32), np.ascontiguousarray(dp[1], np.float32)


def _schedules(group, view_name, attribute, attr, ref_dim, params, what):
    """The on_reset / on_interval schedules of one attribute with the reference's required-key
    errors (randomize.py:313-316,329-331,349-352,368-370,393-396,412-414)."""
    out = []
    for when in ("on_reset", "on_interval"):
        if when not in params:
            continue
        need = ("operation", "distribution", "distribution_parameters")
        if when == "on_interval":
            need = ("frequency_interval",) + need
        if not set(need).issubset(params[when]):
            raise ValueError(f"Please ensure the following randomization parameters for {what} {when} "
                             f"are provided: " + ", ".join(need) + ".")
        path = (group, attribute, when) if group == "simulation" else (group, view_name, attribute, when)
        out.append(PhysicsSchedule(path, attr, when, view_name, attribute, ref_dim, params[when]))
    return out


def parse_physics_randomization(randomization_params, num_dof: int, num_bodies: int, view_name: str) -> list:
    """The `simulation`, `rigid_prim_views` and `articulation_views` groups of a
    `randomization_params` block -> [PhysicsSchedule] (randomize.py:137-162,308-430), for a robot
    view `view_name` of `num_dof` joints and `num_bodies` bodies. No device needed."""
    rp = randomization_params
    out = []
    sim = rp.get("simulation")
    if sim is not None:
        for attribute, params in sim.items():
            if params is None:
                raise ValueError(f"Randomization parameters for simulation {attribute} is not provided.")
            if attribute not in SIMULATION_CONTEXT_ATTRIBUTES:
                raise ValueError(f"The attribute {attribute} for simulation is invalid for domain randomization.")
            out += _schedules("simulation", "simulation", attribute, N.MI_ENVP_GRAVITY, 3, params,
                              f"simulation {attribute}")
    modelled = {"articulation_views": {"damping": (N.MI_ENVP_DAMPING, num_dof),
                                       "joint_armatures": (N.MI_ENVP_ARMATURE, num_dof),
                                       "material_properties": (N.MI_ENVP_FRICTION, 3 * num_bodies)},
                "rigid_prim_views": {"material_properties": (N.MI_ENVP_FRICTION, 3)}}
    known = {"articulation_views": ARTICULATION_ATTRIBUTES, "rigid_prim_views": RIGID_PRIM_ATTRIBUTES}
    for group in ("rigid_prim_views", "articulation_views"):
        views = rp.get(group)
        if views is None:
            continue
        kind = "rigid prim view" if group == "rigid_prim_views" else "articulation view"
        for name, attrs in views.items():
            if attrs is None:
                continue
            if name != view_name:
                raise ValueError(f"{group}: the view {name} is not part of this scene (the robot view is "
                                 f"{view_name})")
            for attribute, params in attrs.items():
                if params is None:
                    raise ValueError(f"Randomization parameters for {kind} {name} {attribute} is not provided.")
                if attribute not in known[group]:
                    raise ValueError(f"The attribute {attribute} for {name} is invalid for domain randomization.")
                if "on_startup" in params:
                    raise NotImplementedError(f"{name} {attribute}: on_startup randomization ({attribute}) is "
                                              f"not modelled by this build")
                if attribute not in modelled[group]:
                    raise NotImplementedError(f"{name} {attribute}: the attribute {attribute} is not modelled by "
                                              f"this build (gravity, damping, joint_armatures and "
                                              f"material_properties are)")
                attr, ref_dim = modelled[group][attribute]
                out += _schedules(group, name, attribute, attr, ref_dim, params, f"{name} {attribute}")
    seen = {}
    for sc in out:
        if (sc.attr, sc.when) in seen:
            raise ValueError(f"{'/'.join(sc.path)} and {'/'.join(seen[(sc.attr, sc.when)])} both drive the env's "
                             f"friction coefficient")
        seen[(sc.attr, sc.when)] = sc.path
    freqs = {sc.frequency_interval for sc in out if sc.when == "on_interval"}
    if len(freqs) > 1:
        raise ValueError(f"physics on_interval schedules share one frequency_interval in this build, got "
                         f"{sorted(freqs)}")
    return out


def physics_params_struct(schedules: list, min_frequency: int):
    """[PhysicsSchedule] -> (mi_dr_phys_params, the host arrays it points to)."""
    dr = N.MiDrPhysParams()
    dr.min_frequency = int(min_frequency)
    keep = []
    for sc in schedules:
        c = (dr.on_interval if sc.when == "on_interval" else dr.on_reset)[sc.attr]
        p0, p1 = sc.native()
        keep += [p0, p1]
        c.enabled = 1
        c.operation = _PHYS_OPS[sc.operation]
        c.distribution = _DISTS[sc.distribution]
        c.frequency_interval = sc.frequency_interval
        c.p0, c.p1 = N.fptr(p0), N.fptr(p1)
    return dr, keep


def _noise(params: dict, what: str, interval: bool) -> N.MiDrNoise:
    """One schedule -> mi_dr_noise, with the reference's required-key checks
    (randomize.py:183-191 / 200-208)."""
    need = {"operation", "distribution", "distribution_parameters"}
    if interval:
        need = need | {"frequency_interval"}
    if not need.issubset(params.keys()):
        kind = "on_interval" if interval else "on_reset"
        raise ValueError(f"Please ensure the following {what} {kind} randomization parameters are "
                         f"provided: " + ", ".join(sorted(need)) + ".")
    op, dist = params["operation"], params["distribution"]
    if op not in _OPS:
        raise ValueError(f"The specified {op} operation type is not supported.")
    if dist not in _DISTS:
        raise ValueError(f"The specified {dist} distribution is not supported.")
    p = [float(v) for v in params["distribution_parameters"]]
    if len(p) != 2:
        raise ValueError(f"{what}: distribution_parameters must hold 2 scalars, got {p}")
    n = N.MiDrNoise()
    n.enabled = 1
    n.operation = _OPS[op]
    n.distribution = _DISTS[dist]
    n.frequency_interval = int(params.get("frequency_interval", 1))
    n.params[0], n.params[1] = p
    return n


class Randomizer:
    def __init__(self, sim_config) -> None:
        """randomize.py:39-55."""
        self._cfg = sim_config.task_config
        self._config = sim_config.config
        self.randomize = False
        self.distributions = dict()
        self.active_domain_randomizations = dict()
        self._observations_dr_params = None
        self._actions_dr_params = None
        self._task = None
        dr_config = self._cfg.get("domain_randomization", None)
        if dr_config is not None:
            randomize = dr_config.get("randomize", False)
            randomization_params = dr_config.get("randomization_params", None)
            if randomize and randomization_params is not None:
                self.randomize = True
                self.min_frequency = dr_config.get("min_frequency", 1)

    def _physics_groups(self) -> list:
        rp = self._cfg["domain_randomization"]["randomization_params"]
        return [g for g in _PHYSICS_GROUPS if rp.get(g) is not None]

    def _cpu_pipeline(self) -> bool:
        return str(self._config.get("sim_device", "")).startswith("cpu")

    def _refuse_physics(self, groups, task) -> None:
        why = ("needs a task with a robot view on the GPU pipeline" if task is None
               else "is not part of this build on the CPU pipeline")
        raise NotImplementedError(
            f"physics-parameter domain randomization ({', '.join(groups)}) {why} "
            f"(observation / action noise only)")

    def apply_on_startup_domain_randomization(self, task) -> None:
        """randomize.py:57-124: on_startup scale / mass / density of prim views."""
        if self.randomize:
            groups = self._physics_groups()
            if groups and (task is None or self._cpu_pipeline()):
                self._refuse_physics(groups, task)
            rp = self._cfg["domain_randomization"]["randomization_params"]
            for group in ("rigid_prim_views", "articulation_views"):
                for name, attrs in (rp.get(group) or {}).items():
                    for attribute, params in (attrs or {}).items():
                        if params is not None and "on_startup" in params:
                            raise NotImplementedError(f"{name} {attribute}: on_startup randomization "
                                                      f"({attribute}) is not modelled by this build")
        elif self._cfg.get("domain_randomization", None) is None:
            raise ValueError("No domain randomization parameters are specified in the task yaml config file")
        else:
            print("On Startup Domain randomization will not be applied.")

    def set_up_domain_randomization(self, task) -> None:
        """randomize.py:126-174: registers the observation / action schedules with the task's
        mi_sim handle (mi_task_set_dr) and sets task.randomize_observations / randomize_actions."""
        if not self.randomize:
            if self._cfg.get("domain_randomization", None) is None:
                raise ValueError("No domain randomization parameters are specified in the task yaml config file")
            print("Domain randomization will not be applied.")
            return
        groups = self._physics_groups()
        if groups and (task is None or self._cpu_pipeline()):
            self._refuse_physics(groups, task)
        rp = self._cfg["domain_randomization"]["randomization_params"]
        if groups:
            view = task.get_robot()
            self._set_up_physics_randomization(parse_physics_randomization(
                rp, view.num_dof, view.model.num_links, view.name), view)
        dr = N.MiDrParams()
        for key, which in (("observations", "obs"), ("actions", "act")):
            if key not in rp:
                continue
            params = rp[key]
            if params is None:
                raise ValueError(f"{key.capitalize()} randomization parameters are not provided.")
            if key == "observations":
                task.randomize_observations = True
                self._observations_dr_params = params
            else:
                task.randomize_actions = True
                self._actions_dr_params = params
            if "on_reset" in params:
                setattr(dr, f"{which}_on_reset", _noise(params["on_reset"], key, False))
                self.active_domain_randomizations[(key, "on_reset")] = list(params["on_reset"]["distribution_parameters"])
            if "on_interval" in params:
                setattr(dr, f"{which}_on_interval", _noise(params["on_interval"], key, True))
                self.active_domain_randomizations[(key, "on_interval")] = list(params["on_interval"]["distribution_parameters"])
        self._dr = dr
        self._task = task
        view = task.get_robot()
        N.check(N.lib().mi_task_set_dr(view.handle, C.byref(dr)), "mi_task_set_dr")

    def params(self):
        """The mi_dr_params registered with the sim (None before set-up)."""
        return getattr(self, "_dr", None)

    # -- physics groups (randomize.py:308-430,461-510) ---------------------------------------
    def _set_up_physics_randomization(self, schedules: list, view=None) -> None:
        """Keeps the parsed schedules (distributions / active_domain_randomizations with the
        reference's keys) and, with a view, registers them (mi_sim_set_phys_dr)."""
        self._phys = {sc.path: sc for sc in schedules}
        self._phys_view = view
        for sc in schedules:
            d = self.distributions.setdefault(sc.path[0], dict())
            for key in sc.path[1:-1]:
                d = d.setdefault(key, dict())
            d[sc.path[-1]] = sc
            self.active_domain_randomizations[sc.path] = sc.initial.copy()
        self._register_physics()

    def _register_physics(self) -> None:
        self._phys_dr, self._phys_keep = physics_params_struct(list(self._phys.values()), self.min_frequency)
        if self._phys_view is not None:
            N.check(N.lib().mi_sim_set_phys_dr(self._phys_view.handle, C.byref(self._phys_dr)), "mi_sim_set_phys_dr")

    def physics_schedules(self) -> list:
        return list(getattr(self, "_phys", {}).values())

    def step_physics_randomization(self, reset_buf) -> None:
        """dr.physics_view.step_randomization(reset_inds) (in_hand_manipulation.py:271-275) as a
        mask, for the method-by-method step (the fused launch issues it itself)."""
        view = getattr(self, "_phys_view", None)
        if view is not None and self._phys:
            N.check(N.lib().mi_dr_phys_step(view.handle, reset_buf.data_ptr(), view.stream()), "mi_dr_phys_step")

    def _path(self, distribution_path):
        if distribution_path not in self.active_domain_randomizations.keys():
            raise ValueError(f"Cannot find a valid domain randomization distribution using the path {distribution_path}.")
        return distribution_path

    def set_dr_distribution_parameters(self, distribution_parameters, *distribution_path):
        """randomize.py:461-488. A physics schedule is re-registered; per-env state is kept."""
        path = self._path(distribution_path)
        if path[0] in ("observations", "actions"):
            # mi_task_set_dr zeroes the noise schedules' per-env state: not re-registered here
            raise NotImplementedError(f"{path[0]} noise parameters are fixed at set-up in this build")
        self._phys[path].set_params(distribution_parameters)
        self._register_physics()

    def get_dr_distribution_parameters(self, *distribution_path):
        """randomize.py:490-505: [lower, upper] | [mean, std] in the reference's dimension."""
        path = self._path(distribution_path)
        if path[0] == "observations":
            return self._observations_dr_params[path[1]]["distribution_parameters"]
        if path[0] == "actions":
            return self._actions_dr_params[path[1]]["distribution_parameters"]
        return self._phys[path].params.tolist()

    def get_initial_dr_distribution_parameters(self, *distribution_path):
        """randomize.py:507-510."""
        p = self.active_domain_randomizations[self._path(distribution_path)]
        return p.copy() if hasattr(p, "copy") else list(p)

    # -- the two apply calls of VecEnvRLGames.step's method-by-method path ------------------
    def apply_actions_randomization(self, actions, reset_buf):
        """randomize.py:237-260: in place on the clamped [N, A] actions."""
        view = self._task.get_robot()
        a = actions.contiguous()
        N.check(N.lib().mi_dr_apply_actions(view.handle, a.data_ptr(), reset_buf.data_ptr(),
                                            view.stream()), "mi_dr_apply_actions")
        if a.data_ptr() != actions.data_ptr():
            actions.copy_(a)
        return actions

    def apply_observations_randomization(self, observations, reset_buf):
        """randomize.py:212-235: in place on task.obs_buf."""
        view = self._task.get_robot()
        if not observations.is_contiguous():
            raise ValueError("observations must be contiguous (task.obs_buf)")
        N.check(N.lib().mi_dr_apply_observations(view.handle, observations.data_ptr(),
                                                 reset_buf.data_ptr(), view.stream()),
                "mi_dr_apply_observations")
        return observations
