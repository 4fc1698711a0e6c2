"""Scene pieces the reference takes from closed Isaac Sim packages, rebuilt over libmi_sim.so:

* :class:`GridCloner` — env-origin grid of omni.isaac.cloner (used at tasks/base/rl_task.py:92,
  124-126). Restated from its public behaviour; the closed source is absent, so the exact
  layout is unverified.
* :class:`ArticulationView` — the omni.isaac.core tensor API the tasks call
  (get_world_poses / get_velocities / get_joint_positions / get_joint_velocities /
  set_* with indices / get_dof_limits / get_dof_index / _physics_view.get_force_sensor_forces,
  call sites tasks/shared/locomotion.py:81-89,114,130-134, tasks/cartpole.py:81-82,112,
  129-130,137-138). Every getter and setter is one HIP gather / scatter kernel on torch's
  current stream; the physics state itself never leaves HBM.
* :func:`Humanoid` / :func:`Ant` / :func:`Cartpole` — robot constructors
  (robots/articulations/{humanoid,ant,cartpole}.py) returning compiled model descriptions.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Optional

import numpy as np
import torch

from .. import native as N
from .model import CompiledModel, load_robot


class GridCloner:
    def __init__(self, spacing: float, num_per_row: int = -1):
        self._spacing = float(spacing)
        self._num_per_row = num_per_row

    def get_clone_positions(self, num_clones: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """[count, 3] origins of envs first..first+count-1 of a num_clones grid."""
        count = num_clones - first if count is None else count
        per_row = self._num_per_row if self._num_per_row > 0 else int(np.sqrt(num_clones))
        num_rows = np.ceil(num_clones / per_row)
        num_cols = np.ceil(num_clones / num_rows)
        row_offset = 0.5 * self._spacing * (num_rows - 1)
        col_offset = 0.5 * self._spacing * (num_cols - 1)
        i = np.arange(first, first + count, dtype=np.float64)
        row = np.floor(i / num_cols)
        col = i - row * num_cols
        x = row_offset - row * self._spacing
        y = col * self._spacing - col_offset
        return np.stack([x, y, np.zeros_like(x)], axis=1).astype(np.float32)


def Humanoid() -> CompiledModel:
    return load_robot("Humanoid")


def Ant() -> CompiledModel:
    return load_robot("Ant")


def Cartpole() -> CompiledModel:
    return load_robot("Cartpole")


class _PhysicsView:
    """``ArticulationView._physics_view`` (omni.physics.tensors) — force sensors only."""

    def __init__(self, view: "ArticulationView"):
        self._view = view

    def get_force_sensor_forces(self) -> torch.Tensor:
        """[count, S, 6] sensor wrenches: the view's state mirror (omni.physics.tensors hands out
        its own buffer as well; locomotion.py:89 only reads it before the next step)."""
        v = self._view
        v._refresh_mirror()
        return v._mir_sens


class ArticulationView:
    """One articulation replicated over ``count`` envs, backed by one mi_sim handle."""

    def __init__(self, model: CompiledModel, name: str = "view", prim_paths_expr: str = "",
                 reset_xform_properties: bool = False):
        self.model = model
        self.name = name
        self.prim_paths_expr = prim_paths_expr
        self.handle = None
        self.count = 0
        self.device = None
        self._desc = None
        self._physics_view = _PhysicsView(self)

    # ---- lifecycle (called by Scene.add / World) ----
    def initialize(self, sim_params: "N.MiSimParams", num_envs: int, env_origins: np.ndarray,
                   device: str, seed: int, env_id_offset: int = 0) -> None:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise N.NativeUnavailable(
                f"sim_device={device!r}: libmi_sim.so runs on the GPU only (no CPU fallback; the "
                f"CPU pipeline, robots/cpu_cartpole.py, serves the Cartpole task alone)")
        lib = N.lib()
        self.device = dev
        self.count = int(num_envs)
        self.sim_params = sim_params
        self._desc = self.model.to_desc()
        origins = np.ascontiguousarray(env_origins, dtype=np.float32).reshape(self.count, 3)
        h = C.c_void_p()
        dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        N.check(lib.mi_sim_create(self._desc.ref(), C.byref(sim_params), self.count,
                                  int(env_id_offset), int(dev_index),
                                  origins.ctypes.data, int(seed), C.byref(h)), "mi_sim_create")
        self.handle = h.value
        self.env_origins = origins
        # hot-path bindings (resolved once: the ArticulationView calls are per env-step)
        self._lib = lib
        self._dev_index = int(dev_index)
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        # state mirrors (include/mi_sim.h mi_sim_set_mirror): the tensors the getters hand out
        n, D, S = self.count, self.num_dof, self.num_sensors
        f32 = dict(dtype=torch.float32, device=dev)
        self._mir_pos, self._mir_rot = torch.zeros((n, 3), **f32), torch.zeros((n, 4), **f32)
        self._mir_vel = torch.zeros((n, 6), **f32)
        self._mir_q, self._mir_qd = torch.zeros((n, D), **f32), torch.zeros((n, D), **f32)
        self._mir_sens = torch.zeros((n, S, 6), **f32)
        N.check(lib.mi_sim_set_mirror(self.handle, self._mir_pos.data_ptr(), self._mir_rot.data_ptr(),
                                      self._mir_vel.data_ptr(), self._mir_q.data_ptr(),
                                      self._mir_qd.data_ptr(),
                                      self._mir_sens.data_ptr() if S else None), "mi_sim_set_mirror")

    def close(self) -> None:
        if self.handle:
            N.lib().mi_sim_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self) -> int:
        if self._raw_stream is not None:
            return self._raw_stream(self._dev_index)
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- sizes ----
    @property
    def num_dof(self) -> int:
        return self.model.num_dof

    @property
    def num_sensors(self) -> int:
        return self.model.num_sensors

    @property
    def dof_names(self):
        return list(self.model.dof_names)

    def get_dof_index(self, name: str) -> int:
        return self.model.get_dof_index(name)

    def get_dof_limits(self) -> torch.Tensor:
        lim = torch.from_numpy(self.model.dof_limits())
        return lim.unsqueeze(0).repeat(self.count, 1, 1).to(self.device)

    # ---- getters ----
    # Getters hand out the view's state mirrors (row-major copies the library refreshes in ONE
    # launch after the state changed, include/mi_sim.h mi_get_state_mirror): with clone=False the
    # mirror itself, which the next physics step overwrites — Isaac's clone=False returns its
    # internal buffer the same way (locomotion.py:81-88 reads them before stepping again); with
    # clone=True (the default) a copy. Contract (include/mi_sim.h): a clone=False result, and
    # get_force_sensor_forces', is read-only — an in-place edit would persist into later getters
    # until the state changes (the reference only reads them, locomotion.py:81-89). A read on
    # another stream than the refresh's is ordered after it by the library (event wait).
    def _empty(self, *shape) -> torch.Tensor:
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _refresh_mirror(self) -> None:
        rc = self._lib.mi_get_state_mirror(self.handle, self.stream())
        if rc:
            N.check(rc, "mi_get_state_mirror")

    @staticmethod
    def _out(t: torch.Tensor, indices, clone: bool) -> torch.Tensor:
        if indices is not None:
            return t[indices.long()]
        return t.clone() if clone else t

    def get_world_poses(self, indices=None, clone: bool = True):
        self._refresh_mirror()
        return self._out(self._mir_pos, indices, clone), self._out(self._mir_rot, indices, clone)

    def get_velocities(self, indices=None, clone: bool = True) -> torch.Tensor:
        self._refresh_mirror()
        return self._out(self._mir_vel, indices, clone)

    def get_joint_positions(self, indices=None, clone: bool = True) -> torch.Tensor:
        self._refresh_mirror()
        return self._out(self._mir_q, indices, clone)

    def get_joint_velocities(self, indices=None, clone: bool = True) -> torch.Tensor:
        self._refresh_mirror()
        return self._out(self._mir_qd, indices, clone)

    # ---- bodies: link-frame view (include/mi_sim.h mi_get_link_state / mi_get_link_jacobian) ----
    @property
    def body_names(self):
        return list(self.model.body_names)

    @property
    def num_bodies(self) -> int:
        return self.model.num_bodies

    def get_body_index(self, name: str) -> int:
        return self.model.get_body_index(name)

    @property
    def num_gen_vel(self) -> int:
        """nv: columns of a Jacobian — (root lin, root ang, qd) for a floating root, else qd."""
        return self.num_dof + (6 if self.model.root_free else 0)

    def _frames(self, body_names):
        """(link ids int32 [K], offsets float32 [K,3]) of the named bodies' frames (None: all)."""
        m = self.model
        ids = range(m.num_bodies) if body_names is None else [m.get_body_index(b) for b in body_names]
        ids = list(ids)
        return (np.ascontiguousarray(m.body_link[ids], dtype=np.int32),
                np.ascontiguousarray(m.body_offset[ids], dtype=np.float32))

    def get_link_view(self, body_names, name: str = "link_view") -> "RigidPrimView":
        """RigidPrimView over the named bodies of every env (prims env-major: env 0's bodies in the
        given order, then env 1's, ...)."""
        if isinstance(body_names, RigidPrimView):
            # built from a prim path expression: its last component names the bodies, as a
            # regular expression the way the reference's views use it (".../anymal/.*_SHANK")
            view = body_names
            pat = re.compile(view.prim_paths_expr.rstrip("/").split("/")[-1])
            body_names = [b for b in self.model.body_names if pat.fullmatch(b)]
            if not body_names:
                raise KeyError(f"{view.prim_paths_expr!r} matches no body; bodies: {', '.join(self.model.body_names)}")
        else:
            if isinstance(body_names, str):
                body_names = [body_names]
            view = RigidPrimView(name=name)
        view._bind(self, list(body_names))
        return view

    def get_jacobians(self, body_names=None) -> torch.Tensor:
        """[count, K, 6, nv] Jacobians of the named bodies' frames (all bodies by default): rows
        linear (3), angular (3), world axes; columns the generalized velocity."""
        links, offs = self._frames(body_names)
        out = self._empty(self.count, links.shape[0], 6, self.num_gen_vel)
        N.check(self._lib.mi_get_link_jacobian(self.handle, N.iptr(links), N.fptr(offs), links.shape[0],
                                               out.data_ptr(), self.stream()), "mi_get_link_jacobian")
        return out

    # ---- dynamics view (include/mi_sim.h mi_get_dynamics): M u' + c + g = tau ----
    # One launch fills the view's own output buffers, allocated on the first call and reused, so
    # later calls allocate nothing and can sit inside torch.cuda.graph (call once before
    # capturing). clone=False hands out the buffer itself, which the next call overwrites;
    # ``indices`` selects rows after the launch, as the state getters do.
    def _dynamics(self, M: bool, cor: bool, grav: bool):
        if self.handle is None:
            raise RuntimeError("the articulation view is not initialized")
        buf = getattr(self, "_dyn_buf", None)
        if buf is None:
            nv = self.num_gen_vel
            buf = self._dyn_buf = (self._empty(self.count, nv, nv), self._empty(self.count, nv),
                                   self._empty(self.count, nv))
        rc = self._lib.mi_get_dynamics(self.handle, buf[0].data_ptr() if M else None,
                                       buf[1].data_ptr() if cor else None,
                                       buf[2].data_ptr() if grav else None, self.stream())
        if rc:
            N.check(rc, "mi_get_dynamics")
        return buf

    def get_mass_matrices(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, nv, nv] joint-space inertia of the rigid-body tree (no armature, no damping:
        get_armatures / get_joint_dampings), rows and columns the generalized velocity."""
        return self._out(self._dynamics(True, False, False)[0], indices, clone)

    def get_coriolis_and_centrifugal_forces(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, nv] velocity-product forces c(q, u): the force that holds u' = 0 at gravity 0.
        Neither joint damping nor the per-link angular damping is part of it."""
        return self._out(self._dynamics(False, True, False)[1], indices, clone)

    def get_generalized_gravity_forces(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, nv] generalized gravity forces g(q), with each env's own gravity when
        set_env_gravity gave it one: ``set_joint_efforts(g[:, -num_dof:])`` holds the joints
        against gravity."""
        return self._out(self._dynamics(False, False, True)[2], indices, clone)

    def get_dynamics(self, indices=None, clone: bool = True):
        """(M, c, g) of the three getters above from one launch."""
        return tuple(self._out(t, indices, clone) for t in self._dynamics(True, True, True))

    # ---- mass-matrix solve view (include/mi_sim.h mi_solve_mass / mi_get_forward_dynamics /
    # mi_get_link_task_inertia): products with the inverse of Mt = M + diag(armature [+ dt damping]),
    # factorised on the chip by the stepper's tree LTDL. mode "stepper" is the matrix mi_sim_step
    # inverts, "armature" the continuous-time inertia. Buffers as for the dynamics view: allocated
    # on the first call of a shape and reused; clone=False hands out the buffer itself.
    _MASS_MODES = {"armature": N.MI_MASS_ARMATURE, "stepper": N.MI_MASS_STEPPER}

    @classmethod
    def _mass_mode(cls, mode) -> int:
        try:
            return cls._MASS_MODES[mode]
        except (KeyError, TypeError):
            raise ValueError(f"mode {mode!r}: expected 'stepper' or 'armature'") from None

    def _ms_buf(self, key, *shape) -> torch.Tensor:
        if self.handle is None:
            raise RuntimeError("the articulation view is not initialized")
        bufs = self.__dict__.setdefault("_ms_bufs", {})
        t = bufs.get((key, shape))
        if t is None:
            t = bufs[(key, shape)] = self._empty(*shape)
        return t

    def solve_mass_matrices(self, rhs: torch.Tensor, mode: str = "stepper", clone: bool = True) -> torch.Tensor:
        """Mt^-1 rhs for rhs [count, nv] or [count, R, nv] (the result has rhs' shape)."""
        which = self._mass_mode(mode)
        nv = self.num_gen_vel
        if rhs.dim() not in (2, 3) or rhs.shape[0] != self.count or rhs.shape[-1] != nv:
            raise ValueError(f"rhs {tuple(rhs.shape)}: expected [{self.count}, {nv}] or [{self.count}, R, {nv}]")
        r = self._f32(rhs)
        R = 1 if r.dim() == 2 else int(r.shape[1])
        out = self._ms_buf("solve", *r.shape)
        rc = self._lib.mi_solve_mass(self.handle, which, r.data_ptr(), R, out.data_ptr(), self.stream())
        if rc:
            N.check(rc, "mi_solve_mass")
        return out.clone() if clone else out

    def get_forward_dynamics(self, efforts=None, mode: str = "stepper", indices=None, clone: bool = True) -> torch.Tensor:
        """[count, nv] generalized accelerations Mt^-1 (S^T tau - c - g - B u) under the joint
        efforts ``efforts`` [count, num_dof] (None: the efforts last set). With mode "stepper",
        u + dt * acc is the velocity one contact-free, limit-free substep produces."""
        which = self._mass_mode(mode)
        tau = self._f32(efforts)
        if tau is not None and tuple(tau.shape) != (self.count, self.num_dof):
            raise ValueError(f"efforts {tuple(tau.shape)}: expected [{self.count}, {self.num_dof}]")
        acc = self._ms_buf("fd", self.count, self.num_gen_vel)
        rc = self._lib.mi_get_forward_dynamics(self.handle, which, N.ptr(tau), acc.data_ptr(), self.stream())
        if rc:
            N.check(rc, "mi_get_forward_dynamics")
        return self._out(acc, indices, clone)

    def get_task_space_inertias(self, body_names=None, mode: str = "stepper", clone: bool = True):
        """(minv_jt [count, 6K, nv], lam_inv [count, 6K, 6K]) of the named bodies' frames (all
        bodies by default): rows Mt^-1 J_r^T of the frames' Jacobian rows (get_jacobians' order),
        and the inverse task-space inertia J Mt^-1 J^T, symmetric bit for bit."""
        which = self._mass_mode(mode)
        links, offs = self._frames(body_names)
        K, nv = int(links.shape[0]), self.num_gen_vel
        mj, lam = self._ms_buf("minv_jt", self.count, 6 * K, nv), self._ms_buf("lam_inv", self.count, 6 * K, 6 * K)
        rc = self._lib.mi_get_link_task_inertia(self.handle, which, N.iptr(links), N.fptr(offs), K, mj.data_ptr(),
                                                lam.data_ptr(), self.stream())
        if rc:
            N.check(rc, "mi_get_link_task_inertia")
        return self._out(mj, None, clone), self._out(lam, None, clone)

    # ---- inverse-dynamics view (include/mi_sim.h mi_get_inverse_dynamics / mi_get_momentum): one
    # recursive Newton-Euler launch, no mass matrix in memory. Buffers as for the solve view. mode
    # "rigid" (M alone, no damping) exists for this direction only: M is harmless to multiply.
    def _accelerations(self, accelerations) -> Optional[torch.Tensor]:
        acc = self._f32(accelerations)
        if acc is not None and tuple(acc.shape) != (self.count, self.num_gen_vel):
            raise ValueError(f"accelerations {tuple(acc.shape)}: expected [{self.count}, {self.num_gen_vel}]")
        return acc

    def _inverse_dynamics(self, accelerations, mode, tau: bool, wrench: bool):
        which = N.MI_MASS_RIGID if mode == "rigid" else self._mass_mode(mode)
        acc = self._accelerations(accelerations)
        t = self._ms_buf("id_tau", self.count, self.num_gen_vel) if tau else None
        w = self._ms_buf("id_wrench", self.count, self.model.num_links, 6) if wrench else None
        rc = self._lib.mi_get_inverse_dynamics(self.handle, which, N.ptr(acc), N.ptr(t), N.ptr(w), self.stream())
        if rc:
            N.check(rc, "mi_get_inverse_dynamics")
        return t, w

    def get_inverse_dynamics(self, accelerations=None, mode: str = "rigid", indices=None, clone: bool = True) -> torch.Tensor:
        """[count, nv] generalized forces Mt acc + c + g + B u that produce the generalized
        accelerations ``accelerations`` [count, nv] (None: zero). mode "rigid": Mt = M, B = 0, the
        terms of get_dynamics; "armature" / "stepper": the matrices of get_forward_dynamics and
        B = joint damping, so that call gives ``accelerations`` back from the joint entries."""
        return self._out(self._inverse_dynamics(accelerations, mode, True, False)[0], indices, clone)

    def get_joint_reaction_wrenches(self, accelerations=None, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, num_bodies, 6] (force, torque; world axes) that each body's parent transmits to it
        through its joint for that motion: rigid-body terms only. The torque is taken about the
        origin of the body's link (model.body_link: the last link of the body's joint chain, where
        that joint sits). A copy: the library's rows are per link, the bodies' rows are picked."""
        w = self._inverse_dynamics(accelerations, "rigid", False, True)[1]
        links = getattr(self, "_body_link_t", None)
        if links is None:
            links = self._body_link_t = torch.as_tensor(np.asarray(self.model.body_link), device=self.device).long()
        return (w if indices is None else w[indices.long()])[:, links]

    def _momentum(self, com: bool, mom: bool, cmm: bool, energy: bool):
        n, nv = self.count, self.num_gen_vel
        b = [self._ms_buf(k, *shape) if on else None
             for k, shape, on in (("com", (n, 3), com), ("mom", (n, 6), mom), ("cmm", (n, 6, nv), cmm),
                                  ("energy", (n, 2), energy))]
        rc = self._lib.mi_get_momentum(self.handle, *(N.ptr(t) for t in b), self.stream())
        if rc:
            N.check(rc, "mi_get_momentum")
        return b

    def get_coms(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, 3] world position of the articulation's centre of mass."""
        return self._out(self._momentum(True, False, False, False)[0], indices, clone)

    def get_momenta(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, 6]: total linear momentum, angular momentum about the centre of mass (world axes)."""
        return self._out(self._momentum(False, True, False, False)[1], indices, clone)

    def get_centroidal_momentum_matrices(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, 6, nv] with get_momenta() == cmm @ u; rows 0..2 / total mass are the Jacobian of
        the centre of mass."""
        return self._out(self._momentum(False, False, True, False)[2], indices, clone)

    def get_energies(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, 2]: kinetic energy 1/2 u^T M u, potential energy -sum m_l gravity . com_l (each
        env's own gravity when set_env_gravity gave it one)."""
        return self._out(self._momentum(False, False, False, True)[3], indices, clone)

    # ---- contact view (include/mi_sim.h mi_get_contacts / mi_get_contact_jacobian): the contact set
    # the stepper would build from the current state. Buffers as for the solve view: allocated on
    # the first call and reused; clone=False hands out the buffer itself.
    def _contact_capacity(self):
        cap = getattr(self, "_ct_cap", None)
        if cap is None:
            if self.handle is None:
                raise RuntimeError("the articulation view is not initialized")
            c, g, p = C.c_int32(), C.c_int32(), C.c_int32()
            N.check(self._lib.mi_get_contact_capacity(self.handle, C.byref(c), C.byref(g), C.byref(p)),
                    "mi_get_contact_capacity")
            cap = self._ct_cap = (int(c.value), int(g.value), int(p.value))
        return cap

    @property
    def max_contacts(self) -> int:
        """C: contact slots per env (ground candidates + self-collision pairs, at most MI_MAX_ROWS / 3)."""
        return self._contact_capacity()[0]

    def _ct_ibuf(self, key, *shape) -> torch.Tensor:
        bufs = self.__dict__.setdefault("_ms_bufs", {})
        t = bufs.get((key, shape))
        if t is None:
            t = bufs[(key, shape)] = torch.empty(shape, dtype=torch.int32, device=self.device)
        return t

    def get_contact_data(self, indices=None, clone: bool = True):
        """(count [N] int32, bodies [N, C, 2] int32, points [N, C, 3] world, normals [N, C, 3],
        separations [N, C]) of the contacts the next physics step starts from: ground contacts first,
        then self-contacts, ``count`` of the C = max_contacts slots filled (the others hold 0 and body
        -1). ``bodies`` are body indices (body_names) of A and B, B = -1 for the ground; the normal
        points from B to A; a separation is the surface gap (negative: penetration), below
        contact_offset for every contact. One launch."""
        n, c = self.count, self.max_contacts
        cnt, lnk = self._ct_ibuf("ct_count", n), self._ct_ibuf("ct_links", n, c, 2)
        pt, nr, gp = self._ms_buf("ct_point", n, c, 3), self._ms_buf("ct_normal", n, c, 3), self._ms_buf("ct_gap", n, c)
        rc = self._lib.mi_get_contacts(self.handle, cnt.data_ptr(), lnk.data_ptr(), pt.data_ptr(), nr.data_ptr(),
                                       gp.data_ptr(), self.stream())
        if rc:
            N.check(rc, "mi_get_contacts")
        tab = getattr(self, "_link_body_t", None)
        if tab is None:   # link -> index of the body it belongs to; the last entry serves link -1 (the ground)
            m = self.model
            ids = [m.get_body_index(m.body_of_link[l]) for l in range(m.num_links)] + [-1]
            tab = self._link_body_t = torch.as_tensor(ids, dtype=torch.int32, device=self.device)
        bodies = self._ct_ibuf("ct_bodies", n, c, 2)
        torch.index_select(tab, 0, lnk.view(-1).long() % tab.shape[0], out=bodies.view(-1))
        return tuple(self._out(t, indices, clone) for t in (cnt, bodies, pt, nr, gp))

    def get_contact_jacobians(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[N, C, 3, nv]: rows (normal, tangent 1, tangent 2) of every contact slot of
        get_contact_data; row @ u is the velocity of A's material point at the contact point minus
        B's along that direction. Slots at and above the env's count are zero."""
        J = self._ms_buf("ct_jac", self.count, self.max_contacts, 3, self.num_gen_vel)
        rc = self._lib.mi_get_contact_jacobian(self.handle, J.data_ptr(), self.stream())
        if rc:
            N.check(rc, "mi_get_contact_jacobian")
        return self._out(J, indices, clone)

    def _link_contact_summary(self, links: np.ndarray, count: bool, clearance: bool):
        n, K = self.count, int(links.shape[0])
        key = tuple(int(x) for x in links)
        cnt = self._ct_ibuf(("ct_lcount", key), n, K) if count else None
        clr = self._ms_buf(("ct_clear", key), n, K) if clearance else None
        rc = self._lib.mi_get_link_contact_summary(self.handle, N.iptr(links), K, N.ptr(cnt), N.ptr(clr), self.stream())
        if rc:
            N.check(rc, "mi_get_link_contact_summary")
        return cnt, clr

    # ---- setters (indices: env ids, rows of the value tensors align with them) ----
    @staticmethod
    def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        if t is None:
            return None
        if t.dtype is torch.float32 and t.is_contiguous():
            return t
        return t.to(torch.float32).contiguous()

    def _idx(self, indices, dtype) -> (Optional[torch.Tensor], int):
        if indices is None:
            return None, self.count
        if (isinstance(indices, torch.Tensor) and indices.dtype is dtype and indices.is_cuda
                and indices.get_device() == self._dev_index and indices.is_contiguous()):
            return indices, indices.numel()
        idx = torch.as_tensor(indices, device=self.device).to(dtype).contiguous()
        return idx, int(idx.numel())

    def _state_idx(self, indices) -> (Optional[torch.Tensor], int, bool):
        """(ids, count, int32?) for the state setters: int64 device ids (locomotion.py:130-134)
        and int32 ones (cartpole.py:129-130) pass as they are (the library takes both:
        mi_set_*_state / mi_set_*_state_i32), anything else becomes int64 ids."""
        if indices is None:
            return None, self.count, False
        if (isinstance(indices, torch.Tensor) and indices.is_cuda and indices.get_device() == self._dev_index
                and indices.is_contiguous()):
            if indices.dtype is torch.int32:
                return indices, indices.numel(), True
            if indices.dtype is torch.int64:
                return indices, indices.numel(), False
        idx = torch.as_tensor(indices, device=self.device).to(torch.int64).contiguous()
        return idx, int(idx.numel()), False

    def set_joint_efforts(self, efforts: torch.Tensor, indices=None) -> None:
        e = self._f32(efforts)
        idx, n = self._idx(indices, torch.int32)
        if n == 0:              # empty index list: nothing to write
            return
        rc = self._lib.mi_set_dof_efforts(self.handle, e.data_ptr(), None if idx is None else idx.data_ptr(),
                                          n, self.stream())
        if rc:
            N.check(rc, "mi_set_dof_efforts")

    def _set_dof_state(self, q, qd, indices) -> None:
        idx, n, i32 = self._state_idx(indices)
        if n == 0:              # empty index list: nothing to write
            return
        fn = self._lib.mi_set_dof_state_i32 if i32 else self._lib.mi_set_dof_state
        rc = fn(self.handle, N.ptr(q), N.ptr(qd), None if idx is None else idx.data_ptr(), n, self.stream())
        if rc:
            N.check(rc, "mi_set_dof_state")

    def _set_root_state(self, pos, quat, vel, indices) -> None:
        idx, n, i32 = self._state_idx(indices)
        if n == 0:              # empty index list: nothing to write
            return
        fn = self._lib.mi_set_root_state_i32 if i32 else self._lib.mi_set_root_state
        rc = fn(self.handle, N.ptr(pos), N.ptr(quat), N.ptr(vel), None if idx is None else idx.data_ptr(), n,
                self.stream())
        if rc:
            N.check(rc, "mi_set_root_state")

    def set_joint_positions(self, positions: torch.Tensor, indices=None) -> None:
        self._set_dof_state(self._f32(positions), None, indices)

    def set_joint_velocities(self, velocities: torch.Tensor, indices=None) -> None:
        self._set_dof_state(None, self._f32(velocities), indices)

    def set_world_poses(self, positions=None, orientations=None, indices=None) -> None:
        self._set_root_state(self._f32(positions), self._f32(orientations), None, indices)

    def set_velocities(self, velocities: torch.Tensor, indices=None) -> None:
        self._set_root_state(None, None, self._f32(velocities), indices)

    # ---- body wrenches (include/mi_sim.h mi_apply_link_wrenches): forces and torques on bodies become
    # one generalized force Q [count, nv] that every later substep applies like an effort, the root's
    # six DOFs included, until it is replaced or cleared (a reset keeps it). Applied through link views
    # (RigidPrimView.apply_forces / apply_forces_and_torques_at_pos). The first application allocates
    # the sim's buffers: make it before capturing a graph.
    def _apply_link_wrenches(self, links, offs, forces, torques, indices, is_global: bool, accumulate: bool) -> None:
        idx, n = self._idx(indices, torch.int64)
        if n == 0:
            return
        K = int(links.shape[0])
        f, t = self._f32(forces), self._f32(torques)
        for name, v in (("forces", f), ("torques", t)):
            if v is not None and v.numel() != n * K * 3:       # the kernel trusts the shape
                raise ValueError(f"{name} {tuple(v.shape)}: expected {n} envs x {K} bodies x 3")
        rc = self._lib.mi_apply_link_wrenches(self.handle, N.iptr(links), N.fptr(offs), K, N.ptr(f), N.ptr(t),
                                              None if idx is None else idx.data_ptr(), n, int(bool(is_global)),
                                              int(bool(accumulate)), self.stream())
        if rc:
            N.check(rc, "mi_apply_link_wrenches")

    def _wrench_accumulates(self, view) -> bool:
        """Several link views applying in one step add up (Crazyflie's four rotor views); a view that
        applies again starts the next step's round and replaces."""
        seen = self.__dict__.setdefault("_wrench_round", set())
        if id(view) in seen:
            seen.clear()
        acc = bool(seen)
        seen.add(id(view))
        return acc

    def get_applied_generalized_forces(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, nv] generalized force of the body wrenches in effect (zeros before any was applied):
        sum over the bodies of J^T (force, torque), J of get_jacobians at the time of the application."""
        out = self._ms_buf("wrench_q", self.count, self.num_gen_vel)
        rc = self._lib.mi_get_applied_generalized_forces(self.handle, out.data_ptr(), self.stream())
        if rc:
            N.check(rc, "mi_get_applied_generalized_forces")
        return self._out(out, indices, clone)

    def clear_body_wrenches(self, indices=None) -> None:
        """No body wrench acts on the envs ``indices`` (all by default) from the next substep on."""
        idx, n = self._idx(indices, torch.int64)
        if indices is None:
            self.__dict__.setdefault("_wrench_round", set()).clear()
        if n == 0:
            return
        rc = self._lib.mi_clear_link_wrenches(self.handle, None if idx is None else idx.data_ptr(), n, self.stream())
        if rc:
            N.check(rc, "mi_clear_link_wrenches")

    # ---- implicit PD joint drives (include/mi_sim.h mi_set_drive_gains, include/mi_drive.h): the
    # reference's set_gains / set_joint_position_targets / set_joint_velocity_targets (anymal.py:187,
    # franka_cabinet.py:254,285, ball_balance.py:188). Every substep applies
    # kp (q* - q) + kd (qd* - qd) at its END state, solved with the velocities, on top of the efforts
    # in force; no effort cap. Gains and targets stay until set again or cleared (a reset keeps
    # them). kds are the drive's own: get / set_joint_dampings keep the passive damping. The first
    # setter allocates the sim's buffers: make it before capturing a graph.
    def _set_drive(self, fn_name: str, a, b, indices) -> None:
        idx, n = self._idx(indices, torch.int64)      # i32 or i64 ids, as the other setters take
        if n == 0:
            return
        rows = []
        for v in (a, b):
            v = None if v is None else self._f32(torch.as_tensor(v, device=self.device))
            if v is not None and v.numel() != n * self.num_dof:       # the kernel trusts the shape
                raise ValueError(f"{tuple(v.shape)} values for {n} envs x {self.num_dof} DOFs")
            rows.append(v)
        rc = getattr(self._lib, fn_name)(self.handle, N.ptr(rows[0]), N.ptr(rows[1]),
                                         None if idx is None else idx.data_ptr(), n, self.stream())
        if rc:
            N.check(rc, fn_name)

    def _get_drive(self, line: int, indices, clone: bool) -> torch.Tensor:
        out = self._ms_buf(("drive", line), self.count, self.num_dof)
        ptrs = [None] * 4
        ptrs[line] = out.data_ptr()
        rc = self._lib.mi_get_drives(self.handle, *ptrs, self.stream())
        if rc:
            N.check(rc, "mi_get_drives")
        return self._out(out, None if indices is None else torch.as_tensor(indices, device=self.device), clone)

    def set_gains(self, kps=None, kds=None, indices=None) -> None:
        """Drive stiffness and damping [n, num_dof]; None keeps what is set."""
        if kps is None and kds is None:
            raise ValueError("set_gains: kps and kds are both None")
        self._set_drive("mi_set_drive_gains", kps, kds, indices)

    def get_gains(self, indices=None, clone: bool = True):
        """(kps, kds), each [count, num_dof]: zeros before any was set."""
        return self._get_drive(0, indices, clone), self._get_drive(1, indices, clone)

    def set_joint_position_targets(self, positions, indices=None) -> None:
        self._set_drive("mi_set_drive_targets", positions, None, indices)

    def set_joint_velocity_targets(self, velocities, indices=None) -> None:
        self._set_drive("mi_set_drive_targets", None, velocities, indices)

    def get_joint_position_targets(self, indices=None, clone: bool = True) -> torch.Tensor:
        return self._get_drive(2, indices, clone)

    def get_joint_velocity_targets(self, indices=None, clone: bool = True) -> torch.Tensor:
        return self._get_drive(3, indices, clone)

    def clear_joint_drives(self, indices=None) -> None:
        """Gains and targets of the envs ``indices`` (all by default) <- zeros: no drive from the next
        substep on, and the same bits as a sim that never had one."""
        idx, n = self._idx(indices, torch.int64)
        if n == 0:
            return
        rc = self._lib.mi_clear_drives(self.handle, None if idx is None else idx.data_ptr(), n, self.stream())
        if rc:
            N.check(rc, "mi_clear_drives")

    # ---- per-env physics parameters (include/mi_sim.h mi_set_env_params) ----
    # The values omni.replicator.isaac's physics_view randomizes through the PhysX views
    # (randomize.py:308-430): gravity (SimulationContext), one friction coefficient per env
    # (material_properties' dynamic friction), joint damping (set_gains kds) and armature
    # (set_armatures). The first setter allocates the sim's per-env table.
    def _set_env_param(self, attr: int, values, indices) -> None:
        v = self._f32(torch.as_tensor(values, device=self.device))
        idx, n = self._idx(indices, torch.int64)
        if n == 0:
            return
        dim = {N.MI_ENVP_GRAVITY: 3, N.MI_ENVP_FRICTION: 1}.get(attr, self.num_dof)
        if v.numel() != n * dim:        # the kernel trusts the shape
            raise ValueError(f"{tuple(v.shape)} values for {n} envs x {dim}")
        N.check(self._lib.mi_set_env_params(self.handle, attr, v.data_ptr(), None if idx is None else idx.data_ptr(),
                                            n, self.stream()), "mi_set_env_params")

    def _get_env_param(self, attr: int, dim: int, indices) -> torch.Tensor:
        out = self._empty(self.count, dim)
        N.check(self._lib.mi_get_env_params(self.handle, attr, out.data_ptr(), self.stream()), "mi_get_env_params")
        return out if indices is None else out[torch.as_tensor(indices, device=self.device).long()]

    def set_env_gravity(self, gravity, indices=None) -> None:
        self._set_env_param(N.MI_ENVP_GRAVITY, gravity, indices)

    def get_env_gravity(self, indices=None) -> torch.Tensor:
        return self._get_env_param(N.MI_ENVP_GRAVITY, 3, indices)

    def set_friction_coefficients(self, values, indices=None) -> None:
        self._set_env_param(N.MI_ENVP_FRICTION, values, indices)

    def get_friction_coefficients(self, indices=None) -> torch.Tensor:
        return self._get_env_param(N.MI_ENVP_FRICTION, 1, indices)

    def set_joint_dampings(self, values, indices=None) -> None:
        self._set_env_param(N.MI_ENVP_DAMPING, values, indices)

    def get_joint_dampings(self, indices=None) -> torch.Tensor:
        return self._get_env_param(N.MI_ENVP_DAMPING, self.num_dof, indices)

    def set_armatures(self, values, indices=None) -> None:
        self._set_env_param(N.MI_ENVP_ARMATURE, values, indices)

    def get_armatures(self, indices=None) -> torch.Tensor:
        return self._get_env_param(N.MI_ENVP_ARMATURE, self.num_dof, indices)

    def clear_env_params(self) -> None:
        N.check(self._lib.mi_sim_clear_env_params(self.handle), "mi_sim_clear_env_params")

    def phys_dr_state(self) -> np.ndarray:
        """[count, 4] uint32 physics DR schedule state: since, counter, epoch, draws."""
        out = np.zeros((self.count, 4), np.uint32)
        N.check(self._lib.mi_get_phys_dr_state(self.handle, out.ctypes.data), "mi_get_phys_dr_state")
        return out

    # ---- physics ----
    def sim_step(self, substeps: int = 1) -> None:
        N.check(N.lib().mi_sim_step(self.handle, int(substeps), self.stream()), "mi_sim_step")

    def sim_kernel_path(self) -> tuple:
        """(path, topology, lds_bytes): path 1 = wavefront-per-env kernel, 0 = one lane per
        env; topology = compile-time topology id (0: runtime tables); LDS bytes per env."""
        p, t, b = C.c_int32(), C.c_int32(), C.c_int32()
        N.check(N.lib().mi_sim_kernel_path(self.handle, C.byref(p), C.byref(t), C.byref(b)),
                "mi_sim_kernel_path")
        return int(p.value), int(t.value), int(b.value)

    POST_KERNELS = {2: "k_loco_post_tiled<32s>", 4: "k_loco_post_pipe", 5: "k_post_step",
                    6: "k_loco_post_pipe<16>"}

    def post_kernel(self) -> tuple:
        """(kernel name, grid) of the last mi_task_post_step launch (None before the first)."""
        k, g = C.c_int32(), C.c_int32()
        N.check(N.lib().mi_task_post_kernel(self.handle, C.byref(k), C.byref(g)), "mi_task_post_kernel")
        return self.POST_KERNELS.get(int(k.value)), int(g.value)

    def sim_topology(self) -> int:
        return self.sim_kernel_path()[1]

    def nan_count(self) -> int:
        c = C.c_int64()
        N.check(N.lib().mi_sim_nan_count(self.handle, C.byref(c)), "mi_sim_nan_count")
        return int(c.value)


class RigidPrimView:
    """omni.isaac.core's RigidPrimView over bodies of an articulation (knees and feet,
    tasks/anymal_terrain.py:293-307; hand and finger frames, tasks/franka_cabinet.py:197-217):
    K bodies in each of N envs are ``count = N K`` prims, env-major, so callers can
    ``.view(N, K, ...)``. Every getter is one mi_get_link_state launch on torch's current stream.
    The view owns its output tensors and hands them out like the state mirrors: with clone=False
    the buffer itself, which the next read overwrites. Bodies are moved through their articulation;
    apply_forces / apply_forces_and_torques_at_pos push on them. Built by ``ArticulationView.get_link_view(body_names)``, or the reference's way,
    ``RigidPrimView(prim_paths_expr=".../<Robot>/<body>", name=...)``, then bound with
    ``ArticulationView.get_link_view(view)``."""

    def __init__(self, prim_paths_expr: str = "", name: str = "rigid_prim_view", reset_xform_properties: bool = False):
        self.prim_paths_expr = prim_paths_expr
        self.name = name
        self.count = 0
        self._art = None

    def _bind(self, art: ArticulationView, body_names) -> None:
        if art.handle is None:
            raise RuntimeError("the articulation view is not initialized")
        self._art = art
        self.body_names = list(body_names)
        self._links, self._offs = art._frames(self.body_names)
        self.num_bodies = K = len(self.body_names)
        self.count = art.count * K
        self.device = art.device
        self._pos, self._rot, self._vel = art._empty(self.count, 3), art._empty(self.count, 4), art._empty(self.count, 6)

    def _read(self, pos, rot, vel) -> None:
        a = self._art
        if a is None:
            raise RuntimeError(f"RigidPrimView {self.name!r} is not bound: ArticulationView.get_link_view(view)")
        rc = a._lib.mi_get_link_state(a.handle, N.iptr(self._links), N.fptr(self._offs), self.num_bodies,
                                      N.ptr(pos), N.ptr(rot), N.ptr(vel), a.stream())
        if rc:
            N.check(rc, "mi_get_link_state")

    def get_world_poses(self, indices=None, clone: bool = True):
        """([count, 3] positions, [count, 4] wxyz orientations) of the prims (``indices``: prims)."""
        self._read(self._pos, self._rot, None)
        return ArticulationView._out(self._pos, indices, clone), ArticulationView._out(self._rot, indices, clone)

    def get_velocities(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[count, 6]: linear velocity of the body origin, angular velocity (world axes)."""
        self._read(None, None, self._vel)
        return ArticulationView._out(self._vel, indices, clone)

    def get_linear_velocities(self, indices=None, clone: bool = True) -> torch.Tensor:
        return self.get_velocities(indices, clone=False)[:, :3].clone()

    def get_angular_velocities(self, indices=None, clone: bool = True) -> torch.Tensor:
        return self.get_velocities(indices, clone=False)[:, 3:].clone()

    def get_accelerations(self, accelerations=None, indices=None, clone: bool = True) -> torch.Tensor:
        """[N, K, 6] for the N envs of the articulation: classical linear acceleration of each body
        origin and angular acceleration (world axes), J acc + Jdot u for the generalized
        accelerations ``accelerations`` [N, nv] (None: the bias term Jdot u alone; gravity does not
        enter). ``indices`` selects envs, the rows of ``accelerations``."""
        a = self._art
        if a is None:
            raise RuntimeError(f"RigidPrimView {self.name!r} is not bound: ArticulationView.get_link_view(view)")
        acc = a._accelerations(accelerations)
        out = a._ms_buf(("link_acc", tuple(self._links), self._offs.tobytes()), a.count, self.num_bodies, 6)
        rc = a._lib.mi_get_link_acceleration(a.handle, N.iptr(self._links), N.fptr(self._offs), self.num_bodies,
                                             N.ptr(acc), out.data_ptr(), a.stream())
        if rc:
            N.check(rc, "mi_get_link_acceleration")
        return ArticulationView._out(out, indices, clone)

    # ---- forces on the view's bodies (include/mi_sim.h mi_apply_link_wrenches): the reference's
    # RigidPrimView.apply_forces (quadcopter.py:159, crazyflie.py:261, ingenuity.py:172) and
    # apply_forces_and_torques_at_pos, omni.isaac.core's signatures. ``indices`` are env ids (a view
    # of one body per env, as the reference's rotor views are, has one prim per env); forces and
    # torques are [n, K, 3] for the n envs named (or [n K, 3] env-major, or [n, 3] for K = 1).
    # The wrench becomes a generalized force at the current configuration and acts on every substep
    # until a view applies again (ArticulationView.clear_body_wrenches removes it); views that apply
    # one after the other in the same step add up. ``accumulate`` overrides that rule.
    def apply_forces_and_torques_at_pos(self, forces=None, torques=None, positions=None, indices=None,
                                        is_global: bool = True, accumulate: Optional[bool] = None) -> None:
        """``positions`` [K, 3] (or [n, K, 3] with identical rows): where the forces act, as offsets
        from the body origins in the body's axes. Positions that differ per env are folded into the
        torque in torch before the call (force at the origin + r x f)."""
        a = self._art
        if a is None:
            raise RuntimeError(f"RigidPrimView {self.name!r} is not bound: ArticulationView.get_link_view(view)")
        if forces is None and torques is None:
            raise ValueError("apply_forces_and_torques_at_pos: forces and torques are both None")
        K = self.num_bodies
        shape = lambda v: None if v is None else torch.as_tensor(v, device=a.device).to(torch.float32).reshape(-1, K, 3)
        f, t = shape(forces), shape(torques)
        offs = self._offs
        if positions is not None and f is not None:
            p = torch.as_tensor(positions, device=a.device).to(torch.float32).reshape(-1, K, 3)
            if p.shape[0] == 1 or bool((p == p[:1]).all()):
                offs = np.ascontiguousarray(self._offs + p[0].cpu().numpy(), dtype=np.float32)
            else:
                r = p
                if is_global:       # the offsets turned into world axes by the bodies' orientations
                    quat = self.get_world_poses(clone=False)[1].view(a.count, K, 4)
                    if indices is not None:
                        quat = quat[torch.as_tensor(indices, device=a.device).long()]
                    w, v = quat[..., :1], quat[..., 1:]
                    c = torch.cross(v, r, dim=-1)
                    r = r + 2.0 * (w * c + torch.cross(v, c, dim=-1))
                rf = torch.cross(r, f, dim=-1)
                t = rf if t is None else t + rf
        acc = a._wrench_accumulates(self) if accumulate is None else bool(accumulate)
        a._apply_link_wrenches(self._links, offs, f, t, indices, is_global, acc)

    def apply_forces(self, forces, indices=None, is_global: bool = True) -> None:
        """Forces at the body origins (RigidPrimView.apply_forces)."""
        self.apply_forces_and_torques_at_pos(forces=forces, indices=indices, is_global=is_global)

    # ---- contacts of the view's bodies (include/mi_sim.h mi_get_link_contact_summary): what the
    # reference's tasks read from a RigidContactView — "does the foot touch", "did a knee hit the
    # ground", clearance shaping. A body's geoms ride on its link (model.body_link).
    def _contact_summary(self, count: bool, clearance: bool):
        a = self._art
        if a is None:
            raise RuntimeError(f"RigidPrimView {self.name!r} is not bound: ArticulationView.get_link_view(view)")
        return a._link_contact_summary(self._links, count, clearance)

    def get_contact_counts(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[N, K] int32 for the N envs of the articulation: contacts of the set the next physics step
        starts from (ArticulationView.get_contact_data) that involve each body, ground and
        self-contacts alike. ``indices`` selects envs."""
        return ArticulationView._out(self._contact_summary(True, False)[0], indices, clone)

    def get_min_separations(self, indices=None, clone: bool = True) -> torch.Tensor:
        """[N, K]: the smallest surface gap of any of each body's geoms, to the ground and to every geom
        it may self-collide with, in contact or not; +inf for a body without geoms."""
        return ArticulationView._out(self._contact_summary(False, True)[1], indices, clone)
