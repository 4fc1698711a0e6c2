"""Reference of the inverse-dynamics view (include/mi_sim.h mi_get_inverse_dynamics /
mi_get_link_acceleration / mi_get_momentum) in numpy on top of tests/link_ref.py and
tests/dyn_ref.py, vectorised over envs. float64 by default; ``dtype=np.float32`` runs the very same
operations in float32, which gives the rounding scale the device is held to
(tests/test_gpu_idyn.py). Deliberately not the kernel's algorithm: torques are the dense
(M + diag) a + c + g + B u, wrenches are classical Newton-Euler sums over subtrees, accelerations
are classical point kinematics plus J a, momentum comes from per-link Jacobians at the centres of
mass; no spatial algebra, no common reference point. Helper module, not a test."""
from __future__ import annotations

import numpy as np

from tests.dyn_ref import Dynamics
from tests.link_ref import HINGE

MODES = {"armature": 0, "stepper": 1, "rigid": 2}


class InverseDynamics:
    """All outputs of the three calls for a batch of states ``st`` (dict pos, rot, vel, q, qd as
    tests/link_ref.random_state). gravity [3] or [N,3]; armature / damping [N,D] replace the
    model's values (the per-env parameter table)."""

    def __init__(self, model, st, dt, gravity=(0.0, 0.0, -9.81), armature=None, damping=None, dtype=np.float64):
        self.model, self.dtype, self.dt = model, dtype, dtype(dt)
        self.dyn = Dynamics(model, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], gravity=gravity, dtype=dtype)
        kin = self.kin = self.dyn.kin
        n = self.n = kin.R[0].shape[0]
        self.nr, self.nv, self.L = kin.nr, kin.nv, model.num_links
        D = model.num_dof
        self.gravity = np.broadcast_to(np.asarray(gravity).astype(dtype), (n, 3))
        self.arm = np.broadcast_to(np.asarray(model.armature[1:] if armature is None else armature).astype(dtype), (n, D))
        self.damp = np.broadcast_to(np.asarray(model.damping[1:] if damping is None else damping).astype(dtype), (n, D))
        self.u = kin.u(st["vel"], st["qd"])
        self.mass = model.mass.astype(dtype)

    def _acc(self, acc):
        return np.zeros((self.n, self.nv), self.dtype) if acc is None else np.asarray(acc).astype(self.dtype)

    def tau(self, acc=None, mode="rigid"):
        """[N,nv] = Mt a + c + g + B u."""
        a, d, nr = self._acc(acc), self.dyn, self.nr
        t = (d.M @ a[:, :, None])[:, :, 0] + d.c + d.g
        if MODES[mode] != 2:
            diag = self.arm + self.dt * self.damp if MODES[mode] == 1 else self.arm
            t[:, nr:] += diag * a[:, nr:] + self.damp * self.u[:, nr:]
        return t

    def link_accelerations(self, acc=None):
        """(a [N,L,3] of the centres of mass, wd [N,L,3]): held_accelerations plus J_l a."""
        a, d = self._acc(acc), self.dyn
        Ja = np.einsum("nlrk,nk->nlr", d.J, a)
        return d.acc + Ja[..., :3], d.wd + Ja[..., 3:]

    def joint_wrenches(self, acc=None):
        """[N,L,6] (force, torque about link l's origin): sums over l's subtree of m (a - gravity)
        and I wd + w x I w, the forces' moments taken about the origin of l."""
        m, kin, d = self.model, self.kin, self.dyn
        al, wd = self.link_accelerations(acc)
        com = m.com.astype(self.dtype)
        out = np.zeros((self.n, self.L, 6), self.dtype)
        for l in range(self.L):
            for x in range(l, self.L):
                if not self.mass[x] > 0 or not (x == l or l == 0 or l in kin.ancestors(x)):
                    continue
                w = kin.w[x]
                f = self.mass[x] * (al[:, x] - self.gravity)
                Iw = (d.Iw[:, x] @ w[:, :, None])[:, :, 0]
                t = (d.Iw[:, x] @ wd[:, x, :, None])[:, :, 0] + np.cross(w, Iw)
                arm = kin.o[x] + kin.R[x] @ com[x] - kin.o[l]
                out[:, l, :3] += f
                out[:, l, 3:] += t + np.cross(arm, f)
        return out

    def joint_subspaces(self):
        """[N,L,6]: S_l as (lin, ang) at link l's origin: a slide's axis is a force direction, a
        hinge's a torque direction; the root's row is 0 (its DOFs are the six unit directions)."""
        S = np.zeros((self.n, self.L, 6), self.dtype)
        for l in range(1, self.L):
            o = 3 if int(self.model.jtype[l]) == HINGE else 0
            S[:, l, o:o + 3] = self.kin.a[l]
        return S

    def frame_accelerations(self, link_ids, offsets=None, acc=None):
        """[N,K,6]: held_accelerations moved from the centre of mass to the frame origin, plus J a."""
        m, kin, d = self.model, self.kin, self.dyn
        a = self._acc(acc)
        com = m.com.astype(self.dtype)
        J = kin.jacobians(list(link_ids), offsets)
        Ja = np.einsum("nkrc,nc->nkr", J, a)
        out = []
        for k, l in enumerate(link_ids):
            r = -(kin.R[l] @ com[l])
            if offsets is not None:
                r = r + kin.R[l] @ np.asarray(offsets[k]).astype(self.dtype)
            w, wd = kin.w[l], d.wd[:, l]
            lin = d.acc[:, l] + np.cross(wd, r) + np.cross(w, np.cross(w, r))
            out.append(np.concatenate([lin, wd], axis=1))
        return np.stack(out, axis=1) + Ja

    def momentum(self):
        """dict com [N,3], mom [N,6], cmm [N,6,nv], energy [N,2] from the Jacobians at the centres of mass."""
        m, kin, d = self.model, self.kin, self.dyn
        mass, total = self.mass, self.mass.sum(dtype=self.dtype)
        pc, _, _ = kin.frames(list(range(self.L)), m.com)              # world centres of mass [N,L,3]
        com = np.einsum("l,nlc->nc", mass, pc) / total
        Jv, Jw = d.J[:, :, :3], d.J[:, :, 3:]
        cmm = np.zeros((self.n, 6, self.nv), self.dtype)
        pe = np.zeros(self.n, self.dtype)
        for l in range(self.L):
            if not mass[l] > 0:
                continue
            r = pc[:, l] - com
            lin = mass[l] * Jv[:, l]
            cmm[:, :3] += lin
            cmm[:, 3:] += d.Iw[:, l] @ Jw[:, l] + np.cross(r[:, None, :], lin, axisa=2, axisb=1, axisc=1)
            pe -= mass[l] * (self.gravity * pc[:, l]).sum(1)
        mom = (cmm @ self.u[:, :, None])[:, :, 0]
        ke = self.dtype(0.5) * np.einsum("ni,nij,nj->n", self.u, d.M, self.u)
        return dict(com=com, mom=mom, cmm=cmm, energy=np.stack([ke, pe], axis=1))
