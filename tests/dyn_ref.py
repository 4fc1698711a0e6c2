"""Reference of the dynamics view (include/mi_sim.h mi_get_dynamics): M(q), c(q,u) and g(q) in
numpy on top of tests/link_ref.py's Kinematics, vectorised over envs. float64 by default;
``dtype=np.float32`` runs the very same operations in float32, which gives the rounding scale the
device is held to (tests/test_gpu_dyn_view.py). Deliberately not the kernel's algorithm: M and g
are dense J^T I J / J^T m g sums over the links' centre-of-mass Jacobians, c projects classical
(point) accelerations through the same Jacobians; no spatial algebra, no composite inertias.
Helper module, not a test."""
from __future__ import annotations

import numpy as np

from tests.link_ref import HINGE, Kinematics


def world_inertias(model, kin):
    """[N,L,3,3]: each link's inertia about its centre of mass, world axes (R I R^T)."""
    f = model.inertia.astype(kin.dtype)
    out = []
    for l in range(model.num_links):
        xx, yy, zz, xy, xz, yz = f[l]
        Ib = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=kin.dtype)
        out.append(kin.R[l] @ Ib @ np.swapaxes(kin.R[l], 1, 2))
    return np.stack(out, axis=1)


def held_accelerations(model, kin):
    """(a [N,L,3], wd [N,L,3]): acceleration of every link's centre of mass and its angular
    acceleration while the generalized velocity u is held constant (classical point kinematics
    down the tree: the root origin and the world angular velocity of the root do not change)."""
    n, L, dt = kin.R[0].shape[0], model.num_links, kin.dtype
    zero = np.zeros((n, 3), dt)
    ao, wd = [zero], [zero]
    for l in range(1, L):
        P = int(model.parent[l])
        wP, wdP = kin.w[P], wd[P]
        d = kin.o[l] - kin.o[P]
        a = ao[P] + np.cross(wdP, d) + np.cross(wP, np.cross(wP, d))
        rate = (kin.w[l] - wP) if int(model.jtype[l]) == HINGE else None     # a qd
        if rate is not None:
            wd.append(wdP + np.cross(wP, rate))            # the axis rides on the parent
        else:
            slide = kin.v[l] - kin.v[P] - np.cross(wP, d)  # a qd
            a = a + dt(2) * np.cross(wP, slide)
            wd.append(wdP)
        ao.append(a)
    com = model.com.astype(dt)
    acc = []
    for l in range(L):
        r = kin.R[l] @ com[l]
        acc.append(ao[l] + np.cross(wd[l], r) + np.cross(kin.w[l], np.cross(kin.w[l], r)))
    return np.stack(acc, axis=1), np.stack(wd, axis=1)


class Dynamics:
    """M [N,nv,nv], c [N,nv], g [N,nv] with M u' + c + g = tau; gravity [3] or [N,3]."""

    def __init__(self, model, root_pos, root_quat, root_vel, q, qd, gravity=(0.0, 0.0, -9.81), dtype=np.float64):
        kin = self.kin = Kinematics(model, root_pos, root_quat, root_vel, q, qd, dtype=dtype)
        n, L = kin.R[0].shape[0], model.num_links
        mass = model.mass.astype(dtype)
        J = self.J = kin.jacobians(list(range(L)), model.com)       # at the centres of mass
        Jv, Jw = J[:, :, :3], J[:, :, 3:]
        Iw = self.Iw = world_inertias(model, kin)
        grav = np.broadcast_to(np.asarray(gravity).astype(dtype), (n, 3))
        self.acc, self.wd = held_accelerations(model, kin)
        M = np.zeros((n, kin.nv, kin.nv), dtype)
        c = np.zeros((n, kin.nv), dtype)
        g = np.zeros((n, kin.nv), dtype)
        for l in range(L):
            if not mass[l] > 0:                                     # massless links contribute nothing
                continue
            Jvt, Jwt = np.swapaxes(Jv[:, l], 1, 2), np.swapaxes(Jw[:, l], 1, 2)
            M += mass[l] * (Jvt @ Jv[:, l]) + Jwt @ Iw[:, l] @ Jw[:, l]
            w = kin.w[l]
            Iwv = (Iw[:, l] @ w[:, :, None])[:, :, 0]
            torque = (Iw[:, l] @ self.wd[:, l, :, None])[:, :, 0] + np.cross(w, Iwv)
            c += (Jvt @ (mass[l] * self.acc[:, l])[:, :, None])[:, :, 0] + (Jwt @ torque[:, :, None])[:, :, 0]
            g -= mass[l] * (Jvt @ grav[:, :, None])[:, :, 0]
        self.M, self.c, self.g = M, c, g

    def pattern(self):
        """Boolean [nv,nv]: M[j][k] may be non-zero — one DOF is an ancestor of the other (the
        root's DOFs are ancestors of all)."""
        kin, nv = self.kin, self.kin.nv
        anc = np.stack([kin.ancestor_columns(max(k - kin.nr + 1, 0)) for k in range(nv)])   # anc[k][j]: j moves DOF k's link
        return anc | anc.T
