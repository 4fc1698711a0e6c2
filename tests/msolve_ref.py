"""Reference of the mass-matrix solve view (include/mi_sim.h mi_solve_mass / mi_get_forward_dynamics
/ mi_get_link_task_inertia) in numpy, vectorised over envs. M, c, g come from tests/dyn_ref.py,
Jacobians from tests/link_ref.py; the mode's diagonal is added and the matrix is factorised by a
restatement of the tree LTDL (Mt = L^T D L over the DOF tree, mi_artic.hpp) and solved by its two
sweeps over the model's parent table — no LAPACK. float64 by default; ``dtype=np.float32`` runs the
very same operations, in the same elimination order, in float32, which gives the rounding scale
the device is held to (tests/test_gpu_msolve.py). Helper module, not a test."""
from __future__ import annotations

import numpy as np

from tests.dyn_ref import Dynamics

MODES = {"armature": 0, "stepper": 1}


def dof_parents(model):
    """Parent DOF of every DOF (-1: none): the root's DOFs form a chain, a link's DOF hangs on its
    parent link's (on the last root DOF below the root)."""
    nr = 6 if model.root_free else 0
    out = [k - 1 for k in range(nr)]
    for l in range(1, model.num_links):
        P = int(model.parent[l])
        out.append(nr - 1 if P == 0 else nr + P - 1)
    return out


def ancestors(par, k):
    out, j = [], par[k]
    while j >= 0:
        out.append(j)
        j = par[j]
    return out


def pattern(par):
    """Boolean [nv,nv], lower triangle: [k][j] — j is k or an ancestor DOF of k."""
    nv = len(par)
    p = np.eye(nv, dtype=bool)
    for k in range(nv):
        p[k, ancestors(par, k)] = True
    return p


def mode_diagonal(model, mode, dt, n, armature=None, damping=None, dtype=np.float64):
    """[n,nv]: armature (+ dt damping in mode "stepper") on the joint DOFs, 0 on the root's.
    armature / damping [n,D] replace the model's values (the per-env parameter table)."""
    nr = 6 if model.root_free else 0
    D = model.num_dof
    arm = np.broadcast_to(np.asarray(model.armature[1:] if armature is None else armature).astype(dtype), (n, D))
    damp = np.broadcast_to(np.asarray(model.damping[1:] if damping is None else damping).astype(dtype), (n, D))
    d = np.zeros((n, nr + D), dtype)
    d[:, nr:] = arm + dtype(dt) * damp if MODES[mode] else arm
    return d


def tree_ltdl(Mt, par):
    """In-place LTDL of the lower triangle of Mt [n,nv,nv]: D on the diagonal, L's off-diagonal
    entries below it, the upper triangle 0. k = nv-1 .. 0, ancestors nearest first."""
    H = np.tril(Mt)
    nv = len(par)
    for k in range(nv - 1, -1, -1):
        i = par[k]
        while i >= 0:
            a = H[:, k, i] / H[:, k, k]
            j = i
            while j >= 0:
                H[:, i, j] -= a * H[:, k, j]
                j = par[j]
            H[:, k, i] = a
            i = par[i]
    return H


def tree_solve(H, par, rhs):
    """Mt^-1 rhs for rhs [n,R,nv] with the factor H: the two substitution sweeps."""
    x = np.array(rhs, dtype=H.dtype, copy=True)
    nv = len(par)
    for i in range(nv - 1, -1, -1):
        for j in ancestors(par, i):
            x[:, :, j] -= H[:, i, j, None] * x[:, :, i]
    for i in range(nv):
        x[:, :, i] = x[:, :, i] / H[:, i, i, None]
    for i in range(nv):
        xi = x[:, :, i].copy()
        for j in ancestors(par, i):
            xi -= H[:, i, j, None] * x[:, :, j]
        x[:, :, i] = xi
    return x


class MassSolve:
    """Mt, its tree factor and the three products for a batch of states ``st`` (dict pos, rot, vel,
    q, qd as tests/link_ref.random_state)."""

    def __init__(self, model, st, dt, mode, gravity=(0.0, 0.0, -9.81), armature=None, damping=None,
                 dtype=np.float64):
        self.model, self.dtype = model, dtype
        self.dyn = Dynamics(model, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], gravity=gravity, dtype=dtype)
        kin = self.kin = self.dyn.kin
        n = kin.R[0].shape[0]
        self.nr, self.nv = kin.nr, kin.nv
        self.par = dof_parents(model)
        self.diag = mode_diagonal(model, mode, dt, n, armature, damping, dtype)
        self.Mt = self.dyn.M.copy()
        idx = np.arange(self.nv)
        self.Mt[:, idx, idx] += self.diag
        self.H = tree_ltdl(self.Mt, self.par)
        self.damping = np.broadcast_to(np.asarray(model.damping[1:] if damping is None else damping).astype(dtype),
                                       (n, model.num_dof))
        self.u = kin.u(st["vel"], st["qd"])

    def solve(self, rhs):
        """rhs [n,nv] or [n,R,nv] -> the same shape."""
        r = np.asarray(rhs).astype(self.dtype)
        x = tree_solve(self.H, self.par, r if r.ndim == 3 else r[:, None, :])
        return x if r.ndim == 3 else x[:, 0]

    def forward_rhs(self, tau):
        rhs = -self.dyn.c - self.dyn.g
        rhs[:, self.nr:] += np.asarray(tau).astype(self.dtype) - self.damping * self.u[:, self.nr:]
        return rhs

    def forward_dynamics(self, tau):
        return self.solve(self.forward_rhs(tau))

    def task(self, links, offsets=None):
        """(J [n,6K,nv], minv_jt [n,6K,nv], lam_inv [n,6K,6K])."""
        J = self.kin.jacobians(list(links), offsets)
        J = J.reshape(J.shape[0], -1, self.nv)
        X = self.solve(J)
        return J, X, J @ np.swapaxes(X, 1, 2)
