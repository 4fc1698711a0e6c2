"""Reference of the link-frame view (include/mi_sim.h mi_get_link_state / mi_get_link_jacobian):
a numpy restatement of the forward kinematics, frame velocities and Jacobians from a
CompiledModel and a state, vectorised over envs. float64 by default; ``dtype=np.float32`` runs the
very same operations in float32, which gives the rounding scale the device is held to
(tests/test_gpu_link_view.py). Helper module, not a test."""
from __future__ import annotations

import numpy as np

HINGE, SLIDE = 0, 1


def _rot(q):
    """[N,4] wxyz -> [N,3,3] (the formula for unit quaternions, applied as it stands)."""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _qmul(a, b):
    w1, x1, y1, z1 = (a[:, i] for i in range(4))
    w2, x2, y2, z2 = (b[:, i] for i in range(4))
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def _axis_angle(axis, t):
    """Rodrigues: unit axis [3], angles [N] -> [N,3,3]."""
    c, s = np.cos(t), np.sin(t)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=t.dtype)
    I = np.eye(3, dtype=t.dtype)
    return c[:, None, None] * I + s[:, None, None] * K + (1 - c)[:, None, None] * np.outer(axis, axis).astype(t.dtype)


class Kinematics:
    """Every link's world frame for a batch of states. Origins ``o`` are relative to the root
    origin; ``a`` is the world joint axis of the link; ``w`` / ``v`` the link's angular velocity
    and the velocity of its origin."""

    def __init__(self, model, root_pos, root_quat, root_vel, q, qd, dtype=np.float64):
        f = lambda x: np.asarray(x).astype(dtype)
        self.model, self.dtype = model, dtype
        self.root_pos, rq, rv, q, qd = f(root_pos), f(root_quat), f(root_vel), f(q), f(qd)
        n, L = rq.shape[0], model.num_links
        self.free = bool(model.root_free)
        self.nr = 6 if self.free else 0
        self.nv = self.nr + model.num_dof
        zero = np.zeros((n, 3), dtype)
        self.R, self.o, self.quat, self.a = [_rot(rq)], [zero], [rq], [zero]
        self.v = [rv[:, :3] if self.free else zero]
        self.w = [rv[:, 3:] if self.free else zero]
        for l in range(1, L):
            P = int(model.parent[l])
            ql, ax, pl = f(model.quat[l]), f(model.axis[l]), f(model.pos[l])
            Rj = self.R[P] @ _rot(ql[None])[0]
            a = Rj @ ax
            d = self.R[P] @ pl
            qj, qdj = q[:, l - 1], qd[:, l - 1]
            quat = _qmul(self.quat[P], np.broadcast_to(ql, (n, 4)))
            if int(model.jtype[l]) == HINGE:
                R = Rj @ _axis_angle(ax, qj)
                half = qj * dtype(0.5)
                quat = _qmul(quat, np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * ax], axis=1))
                v = self.v[P] + np.cross(self.w[P], d)
                w = self.w[P] + a * qdj[:, None]
            else:
                R = Rj
                d = d + a * qj[:, None]
                v = self.v[P] + np.cross(self.w[P], d) + a * qdj[:, None]
                w = self.w[P]
            self.R.append(R); self.o.append(self.o[P] + d); self.quat.append(quat); self.a.append(a)
            self.v.append(v); self.w.append(w)

    def u(self, root_vel, qd):
        """Generalized velocity [N, nv]: (root lin, root ang, qd) for a floating root, else qd."""
        qd = np.asarray(qd).astype(self.dtype)
        return np.concatenate([np.asarray(root_vel).astype(self.dtype), qd], axis=1) if self.free else qd

    def _rel(self, link_ids, offsets):
        """[N,K,3] frame origins relative to the root origin."""
        out = []
        for k, l in enumerate(link_ids):
            p = self.o[l]
            if offsets is not None:
                p = p + self.R[l] @ np.asarray(offsets[k]).astype(self.dtype)
            out.append(p)
        return np.stack(out, axis=1)

    def frames(self, link_ids, offsets=None):
        """pos [N,K,3] world, quat [N,K,4] wxyz, vel [N,K,6] (lin of the frame origin, ang)."""
        rel = self._rel(link_ids, offsets)
        pos = self.root_pos[:, None, :] + rel
        quat = np.stack([self.quat[l] for l in link_ids], axis=1)
        vel = []
        for k, l in enumerate(link_ids):
            v = self.v[l]
            if offsets is not None:
                v = v + np.cross(self.w[l], rel[:, k] - self.o[l])
            vel.append(np.concatenate([v, self.w[l]], axis=1))
        return pos, quat, np.stack(vel, axis=1)

    def ancestors(self, l):
        """Links whose joint moves link l (itself included, the root excluded)."""
        out = []
        while l > 0:
            out.append(l)
            l = int(self.model.parent[l])
        return out

    def jacobians(self, link_ids, offsets=None):
        """[N,K,6,nv]: rows lin, ang; columns u()."""
        rel = self._rel(link_ids, offsets)
        n, nr = rel.shape[0], self.nr
        J = np.zeros((n, len(link_ids), 6, self.nv), self.dtype)
        for k, l in enumerate(link_ids):
            p = rel[:, k]
            if self.free:
                for i in range(3):
                    e = np.zeros(3, self.dtype); e[i] = 1
                    J[:, k, i, i] = 1
                    J[:, k, :3, 3 + i] = np.cross(e, p)
                    J[:, k, 3 + i, 3 + i] = 1
            for j in self.ancestors(l):
                c = nr + j - 1
                if int(self.model.jtype[j]) == HINGE:
                    J[:, k, :3, c] = np.cross(self.a[j], p - self.o[j])
                    J[:, k, 3:, c] = self.a[j]
                else:
                    J[:, k, :3, c] = self.a[j]
        return J

    def ancestor_columns(self, l):
        """Boolean [nv]: the columns of link l's Jacobian that may be non-zero."""
        m = np.zeros(self.nv, bool)
        m[:self.nr] = True
        for j in self.ancestors(l):
            m[self.nr + j - 1] = True
        return m


def integrate(model, root_pos, root_quat, root_vel, q, qd, h):
    """The configuration moved along the generalized velocity for time h (float64): root origin
    by its linear velocity, root orientation by the world angular velocity (exact exponential),
    joints by qd."""
    root_pos, root_quat, root_vel, q, qd = (np.asarray(x, np.float64) for x in (root_pos, root_quat, root_vel, q, qd))
    if not model.root_free:
        return root_pos, root_quat, q + h * qd
    w = root_vel[:, 3:]
    ang = np.linalg.norm(w, axis=1) * h
    ax = w / np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-300)
    dq = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * ax], axis=1)
    return root_pos + h * root_vel[:, :3], _qmul(dq, root_quat), q + h * qd


def random_state(model, n, origins, seed):
    """The random state of the GPU tests, float32: q inside the limits (unlimited joints in
    +-pi), unit root quaternions, root positions within 5 m of the env origins, velocities up to
    a few units. A fixed base keeps zero root velocity (it has none)."""
    g = np.random.default_rng(seed)
    lo, hi = model.lower[1:].copy(), model.upper[1:].copy()
    free = lo >= hi
    lo[free], hi[free] = -np.pi, np.pi
    q = g.uniform(lo, hi, size=(n, model.num_dof))
    quat = g.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    pos = np.asarray(origins, np.float64).reshape(n, 3) + g.uniform(-5, 5, size=(n, 3))
    vel = g.uniform(-3, 3, size=(n, 6)) if model.root_free else np.zeros((n, 6))
    qd = g.uniform(-3, 3, size=(n, model.num_dof))
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return dict(pos=f(pos), rot=f(quat), vel=f(vel), q=f(q), qd=f(qd))
