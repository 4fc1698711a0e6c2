"""Reference of the contact view (include/mi_sim.h mi_get_contacts / mi_get_contact_jacobian /
mi_get_link_contact_summary): a numpy restatement of the stepper's contact detection (P8 of
csrc/mi_wave.hpp, include/mi_geom.h) on the frames of tests/link_ref.py, vectorised over envs.
float64 by default; ``dtype=np.float32`` runs the very same operations in float32, which gives the
rounding scale the device is held to (tests/test_gpu_contact_view.py). Helper module, not a test."""
from __future__ import annotations

import numpy as np

from tests.link_ref import HINGE, Kinematics, random_state

MAX_ROWS = 128          # MI_MAX_ROWS
CAPSULE = 1


def tables(model, self_on):
    """The stepper's candidate tables: ground points (geom, end) in create_model's order, the geom
    pairs (none with self-collision off), the limited-joint count of the row budget, capacity C."""
    pts = []
    for g in range(model.num_geoms):
        pts.append((g, 0))
        if int(model.geom_type[g]) == CAPSULE:
            pts.append((g, 1))
    pairs = [tuple(int(x) for x in p) for p in model.pairs] if self_on else []
    nlimc = int((model.lower[1:] < model.upper[1:]).sum())
    return pts, pairs, nlimc, min(len(pts) + len(pairs), MAX_ROWS // 3)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _clamp01(x):
    return np.minimum(np.maximum(x, 0), 1).astype(x.dtype)


def segment_closest(a0, a1, b0, b1):
    """mi_segment_closest over envs: closest points ca, cb and their parameters s, t."""
    dt = a0.dtype
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
    eps = dt.type(1e-12)
    with np.errstate(all="ignore"):
        den = a * e - b * b
        sg = np.where(den > eps, _clamp01((b * f - c * e) / den), 0).astype(dt)
        tg = (b * sg + f) / e
        sg = np.where(tg < 0, _clamp01(-c / a), np.where(tg > 1, _clamp01((b - c) / a), sg)).astype(dt)
        tg = _clamp01(tg)
        sa, se = a <= eps, e <= eps
        s = np.where(sa, 0, np.where(se, _clamp01(-c / a), sg)).astype(dt)
        t = np.where(sa & se, 0, np.where(sa, _clamp01(f / e), np.where(se, 0, tg))).astype(dt)
    return a0 + d1 * s[:, None], b0 + d2 * t[:, None], s, t, sa, se


def contact_basis(n):
    """mi_contact_basis over envs."""
    dt = n.dtype
    k = dt.type(0.57735)
    small = (n[:, 0] < k) & (n[:, 0] > -k)
    ax = np.zeros_like(n)
    ax[:, 0] = small
    ax[:, 1] = ~small
    c = np.cross(n, ax).astype(dt)
    t1 = c / np.sqrt(_dot(c, c))[:, None]
    return t1, np.cross(n, t1).astype(dt)


class Contacts:
    """Every candidate of every env, then each env's kept contacts in the stepper's order.

    Candidates (index j: ground points, then pairs): ``cgap [N,NC]``, ``cpoint`` (root-relative),
    ``cnormal``, ``ct1``, ``ct2`` [N,NC,3], ``clinks [NC,2]``, ``smooth [N,NC]`` (the gap is a smooth
    function of the configuration there). Kept: ``count [N]``, ``slot [N,C]`` (candidate index or
    -1), ``links [N,C,2]``, ``point [N,C,3]`` world, ``normal``, ``gap [N,C]``, ``truncated [N]``."""

    def __init__(self, model, st, contact_offset, self_on, dtype=np.float64):
        self.model, self.dtype = model, dtype
        self.kin = kin = Kinematics(model, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], dtype=dtype)
        self.pts, self.pairs, self.nlimc, self.C = tables(model, self_on)
        f = lambda x: np.asarray(x).astype(dtype)
        n = kin.R[0].shape[0]
        self.n, self.npts, self.NC = n, len(self.pts), len(self.pts) + len(self.pairs)
        NC = self.NC
        self.cgap = np.zeros((n, NC), dtype)
        self.cpoint, self.cnormal, self.ct1, self.ct2 = (np.zeros((n, NC, 3), dtype) for _ in range(4))
        self.clinks = np.full((NC, 2), -1, np.int32)
        self.smooth = np.ones((n, NC), bool)
        rz = kin.root_pos[:, 2]

        def world(g, p):
            l = int(model.geom_link[g])
            return np.einsum("nij,j->ni", kin.R[l], f(p)) + kin.o[l]

        for j, (g, end) in enumerate(self.pts):
            x = world(g, model.geom_p1[g] if end else model.geom_p0[g])
            r = dtype(model.geom_radius[g])
            self.cgap[:, j] = rz + x[:, 2] - r
            self.cpoint[:, j] = np.stack([x[:, 0], x[:, 1], x[:, 2] - r], axis=1)
            self.cnormal[:, j, 2], self.ct1[:, j, 0], self.ct2[:, j, 1] = 1, 1, 1
            self.clinks[j, 0] = model.geom_link[g]
        for i, (ga, gb) in enumerate(self.pairs):
            j = self.npts + i
            ra, rb = dtype(model.geom_radius[ga]), dtype(model.geom_radius[gb])
            ca, cb, s, t, sa, sb = segment_closest(world(ga, model.geom_p0[ga]), world(ga, model.geom_p1[ga]),
                                                   world(gb, model.geom_p0[gb]), world(gb, model.geom_p1[gb]))
            d = ca - cb
            dist = np.sqrt(_dot(d, d))
            with np.errstate(all="ignore"):
                nrm = np.where((dist > dtype(1e-9))[:, None], d / dist[:, None], f([0, 0, 1])[None]).astype(dtype)
            gap = dist - ra - rb
            self.cgap[:, j] = gap
            self.cnormal[:, j] = nrm
            self.cpoint[:, j] = cb + nrm * (rb + dtype(0.5) * gap)[:, None]
            self.ct1[:, j], self.ct2[:, j] = contact_basis(nrm)
            self.clinks[j] = (model.geom_link[ga], model.geom_link[gb])
            self.smooth[:, j] = (sa | ((s > 0) & (s < 1))) & (sb | ((t > 0) & (t < 1))) & (dist > 1e-6)
        # compaction: active ground candidates in order, then active pairs under the budget
        C = self.C
        act = self.cgap < dtype(contact_offset)
        self.active = act
        self.count = np.zeros(n, np.int32)
        self.truncated = np.zeros(n, bool)
        self.slot = np.full((n, C), -1, np.int64)
        for e in range(n):
            ground = np.flatnonzero(act[e, :self.npts])
            pairs = self.npts + np.flatnonzero(act[e, self.npts:])
            budget = (MAX_ROWS - 3 * len(ground) - self.nlimc) // 3
            self.truncated[e] = len(pairs) > budget
            keep = np.concatenate([ground, pairs[:max(budget, 0)]])
            self.count[e] = len(keep)
            self.slot[e, :len(keep)] = keep
        kept = self.slot >= 0
        idx = np.where(kept, self.slot, 0)
        take = lambda a: np.take_along_axis(a, idx[..., None] if a.ndim == 3 else idx, axis=1)
        self.links = np.where(kept[..., None], self.clinks[idx], -1).astype(np.int32)
        self.point = np.where(kept[..., None], kin.root_pos[:, None, :] + take(self.cpoint), 0)
        self.normal = np.where(kept[..., None], take(self.cnormal), 0)
        self.gap = np.where(kept, take(self.cgap), 0)
        self.kept, self.idx = kept, idx

    # ---- Jacobians ----
    def point_jacobian(self, l, p):
        """[N,3,nv] linear Jacobian of link l's material point at the root-relative point p [N,3]."""
        kin, m = self.kin, self.model
        J = np.zeros((self.n, 3, kin.nv), self.dtype)
        if kin.free:
            for i in range(3):
                e = np.zeros(3, self.dtype)
                e[i] = 1
                J[:, i, i] = 1
                J[:, :, 3 + i] = np.cross(e, p)
        for j in kin.ancestors(l):
            c = kin.nr + j - 1
            J[:, :, c] = np.cross(kin.a[j], p - kin.o[j]) if int(m.jtype[j]) == HINGE else kin.a[j]
        return J

    def candidate_rows(self, j):
        """[N,3,nv]: rows (normal, t1, t2) of candidate j: direction . (J of A's point - J of B's)."""
        la, lb = (int(x) for x in self.clinks[j])
        p = self.cpoint[:, j]
        Ja = self.point_jacobian(la, p)
        if lb >= 0:
            Jb = self.point_jacobian(lb, p)
            both = self.kin.ancestor_columns(la) & self.kin.ancestor_columns(lb)
            Ja = Ja - Jb
            Ja[:, :, both] = 0            # DOFs above the common ancestor move both alike
        basis = np.stack([self.cnormal[:, j], self.ct1[:, j], self.ct2[:, j]], axis=1)
        return np.einsum("nrk,nkc->nrc", basis, Ja)

    def live_columns(self, j):
        """Boolean [nv]: the columns of candidate j's rows that may be non-zero."""
        la, lb = (int(x) for x in self.clinks[j])
        a = self.kin.ancestor_columns(la)
        return a ^ self.kin.ancestor_columns(lb) if lb >= 0 else a

    def jacobian(self):
        """[N,C,3,nv] rows of the kept contacts (zeros at and above count), and the mask of columns
        that must be exactly zero [N,C,nv]."""
        J = np.zeros((self.n, self.C, 3, self.kin.nv), self.dtype)
        dead = np.ones((self.n, self.C, self.kin.nv), bool)
        for j in np.unique(self.slot[self.slot >= 0]):
            e, k = np.nonzero(self.slot == j)
            J[e, k] = self.candidate_rows(int(j))[e]
            dead[e, k] = ~self.live_columns(int(j))
        return J, dead

    def point_velocity(self, l, p):
        """[N,3] velocity of link l's material point at the root-relative point p."""
        return self.kin.v[l] + np.cross(self.kin.w[l], p - self.kin.o[l])

    # ---- per-link summary ----
    def summary(self, link_ids):
        """count [N,K] of kept contacts that involve each link, clearance [N,K]: the smallest gap
        over all of the link's candidates, +inf without any."""
        cnt = np.zeros((self.n, len(link_ids)), np.int32)
        clr = np.full((self.n, len(link_ids)), np.inf, self.dtype)
        for k, l in enumerate(link_ids):
            cnt[:, k] = ((self.links == l).any(axis=2) & self.kept).sum(axis=1)
            mine = (self.clinks == l).any(axis=1)
            if mine.any():
                clr[:, k] = self.cgap[:, mine].min(axis=1)
        return cnt, clr


def contact_state(model, n, origins, seed, contact_offset, self_on, zband=None):
    """The state of the contact tests: ``random_state`` for 2n draws with the root height drawn in
    ``zband`` (lying to standing height, so that some contact points touch the ground), of which the
    first n are kept that have no candidate whose float64 gap lies within ``band`` of
    contact_offset; band = 4 x the worst |gap32 - gap64| of the draw, at least 2 ulp of the largest
    |gap|. Every kept env's contact set is then the same in float32 and float64 arithmetic, so it is
    compared exactly. Returns (state, info); raises when fewer than n draws survive."""
    zband = (0.0, 1.5) if zband is None else zband
    org =np.asarray(origins, np.float64).reshape(-1, 3)
    org2 = org[np.arange(2 * n) % org.shape[0]]
    st = random_state(model, 2 * n, org2, seed)
    g = np.random.default_rng(seed + 1)
    st["pos"][:, 2] = (org2[:, 2] + g.uniform(zband[0], zband[1], size=2 * n)).astype(np.float32)
    c64 = Contacts(model, st, contact_offset, self_on)
    c32 = Contacts(model, st, contact_offset, self_on, dtype=np.float32)
    if c64.NC:
        dev = float(np.abs(c32.cgap.astype(np.float64) - c64.cgap).max())
        band = max(4.0 * dev, 2.0 * float(np.finfo(np.float32).eps) * float(np.abs(c64.cgap).max()))
        ok = (np.abs(c64.cgap - contact_offset) >= band).all(axis=1)
    else:
        dev, band, ok = 0.0, 0.0, np.ones(2 * n, bool)
    keep = np.flatnonzero(ok)
    if len(keep) < n:
        raise ValueError(f"only {len(keep)} of {2 * n} draws are clear of the threshold band {band:.3e}")
    keep = keep[:n]
    return {k: np.ascontiguousarray(v[keep]) for k, v in st.items()}, dict(band=band, dev=dev, survivors=int(ok.sum()))


# root height bands of the generator, per robot: from the lowest geom resting on the ground to
# the spawn (standing) height of the task
ZBAND = {"Humanoid": (0.05, 1.34), "Ant": (0.05, 0.9)}
