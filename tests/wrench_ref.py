"""Reference of the body wrenches (include/mi_sim.h mi_apply_link_wrenches): the generalized force
Q = sum_k J_k^T (f_k, tau_k) from tests/link_ref.py's Jacobians, in float64 or, with
``dtype=np.float32``, the same operations in float32 (the rounding scale the device is held to,
tests/test_gpu_wrench.py). Helper module, not a test."""
from __future__ import annotations

import numpy as np

from tests.link_ref import Kinematics


def world_wrench(kin: Kinematics, link_ids, force, torque, is_global):
    """(f, tau) [N,K,3] in world axes; is_global False: given in each link's axes."""
    n, K = kin.R[0].shape[0], len(link_ids)
    z = np.zeros((n, K, 3), kin.dtype)
    f = z if force is None else np.asarray(force).astype(kin.dtype)
    t = z if torque is None else np.asarray(torque).astype(kin.dtype)
    if not is_global:
        R = np.stack([kin.R[l] for l in link_ids], axis=1)                  # [N,K,3,3]
        f, t = np.einsum("nkij,nkj->nki", R, f), np.einsum("nkij,nkj->nki", R, t)
    return f, t


def generalized_force(model, st, link_ids, offsets, force, torque, is_global=True, dtype=np.float64):
    """Q [N,nv] of wrenches force / torque [N,K,3] (either may be None) on the frames
    (link_ids[k], offsets[k]) of every env of the state dict st (pos, rot, vel, q, qd)."""
    kin = Kinematics(model, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], dtype=dtype)
    f, t = world_wrench(kin, link_ids, force, torque, is_global)
    J = kin.jacobians(link_ids, offsets)                                       # [N,K,6,nv]
    Q = np.zeros((J.shape[0], J.shape[3]), dtype)
    for k in range(len(link_ids)):                                             # the call's order
        Q = Q + np.einsum("nrc,nr->nc", J[:, k, :3], f[:, k]) + np.einsum("nrc,nr->nc", J[:, k, 3:], t[:, k])
    return Q


def moved_columns(model, link_ids):
    """Boolean [nv]: DOFs that move at least one of the frames."""
    nr = 6 if model.root_free else 0
    m = np.zeros(nr + model.num_dof, bool)
    m[:nr] = True
    for l in link_ids:
        l = int(l)
        while l > 0:
            m[nr + l - 1] = True
            l = int(model.parent[l])
    return m


def virtual_power(model, st, link_ids, offsets, force, torque, is_global=True):
    """sum_k f_k . v_k + tau_k . w_k [N] from the frame velocities (no Jacobian), float64."""
    kin = Kinematics(model, st["pos"], st["rot"], st["vel"], st["q"], st["qd"])
    f, t = world_wrench(kin, link_ids, force, torque, is_global)
    vel = kin.frames(link_ids, offsets)[2]
    return (f * vel[:, :, :3]).sum(axis=(1, 2)) + (t * vel[:, :, 3:]).sum(axis=(1, 2))
