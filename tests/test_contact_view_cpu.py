"""Contact view, the parts that need no GPU: the binding of the four entry points, the state
generator's coverage, the budget case, and the numpy reference's own consistency
(tests/contact_ref.py)."""
import ctypes as C
import re

import numpy as np
import pytest

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.robots.model import asset_path, load_robot
from tests.contact_ref import MAX_ROWS, ZBAND, Contacts, contact_state
from tests.link_ref import integrate

# contact_offset / self-collision of the task YAMLs (cfg/task/Humanoid.yaml, Ant.yaml)
ROBOTS = {"Humanoid": (0.02, True), "Ant": (0.02, False)}
# Budget case: Humanoid, N = 33, seed 17. At contact_offset 0.15 the reference cuts the pair list of
# 5 of the 33 envs at the row budget (0.05: none, 0.1: 1, 0.2: 7, 0.3: 24).
BUDGET_OFFSET, BUDGET_N, BUDGET_TRUNCATED = 0.15, 33, 5


def test_native_binds_the_contact_entry_points():
    """include/mi_sim.h declares the four entries, MI_ABI_VERSION stays 4, native.py binds them."""
    p, i32p = C.c_void_p, C.POINTER(C.c_int32)
    want = {"mi_get_contact_capacity": [p, i32p, i32p, i32p],
            "mi_get_contacts": [p] * 7,
            "mi_get_contact_jacobian": [p] * 3,
            "mi_get_link_contact_summary": [p, i32p, C.c_int32, p, p, p]}
    hdr = open(asset_path("../../../include/mi_sim.h")).read()
    for name, args in want.items():
        assert name in N.EXPORTED_SYMBOLS
        res, got = N._SIGS[name]
        assert res is C.c_int and got == args
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
        assert len(params) == len(args), (name, params)
    assert re.search(r"#define MI_ABI_VERSION 4\b", hdr)


@pytest.mark.parametrize("name", list(ROBOTS))
@pytest.mark.parametrize("n", [257, 1])
def test_generator_covers_the_cases(name, n):
    """On the reference alone: enough draws survive the threshold filter, and at N = 257 the kept
    envs hold ground contacts, contact-free envs and (Humanoid) self-contacts. At N = 1 the three
    population conditions contradict one another (one env cannot both touch and not touch, and 16
    envs do not exist), so there the survival and the float32 / float64 agreement are asserted."""
    off, self_on = ROBOTS[name]
    m = load_robot(name)
    st, info = contact_state(m, n, np.zeros((n, 3)), 17, off, self_on, ZBAND[name])
    assert info["survivors"] >= n and st["q"].shape[0] == n
    c64 = Contacts(m, st, off, self_on)
    c32 = Contacts(m, st, off, self_on, dtype=np.float32)
    assert np.array_equal(c64.slot, c32.slot)                  # every kept env compares exactly
    assert (np.abs(c64.cgap - off) >= info["band"]).all()
    ground = ((c64.links[:, :, 1] == -1) & c64.kept).any(axis=1)
    selfc = ((c64.links[:, :, 1] >= 0) & c64.kept).any(axis=1)
    print(f"{name}-{n}: band {info['band']:.2e} ground {ground.sum()} none {(c64.count == 0).sum()} self {selfc.sum()}")
    if n == 257:
        assert ground.sum() >= n / 4
        assert (c64.count == 0).sum() >= 1
        if name == "Humanoid":
            assert selfc.sum() >= 16
        else:
            assert not selfc.any()


def test_budget_case_truncates():
    m = load_robot("Humanoid")
    st, _ = contact_state(m, BUDGET_N, np.zeros((BUDGET_N, 3)), 17, BUDGET_OFFSET, True, ZBAND["Humanoid"])
    c = Contacts(m, st, BUDGET_OFFSET, True)
    assert int(c.truncated.sum()) == BUDGET_TRUNCATED >= 1
    for e in np.flatnonzero(c.truncated):
        ng = int(((c.links[e, :, 1] == -1) & c.kept[e]).sum())
        assert c.count[e] == ng + (MAX_ROWS - 3 * ng - c.nlimc) // 3 <= c.C
        assert c.active[e].sum() > c.count[e]
    # order: ground candidates first and ascending, then pairs ascending
    for e in range(BUDGET_N):
        s = c.slot[e, :c.count[e]]
        assert np.all(np.diff(s) > 0)


def _f64_state(name, n, seed=17):
    off, self_on = ROBOTS[name]
    m = load_robot(name)
    st, _ = contact_state(m, n, np.zeros((n, 3)), seed, off, self_on, ZBAND[name])
    st = {k: v.astype(np.float64) for k, v in st.items()}
    st["rot"] /= np.linalg.norm(st["rot"], axis=1, keepdims=True)
    return m, st, off, self_on


@pytest.mark.parametrize("name", list(ROBOTS))
def test_normal_row_is_the_gap_rate(name):
    """float64: the normal row of the reference Jacobian times u against the central difference
    (h = 1e-6) of the candidate's gap along link_ref.integrate, over the kept contacts whose gap is
    smooth (ground points; pairs whose closest-point parameters are strictly inside (0, 1), a
    sphere's own parameter aside). Measured residual: Humanoid 2.2e-10 (323 contacts), Ant 2.0e-10
    (282); the bound is 10 x the larger, 2.2e-9."""
    m, st, off, self_on = _f64_state(name, 65)
    c = Contacts(m, st, off, self_on)
    u = c.kin.u(st["vel"], st["qd"])
    h = 1e-6
    side = []
    for sgn in (+1, -1):
        p, r, q = integrate(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], sgn * h)
        side.append(Contacts(m, dict(st, pos=p, rot=r, q=q), off, self_on))
    worst, used = 0.0, 0
    for j in np.unique(c.slot[c.slot >= 0]):
        e = np.flatnonzero((c.slot == j).any(axis=1) & c.smooth[:, j] & side[0].smooth[:, j] & side[1].smooth[:, j])
        if not len(e):
            continue
        rate = (side[0].cgap[e, j] - side[1].cgap[e, j]) / (2 * h)
        row = np.einsum("nc,nc->n", c.candidate_rows(int(j))[e, 0], u[e])
        worst = max(worst, float(np.abs(row - rate).max()))
        used += len(e)
    print(f"{name}: normal row . u - d gap / dt: {worst:.3e} over {used} contacts")
    assert used > 50
    assert worst <= 2.2e-9


@pytest.mark.parametrize("name", list(ROBOTS))
def test_rows_are_the_basis_on_the_frame_velocities(name):
    """J_c u equals (normal, t1, t2) applied to the velocity of A's material point at the contact
    point minus B's, from the link view's reference; cancelled columns are exactly zero."""
    m, st, off, self_on = _f64_state(name, 65)
    c = Contacts(m, st, off, self_on)
    u = c.kin.u(st["vel"], st["qd"])
    J, dead = c.jacobian()
    assert J.shape == (65, c.C, 3, c.kin.nv)
    assert np.all(J[np.broadcast_to(dead[:, :, None, :], J.shape)] == 0.0)
    got = np.einsum("nkrc,nc->nkr", J, u)
    want = np.zeros_like(got)
    for j in np.unique(c.slot[c.slot >= 0]):
        e, k = np.nonzero(c.slot == j)
        la, lb = (int(x) for x in c.clinks[j])
        p = c.cpoint[:, j]
        dv = c.point_velocity(la, p) - (c.point_velocity(lb, p) if lb >= 0 else 0)
        basis = np.stack([c.cnormal[:, j], c.ct1[:, j], c.ct2[:, j]], axis=1)
        want[e, k] = np.einsum("nrk,nk->nr", basis, dv)[e]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # a self-contact's rows do not see the root: its six columns cancel
    if self_on:
        e, k = np.nonzero((c.links[:, :, 1] >= 0) & c.kept)
        assert len(e) and np.all(J[e, k][:, :, :6] == 0.0)
    # the summary tallies the kept contacts; clearance never exceeds a kept contact's gap
    links = list(range(m.num_links))
    cnt, clr = c.summary(links)
    assert cnt.sum() == (c.links[c.kept] >= 0).sum()
    for e in range(65):
        for i in range(c.count[e]):
            for l in c.links[e, i]:
                if l >= 0:
                    assert clr[e, l] <= c.gap[e, i]
    no_geom = [l for l in links if l not in set(m.geom_link)]
    assert np.all(np.isinf(clr[:, no_geom]))
