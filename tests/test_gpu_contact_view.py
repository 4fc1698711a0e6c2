"""Contact view on the GPU (include/mi_sim.h mi_get_contacts / mi_get_contact_jacobian /
mi_get_link_contact_summary, robots/articulations.py) against the numpy reference of
tests/contact_ref.py.

Exact outputs (count, links, their order) are compared for every env: the state generator keeps no
env with a candidate within rounding of contact_offset (tests/contact_ref.py contact_state).
Toleranced outputs follow the link view's rule, nothing tuned: the reference runs twice on the
float32 state read back from the device, in float64 and in float32; the device may be off the
float64 run by 4 x the float32 run's worst deviation per output kind, floored at 2 ulp of the
output's magnitude. Measured (MI355X, Humanoid N = 257, device error / bound): point 1.9e-6 / 1.1e-5,
normal 8.6e-6 / 3.5e-5, gap 1.9e-7 / 7.5e-7, J 2.8e-6 / 1.8e-5, clearance 1.9e-7 / 7.5e-7. Every case
prints its own figures (pytest -s); DESIGN §2 has the table."""
import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests.contact_ref import ZBAND, Contacts, contact_basis, contact_state
from tests.test_contact_view_cpu import BUDGET_N, BUDGET_OFFSET, BUDGET_TRUNCATED
from tests.test_gpu_link_view import link_state, read_state, write_state

pytestmark = pytest.mark.gpu
# (robot, envs, contact_offset override): ragged last workgroup, ground + self, ground only, C = 0,
# a single env, and the budget case (pairs cut at the row budget)
CASES = [("Humanoid", 257, None), ("Ant", 257, None), ("Cartpole", 257, None), ("Ant", 1, None),
         ("Humanoid", BUDGET_N, BUDGET_OFFSET)]
EPS = float(np.finfo(np.float32).eps)
SENT = 123456789
MI_E_NULL, MI_E_SHAPE, MI_E_ARG = -1, -2, -5


# ---- device calls: fresh NaN / sentinel filled buffers, `shift` floats off 16-B alignment ----
def _buf(shape, dtype, shift=0):
    n = int(np.prod(shape))
    t = torch.full((n + 4,), float("nan") if dtype is torch.float32 else SENT, dtype=dtype, device="cuda:0")
    return t[shift:shift + n].view(*shape) if n else t[:0].view(*shape)


def contacts(view, C, want=("count", "links", "point", "normal", "gap"), shift=0):
    n = view.count
    shapes = dict(count=((n,), torch.int32), links=((n, C, 2), torch.int32), point=((n, C, 3), torch.float32),
                  normal=((n, C, 3), torch.float32), gap=((n, C), torch.float32))
    t = {k: _buf(*shapes[k], shift=shift) if k in want else None for k in shapes}
    rc = N.lib().mi_get_contacts(view.handle, *(N.ptr(t[k]) for k in shapes), view.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in t.items() if v is not None}


def contact_jac(view, C, shift=0):
    J = _buf((view.count, C, 3, view.num_gen_vel), torch.float32, shift)
    rc = N.lib().mi_get_contact_jacobian(view.handle, N.ptr(J), view.stream())
    torch.cuda.synchronize()
    return rc, J.cpu().numpy()


def summary(view, links, count=True, clearance=True, K=None, shift=0):
    ids = np.ascontiguousarray(links, dtype=np.int32)
    K = len(ids) if K is None else K
    cnt = _buf((view.count, max(K, 0)), torch.int32, shift) if count else None
    clr = _buf((view.count, max(K, 0)), torch.float32, shift) if clearance else None
    rc = N.lib().mi_get_link_contact_summary(view.handle, N.iptr(ids), K, N.ptr(cnt), N.ptr(clr), view.stream())
    torch.cuda.synchronize()
    return rc, None if cnt is None else cnt.cpu().numpy(), None if clr is None else clr.cpu().numpy()


def rule(a32, a64):
    return max(4.0 * float(np.abs(a32.astype(np.float64) - a64).max(initial=0.0)),
               2.0 * EPS * float(np.abs(a64).max(initial=0.0)))


def within(tag, got, ref, bound):
    err = float(np.abs(got.astype(np.float64) - ref).max(initial=0.0))
    print(f"{tag}: device error {err:.3e} bound {bound:.3e}")
    assert np.isfinite(got).all(), tag
    assert err <= bound, (tag, err, bound)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}" + ("-budget" if c[2] else ""))
def case(request, gpu):
    name, n, off = request.param
    ov = [f"task.sim.{name}.contact_offset={off}"] if off else None
    env = make_env(name, num_envs=n, device="cuda:0", seed=11, overrides=ov)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    offset = float(view.sim_params.contact_offset)
    self_on = bool(view.sim_params.enable_self_collisions) and len(m.pairs) > 0
    gen, _ = contact_state(m, n, view.env_origins, 17, offset, self_on, ZBAND.get(name, (0.0, 0.0)))
    write_state(view, gen)
    st = read_state(view)
    c64, c32 = Contacts(m, st, offset, self_on), Contacts(m, st, offset, self_on, dtype=np.float32)
    if c64.NC:                                             # the generator's guarantee, on the state read back
        band = max(4.0 * float(np.abs(c32.cgap - c64.cgap).max()), 2.0 * EPS * float(np.abs(c64.cgap).max()))
        assert (np.abs(c64.cgap - offset) >= band).all()
    assert np.array_equal(c64.slot, c32.slot)
    J64, dead = c64.jacobian()
    J32, _ = c32.jacobian()
    links = list(range(m.num_links))
    s64, s32 = c64.summary(links), c32.summary(links)
    fin = np.isfinite(s64[1])
    bound = dict(point=rule(c32.point, c64.point), normal=rule(c32.normal, c64.normal), gap=rule(c32.gap, c64.gap),
                 jac=rule(J32, J64), clearance=rule(s32[1][fin], s64[1][fin]))
    c = dict(name=name, n=n, tag=f"{name}-{n}" + ("-budget" if off else ""), env=env, view=view, model=m, st=st, c64=c64, J64=J64,
             dead=dead, s64=s64, bound=bound, links=links, C=c64.C, budget=off is not None)
    yield c
    env.close()


def test_capacity(case):
    view, c64, m = case["view"], case["c64"], case["model"]
    cap, ng, npr = (np.zeros(1, np.int32) for _ in range(3))
    assert N.lib().mi_get_contact_capacity(view.handle, N.iptr(cap), N.iptr(ng), N.iptr(npr)) == 0
    assert (int(cap[0]), int(ng[0]), int(npr[0])) == (c64.C, c64.npts, len(c64.pairs))
    assert view.max_contacts == c64.C
    if case["name"] == "Cartpole":
        assert c64.C == 0
    assert N.lib().mi_abi_version() == 4


def test_contact_set(case):
    """count, links and their order are the reference's for every env; point, normal and gap within
    the rule; slots at and above count hold 0.0 / -1; NaN-filled buffers come back without NaN."""
    view, c64, b, tag = case["view"], case["c64"], case["bound"], case["tag"]
    rc, got = contacts(view, case["C"])
    assert rc == 0
    assert np.array_equal(got["count"], c64.count)
    assert np.array_equal(got["links"], c64.links)
    for k in ("point", "normal", "gap"):
        within(f"{tag} {k}", got[k], getattr(c64, k), b[k])
    free = ~c64.kept
    assert np.all(got["links"][free] == -1)
    for k in ("point", "normal", "gap"):
        assert np.all(got[k][free] == 0.0)
    if case["C"]:
        assert np.all(got["gap"][c64.kept] < float(view.sim_params.contact_offset))
    if case["budget"]:
        assert int(c64.truncated.sum()) == BUDGET_TRUNCATED
    print(f"{tag}: contacts per env max {got['count'].max()}, envs with contacts {(got['count'] > 0).sum()}, "
          f"truncated {int(c64.truncated.sum())}")


def test_jacobian(case):
    """J within the rule; cancelled columns and free slots exactly 0.0f. Self-consistency on the
    device's own outputs: J_c u against (normal, t1, t2) applied to the point velocities from
    mi_get_link_state at the device's contact points. Its tolerance: nv max|u| x the Jacobian bound
    (the sum's worst case) plus twice the rule's bound for the reference's own basis . dv (each
    side within one bound of the float64 value)."""
    view, c64, m, st, tag, C = case["view"], case["c64"], case["model"], case["st"], case["tag"], case["C"]
    rc, J = contact_jac(view, C)
    assert rc == 0 and J.shape == (case["n"], C, 3, view.num_gen_vel)
    if C == 0:
        return
    within(f"{tag} jac", J, case["J64"], case["bound"]["jac"])
    deadx = np.broadcast_to(case["dead"][:, :, None, :], J.shape)
    assert np.all(J[deadx] == 0.0) and not np.signbit(J[deadx]).any()
    # the device's own frame velocities at its own contact points
    rc, got = contacts(view, C)
    rc2, ls = link_state(view, case["links"], None)
    assert rc == 0 and rc2 == 0
    u = c64.kin.u(st["vel"], st["qd"])
    Ju = np.einsum("nkrc,nc->nkr", J.astype(np.float64), u)
    want, ref64, ref32 = np.zeros_like(Ju), np.zeros_like(Ju), np.zeros(Ju.shape, np.float32)
    c32 = Contacts(m, st, float(view.sim_params.contact_offset), len(c64.pairs) > 0, dtype=np.float32)
    e, k = np.nonzero(c64.kept)
    la, lb = got["links"][e, k, 0], got["links"][e, k, 1]
    p = got["point"][e, k].astype(np.float64)
    vel = ls["vel"].astype(np.float64)
    pos = ls["pos"].astype(np.float64)
    pv = lambda l: vel[e, l, :3] + np.cross(vel[e, l, 3:], p - pos[e, l])
    dv = pv(la) - np.where((lb >= 0)[:, None], pv(np.maximum(lb, 0)), 0.0)
    nrm = got["normal"][e, k].astype(np.float64)
    t1, t2 = contact_basis(nrm)
    ground = lb < 0
    t1[ground], t2[ground] = (1, 0, 0), (0, 1, 0)
    want[e, k] = np.stack([(nrm * dv).sum(1), (t1 * dv).sum(1), (t2 * dv).sum(1)], axis=1)
    for c, out in ((c64, ref64), (c32, ref32)):
        for j in np.unique(c.slot[c.slot >= 0]):
            ee, kk = np.nonzero(c.slot == j)
            a_, b_ = (int(x) for x in c.clinks[j])
            q = c.cpoint[:, j]
            d = c.point_velocity(a_, q) - (c.point_velocity(b_, q) if b_ >= 0 else 0)
            basis = np.stack([c.cnormal[:, j], c.ct1[:, j], c.ct2[:, j]], axis=1)
            out[ee, kk] = np.einsum("nrk,nk->nr", basis, d)[ee]
    tol = view.num_gen_vel * float(np.abs(u).max()) * case["bound"]["jac"] + 2.0 * rule(ref32, ref64)
    err = float(np.abs(Ju - want).max())
    print(f"{tag} jac @ u - basis . dv: {err:.3e} bound {tol:.3e}")
    assert err <= tol


def test_summary(case):
    view, c64, m, tag = case["view"], case["c64"], case["model"], case["tag"]
    links = case["links"]
    rc, cnt, clr = summary(view, links)
    assert rc == 0
    rc, got = contacts(view, case["C"])
    tally = np.zeros_like(cnt)
    for k, l in enumerate(links):
        tally[:, k] = (got["links"] == l).any(axis=2).sum(axis=1)
    assert np.array_equal(cnt, tally) and np.array_equal(cnt, case["s64"][0])
    r = case["s64"][1]
    assert np.array_equal(np.isinf(clr), np.isinf(r)) and np.all(clr[np.isinf(clr)] > 0)
    fin = np.isfinite(r)
    within(f"{tag} clearance", clr[fin], r[fin], case["bound"]["clearance"])
    for e, k in zip(*np.nonzero(c64.kept)):
        for l in got["links"][e, k]:
            if l >= 0:
                assert clr[e, l] <= got["gap"][e, k]
    if case["name"] == "Cartpole":
        assert not cnt.any() and np.all(np.isinf(clr))
    # a selection in another order, one id twice; either output alone
    sel = [links[-1], links[0], links[-1]]
    rc, c2, r2 = summary(view, sel)
    assert rc == 0 and np.array_equal(c2, cnt[:, sel]) and np.array_equal(r2, clr[:, sel])
    rc, c3, r3 = summary(view, sel, clearance=False)
    assert rc == 0 and r3 is None and np.array_equal(c3, c2)
    rc, c4, r4 = summary(view, sel, count=False)
    assert rc == 0 and c4 is None and np.array_equal(r4, r2)


def test_repeatable(case):
    """Two calls give identical bits; NULL outputs leave the others' bits unchanged; caller buffers
    4 B off 16-B alignment give the same values."""
    view, C = case["view"], case["C"]
    rc, a = contacts(view, C)
    rc2, b = contacts(view, C)
    assert rc == 0 and rc2 == 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for want in (("count",), ("links", "gap"), ("point",), ("normal", "count")):
        rc, part = contacts(view, C, want=want)
        assert rc == 0 and sorted(part) == sorted(want)
        for k in want:
            assert part[k].tobytes() == a[k].tobytes(), (want, k)
    assert contacts(view, C, want=())[0] == 0
    rc, un = contacts(view, C, shift=1)
    assert rc == 0
    for k in a:
        assert un[k].tobytes() == a[k].tobytes(), k
    rc, J = contact_jac(view, C)
    rc2, J2 = contact_jac(view, C)
    rc3, J3 = contact_jac(view, C, shift=1)
    assert rc == rc2 == rc3 == 0 and J.tobytes() == J2.tobytes() == J3.tobytes()
    rc, c1, r1 = summary(view, case["links"])
    rc2, c2, r2 = summary(view, case["links"], shift=1)
    assert rc == rc2 == 0 and c1.tobytes() == c2.tobytes() and r1.tobytes() == r2.tobytes()


def test_python_surface(case):
    view, m, n, C = case["view"], case["model"], case["n"], case["C"]
    rc, raw = contacts(view, C)
    cnt, bodies, pts, nrm, sep = view.get_contact_data()
    assert cnt.dtype == bodies.dtype == torch.int32 and pts.dtype == nrm.dtype == sep.dtype == torch.float32
    assert tuple(cnt.shape) == (n,) and tuple(bodies.shape) == (n, C, 2) and tuple(pts.shape) == (n, C, 3)
    assert tuple(nrm.shape) == (n, C, 3) and tuple(sep.shape) == (n, C)
    assert np.array_equal(cnt.cpu().numpy(), raw["count"]) and np.array_equal(pts.cpu().numpy(), raw["point"])
    assert np.array_equal(sep.cpu().numpy(), raw["gap"]) and np.array_equal(nrm.cpu().numpy(), raw["normal"])
    body_of = np.array([m.get_body_index(m.body_of_link[l]) for l in range(m.num_links)] + [-1])
    assert np.array_equal(bodies.cpu().numpy(), body_of[raw["links"]])
    J = view.get_contact_jacobians()
    assert tuple(J.shape) == (n, C, 3, view.num_gen_vel) and np.array_equal(J.cpu().numpy(), contact_jac(view, C)[1])
    idx = torch.tensor([n - 1, 0], device="cuda:0")
    sub = view.get_contact_data(indices=idx)
    for a, b in zip(sub, (cnt, bodies, pts, nrm, sep)):
        assert torch.equal(a, b[idx])
    assert torch.equal(view.get_contact_jacobians(indices=idx), J[idx])
    a, b = view.get_contact_data(clone=False), view.get_contact_data(clone=False)
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(a, b)) and a[0].data_ptr() != cnt.data_ptr()
    assert view.get_contact_jacobians(clone=False).data_ptr() == view.get_contact_jacobians(clone=False).data_ptr()
    # bodies of a RigidPrimView
    names = [m.body_names[-1], m.body_names[0]]
    lv = view.get_link_view(names)
    ids = [int(m.body_link[m.get_body_index(b)]) for b in names]
    rc, want_c, want_r = summary(view, ids)
    cc, ms = lv.get_contact_counts(), lv.get_min_separations()
    assert cc.dtype == torch.int32 and ms.dtype == torch.float32 and tuple(cc.shape) == tuple(ms.shape) == (n, 2)
    assert np.array_equal(cc.cpu().numpy(), want_c) and np.array_equal(ms.cpu().numpy(), want_r)
    assert torch.equal(lv.get_contact_counts(indices=idx), cc[idx])
    assert lv.get_min_separations(clone=False).data_ptr() == lv.get_min_separations(clone=False).data_ptr() != ms.data_ptr()


def test_argument_errors(case):
    """Bad arguments return the error codes, name the argument and leave the outputs untouched."""
    view, L = case["view"], case["model"].num_links
    lib = N.lib()
    if case["C"]:
        assert lib.mi_get_contact_jacobian(view.handle, None, view.stream()) == MI_E_NULL and b"J" in lib.mi_last_error()
    else:                                                  # C = 0: nothing to write, every call returns 0
        assert lib.mi_get_contact_jacobian(view.handle, None, view.stream()) == 0
    untouched = lambda c, r: np.all(c == SENT) and np.isnan(r).all()
    rc, c, r = summary(view, [0], K=-1)
    assert rc == MI_E_SHAPE and b"K=-1" in lib.mi_last_error()
    rc, c, r = summary(view, [0] * (L + 1))
    assert rc == MI_E_SHAPE and untouched(c, r)
    rc, c, r = summary(view, [0, L])
    assert rc == MI_E_ARG and f"link_ids[1]={L}".encode() in lib.mi_last_error() and untouched(c, r)
    rc, c, r = summary(view, [-1])
    assert rc == MI_E_ARG and b"link_ids[0]=-1" in lib.mi_last_error() and untouched(c, r)
    cnt = _buf((view.count, 1), torch.int32)
    assert lib.mi_get_link_contact_summary(view.handle, None, 1, N.ptr(cnt), None, view.stream()) == MI_E_NULL
    torch.cuda.synchronize()
    assert np.all(cnt.cpu().numpy() == SENT)
    assert lib.mi_get_contacts(None, None, None, None, None, None, view.stream()) == MI_E_NULL
    assert summary(view, [], K=0)[0] == 0


def test_after_stepping(gpu):
    """Deferred substeps are issued by the getter itself, and after real steps (bodies resting on the
    ground) the device's set is the reference's on the state read back, for every env whose gaps
    are clear of the threshold by the generator's band."""
    n = 64
    env = make_env("Ant", num_envs=n, device="cuda:0", seed=23)
    env.reset()
    view = env.task.get_robot()
    g = torch.Generator().manual_seed(4)
    for _ in range(40):
        env.step((torch.rand((n, env.num_actions), generator=g) * 2 - 1).cuda())
    view.sim_step(2)                                       # deferred
    rc, got = contacts(view, view.max_contacts)            # must flush
    st = read_state(view)
    off = float(view.sim_params.contact_offset)
    c64, c32 = Contacts(view.model, st, off, False), Contacts(view.model, st, off, False, dtype=np.float32)
    band = max(4.0 * float(np.abs(c32.cgap - c64.cgap).max()), 2.0 * EPS * float(np.abs(c64.cgap).max()))
    clear = (np.abs(c64.cgap - off) >= band).all(axis=1)
    print(f"Ant after stepping: {int(clear.sum())} of {n} envs clear of the band {band:.2e}, "
          f"{int((got['count'] > 0).sum())} touch the ground")
    assert rc == 0 and clear.any()
    assert np.array_equal(got["count"][clear], c64.count[clear])
    assert np.array_equal(got["links"][clear], c64.links[clear])
    env.close()
