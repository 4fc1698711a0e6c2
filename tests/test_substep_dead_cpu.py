"""The paired kernel's narrow TGS sweeps (mi_pair.hpp, Delassus space, lane r = row r of its half)
find each lane's own row's lambda after a sweep in one of two ways:

  * the chain: after the sweep, one compare / select per row over all RMAX rows of the lambda
    registers every lane keeps (lamv), whatever the row count;
  * the capture: the owner lane keeps the value it projects (`mine`) at its own row step, under the
    sweep's per-group guard, reset to 0 at each sweep's start.

This is a numpy float32 model of one sweep set (iters position sweeps + viters velocity sweeps) of
a wave's two halves, which run in lock step over max(rows of the two halves) rounded up to a group
of four. It checks that the two ways give bit-equal lsum (the lambda sum of the position sweeps)
and bit-equal final lambdas (what the final substep publishes for the force sensors), for row
counts that leave dead rows in the last group of four and groups never run, with friction rows
clamped at +-mu lambda_n. The arithmetic of the projection is the kernel's non-FMA form; what is
compared is only where the lane's lambda is taken from, so the model's roundings need not be the
GPU's."""
import numpy as np
import pytest

RMAX = 32
F = np.float32
MU = F(1.0)
H = F(1.0 / 240.0)
ERP = F(0.2)
MAX_DEPEN = F(10.0)
ITERS, VITERS = 3, 1


def _row_bias(e, step, correct):
    num = np.where(e >= 0, -e, (-ERP * e) if correct else F(0.0)).astype(F)
    b = (num / step).astype(F)
    return np.where(b > MAX_DEPEN, MAX_DEPEN, b).astype(F)


def _med3(x, lo, hi):
    return np.sort(np.stack([x, lo, hi]).astype(F), axis=0)[1]


def _half(rng, nrows):
    """One env's rows: contact triples (normal, friction, friction) then limit rows; lanes past
    the count are dead (A row / column 0, v 0, 1 / A_rr 0, kind 0, separation 0)."""
    ncon = int(rng.integers(0, nrows // 3 + 1)) if nrows else 0
    if nrows >= 3 and ncon == 0:
        ncon = 1
    nc = 3 * ncon
    G = rng.standard_normal((RMAX, 12)).astype(F)
    A = (G @ G.T + np.eye(RMAX, dtype=F) * F(0.5)).astype(F)
    A[nrows:, :] = 0
    A[:, nrows:] = 0
    lane = np.arange(RMAX)
    kd = np.where(lane < nc, lane % 3, 3)
    kd[nrows:] = 0
    v = (rng.standard_normal(RMAX) * 3).astype(F)
    v[:nc:3] = -np.abs(v[:nc:3]) - F(1.0)          # approaching contacts: lambda_n > 0
    v[1:nc:3] *= F(40.0)                           # fast sliding: these friction rows clamp
    v[nrows:] = 0
    sep = (rng.standard_normal(RMAX) * 0.01).astype(F)
    sep[kd == 1] = 0
    sep[kd == 2] = 0
    sep[nrows:] = 0
    ia = np.zeros(RMAX, F)
    ia[:nrows] = F(1.0) / np.diag(A)[:nrows]
    return {"A": A, "kd": kd, "v": v, "sep": sep, "ia": ia, "nrows": nrows, "nnorm": nc}


def _sweeps(h, nrows_max):
    """One half's sweep set. Returns (lsum, final lambda) per lane, found by the chain and by the
    capture, and whether a friction row ended a sweep at its clamp."""
    lane = np.arange(RMAX)
    A, kd, ia, sep = h["A"], h["kd"], h["ia"], h["sep"]
    v = h["v"].copy()
    lamv = np.zeros(RMAX, F)                       # every lane's copy of every row's lambda
    ds = np.zeros(RMAX, F)
    lsum_chain = np.zeros(RMAX, F)
    lsum_cap = np.zeros(RMAX, F)
    cap = np.zeros(RMAX, F)
    clamped = False
    fric = (kd == 1) | (kd == 2)
    for it in range(ITERS + VITERS):
        b = np.where(fric, F(0.0), _row_bias((sep + ds).astype(F), H, it < ITERS)).astype(F)
        lamn = F(0.0)
        cap = np.zeros(RMAX, F)                    # the capture starts every sweep at 0
        for rr in range(RMAX):
            if (rr & ~3) >= nrows_max:             # the group of four is not run
                continue
            l0 = lamv[rr]
            lim = F(MU * lamn)
            x = (l0 + ((b - v).astype(F) * ia).astype(F)).astype(F)   # on every lane; the owner's counts
            mine = _med3(x, np.where(fric, -lim, F(0.0)).astype(F),
                         np.where(fric, lim, F(np.inf)).astype(F))
            ln = mine[rr]                          # the broadcast of the owner's value
            if rr % 3 == 0 and rr < h["nnorm"]:
                lamn = ln
            if fric[rr] and lim > 0 and abs(ln) == lim:
                clamped = True
            v = (v + (A[:, rr] * F(ln - l0)).astype(F)).astype(F)
            lamv[rr] = ln
            cap = np.where(lane == rr, mine, cap).astype(F)
        lo = np.zeros(RMAX, F)                     # the chain: over all RMAX rows
        for rr in range(RMAX):
            lo = np.where(lane == rr, lamv[rr], lo).astype(F)
        if it < ITERS:
            ds = (ds + (H * v).astype(F)).astype(F)
            lsum_chain = (lsum_chain + lo).astype(F)
            lsum_cap = (lsum_cap + cap).astype(F)
    return lsum_chain, lo, lsum_cap, cap, clamped


COUNTS = [0, 1, 3, 4, 5, 31, 32]
# the partner half's count: always another one, smaller and larger ones both occur
PARTNER = {0: 5, 1: 0, 3: 32, 4: 1, 5: 31, 31: 4, 32: 3}


@pytest.mark.parametrize("nrows", COUNTS)
def test_capture_equals_chain(nrows):
    rng = np.random.default_rng(100 + nrows)
    halves = [_half(rng, nrows), _half(rng, PARTNER[nrows])]
    nrows_max = max(h["nrows"] for h in halves)
    any_clamped = False
    for h in halves:
        ls_a, lam_a, ls_b, lam_b, clamped = _sweeps(h, nrows_max)
        any_clamped |= clamped
        assert np.array_equal(ls_a.view(np.uint32), ls_b.view(np.uint32)), "lsum"
        assert np.array_equal(lam_a.view(np.uint32), lam_b.view(np.uint32)), "final lambda"
        n = h["nrows"]
        assert not lam_a[n:].any() and not ls_a[n:].any(), "a dead row's lambda stays 0"
        if n >= 3:
            assert lam_a[:n].any(), "live rows must carry force, or the case shows nothing"
    if nrows_max >= 3:
        assert any_clamped, "no friction row at its clamp"
