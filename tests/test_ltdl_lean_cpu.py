"""numpy float32 model of the lane-per-column tree LTDL of the compiled-topology kernels
(mi_wave.hpp ct_load_columns / ct_ltdl / ct_publish_factor, mi_pair.hpp ct_ltdl_pair), for both
generated topologies (csrc/mi_topo_gen.hpp), in two statements:
  (a) masked: columns loaded with everything outside the tree pattern zeroed, the multiplier of
      ancestor ii scaled after the broadcast (M[k][ii] * inv), the update of row ii in lanes
      c <= ii only, row k scaled in lanes c < k, 1 / D from the diagonal afterwards;
  (b) lean: row k scaled once per pivot in every lane (t), multipliers broadcast from t, updates
      in every lane, t stored over row k in every lane, 1 / D_k taken from the pivot's inv.
What is read afterwards must be bit-equal: the strict lower triangle, 1 / D, and the factor rows
as ct_publish_factor lays them out. (b) runs with the columns loaded as the kernel loads them (only
the tree pattern kept) and with the upper triangle of the input passed through unmasked, the
input's upper triangle holding arbitrary finite values: nothing below the diagonal may depend on
what is above it. Both variants use the same fused-multiply-add emulation (the product of two
float32 is exact in float64; one rounding of the sum to float32) and the same reciprocal."""
import os
import re

import numpy as np
import pytest

F = np.float32
LANES = 32
HERE = os.path.dirname(os.path.abspath(__file__))
TOPO_GEN = os.path.join(HERE, "..", "omniisaacgymenvs_amd", "csrc", "mi_topo_gen.hpp")


def topologies():
    """{name: (nr, link_parent)} from the generated header."""
    txt = open(TOPO_GEN).read()
    out = {}
    for m in re.finditer(r"struct Robot(\w+)\s*\{(.*?)\n\};", txt, re.S):
        body = m.group(2)
        nr = int(re.search(r"\bnr = (\d+)", body).group(1))
        lp = [int(v) for v in re.search(r"link_parent\[\d+\] = \{([^}]*)\}", body).group(1).split(",")]
        out[m.group(1)] = (nr, lp)
    return out


class DofTree:
    """mi_topo.hpp make_dof_tree: root DOFs 0..nr-1 form a chain, link l's DOF is nr + l - 1."""

    def __init__(self, nr, link_parent):
        L = len(link_parent)
        self.nv = nv = nr + L - 1
        self.parent = [k - 1 for k in range(nr)] + [
            (nr - 1 if link_parent[l] == 0 else nr + link_parent[l] - 1) for l in range(1, L)]
        self.anc = []
        for k in range(nv):
            a, j = [], self.parent[k]
            while j >= 0:
                a.append(j)
                j = self.parent[j]
            self.anc.append(a)                      # nearest first
        self.lrow, o = [], 0
        for k in range(nv):
            self.lrow.append(o)
            o += (len(self.anc[k]) + 3) & ~3
        self.lrow.append(o)
        # keep[r, c]: lane c keeps row r (c == r or c an ancestor of r); lanes >= nv keep nothing
        self.keep = np.zeros((nv, LANES), bool)
        for r in range(nv):
            self.keep[r, [r] + self.anc[r]] = True


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def rcp(x):
    return F(1.0) / F(x)


def load_columns(t, Mx, upper_through):
    """Mc[r, c] = entry r of lane c's column. Lanes >= nv read column 0 and keep nothing."""
    nv = t.nv
    Mc = np.zeros((nv, LANES), F)
    Mc[:, :nv] = Mx
    keep = t.keep.copy()
    if upper_through:
        keep[:, :nv] |= np.triu(np.ones((nv, nv), bool), 1)
    return np.where(keep, Mc, F(0.0))


def ltdl_masked(t, Mc):
    Mc = Mc.copy()
    ln = np.arange(LANES)
    for k in range(t.nv - 1, -1, -1):
        inv = rcp(Mc[k, k])
        for ii in t.anc[k]:
            s = F(Mc[k, ii] * inv)
            m = ln <= ii
            Mc[ii, m] = fma(-s, Mc[k, m], Mc[ii, m])
        m = ln < k
        Mc[k, m] = Mc[k, m] * inv
    dvec = np.ones(LANES, F)
    for c in range(t.nv):
        dvec[c] = rcp(Mc[c, c])
    return Mc, dvec


def ltdl_lean(t, Mc):
    Mc = Mc.copy()
    dvec = np.ones(LANES, F)
    for k in range(t.nv - 1, -1, -1):
        inv = rcp(Mc[k, k])
        tk = (Mc[k] * inv).astype(F)
        for ii in t.anc[k]:
            Mc[ii] = fma(-tk[ii], Mc[k], Mc[ii])
        Mc[k] = tk
        dvec[k] = inv
    return Mc, dvec


def publish(t, Mc, dvec):
    """ct_publish_factor: lane j writes L[i][j] (j an ancestor of i) at lrow[i] + na - 1 - depth(j)."""
    Lr = np.zeros(t.lrow[t.nv] + LANES, F)
    for j in range(t.nv):
        for i in range(t.nv):
            if j in t.anc[i]:
                Lr[t.lrow[i] + len(t.anc[i]) - 1 - len(t.anc[j])] = Mc[i, j]
        Lr[t.lrow[t.nv] + j] = dvec[j]
    return Lr


def tree_spd(t, rng):
    """Random symmetric positive definite float32 matrix with the tree pattern: L^T D L."""
    nv = t.nv
    Lm = np.eye(nv)
    for i in range(nv):
        for j in t.anc[i]:
            Lm[i, j] = rng.uniform(-0.8, 0.8)
    D = np.diag(rng.uniform(0.05, 5.0, nv))
    return (Lm.T @ D @ Lm).astype(F)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name", sorted(topologies()))
def test_lean_ltdl_is_bit_equal_where_it_is_read(name):
    nr, lp = topologies()[name]
    t = DofTree(nr, lp)
    assert t.nv <= LANES
    rng = np.random.default_rng(2024)
    low = np.tril(np.ones((t.nv, t.nv), bool), -1)
    for trial in range(20):
        M = tree_spd(t, rng)
        assert np.array_equal(M != 0, (t.keep[:, :t.nv] | t.keep[:, :t.nv].T)), "tree pattern"
        inputs = [M]
        # the kernel's Mx holds S_j . f in every entry; here: arbitrary finite values above the
        # diagonal, large and tiny magnitudes and both signs included
        J = M.copy()
        up = np.triu(np.ones_like(low), 1)
        J[up] = (rng.standard_normal(up.sum()) * 10.0 ** rng.integers(-20, 20, up.sum())).astype(F)
        inputs.append(J)
        ref = None
        for Mx in inputs:
            a_M, a_d = ltdl_masked(t, load_columns(t, Mx, False))
            if ref is None:
                ref = (a_M, a_d)
            # (a) itself never sees the upper triangle
            assert np.array_equal(bits(a_M), bits(ref[0])) and np.array_equal(bits(a_d), bits(ref[1]))
            assert np.all(a_M[:, :t.nv][np.triu(np.ones_like(low), 1)] == 0)
            for through in (False, True):
                with np.errstate(all="ignore"):            # junk above the diagonal may overflow
                    b_M, b_d = ltdl_lean(t, load_columns(t, Mx, through))
                assert np.array_equal(bits(b_M[:, :t.nv][low]), bits(a_M[:, :t.nv][low])), (trial, through)
                assert np.array_equal(bits(b_d), bits(a_d)), (trial, through)
                assert np.array_equal(bits(publish(t, b_M, b_d)), bits(publish(t, a_M, a_d))), (trial, through)
                assert np.all(b_M[:, t.nv:] == 0)          # lanes >= nv start and stay at zero
                if not through:
                    assert np.isfinite(b_M).all()          # the junk above the diagonal is finite
        # the factor is one: L^T D L gives M back
        Lf = np.eye(t.nv) + np.where(low, ref[0][:, :t.nv].astype(np.float64), 0.0)
        Dm = np.diag(1.0 / ref[1][:t.nv].astype(np.float64))
        assert np.allclose(Lf.T @ Dm @ Lf, M, rtol=1e-4, atol=1e-5)

