"""Numpy restatement of the physics DR schedule (include/mi_dr_phys.h) for the tests, written
from the schedule's description, not from the header:

  per env and step:  r = reset != 0 and since >= min_frequency
                     if r: since = 0, epoch += 1;  since += 1
                     counter = (0 if r else counter) + 1
                     if an on_interval schedule exists and counter >= frequency_interval:
                         counter = 0, draws += 1 (the interval schedules fire)
  component c of attribute a:
      v = nominal
      on_reset    and epoch > 0: v = op_r(v, draw(stream 6 + 2a, key epoch, c))
      on_interval and draws > 0: v = op_i(v, draw(stream 7 + 2a, key draws, c))
  draw: Philox4x32-10 block (c >> 1) of (seed, stream, global env id, key); the pair of 24-bit
  uniforms (ua, ub) = words 2 (c & 1), 2 (c & 1) + 1;
      gaussian   p0 + p1 sqrt(-2 ln(1 - ua)) cos(2 pi ub)
      uniform    (p1 - p0) ua + p0
      loguniform exp((ln p1 - ln p0) ua + ln p0)

Values are computed in float64 from the float32 inputs, together with a bound on what a float32
evaluation of the same expression may differ by. With eps = 2^-24 (float32 unit round-off) and
every libm call (logf, cosf, expf, sqrtf) within ULP = 4 ulp (glibc stays below 1 ulp, the
device math library documents 1-2 ulp):
  uniform:    three roundings of terms bounded by |p0| + |p1|          -> 4 eps (|p0| + |p1|)
  gaussian:   ln: relative 2 ULP eps, halved by the root (+ its own ULP eps); the cosine's
              argument 2 pi ub is rounded (absolute 2 pi eps) and the cosine adds 2 ULP eps
              absolute; r <= sqrt(48 ln 2) < 5.77; product and the final multiply-add round
              once each                                                 -> eps (2 |p0| + 128 |p1|)
  loguniform: x = (l1 - l0) ua + l0 carries 2 ULP eps |l| per logarithm and three roundings;
              exp turns the absolute error of x into a relative one and adds 2 ULP eps
                                                    -> v eps ((2 ULP + 4) (|l0| + |l1|) + 2 ULP)
  operations: additive e_x + e_d + eps |v|; scaling |d| e_x + |x| e_d + eps |v|; direct e_d.
"""
import math

import numpy as np

from oracle.oracle import philox

EPS = 2.0 ** -24
ULP = 4
OPS = {"additive": 0, "scaling": 1, "direct": 2}
DISTS = {"gaussian": 0, "normal": 0, "uniform": 1, "loguniform": 2, "log_uniform": 2}
TWO_PI_F32 = float(np.float32(6.283185307179586))


def uniform4(seed, gid, cnt, blk, stream):
    c = philox([blk, cnt, gid & 0xFFFFFFFF, ((gid >> 32) ^ (stream << 28)) & 0xFFFFFFFF],
               [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    return (c >> 8).astype(np.float64) / 16777216.0


def draw(dist, p0, p1, u, c):
    """(value, float32 evaluation bound) of one draw."""
    p0, p1 = float(np.float32(p0)), float(np.float32(p1))
    ua, ub = u[2 * (c & 1)], u[2 * (c & 1) + 1]
    if dist == 0:
        v = p0 + p1 * (math.sqrt(-2.0 * math.log(1.0 - ua)) * math.cos(TWO_PI_F32 * ub))
        return v, EPS * (2 * abs(p0) + 128 * abs(p1))
    if dist == 1:
        return (p1 - p0) * ua + p0, 4 * EPS * (abs(p0) + abs(p1))
    l0, l1 = math.log(p0), math.log(p1)
    v = math.exp((l1 - l0) * ua + l0)
    return v, v * EPS * ((2 * ULP + 4) * (abs(l0) + abs(l1)) + 2 * ULP)


def apply(op, x, ex, d, ed):
    if op == 2:
        return d, ed
    v = x + d if op == 0 else x * d
    e = (ex + ed) if op == 0 else (abs(d) * ex + abs(x) * ed)
    return v, e + EPS * abs(v)


def begin(state, reset, min_frequency, any_interval, frequency_interval):
    """state (since, counter, epoch, draws) -> (new state, r, fire); uint32 arithmetic."""
    since, counter, epoch, draws = (int(x) for x in state)
    r = bool(reset) and since >= min_frequency
    if r:
        since, epoch = 0, (epoch + 1) & 0xFFFFFFFF
    since = (since + 1) & 0xFFFFFFFF
    counter = ((0 if r else counter) + 1) & 0xFFFFFFFF
    fire = False
    if any_interval and counter >= frequency_interval:
        counter, draws, fire = 0, (draws + 1) & 0xFFFFFFFF, True
    return (since, counter, epoch, draws), r, fire


def value(nominal, attr, c, seed, gid, epoch, draws, on_reset, on_interval):
    """Component c of attribute attr after both schedules: (value, bound). A schedule is None or
    (op, dist, p0[dim], p1[dim])."""
    v, e = float(np.float32(nominal)), 0.0
    if on_reset is not None and epoch:
        op, dist, p0, p1 = on_reset
        d, ed = draw(dist, p0[c], p1[c], uniform4(seed, gid, epoch, c >> 1, 6 + 2 * attr), c)
        v, e = apply(op, v, e, d, ed)
    if on_interval is not None and draws:
        op, dist, p0, p1 = on_interval
        d, ed = draw(dist, p0[c], p1[c], uniform4(seed, gid, draws, c >> 1, 7 + 2 * attr), c)
        v, e = apply(op, v, e, d, ed)
    return v, e


class Schedule:
    """Restated schedule of one sim: `sched[(attr, when)] = (op, dist, p0, p1)`, one
    frequency_interval, min_frequency; per-env state [N, 4] and records {attr: [N, dim]}."""

    def __init__(self, nominal, sched, frequency_interval, min_frequency, seed, n, env_id_offset=0):
        self.sched, self.freq, self.minf, self.seed, self.off = sched, frequency_interval, min_frequency, seed, env_id_offset
        self.nominal = {a: np.asarray(v, np.float32) for a, v in nominal.items()}
        self.state = np.zeros((n, 4), np.uint32)
        self.val = {a: np.tile(v.astype(np.float64), (n, 1)) for a, v in self.nominal.items()}
        self.err = {a: np.zeros((n, len(v))) for a, v in self.nominal.items()}

    def step(self, reset):
        any_i = any(w == "on_interval" for (_, w) in self.sched)
        for i in range(len(self.state)):
            st, r, fire = begin(self.state[i], reset[i], self.minf, any_i, self.freq)
            self.state[i] = st
            for a in self.nominal:
                sr, si = self.sched.get((a, "on_reset")), self.sched.get((a, "on_interval"))
                if not ((r and sr is not None) or (fire and si is not None)):
                    continue
                for c in range(len(self.nominal[a])):
                    self.val[a][i, c], self.err[a][i, c] = value(self.nominal[a][c], a, c, self.seed, self.off + i,
                                                                st[2], st[3], sr, si)
