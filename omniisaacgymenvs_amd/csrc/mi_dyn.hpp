// mi_dyn.hpp — dynamics view: joint-space inertia M(q), velocity-product forces c(q,u) and
// generalized gravity forces g(q) of the rigid-body tree (include/mi_sim.h mi_get_dynamics), gfx950.
//
// The stepper's own passes 1-3 (mi_artic.hpp), restated so that nothing serial is longer than one
// ancestor chain and the nv^2 output leaves in 16-B stores. Every spatial quantity is taken about
// one point p0 with world axes ([ang; lin]), so composite inertias and forces add up without
// coordinate transforms. p0 is the origin of the first joint (link 1), not the root origin as in
// the stepper: moments about p0 cancel at the magnitude of the links' distance from it, and behind
// a fixed base whose first joint slides (a cart on its rail) the mechanism is metres from the root. Like the Jacobian kernel this one is bound by its stores
// (4 (nv^2 + 2 nv) bytes per env against 4 (13 + 2 D) read). Per workgroup of kDynEnvs envs:
//   phase 0  state -> LDS (link_load_state), each env's gravity, the descendant bit mask of
//            every link;
//   phase 1a one lane per (env, link): link_walk gives the link's world frame and velocity in
//            registers; from them the motion subspace S of its DOF, the spatial velocity V, the
//            compact spatial inertia I (the stepper's 10 floats) and the link's own velocity-
//            product term T = (V x S) u  (root: (0, -w x v), the classical -> spatial shift);
//   phase 1b one lane per (env, link): A = sum of T over the link's chain (ascending = root ->
//            leaf), Newton-Euler force F = I A + V x* I V. No gravity, no damping of any kind;
//   phase 2  one lane per (env, link, component): composite inertia Ic and subtree force Fc as
//            sums over the link's descendant mask in ascending link order. No atomics: the result
//            is the same bits on every run;
//   phase 2b one lane per (env, DOF): f = Ic S, cor = S . Fc, grav = S . Ic (0, -gravity);
//   phase 3  M's block [envs, nv, nv] of the workgroup is contiguous: each lane forms four
//            consecutive elements, M[j][k] = S_min . f_max for an ancestor pair, a literal 0
//            otherwise, and stores them as 16 B; cor / grav go through link_block_store.
// Staged per env: S [nv][6], Ic [L][10], f [nv][6] and the force sums; never the nv^2 rows.
#pragma once
#include "mi_link.hpp"

namespace mi {

constexpr int kDynEnvs = 8;     // envs per workgroup, a multiple of 4: output blocks start on 16-B boundaries

// LDS floats of one env's tables. V and f share one region (V is dead after phase 1b, f is
// written in 2b), so do T and Fc.
struct DynLds {
    int oS, oT, oV, oI, oF, oIc, oG, per;
    __host__ __device__ DynLds(int L, int nv) {
        oS = 0;
        oT = oS + 6 * nv;
        oV = oT + 6 * L;
        oI = oV + 6 * (L > nv ? L : nv);
        oF = oI + 10 * L;
        oIc = oF + 6 * L;
        oG = oIc + 10 * L;
        per = oG + 3;
    }
};

// bytes: descendant masks [L] (8 B each, padded to 16), cor [E][nv], grav [E][nv], state
// [E][13 + 2D], tables [E][per]. The largest model mi_sim_create accepts (L = 33, nv = 38) needs
// 53 KB of the 64 KB a workgroup may have; Humanoid 36 KB.
static inline size_t dyn_lds(int D, int L, int nv) {
    const DynLds o(L, nv);
    return sizeof(uint64_t) * (size_t)((L + 1) & ~1) +
           sizeof(float) * (size_t)(kDynEnvs * (2 * nv + kLinkRootW + 2 * D + o.per));
}

// Gravity of the call: the sim-wide vector, or the first three floats of each env's record of the
// per-env parameter table (mi_set_env_params) when it exists.
struct DynGravity {
    float g[3];
    const float* envp;
    int stride;
};

__global__ __launch_bounds__(kLinkThreads) void k_dynamics(DevModel m, DevState st, DynGravity gv,
                                                          float* __restrict__ M, float* __restrict__ cor,
                                                          float* __restrict__ grav) {
    extern __shared__ float4 link_smem[];
    constexpr int E = kDynEnvs;
    const int L = m.L, D = m.D, nv = m.nv, nr = m.nr;
    const DynLds o(L, nv);
    const int SW = link_state_width(m);
    const int e0 = blockIdx.x * E, ne = min(E, st.N - e0);
    uint64_t* desc = reinterpret_cast<uint64_t*>(link_smem);
    float* scor = reinterpret_cast<float*>(desc + ((L + 1) & ~1));
    float* sgrav = scor + E * nv;
    float* se = sgrav + E * nv;
    float* tab = se + E * SW;
    auto T_ = [&](int e, int off) { return tab + e * o.per + off; };
    link_load_state(m, st, e0, ne, E, se);
    for (int l = threadIdx.x; l < L; l += kLinkThreads) {
        uint64_t d = 0;
        for (int x = l; x < L; ++x)
            if (l == 0 || ((link_chain(m, x) >> l) & 1)) d |= 1ull << x;
        desc[l] = d;
    }
    for (int t = threadIdx.x; t < 3 * ne; t += kLinkThreads) {
        const int e = t / 3, c = t - 3 * e;
        T_(e, o.oG)[c] = gv.envp ? gv.envp[(size_t)(e0 + e) * gv.stride + c] : gv.g[c];
    }
    __syncthreads();
    // ---- phase 1a: frames, S, V, I, T ----
    for (int t = threadIdx.x; t < E * L; t += kLinkThreads) {
        const int l = t / E, e = t - l * E;
        if (e >= ne) continue;
        const float* s = se + e * SW;
        LinkFrame f;
        link_walk<true>(m, s, l, f);
        if (L > 1) {                        // origins relative to p0 = the first joint's origin
            LinkFrame f1;
            link_walk<false>(m, s, 1, f1);
#pragma unroll
            for (int c = 0; c < 3; ++c) f.o[c] -= f1.o[c];
        }
        float V[6], S[6], Tl[6], oxw[3];
        cross3(f.o, f.w, oxw);              // velocity of the link's point at p0: v - w x o
#pragma unroll
        for (int c = 0; c < 3; ++c) { V[c] = f.w[c]; V[3 + c] = f.v[c] + oxw[c]; }
        if (l > 0) {
            if (m.jtype[l] == MI_JOINT_HINGE) {
                S[0] = f.a[0]; S[1] = f.a[1]; S[2] = f.a[2];
                cross3(f.o, f.a, S + 3);
            } else {
                S[0] = S[1] = S[2] = 0.0f;
                S[3] = f.a[0]; S[4] = f.a[1]; S[5] = f.a[2];
            }
            const float ul = s[kLinkRootW + D + l - 1];
            crm(V, S, Tl);                  // = (V_parent x S): S x S = 0
            float* Sk = T_(e, o.oS) + 6 * (nr + l - 1);
#pragma unroll
            for (int c = 0; c < 6; ++c) { Tl[c] *= ul; Sk[c] = S[c]; }
        } else {
            // u' = 0 holds the root origin's classical acceleration at 0 and w constant: the point
            // at p0 has the classical acceleration -w x (w x o), the spatial one less w x v(p0)
            float wv[3], wo[3], wwo[3];
            cross3(V, V + 3, wv);
            cross3(V, f.o, wo);
            cross3(V, wo, wwo);
#pragma unroll
            for (int c = 0; c < 3; ++c) { Tl[c] = 0.0f; Tl[3 + c] = -wwo[c] - wv[c]; }
            float* S0 = T_(e, o.oS);
            for (int k = 0; k < nr; ++k) {  // root DOFs: lin k -> (0, e_k), ang k -> (e_k, o x e_k)
                const int ax = k < 3 ? k : k - 3;
                const float ek[3] = {ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f};
                float oe[3];
                cross3(f.o, ek, oe);
#pragma unroll
                for (int c = 0; c < 3; ++c) { S0[6 * k + c] = k < 3 ? 0.0f : ek[c]; S0[6 * k + 3 + c] = k < 3 ? ek[c] : oe[c]; }
            }
        }
        float I[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const float mass = m.mass[l];
        if (mass > 0.0f) {                  // the stepper's compact inertia about p0 (mi_artic.hpp pass 1)
            float c[3], Tm[9], Iw[9];
            m3_vec(f.R, m.com + 3 * l, c);
            c[0] += f.o[0]; c[1] += f.o[1]; c[2] += f.o[2];
            const float* in = m.inertia + 6 * l;
            const float Ib[9] = {in[0], in[3], in[4], in[3], in[1], in[5], in[4], in[5], in[2]};
            m3_mul(f.R, Ib, Tm);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    Iw[3 * a + b] = Tm[3 * a] * f.R[3 * b] + Tm[3 * a + 1] * f.R[3 * b + 1] + Tm[3 * a + 2] * f.R[3 * b + 2];
            const float cc = dot3(c, c);
            I[0] = mass;
            I[1] = mass * c[0]; I[2] = mass * c[1]; I[3] = mass * c[2];
            I[4] = Iw[0] + mass * (cc - c[0] * c[0]);
            I[5] = Iw[4] + mass * (cc - c[1] * c[1]);
            I[6] = Iw[8] + mass * (cc - c[2] * c[2]);
            I[7] = Iw[1] - mass * c[0] * c[1];
            I[8] = Iw[2] - mass * c[0] * c[2];
            I[9] = Iw[5] - mass * c[1] * c[2];
        }
        float* pT = T_(e, o.oT) + 6 * l;
        float* pV = T_(e, o.oV) + 6 * l;
        float* pI = T_(e, o.oI) + 10 * l;
#pragma unroll
        for (int c = 0; c < 6; ++c) { pT[c] = Tl[c]; pV[c] = V[c]; }
#pragma unroll
        for (int c = 0; c < 10; ++c) pI[c] = I[c];
    }
    __syncthreads();
    // ---- phase 1b: velocity-product acceleration along the chain, Newton-Euler force ----
    if (cor) {
        for (int t = threadIdx.x; t < E * L; t += kLinkThreads) {
            const int l = t / E, e = t - l * E;
            if (e >= ne) continue;
            const float* pT = T_(e, o.oT);
            float A[6], V[6], I[10], IA[6], IV[6], x[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) A[c] = pT[c];
            uint64_t mask = link_chain(m, l);
            while (mask) {
                const int k = __ffsll((unsigned long long)mask) - 1;
                mask &= mask - 1;
#pragma unroll
                for (int c = 0; c < 6; ++c) A[c] += pT[6 * k + c];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) V[c] = T_(e, o.oV)[6 * l + c];
#pragma unroll
            for (int c = 0; c < 10; ++c) I[c] = T_(e, o.oI)[10 * l + c];
            inertia_mul(I, A, IA);
            inertia_mul(I, V, IV);
            crf(V, IV, x);
            float* pF = T_(e, o.oF) + 6 * l;
#pragma unroll
            for (int c = 0; c < 6; ++c) pF[c] = IA[c] + x[c];   // a massless link: I = 0, F = 0
        }
    }
    __syncthreads();
    // ---- phase 2: composite inertia (10) and subtree force (6) per link, fixed order ----
    for (int t = threadIdx.x; t < E * L * 16; t += kLinkThreads) {
        const int c = t & 15, x = t >> 4;
        const int e = x / L, l = x - e * L;
        if (e >= ne) continue;
        const bool force = c >= 10;
        if (force && !cor) continue;
        const float* src = force ? T_(e, o.oF) + (c - 10) : T_(e, o.oI) + c;
        const int w = force ? 6 : 10;
        uint64_t mask = desc[l];
        float sum = 0.0f;
        while (mask) {
            const int d = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            sum += src[w * d];
        }
        (force ? T_(e, o.oT) + 6 * l + (c - 10) : T_(e, o.oIc) + 10 * l + c)[0] = sum;   // Fc reuses T
    }
    __syncthreads();
    // ---- phase 2b: f = Ic S per DOF, cor, grav ----
    for (int t = threadIdx.x; t < E * nv; t += kLinkThreads) {
        const int e = t / nv, k = t - e * nv;
        if (e >= ne) continue;
        const int l = k < nr ? 0 : k - nr + 1;
        float S[6], I[10], fk[6], Fc[6], Ig[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) { S[c] = T_(e, o.oS)[6 * k + c]; Fc[c] = T_(e, o.oT)[6 * l + c]; }
#pragma unroll
        for (int c = 0; c < 10; ++c) I[c] = T_(e, o.oIc)[10 * l + c];
        inertia_mul(I, S, fk);
        const float* g = T_(e, o.oG);
        const float Ag[6] = {0.0f, 0.0f, 0.0f, -g[0], -g[1], -g[2]};   // gravity as a base acceleration
        inertia_mul(I, Ag, Ig);
        float* pf = T_(e, o.oV) + 6 * k;    // f reuses V
#pragma unroll
        for (int c = 0; c < 6; ++c) pf[c] = fk[c];
        scor[t] = cor ? dot6(S, Fc) : 0.0f;
        sgrav[t] = dot6(S, Ig);
    }
    __syncthreads();
    // ---- phase 3: stores ----
    if (cor) link_block_store(cor + (size_t)e0 * nv, scor, ne * nv);
    if (grav) link_block_store(grav + (size_t)e0 * nv, sgrav, ne * nv);
    if (!M) return;
    const int per = nv * nv, n = ne * per;
    float* __restrict__ dst = M + (size_t)e0 * per;
    struct Pos { int e, j, k; };
    auto locate = [&](int i) {
        Pos p;
        p.e = i / per;
        const int x = i - p.e * per;
        p.j = x / nv;
        p.k = x - p.j * nv;
        return p;
    };
    // M[j][k] from the ordered pair (a, b) = (min, max): both triangles hold the same bits
    auto elem = [&](const Pos& p) {
        const int a = min(p.j, p.k), b = max(p.j, p.k);
        if (a >= nr && !((desc[a - nr + 1] >> (b - nr + 1)) & 1)) return 0.0f;   // a root DOF moves every link
        return dot6(T_(p.e, o.oS) + 6 * a, T_(p.e, o.oV) + 6 * b);
    };
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += kLinkThreads) {
            Pos p = locate(4 * i);
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = elem(p);
                if (++p.k == nv) { p.k = 0; if (++p.j == nv) { p.j = 0; ++p.e; } }
            }
            reinterpret_cast<float4*>(dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += kLinkThreads) dst[i] = elem(locate(i));
}

}  // namespace mi
