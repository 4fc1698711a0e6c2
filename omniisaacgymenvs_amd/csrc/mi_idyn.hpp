// mi_idyn.hpp — inverse-dynamics view: recursive Newton-Euler torques and joint wrenches, frame
// accelerations, whole-body momentum (include/mi_sim.h mi_get_inverse_dynamics /
// mi_get_link_acceleration / mi_get_momentum), gfx950. One kernel template, k_inverse_dynamics,
// three instantiations (ID_*): an output that is not asked for costs neither LDS nor a phase.
//
// The phases are those of mi_dyn.hpp with the acceleration carried along, and nothing of size nv^2
// exists anywhere: the calls write 4 nv (+ 24 L), 24 K and 4 (11 + 6 nv) bytes per env against
// 4 (13 + 2 D [+ nv]) read. Every spatial quantity is taken about p0, the origin of the first joint
// (link 1), with world axes ([ang; lin]), for mi_dyn.hpp's reason: moments about p0 cancel at the
// magnitude of the links' distance from it, and behind a fixed base whose first joint slides the
// mechanism is metres from the root. Per workgroup of kIdEnvs envs:
//   phase 0   state -> LDS (link_load_state), the accelerations u' [E][nv] (zeros for NULL: one code
//             path, so NULL and an all-zero buffer give the same bits), gravity, descendant masks;
//   phase 1a  one lane per (env, link): link_walk gives the frame; from it S, V, the compact
//             inertia I and the link's own acceleration term T = S u' + (V x S) u (root: its
//             DOFs' S u' plus the classical -> spatial shift of mi_dyn.hpp). ID_MOM: the link's
//             momentum I V and its kinetic energy about its own centre of mass instead of T;
//   ID_TAU    1b: A = sum of T over the link's chain (ascending) + (0, -gravity), the gravity base
//             acceleration; F = I A + V x* I V. 2: subtree sums of F over the descendant masks in
//             ascending order. 3: tau = S . Fc + the mode's diagonal terms; joint_wrench = Fc with
//             its moment shifted to the link's origin;
//   ID_ACC    one lane per (env, frame): A of the frame's link (chain sum, no gravity), spatial ->
//             classical at the frame origin p: a = A_lin + w' x p + w x (V_lin + w x p). Frames on
//             a floating root are formed classically from the root's own entries of u', so the
//             frame (link 0, no offset) is u'[0:6] itself;
//   ID_MOM    2: composite inertias Ic, the total momentum sum I V about p0 and the energy sums, in
//             ascending link order. 3: centre of mass from Ic of the root, momentum shifted to it,
//             cmm column k = Ic_link(k) S_k shifted to it.
// No atomics and a fixed summation order: the same bits on every run. The outputs are staged in
// LDS in output order and leave through link_block_store (16 B per lane).
#pragma once
#include "mi_dyn.hpp"
#include "mi_topo.hpp"

namespace mi {

constexpr int kIdEnvs = 8;      // envs per workgroup, a multiple of 4: output blocks start on 16-B boundaries

enum { ID_TAU = 0, ID_ACC = 1, ID_MOM = 2 };

struct IdArgs {
    int which;                  // MI_MASS_* (ID_TAU)
    float dt;
    const float* acc;           // u' [N,nv] or nullptr (ID_TAU, ID_ACC)
    float* tau;                 // ID_TAU [N,nv]
    float* wrench;              // ID_TAU [N,L,6]
    float* out;                 // ID_ACC [N,K,6]
    float* com;                 // ID_MOM [N,3]
    float* mom;                 // ID_MOM [N,6]
    float* cmm;                 // ID_MOM [N,6,nv]
    float* energy;              // ID_MOM [N,2]
};

// LDS floats behind the descendant masks: u', the staged outputs (each block a multiple of 4
// floats: E is a multiple of 4), the state, then one table per env (odd length: the envs' tables
// start in different banks). Only what the operation uses has a size.
struct IdLds {
    int nmask, oAcc, oOut, oSe, oTab, total;
    int oS, oT, oV, oI, oF, oIc, oO, oK, oG, per;
    __host__ __device__ IdLds(int op, int L, int D, int nv, int K) {
        constexpr int E = kIdEnvs;
        const bool tau = op == ID_TAU, acc = op == ID_ACC, mom = op == ID_MOM;
        nmask = (L + 1) & ~1;
        oAcc = 0;
        oOut = oAcc + (mom ? 0 : E * nv);
        const int out = tau ? nv + 6 * L : acc ? 6 * K : 11 + 6 * nv;
        oSe = oOut + E * out;
        oTab = oSe + E * (kLinkRootW + 2 * D);
        oS = 0;                                     // S [nv][6]
        oT = oS + (acc ? 0 : 6 * nv);               // T [L][6]; ID_TAU: then the subtree forces Fc
        oV = oT + (mom ? 0 : 6 * L);                // V [L][6]
        oI = oV + (mom ? 0 : 6 * L);                // I [L][10]
        oF = oI + (acc ? 0 : 10 * L);               // F [L][6] (ID_MOM: I V)
        oIc = oF + (acc ? 0 : 6 * L);               // Ic [L][10]
        oO = oIc + (mom ? 10 * L : 0);              // link origins [L][3]
        oK = oO + (mom ? 0 : 3 * L);                // ID_MOM: kinetic energy [L], then p0 3, sum I V 6, energy sum 1
        oG = oK + (mom ? L + 10 : 0);               // gravity 3
        per = (oG + 3) | 1;
        total = oTab + E * per;
    }
    __host__ __device__ size_t bytes() const { return sizeof(uint64_t) * (size_t)nmask + sizeof(float) * (size_t)total; }
};
// The largest model mi_sim_create accepts (L = 33, D = 32, nv = 38): ID_TAU 8 x (38 u' + 236 out +
// 77 state + 1255 table) floats = 51.7 KB of the 64 KB a workgroup may have, ID_MOM 46.6 KB, ID_ACC
// with all 33 frames 26.3 KB. Humanoid (L = 22, nv = 27): 35.0 / 32.1 / 17.7 (13 bodies: 16.0) KB.

template <int OP>
__global__ __launch_bounds__(kLinkThreads) void k_inverse_dynamics(DevModel m, DevState st, DynGravity gv, IdArgs a,
                                                                  LinkReq rq) {
    extern __shared__ float4 link_smem[];
    constexpr int E = kIdEnvs;
    constexpr bool kTau = OP == ID_TAU, kAcc = OP == ID_ACC, kMom = OP == ID_MOM;
    const int L = m.L, D = m.D, nv = m.nv, nr = m.nr, K = kAcc ? rq.K : 0;
    const IdLds o(OP, L, D, nv, K);
    const int SW = link_state_width(m);
    const int e0 = blockIdx.x * E, ne = min(E, st.N - e0);
    uint64_t* desc = reinterpret_cast<uint64_t*>(link_smem);
    float* base = reinterpret_cast<float*>(desc + o.nmask);
    float* sacc = base + o.oAcc;
    float* sout = base + o.oOut;
    float* se = base + o.oSe;
    float* tab = base + o.oTab;
    auto T_ = [&](int e, int off) { return tab + e * o.per + off; };
    // ---- phase 0 ----
    link_load_state(m, st, e0, ne, E, se);
    if constexpr (!kAcc) {
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
    }
    if constexpr (!kMom) {
        for (int t = threadIdx.x; t < ne * nv; t += kLinkThreads) sacc[t] = a.acc ? a.acc[(size_t)e0 * nv + t] : 0.0f;
    }
    __syncthreads();
    // ---- phase 1a: frames, S, V, I, T ----
    for (int t = threadIdx.x; t < E * L; t += kLinkThreads) {
        const int l = t / E, e = t - l * E;
        if (e >= ne) continue;
        const float* s = se + e * SW;
        LinkFrame f;
        link_walk<true>(m, s, l, f);
        float p0[3] = {0.0f, 0.0f, 0.0f};
        if (L > 1) {                        // origins relative to p0 = the first joint's origin
            LinkFrame f1;
            link_walk<false>(m, s, 1, f1);
#pragma unroll
            for (int c = 0; c < 3; ++c) { p0[c] = f1.o[c]; f.o[c] -= f1.o[c]; }
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
            if constexpr (!kMom) {
                const float ul = s[kLinkRootW + D + l - 1], al = sacc[e * nv + nr + l - 1];
                crm(V, S, Tl);              // = (V_parent x S): S x S = 0
#pragma unroll
                for (int c = 0; c < 6; ++c) Tl[c] = Tl[c] * ul + S[c] * al;
            }
            if constexpr (!kAcc) {
                float* Sk = T_(e, o.oS) + 6 * (nr + l - 1);
#pragma unroll
                for (int c = 0; c < 6; ++c) Sk[c] = S[c];
            }
        } else {
            if constexpr (!kMom) {
                // the root origin's classical acceleration a and w' are the root's entries of u':
                // the point at p0 has the classical acceleration a - w' x o - w x (w x o), the
                // spatial one less w x v(p0)
                float wv[3], wo[3], wwo[3];
                cross3(V, V + 3, wv);
                cross3(V, f.o, wo);
                cross3(V, wo, wwo);
#pragma unroll
                for (int c = 0; c < 3; ++c) { Tl[c] = 0.0f; Tl[3 + c] = -wwo[c] - wv[c]; }
                if (nr) {
                    const float* ar = sacc + e * nv;
                    float owd[3];
                    cross3(f.o, ar + 3, owd);
#pragma unroll
                    for (int c = 0; c < 3; ++c) { Tl[c] += ar[3 + c]; Tl[3 + c] += ar[c] + owd[c]; }
                }
            }
            if constexpr (!kAcc) {
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
        }
        if constexpr (!kMom) {
            float* pT = T_(e, o.oT) + 6 * l;
            float* pV = T_(e, o.oV) + 6 * l;
            float* pO = T_(e, o.oO) + 3 * l;
#pragma unroll
            for (int c = 0; c < 6; ++c) { pT[c] = Tl[c]; pV[c] = V[c]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) pO[c] = f.o[c];
        }
        if constexpr (!kAcc) {
            float I[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            float ke = 0.0f;
            const float mass = m.mass[l];
            if (mass > 0.0f) {              // the stepper's compact inertia about p0 (mi_artic.hpp pass 1)
                float rc[3], c[3], Tm[9], Iw[9];
                m3_vec(f.R, m.com + 3 * l, rc);
                c[0] = rc[0] + f.o[0]; c[1] = rc[1] + f.o[1]; c[2] = rc[2] + f.o[2];
                const float* in = m.inertia + 6 * l;
                const float Ib[9] = {in[0], in[3], in[4], in[3], in[1], in[5], in[4], in[5], in[2]};
                m3_mul(f.R, Ib, Tm);
#pragma unroll
                for (int x = 0; x < 3; ++x)
#pragma unroll
                    for (int b = 0; b < 3; ++b)
                        Iw[3 * x + b] = Tm[3 * x] * f.R[3 * b] + Tm[3 * x + 1] * f.R[3 * b + 1] + Tm[3 * x + 2] * f.R[3 * b + 2];
                const float cc = dot3(c, c);
                I[0] = mass;
                I[1] = mass * c[0]; I[2] = mass * c[1]; I[3] = mass * c[2];
                I[4] = Iw[0] + mass * (cc - c[0] * c[0]);
                I[5] = Iw[4] + mass * (cc - c[1] * c[1]);
                I[6] = Iw[8] + mass * (cc - c[2] * c[2]);
                I[7] = Iw[1] - mass * c[0] * c[1];
                I[8] = Iw[2] - mass * c[0] * c[2];
                I[9] = Iw[5] - mass * c[1] * c[2];
                if constexpr (kMom) {       // kinetic energy about the link's own centre of mass
                    float wr[3], vc[3], Iww[3];
                    cross3(f.w, rc, wr);
#pragma unroll
                    for (int x = 0; x < 3; ++x) vc[x] = f.v[x] + wr[x];
                    m3_vec(Iw, f.w, Iww);
                    ke = 0.5f * (mass * dot3(vc, vc) + dot3(f.w, Iww));
                }
            }
            float* pI = T_(e, o.oI) + 10 * l;
#pragma unroll
            for (int c = 0; c < 10; ++c) pI[c] = I[c];
            if constexpr (kMom) {
                float IV[6];
                inertia_mul(I, V, IV);
                float* pF = T_(e, o.oF) + 6 * l;
#pragma unroll
                for (int c = 0; c < 6; ++c) pF[c] = IV[c];
                T_(e, o.oK)[l] = ke;
                if (l == 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) T_(e, o.oK)[L + c] = p0[c];
                }
            }
        }
    }
    __syncthreads();

    if constexpr (kAcc) {
        // ---- frame accelerations: spatial -> classical at the frame origin ----
        for (int t = threadIdx.x; t < E * K; t += kLinkThreads) {
            const int k = t / E, e = t - k * E;
            if (e >= ne) continue;
            const int link = rq.link[k];
            float r[3] = {0.0f, 0.0f, 0.0f};
            if (rq.has_off) {
                LinkFrame f;
                link_walk<false>(m, se + e * SW, link, f);
                const float off[3] = {rq.off[3 * k], rq.off[3 * k + 1], rq.off[3 * k + 2]};
                m3_vec(f.R, off, r);
            }
            const float* V = T_(e, o.oV) + 6 * link;
            const float w[3] = {V[0], V[1], V[2]};
            float* dst = sout + (e * K + k) * 6;
            if (link == 0) {
                // the root: a + w' x r + w x (w x r) from its own entries of u' (a fixed base: zeros)
                const float* ar = sacc + e * nv;
                const float ao[3] = {nr ? ar[0] : 0.0f, nr ? ar[1] : 0.0f, nr ? ar[2] : 0.0f};
                const float wd[3] = {nr ? ar[3] : 0.0f, nr ? ar[4] : 0.0f, nr ? ar[5] : 0.0f};
                float wdr[3], wr[3], wwr[3];
                cross3(wd, r, wdr);
                cross3(w, r, wr);
                cross3(w, wr, wwr);
#pragma unroll
                for (int c = 0; c < 3; ++c) { dst[c] = ao[c] + (wdr[c] + wwr[c]); dst[3 + c] = wd[c]; }
                continue;
            }
            const float* pT = T_(e, o.oT);
            float A[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) A[c] = pT[c];
            uint64_t mask = link_chain(m, link);
            while (mask) {
                const int j = __ffsll((unsigned long long)mask) - 1;
                mask &= mask - 1;
#pragma unroll
                for (int c = 0; c < 6; ++c) A[c] += pT[6 * j + c];
            }
            const float* pO = T_(e, o.oO) + 3 * link;
            const float p[3] = {pO[0] + r[0], pO[1] + r[1], pO[2] + r[2]};
            float wp[3], vp[3], wvp[3], wdp[3];
            cross3(w, p, wp);
#pragma unroll
            for (int c = 0; c < 3; ++c) vp[c] = V[3 + c] + wp[c];
            cross3(w, vp, wvp);
            cross3(A, p, wdp);
#pragma unroll
            for (int c = 0; c < 3; ++c) { dst[c] = A[3 + c] + wdp[c] + wvp[c]; dst[3 + c] = A[c]; }
        }
        __syncthreads();
        link_block_store(a.out + (size_t)e0 * K * 6, sout, ne * K * 6);
    }

    if constexpr (kTau) {
        // ---- phase 1b: acceleration along the chain, gravity as a base acceleration, force ----
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
            const float* g = T_(e, o.oG);
#pragma unroll
            for (int c = 0; c < 3; ++c) A[3 + c] -= g[c];
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
        __syncthreads();
        // ---- phase 2: subtree force per link, fixed order (Fc reuses T) ----
        for (int t = threadIdx.x; t < E * L * 6; t += kLinkThreads) {
            const int x = t / 6, c = t - 6 * x;
            const int e = x / L, l = x - e * L;
            if (e >= ne) continue;
            const float* src = T_(e, o.oF) + c;
            uint64_t mask = desc[l];
            float sum = 0.0f;
            while (mask) {
                const int d = __ffsll((unsigned long long)mask) - 1;
                mask &= mask - 1;
                sum += src[6 * d];
            }
            T_(e, o.oT)[6 * l + c] = sum;
        }
        __syncthreads();
        // ---- phase 3: projection onto S, the mode's diagonal terms; wrenches at the link origins ----
        float* stau = sout;
        float* swr = sout + E * nv;
        if (a.tau) {
            for (int t = threadIdx.x; t < ne * nv; t += kLinkThreads) {
                const int e = t / nv, k = t - e * nv;
                const int l = k < nr ? 0 : k - nr + 1;
                float v = dot6(T_(e, o.oS) + 6 * k, T_(e, o.oT) + 6 * l);
                if (k >= nr && a.which != MI_MASS_RIGID) {
                    const int j = k - nr;
                    const float* rec = gv.envp ? gv.envp + (size_t)(e0 + e) * gv.stride : nullptr;
                    const float damp = rec ? rec[kEnvpDamping + j] : m.damping[j + 1];
                    const float arm = rec ? rec[kEnvpDamping + D + j] : m.armature[j + 1];
                    const float diag = a.which == MI_MASS_STEPPER ? arm + a.dt * damp : arm;
                    v += diag * sacc[t] + damp * se[e * SW + kLinkRootW + D + j];
                }
                stau[t] = v;
            }
        }
        if (a.wrench) {
            for (int t = threadIdx.x; t < ne * L; t += kLinkThreads) {
                const int e = t / L, l = t - e * L;
                const float* Fc = T_(e, o.oT) + 6 * l;
                float of[3];
                cross3(T_(e, o.oO) + 3 * l, Fc + 3, of);
#pragma unroll
                for (int c = 0; c < 3; ++c) { swr[6 * t + c] = Fc[3 + c]; swr[6 * t + 3 + c] = Fc[c] - of[c]; }
            }
        }
        __syncthreads();
        if (a.tau) link_block_store(a.tau + (size_t)e0 * nv, stau, ne * nv);
        if (a.wrench) link_block_store(a.wrench + (size_t)e0 * L * 6, swr, ne * L * 6);
    }

    if constexpr (kMom) {
        // ---- phase 2: composite inertias (10 per link), total momentum (6) and energy sum (1) ----
        for (int t = threadIdx.x; t < E * L * 10; t += kLinkThreads) {
            const int x = t / 10, c = t - 10 * x;
            const int e = x / L, l = x - e * L;
            if (e >= ne) continue;
            if (!a.cmm && l > 0) continue;  // com / mom / energy need the root's composite only
            const float* src = T_(e, o.oI) + c;
            uint64_t mask = desc[l];
            float sum = 0.0f;
            while (mask) {
                const int d = __ffsll((unsigned long long)mask) - 1;
                mask &= mask - 1;
                sum += src[10 * d];
            }
            T_(e, o.oIc)[10 * l + c] = sum;
        }
        for (int t = threadIdx.x; t < ne * 7; t += kLinkThreads) {
            const int e = t / 7, c = t - 7 * e;
            const float* src = c < 6 ? T_(e, o.oF) + c : T_(e, o.oK);
            const int w = c < 6 ? 6 : 1;
            float sum = 0.0f;
            for (int l = 0; l < L; ++l) sum += src[w * l];
            T_(e, o.oK)[L + 3 + c] = sum;
        }
        __syncthreads();
        // ---- phase 3: centre of mass, momentum about it, energies; cmm columns ----
        float* scom = sout;
        float* smom = scom + E * 3;
        float* sen = smom + E * 6;
        float* scmm = sen + E * 2;
        auto com_p0 = [&](int e, float* c) {   // the centre of mass relative to p0
            const float* Ic = T_(e, o.oIc);
            const float inv = Ic[0] > 0.0f ? 1.0f / Ic[0] : 0.0f;
#pragma unroll
            for (int x = 0; x < 3; ++x) c[x] = Ic[1 + x] * inv;
        };
        for (int e = threadIdx.x; e < ne; e += kLinkThreads) {
            float c[3], cf[3];
            com_p0(e, c);
            const float* s = se + e * SW;
            const float* P = T_(e, o.oK) + L;
            const float* h = P + 3;
            const float* g = T_(e, o.oG);
            cross3(c, h + 3, cf);
            double pe = 0.0;                // -M gravity . com: world positions are large, one rounding
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                scom[3 * e + x] = s[x] + (P[x] + c[x]);
                smom[6 * e + x] = h[3 + x];
                smom[6 * e + 3 + x] = h[x] - cf[x];
                pe -= (double)g[x] * ((double)s[x] + ((double)P[x] + (double)c[x]));
            }
            sen[2 * e] = h[6];
            sen[2 * e + 1] = (float)(pe * (double)T_(e, o.oIc)[0]);
        }
        if (a.cmm) {
            for (int t = threadIdx.x; t < ne * nv; t += kLinkThreads) {
                const int e = t / nv, k = t - e * nv;
                const int l = k < nr ? 0 : k - nr + 1;
                float c[3], fk[6], cf[3];
                com_p0(e, c);
                inertia_mul(T_(e, o.oIc) + 10 * l, T_(e, o.oS) + 6 * k, fk);
                cross3(c, fk + 3, cf);
                float* col = scmm + e * 6 * nv + k;
#pragma unroll
                for (int x = 0; x < 3; ++x) { col[x * nv] = fk[3 + x]; col[(3 + x) * nv] = fk[x] - cf[x]; }
            }
        }
        __syncthreads();
        if (a.com) link_block_store(a.com + (size_t)e0 * 3, scom, ne * 3);
        if (a.mom) link_block_store(a.mom + (size_t)e0 * 6, smom, ne * 6);
        if (a.energy) link_block_store(a.energy + (size_t)e0 * 2, sen, ne * 2);
        if (a.cmm) link_block_store(a.cmm + (size_t)e0 * 6 * nv, scmm, ne * 6 * nv);
    }
}

}  // namespace mi
