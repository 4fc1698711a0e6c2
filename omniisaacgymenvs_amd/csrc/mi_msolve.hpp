// mi_msolve.hpp — mass-matrix solve view: products with the inverse of the joint-space inertia the
// stepper factorises (include/mi_sim.h mi_solve_mass / mi_get_forward_dynamics /
// mi_get_link_task_inertia), gfx950. One kernel, k_mass_solve, three operations (MS_*).
//
// Mt = M + diag(armature [+ dt damping]) on the joint DOFs, M the rigid-body inertia of
// mi_dyn.hpp (the same value, formed in double: see ms_terms). Mt never leaves the chip: per
// workgroup of kMsEnvs envs
//   phases 0-2b  ms_terms (mi_dyn.hpp's phases, restated below): for MS_FD cor / grav in float as
//                there; for M each link's inertia about p0 and the composite inertias in double;
//   assemble     lower triangle of Mt into the env's LDS block H [nv][ms], ms = nv | 1:
//                H[r][c] = S_c . (Ic_r S_r) in double, rounded once, for c an ancestor DOF of r (the root's DOFs form a chain, as in
//                the stepper's dof_parent table), the mode's diagonal added; armature / damping
//                from the env's record of the per-env parameter table when it exists, else the model;
//   factor       tree LTDL in place (mi_artic.hpp: Mt = L^T D L, k = nv-1 .. 0, no fill-in because
//                parent[l] < l): for each k one lane per (env, ancestor pair (i, j) of k, j <= i):
//                H[i][j] -= (H[k][i] / H[k][k]) H[k][j]; one barrier per k. Every element gets one
//                update per k in descending k: a fixed order, no atomics. Row k is final once k is
//                reached and is read unscaled; all rows are scaled to L after the loop;
//   solves       the R vectors of an env go through LDS tiles of VT vectors [E][VT][nvs], nvs =
//                nv | 1 (odd: the lanes of a wave, one per (env, vector), hit distinct banks; H is
//                read at one address per env, a broadcast). Tile <- rhs (coalesced), or the
//                forward-dynamics right-hand side, or Jacobian rows formed from the per-env column
//                table (k_link_jacobian's); two substitution sweeps along the ancestor lists
//                (wave-uniform indices: no runtime-indexed register array, no scratch); tile ->
//                global in 16-B stores on 16-B lines of the caller's buffer, dwords at ragged ends;
//   MS_TASK      lam_inv[i][j] = J_min . X_max with X = Mt^-1 J^T rows of the tile: one lane per
//                (frame, vector) forms the frame's six rows in one walk over its columns; each pair
//                is computed by one code path for both triangles.
// The H blocks overlay ms_terms' float tables, which the assembly (double tables only) no longer reads.
#pragma once
#include "mi_dyn.hpp"
#include "mi_topo.hpp"

namespace mi {

constexpr int kMsEnvs = 4;                          // envs per workgroup, a multiple of 4 (16-B output blocks)
constexpr int kMsMaxVT = kLinkThreads / kMsEnvs;    // one lane per (env, vector of the tile)
constexpr size_t kMsLdsLimit = 96 * 1024;            // of the 160 KB of a gfx950 CU (set as the kernel's dynamic-LDS limit at mi_sim_create)

enum { MS_SOLVE = 0, MS_FD = 1, MS_TASK = 2 };

struct MsArgs {
    int op, which, R, VT;     // R vectors per env (MS_FD: 1, MS_TASK: 6 K), VT of them per LDS tile
    float dt;
    const float* rhs;         // MS_SOLVE: [N,R,nv]; MS_FD: tau [N,D] or nullptr (the state's efforts)
    float* out;               // MS_SOLVE: out; MS_FD: acc; MS_TASK: minv_jt or nullptr
    float* lam;               // MS_TASK: lam_inv or nullptr
    const float* wq;          // MS_FD: the body wrenches' generalized forces [N,nv] (mi_wrench.hpp) or nullptr
    const float* drv;         // the joint drives' records [N][4][D] (include/mi_drive.h) or nullptr: MI_MASS_STEPPER's
                              // diagonal takes dt * mi_drive_damping; MS_FD its damping (kd alone in
                              // MI_MASS_ARMATURE, continuous time) and mi_drive_effort
};

// LDS. Masks, the double inertias of the M path, cor / grav, state, ancestor lists (bytes), DOF axes
// and origins; MS_TASK adds the column table, frame origins and column kinds; one region holds
// ms_terms' float tables and then the H blocks; the vector tile.
struct MsLds {
    int nmask, ndbl, ms, MB, nvs, anc_f, task_f, uni, oScor, oSe, oAnc, oCol, oSp, oKind, oSD, oUni, oTile, total;
    __host__ __device__ MsLds(int L, int D, int nv, int K, int VT) {
        constexpr int E = kMsEnvs;
        const DynLds o(L, nv);
        nmask = ((L + 1) & ~1) + ((K + 1) & ~1);    // uint64 each
        ndbl = E * L * 20;                          // double I [L][10], Ic [L][10] per env (the M path)
        ms = nv | 1;
        MB = (nv * ms) | 1;                         // odd: the envs' blocks start in different banks
        nvs = nv | 1;
        anc_f = (nv * nv + nv + 3) / 4;             // uint8 anc[nv][nv], dep[nv]
        oScor = 0;
        oSe = oScor + 2 * E * nv;
        oAnc = oSe + E * (kLinkRootW + 2 * D);
        oCol = oAnc + anc_f;
        oSp = oCol + (K ? E * 6 * nv : 0);
        oKind = oSp + E * K * 3;
        oSD = oKind + (K ? nv : 0);                 // axis 3, origin 3 of every DOF
        oUni = oSD + E * 6 * nv;
        uni = o.per > MB ? o.per : MB;              // ms_terms' float tables, then the H blocks
        oTile = oUni + E * uni;
        total = oTile + E * VT * nvs;
    }
    __host__ __device__ size_t bytes() const { return sizeof(uint64_t) * (size_t)nmask + sizeof(double) * (size_t)ndbl + sizeof(float) * (size_t)total; }
};

// The largest model mi_sim_create accepts (L = 33, D = 32, nv = 38): masks 0.3 KB, double inertias
// 4 x 33 x 160 B = 20.6 KB, cor / grav 1.2 KB, state 1.2 KB, ancestor lists 1.5 KB, DOF axes /
// origins 3.6 KB, tables / H 4 x 5.9 KB = 23.7 KB: 52.6 KB for a solve of one vector, 91.0 KB with
// a full tile of 64 vectors per env (4 x 64 x 39 floats = 39 KB); all 33 frames add the column
// table 3.6 KB, origins 1.5 KB, kinds and masks 0.4 KB and run at 63 vectors per tile in 95.9 KB.
// A full tile is above the 64 KB a workgroup gets by default, so kMsLdsLimit = 96 KB (of a CU's
// 160 KB) is set as the kernel's dynamic-LDS limit; ms_tile_vectors shrinks the tile to fit it.
// Humanoid (L = 22, nv = 27): 35.4 KB for a solve (R = 6: 37.5 KB; four workgroups per CU, which
// 4096 envs need to run in one round), 65.4 KB for all 13 bodies; Ant 15.5 / 29.8 KB.
static inline int ms_tile_vectors(int L, int D, int nv, int K, int R) {
    int VT = R < kMsMaxVT ? R : kMsMaxVT;
    while (VT > 1 && MsLds(L, D, nv, K, VT).bytes() > kMsLdsLimit) --VT;
    return VT;
}

// Phases 0-2b of mi_dyn.hpp for the workgroup's ne envs at e0 (E env slots), restated: k_dynamics
// calling a shared function compiled to other float contractions and its M and cor changed bits,
// so that kernel stays as it is and this one has its own copy of the same statements. Leaves in
// LDS, per env: S at oS, f = Ic S at oV, Ic at oIc; cor / grav in scor / sgrav [E][nv] (cor = 0
// unless `cor`); the state in se, the descendant masks in desc. Ends on a barrier.
template <int E>
MI_D void ms_terms(const DevModel& m, const DevState& st, const DynGravity& gv, const DynLds& o, int e0, int ne,
                    uint64_t* desc, float* scor, float* sgrav, float* se, float* tab, bool cor, double* dI, float* sD) {
    const int L = m.L, D = m.D, nv = m.nv, nr = m.nr;
    const int SW = link_state_width(m);
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
        // The M path (k_mass_solve's assembly) in double from the same float frame: the link's
        // inertia about p0, and the axis and origin of its DOF. About one common point a distal
        // joint's small inertia is a difference of m |c|^2-sized terms; rounded to float that
        // difference, times Mt's condition number, was several times the float32 reference's error.
        double Id[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (mass > 0.0f) {
            const float* cb = m.com + 3 * l;
            const float* in = m.inertia + 6 * l;
            const double Ib[9] = {in[0], in[3], in[4], in[3], in[1], in[5], in[4], in[5], in[2]};
            double c[3], Tm[9], Iw[9];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                c[a] = (double)f.R[3 * a] * cb[0] + (double)f.R[3 * a + 1] * cb[1] + (double)f.R[3 * a + 2] * cb[2] + (double)f.o[a];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    Tm[3 * a + b] = (double)f.R[3 * a] * Ib[b] + (double)f.R[3 * a + 1] * Ib[3 + b] + (double)f.R[3 * a + 2] * Ib[6 + b];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    Iw[3 * a + b] = Tm[3 * a] * f.R[3 * b] + Tm[3 * a + 1] * f.R[3 * b + 1] + Tm[3 * a + 2] * f.R[3 * b + 2];
            const double md = mass, cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
            Id[0] = md;
            Id[1] = md * c[0]; Id[2] = md * c[1]; Id[3] = md * c[2];
            Id[4] = Iw[0] + md * (cc - c[0] * c[0]);
            Id[5] = Iw[4] + md * (cc - c[1] * c[1]);
            Id[6] = Iw[8] + md * (cc - c[2] * c[2]);
            Id[7] = Iw[1] - md * c[0] * c[1];
            Id[8] = Iw[2] - md * c[0] * c[2];
            Id[9] = Iw[5] - md * c[1] * c[2];
        }
        double* pd = dI + ((size_t)e * L + l) * 20;
#pragma unroll
        for (int c = 0; c < 10; ++c) pd[c] = Id[c];
        if (l > 0) {
            float* q = sD + (e * nv + nr + l - 1) * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) { q[c] = f.a[c]; q[3 + c] = f.o[c]; }
        } else {
            for (int k = 0; k < nr; ++k) {
                float* q = sD + (e * nv + k) * 6;
#pragma unroll
                for (int c = 0; c < 3; ++c) { q[c] = (k % 3 == c) ? 1.0f : 0.0f; q[3 + c] = f.o[c]; }
            }
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
    for (int t = threadIdx.x; t < E * L * 10; t += kLinkThreads) {     // the composite inertia in double
        const int c = t % 10, x = t / 10;
        const int e = x / L, l = x - e * L;
        if (e >= ne) continue;
        const double* src = dI + (size_t)e * L * 20 + c;
        uint64_t mask = desc[l];
        double sum = 0.0;
        while (mask) {
            const int d = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            sum += src[20 * d];
        }
        dI[((size_t)e * L + l) * 20 + 10 + c] = sum;
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
}

// Motion subspace of DOF k about p0 in double from its staged axis and origin q = (a, o): a
// rotation (hinge, root angular) is (a, o x a), a translation (slide, root linear) (0, a).
MI_D void ms_dof_subspace(const DevModel& m, const float* q, int k, double* S) {
    const bool rot = k < m.nr ? k >= 3 : m.jtype[k - m.nr + 1] == MI_JOINT_HINGE;
    const double a[3] = {q[0], q[1], q[2]}, o[3] = {q[3], q[4], q[5]};
    if (rot) {
        S[0] = a[0]; S[1] = a[1]; S[2] = a[2];
        S[3] = o[1] * a[2] - o[2] * a[1]; S[4] = o[2] * a[0] - o[0] * a[2]; S[5] = o[0] * a[1] - o[1] * a[0];
    } else {
        S[0] = S[1] = S[2] = 0.0;
        S[3] = a[0]; S[4] = a[1]; S[5] = a[2];
    }
}
// inertia_mul (mi_device.hpp) in double
MI_D void ms_inertia_mul(const double* I, const double* v, double* o) {
    const double* w = v;
    const double* l = v + 3;
    const double* h = I + 1;
    const double hxv[3] = {h[1] * l[2] - h[2] * l[1], h[2] * l[0] - h[0] * l[2], h[0] * l[1] - h[1] * l[0]};
    const double hxw[3] = {h[1] * w[2] - h[2] * w[1], h[2] * w[0] - h[0] * w[2], h[0] * w[1] - h[1] * w[0]};
    o[0] = I[4] * w[0] + I[7] * w[1] + I[8] * w[2] + hxv[0];
    o[1] = I[7] * w[0] + I[5] * w[1] + I[9] * w[2] + hxv[1];
    o[2] = I[8] * w[0] + I[9] * w[1] + I[6] * w[2] + hxv[2];
    o[3] = I[0] * l[0] - hxw[0];
    o[4] = I[0] * l[1] - hxw[1];
    o[5] = I[0] * l[2] - hxw[2];
}

// nt vectors [v0, v0 + nt) of each of the workgroup's ne envs, LDS tile -> dst [N][R][nv]. Per env
// the segment is contiguous; it is cut at the 16-B lines of dst itself, so whole lines leave as one
// 16-B store whatever the caller's alignment, and the ragged ends as dwords.
MI_D void ms_store(float* dst, const float* tile, int e0, int ne, int R, int v0, int nt, int VT, int nv, int nvs) {
    const int n = nt * nv, qmax = (n + 6) >> 2;
    for (int t = threadIdx.x; t < ne * qmax; t += kLinkThreads) {
        const int e = t / qmax, qi = t - e * qmax;
        float* de = dst + ((size_t)(e0 + e) * R + v0) * nv;
        const int a = (int)((reinterpret_cast<uintptr_t>(de) >> 2) & 3);
        const int x0 = 4 * qi - a;
        if (x0 >= n) continue;
        const float* te = tile + (size_t)e * VT * nvs;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = min(max(x0 + j, 0), n - 1);
            const int r = x / nv;
            v[j] = te[r * nvs + (x - r * nv)];
        }
        if (x0 >= 0 && x0 + 4 <= n) {
            *reinterpret_cast<float4*>(de + x0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j >= 0 && x0 + j < n) de[x0 + j] = v[j];
        }
    }
}

__global__ __launch_bounds__(kLinkThreads) void k_mass_solve(DevModel m, DevState st, DynGravity gv, MsArgs a,
                                                            LinkReq rq) {
    extern __shared__ float4 link_smem[];
    constexpr int E = kMsEnvs;
    const int L = m.L, D = m.D, nv = m.nv, nr = m.nr, K = a.op == MS_TASK ? rq.K : 0;
    const int R = a.R, VT = a.VT;
    const DynLds o(L, nv);
    const MsLds ml(L, D, nv, K, VT);
    const int SW = link_state_width(m), ms = ml.ms, MB = ml.MB, nvs = ml.nvs;
    const int e0 = blockIdx.x * E, ne = min(E, st.N - e0);
    uint64_t* desc = reinterpret_cast<uint64_t*>(link_smem);
    uint64_t* cm = desc + ((L + 1) & ~1);
    double* dI = reinterpret_cast<double*>(desc + ml.nmask);
    float* base = reinterpret_cast<float*>(dI + ml.ndbl);
    float* scor = base + ml.oScor;
    float* sgrav = scor + E * nv;
    float* se = base + ml.oSe;
    unsigned char* anc = reinterpret_cast<unsigned char*>(base + ml.oAnc);
    unsigned char* dep = anc + nv * nv;
    float* colT = base + ml.oCol;
    float* sp = base + ml.oSp;
    int* kind = reinterpret_cast<int*>(base + ml.oKind);
    float* sD = base + ml.oSD;
    float* tab = base + ml.oUni;       // ms_terms' tables [E][o.per], then the H blocks [E][MB]: the
    float* Hb = tab;                   // assembly reads the double tables only
    float* tile = base + ml.oTile;

    // ancestor DOFs of every DOF, nearest first (the stepper's dof_parent chains)
    for (int k = threadIdx.x; k < nv; k += kLinkThreads) {
        int d = 0;
        for (int j = m.dof_parent[k]; j >= 0; j = m.dof_parent[j]) anc[k * nv + d++] = (unsigned char)j;
        dep[k] = (unsigned char)d;
    }
    if (K) {
        for (int k = threadIdx.x; k < K; k += kLinkThreads)
            cm[k] = ((1ull << nr) - 1) | ((link_chain(m, rq.link[k]) >> 1) << nr);
        for (int c = threadIdx.x; c < nv; c += kLinkThreads)
            kind[c] = c < nr ? (c >= 3) : (m.jtype[c - nr + 1] == MI_JOINT_HINGE);
    }
    ms_terms<E>(m, st, gv, o, e0, ne, desc, scor, sgrav, se, tab, a.op == MS_FD, dI, sD);

    // ---- MS_TASK: column table and frame origins, as k_link_jacobian forms them ----
    for (int t = threadIdx.x; t < (K ? E * (L + K) : 0); t += kLinkThreads) {
        const int j = t / E, e = t - j * E;
        if (e >= ne) continue;
        const float* s = se + e * SW;
        float* T = colT + e * 6 * nv;
        LinkFrame f;
        if (j >= L) {
            const int k = j - L;
            link_walk<false>(m, s, rq.link[k], f);
            float r[3] = {0.0f, 0.0f, 0.0f};
            if (rq.has_off) {
                const float off[3] = {rq.off[3 * k], rq.off[3 * k + 1], rq.off[3 * k + 2]};
                m3_vec(f.R, off, r);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) sp[(e * K + k) * 3 + c] = f.o[c] + r[c];
        } else if (j > 0) {
            link_walk<false>(m, s, j, f);
            const int c = nr + j - 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) { T[k * nv + c] = f.a[k]; T[(3 + k) * nv + c] = f.o[k]; }
        } else {
            for (int c = 0; c < nr; ++c)
#pragma unroll
                for (int k = 0; k < 3; ++k) { T[k * nv + c] = (c % 3 == k) ? 1.0f : 0.0f; T[(3 + k) * nv + c] = 0.0f; }
        }
    }
    // ---- assemble the lower triangle of Mt ----
    for (int t = threadIdx.x; t < E * nv * nv; t += kLinkThreads) {
        const int e = t / (nv * nv), x = t - e * nv * nv;
        const int r = x / nv, c = x - r * nv;
        if (e >= ne || c > r) continue;
        float v = 0.0f;
        if (c < nr || ((desc[c - nr + 1] >> (r - nr + 1)) & 1)) {    // a root DOF moves every link
            double Sr[6], Sc[6], fr[6];
            ms_dof_subspace(m, sD + (e * nv + r) * 6, r, Sr);
            ms_dof_subspace(m, sD + (e * nv + c) * 6, c, Sc);
            ms_inertia_mul(dI + ((size_t)e * L + (r < nr ? 0 : r - nr + 1)) * 20 + 10, Sr, fr);
            v = (float)(Sc[0] * fr[0] + Sc[1] * fr[1] + Sc[2] * fr[2] + Sc[3] * fr[3] + Sc[4] * fr[4] + Sc[5] * fr[5]);
        }
        if (r == c && r >= nr) {
            const int j = r - nr;
            const float* rec = gv.envp ? gv.envp + (size_t)(e0 + e) * gv.stride : nullptr;
            float damp = rec ? rec[kEnvpDamping + j] : m.damping[j + 1];
            const float arm = rec ? rec[kEnvpDamping + D + j] : m.armature[j + 1];
            if (a.drv && a.which == MI_MASS_STEPPER) {
                const float* dl = a.drv + (size_t)(e0 + e) * MI_DRIVE_LINES * D + j;
                damp = mi_drive_damping(damp, dl[MI_DRIVE_KP * D], dl[MI_DRIVE_KD * D], a.dt);
            }
            v += a.which == MI_MASS_STEPPER ? arm + a.dt * damp : arm;
        }
        Hb[e * MB + r * ms + c] = v;
    }
    __syncthreads();
    // ---- tree LTDL in place ----
    for (int k = nv - 1; k > 0; --k) {
        const int d = dep[k];
        const unsigned char* ak = anc + k * nv;
        for (int t = threadIdx.x; t < E * d * d; t += kLinkThreads) {
            const int e = t & (E - 1), p = t / E;
            const int ia = p / d, ib = p - ia * d;
            if (e >= ne || ib < ia) continue;       // nearest first: ib >= ia is j <= i
            const int i = ak[ia], j = ak[ib];
            float* H = Hb + e * MB;
            H[i * ms + j] -= (H[k * ms + i] / H[k * ms + k]) * H[k * ms + j];
        }
        __syncthreads();
    }
    for (int t = threadIdx.x; t < E * nv * nv; t += kLinkThreads) {
        const int e = t / (nv * nv), x = t - e * nv * nv;
        const int k = x / nv, ia = x - k * nv;
        if (e >= ne || ia >= dep[k]) continue;
        float* H = Hb + e * MB;
        const int i = anc[k * nv + ia];
        H[k * ms + i] = H[k * ms + i] / H[k * ms + k];
    }
    __syncthreads();
    // ---- the vectors, VT per env at a time ----
    const int Q = 6 * K;
    for (int v0 = 0; v0 < R; v0 += VT) {
        const int nt = min(VT, R - v0), per = nt * nv;
        for (int t = threadIdx.x; t < ne * per; t += kLinkThreads) {
            const int e = t / per, x = t - e * per;
            const int v = x / nv, c = x - v * nv;
            float val;
            if (a.op == MS_SOLVE) {
                val = a.rhs[((size_t)(e0 + e) * R + v0) * nv + x];
            } else if (a.op == MS_FD) {
                val = -scor[e * nv + c] - sgrav[e * nv + c];
                if (c >= nr) {
                    const int j = c - nr;
                    float damp = gv.envp ? gv.envp[(size_t)(e0 + e) * gv.stride + kEnvpDamping + j] : m.damping[j + 1];
                    float tau = a.rhs ? a.rhs[(size_t)(e0 + e) * D + j] : st.eff[sx(st, j, e0 + e)];
                    if (a.drv) {
                        // the stepper's B_E and tau + F_d; in continuous time the spring is all force
                        const float* dl = a.drv + (size_t)(e0 + e) * MI_DRIVE_LINES * D + j;
                        const float kp = dl[MI_DRIVE_KP * D], kd = dl[MI_DRIVE_KD * D];
                        tau = mi_drive_effort(tau, kp, kd, se[e * SW + kLinkRootW + j], dl[MI_DRIVE_QT * D], dl[MI_DRIVE_QDT * D]);
                        damp = mi_drive_damping(damp, a.which == MI_MASS_STEPPER ? kp : 0.0f, kd, a.dt);
                    }
                    val += tau - damp * se[e * SW + kLinkRootW + D + j];
                }
                if (a.wq) val += a.wq[(size_t)(e0 + e) * nv + c];
            } else {
                const int row = v0 + v, k = row / 6;
                val = link_jac_elem(colT + e * 6 * nv, sp + (e * K + k) * 3, kind, cm[k], nv, row - 6 * k, c);
            }
            tile[(e * VT + v) * nvs + c] = val;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < E * nt; t += kLinkThreads) {
            const int e = t / nt, v = t - e * nt;
            if (e >= ne) continue;
            float* x = tile + (e * VT + v) * nvs;
            const float* H = Hb + e * MB;
            for (int i = nv - 1; i > 0; --i) {
                const float xi = x[i];
                for (int j = m.dof_parent[i]; j >= 0; j = m.dof_parent[j]) x[j] -= H[i * ms + j] * xi;
            }
            for (int i = 0; i < nv; ++i) x[i] = x[i] / H[i * ms + i];
            for (int i = 1; i < nv; ++i) {
                float xi = x[i];
                for (int j = m.dof_parent[i]; j >= 0; j = m.dof_parent[j]) xi -= H[i * ms + j] * x[j];
                x[i] = xi;
            }
        }
        __syncthreads();
        if (a.out) ms_store(a.out, tile, e0, ne, R, v0, nt, VT, nv, nvs);
        if (a.lam) {
            // pair (i, j), j = v0 + v in the tile: the first half of the items writes row j (i <= j,
            // i fastest), the second half column j (i < j, v fastest); one code path forms the value
            // An item is (frame k, vector): one walk over the frame's columns forms the frame's six
            // rows at once, element by element what link_jac_elem forms.
            const int half = ne * nt * K;
            for (int t = threadIdx.x; t < 2 * half; t += kLinkThreads) {
                const bool col = t >= half;
                const int y = col ? t - half : t;
                const int e = y / (nt * K), z = y - e * nt * K;
                const int v = col ? z % nt : z / K, k = col ? z / nt : z - v * K;
                const int j = v0 + v;
                if (6 * k > j) continue;
                const float* x = tile + (e * VT + v) * nvs;
                const float* T = colT + e * 6 * nv;
                const float p[3] = {sp[(e * K + k) * 3], sp[(e * K + k) * 3 + 1], sp[(e * K + k) * 3 + 2]};
                uint64_t cols = cm[k];
                float val[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                while (cols) {
                    const int c = __ffsll((unsigned long long)cols) - 1;
                    cols &= cols - 1;
                    const float xc = x[c];
                    const float ax[3] = {T[c], T[nv + c], T[2 * nv + c]};
                    if (kind[c]) {
                        const float d[3] = {p[0] - T[3 * nv + c], p[1] - T[4 * nv + c], p[2] - T[5 * nv + c]};
                        float ad[3];
                        cross3(ax, d, ad);
#pragma unroll
                        for (int r = 0; r < 3; ++r) { val[r] += ad[r] * xc; val[3 + r] += ax[r] * xc; }
                    } else {
#pragma unroll
                        for (int r = 0; r < 3; ++r) val[r] += ax[r] * xc;
                    }
                }
                float* le = a.lam + (size_t)(e0 + e) * Q * Q;
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    const int i = 6 * k + r;
                    if (col ? i < j : i <= j) le[(size_t)(col ? i : j) * Q + (col ? j : i)] = val[r];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace mi
