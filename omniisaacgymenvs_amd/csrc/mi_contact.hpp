// mi_contact.hpp — contact view: the stepper's contact set for the current state, its gaps and
// its Jacobian rows (include/mi_sim.h mi_get_contacts / mi_get_contact_jacobian /
// mi_get_link_contact_summary), gfx950.
//
// The definitions are P8's of mi_wave.hpp / mi_pair.hpp, restated: ground candidates are the
// model's contact points in pt_geom / pt_end order (gap = root z + x z - r against z = 0, normal
// +z, friction directions +x / +y), self candidates the geom pairs in table order through
// mi_pair_contact / mi_contact_basis of include/mi_geom.h; a candidate is active when gap <
// contact_offset; active ground candidates come first, active pairs follow and are cut at
// (MI_MAX_ROWS - 3 ground - limited joints) / 3. Frames are relative to the root origin, as the
// stepper's; the root position enters the gap's z and the reported world point only.
//
// One kernel, three instantiations, a tile of E envs per 256-lane workgroup:
//   phase 0  the tile's state -> LDS (link_load_state), the slots' fill values (0.0f, link -1);
//   phase 1  forward kinematics, one lane per (env, link): R and root-relative o of every link
//            -> LDS (link_walk<false> of mi_link.hpp restated here, not shared: DESIGN, solve
//            view); the Jacobian call also files each DOF's column (world axis, origin);
//   phase 2  candidates, one lane per (env, candidate): a wave takes one env at a time, its 64
//            lanes the next 64 candidates, ground points and then pairs; every pair goes
//            through the narrow phase (the stepper's broad phase is conservative, and the
//            clearance needs every gap);
//   phase 3  compaction per env in candidate order: ballot + prefix popcount under the budget,
//            no atomics, so every run gives the same bits; the kept contacts are filed in LDS in
//            output order;
//   phase 4  each output is the workgroup's contiguous block [envs, C, ...], stored 16 B per lane
//            (ragged ends and unaligned caller buffers: dwords). The Jacobian rows are formed at
//            store time from the per-env column table and the compacted contacts, four
//            consecutive elements per lane; the 3 C nv rows are never staged.
// LDS per env: state, frames (12 L), C slots of at most 16 words, 6 nv for the Jacobian: no nv^2
// or C nv table. The host shrinks E until the tile fits kCtLdsLimit (E = 1 always does).
#pragma once
#include "mi_link.hpp"
#include "../../include/mi_geom.h"

namespace mi {

constexpr int kCtThreads = 256;
constexpr int kCtWaves = kCtThreads / 64;
constexpr int kCtEnvs = 8;               // envs per workgroup, multiples of 4: a workgroup's
constexpr int kCtJacEnvs = 4;            // output blocks start on 16-B boundaries
constexpr size_t kCtLdsLimit = 64 * 1024;   // what a workgroup gets without a raised limit, as the link / dynamics views

enum { CT_DATA = 0, CT_JAC = 1, CT_SUMMARY = 2 };

struct CtArgs {
    int E, C;                 // env tile; contact capacity per env (ncmax)
    int npairs, nlimc;        // geom pairs (0: self-collision off), joints with a limit
    float contact_offset;
    const int* pairs;         // [npairs][2] geom ids
    int* count; int* links; float* point; float* normal; float* gap;   // CT_DATA
    float* jac;                                                        // CT_JAC
    int* lcount; float* clearance;                                     // CT_SUMMARY
};

// LDS of k_contacts, in floats; every staged output starts on a 16-B boundary
struct CtLds {
    int mask, se, fr, frw, cnt, lnk, pt, dir, gp, tab, kind, clr, tal, total;
    static __host__ __device__ int al4(int x) { return (x + 3) & ~3; }
    __host__ __device__ CtLds(int op, int E, int L, int D, int nv, int C, int K) {
        int o = 0;
        mask = o; o += op == CT_JAC ? al4(4 * E * C) : 0;       // two 64-bit column sets per slot (8-B aligned first)
        se = o; o += al4(E * (kLinkRootW + 2 * D));
        frw = 12 * L + 1;                                       // odd: no bank conflicts across envs
        fr = o; o += al4(E * frw);
        cnt = o; o += al4(E);
        lnk = o; o += al4(E * C * 2);
        pt = o; o += op != CT_SUMMARY ? al4(E * C * 3) : 0;     // world (data) / root-relative (Jacobian)
        dir = o; o += op == CT_JAC ? al4(E * C * 9) : op == CT_DATA ? al4(E * C * 3) : 0;   // n, t1, t2 / n
        gp = o; o += op == CT_DATA ? al4(E * C) : 0;
        tab = o; o += op == CT_JAC ? al4(E * 6 * nv) : 0;       // column table [E][6][nv], as k_link_jacobian's
        kind = o; o += op == CT_JAC ? al4(nv) : 0;
        clr = o; o += op == CT_SUMMARY ? al4(E * K) : 0;
        tal = o; o += op == CT_SUMMARY ? al4(E * K) : 0;
        total = o;
    }
    __host__ __device__ size_t bytes() const { return sizeof(float) * (size_t)total; }
};

// link_walk<false> of mi_link.hpp, restated: world rotation R, origin o relative to the root
// origin and world joint axis a of `link`
MI_D void ct_walk(const DevModel& m, const float* se, int link, float* R, float* o, float* a) {
    m3_from_quat(se + 3, R);
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = 0.0f; a[c] = 0.0f; }
    uint64_t mask = link_chain(m, link);
    while (mask) {
        const int l = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        // R, o hold the parent's frame
        float Rq[9], Rj[9], d[3];
        const float* ql = m.quat + 4 * l;
        const float* al = m.axis + 3 * l;
        m3_from_quat(ql, Rq);
        m3_mul(R, Rq, Rj);
        m3_vec(Rj, al, a);
        m3_vec(R, m.pos + 3 * l, d);
        const float qj = se[kLinkRootW + l - 1];
        if (m.jtype[l] == MI_JOINT_HINGE) {
            float Ra[9];
            m3_axis_angle(al, qj, Ra);
            m3_mul(Rj, Ra, R);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += a[c] * qj;
#pragma unroll
            for (int c = 0; c < 9; ++c) R[c] = Rj[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] += d[c];
    }
}

// Jacobian columns that move `link`: the root's nr, then link l at nr + l - 1
MI_D uint64_t ct_cols(const DevModel& m, int link) {
    return ((1ull << m.nr) - 1) | ((link_chain(m, link) >> 1) << m.nr);
}

// world segment of geom g on its link's frame f (R 9, o 3): the stepper's seg[] of P8
MI_D void ct_segment(const DevModel& m, const float* f, int g, float* p0, float* p1) {
    m3_vec(f, m.geom_p0 + 3 * g, p0);
    m3_vec(f, m.geom_p1 + 3 * g, p1);
#pragma unroll
    for (int q = 0; q < 3; ++q) { p0[q] = p0[q] + f[9 + q]; p1[q] = p1[q] + f[9 + q]; }
}

// n elements of the workgroup's contiguous output block, LDS -> global (link_block_store for
// either element type)
template <typename T>
MI_D void ct_block_store(T* __restrict__ dst, const T* src, int n) {
    static_assert(sizeof(T) == 4, "dword elements");
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += kCtThreads)
            reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += kCtThreads) dst[i] = src[i];
}

template <int OP>
__global__ __launch_bounds__(kCtThreads) void k_contacts(DevModel m, DevState st, CtArgs a, LinkReq rq) {
    extern __shared__ float4 ct_smem[];
    const int E = a.E, C = a.C, L = m.L, nv = m.nv, nr = m.nr, K = rq.K, SW = link_state_width(m);
    const int e0 = blockIdx.x * E, ne = min(E, st.N - e0);
    const CtLds ly(OP, E, L, m.D, nv, C, K);
    float* sm = reinterpret_cast<float*>(ct_smem);
    uint64_t* cm = reinterpret_cast<uint64_t*>(sm + ly.mask);
    float* se = sm + ly.se;
    float* fr = sm + ly.fr;
    int* cnt = reinterpret_cast<int*>(sm + ly.cnt);
    int* lnk = reinterpret_cast<int*>(sm + ly.lnk);
    float* pt = sm + ly.pt;
    float* dir = sm + ly.dir;
    float* gp = sm + ly.gp;
    float* tab = sm + ly.tab;
    int* kind = reinterpret_cast<int*>(sm + ly.kind);
    float* clr = sm + ly.clr;
    int* tal = reinterpret_cast<int*>(sm + ly.tal);
    const int FRW = ly.frw;

    // ---- phase 0: state, and what a slot at or above the env's count holds
    link_load_state(m, st, e0, ne, E, se);
    for (int t = threadIdx.x; t < E * C; t += kCtThreads) {
        lnk[2 * t] = -1; lnk[2 * t + 1] = -1;
        if constexpr (OP != CT_SUMMARY) {
#pragma unroll
            for (int q = 0; q < 3; ++q) pt[3 * t + q] = 0.0f;
        }
        if constexpr (OP == CT_DATA) {
#pragma unroll
            for (int q = 0; q < 3; ++q) dir[3 * t + q] = 0.0f;
            gp[t] = 0.0f;
        }
        if constexpr (OP == CT_JAC) {
#pragma unroll
            for (int q = 0; q < 9; ++q) dir[9 * t + q] = 0.0f;
            cm[2 * t] = 0ull; cm[2 * t + 1] = 0ull;
        }
    }
    for (int t = threadIdx.x; t < E; t += kCtThreads) cnt[t] = 0;
    if constexpr (OP == CT_SUMMARY)
        for (int t = threadIdx.x; t < E * K; t += kCtThreads) clr[t] = INFINITY;
    if constexpr (OP == CT_JAC)
        for (int c = threadIdx.x; c < nv; c += kCtThreads)
            kind[c] = c < nr ? (c >= 3) : (m.jtype[c - nr + 1] == MI_JOINT_HINGE);
    __syncthreads();

    // ---- phase 1: forward kinematics, one lane per (env, link)
    if (C > 0) {
        for (int t = threadIdx.x; t < E * L; t += kCtThreads) {
            const int l = t / E, e = t - l * E;
            if (e >= ne) continue;
            float R[9], o[3], ax[3];
            ct_walk(m, se + e * SW, l, R, o, ax);
            float* f = fr + e * FRW + 12 * l;
#pragma unroll
            for (int q = 0; q < 9; ++q) f[q] = R[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) f[9 + q] = o[q];
            if constexpr (OP == CT_JAC) {
                float* T = tab + e * 6 * nv;
                if (l > 0) {            // a hinge turns about its own origin; a slide's column has no origin term
                    const int c = nr + l - 1;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { T[k * nv + c] = ax[k]; T[(3 + k) * nv + c] = o[k]; }
                } else {                // the root's columns: unit translations, unit rotations about its origin
                    for (int c = 0; c < nr; ++c)
#pragma unroll
                        for (int k = 0; k < 3; ++k) { T[k * nv + c] = (c % 3 == k) ? 1.0f : 0.0f; T[(3 + k) * nv + c] = 0.0f; }
                }
            }
        }
    }
    __syncthreads();

    // ---- phases 2, 3: a wave per env, lanes over candidates, ballot compaction in candidate order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    for (int e = wave; e < ne && C > 0; e += kCtWaves) {
        const float* s = se + e * SW;
        const float* F = fr + e * FRW;
        // slot ci of env e <- a kept contact: links, point pc (root-relative), normal n, gap
        auto file = [&](int ci, int la, int lb, const float* pc, const float* n, float gap) {
            if (ci >= C) return;        // (cannot happen: 3 C covers the row budget)
            const int t = e * C + ci;
            lnk[2 * t] = la; lnk[2 * t + 1] = lb;
            if constexpr (OP == CT_DATA) {
#pragma unroll
                for (int q = 0; q < 3; ++q) { pt[3 * t + q] = s[q] + pc[q]; dir[3 * t + q] = n[q]; }
                gp[t] = gap;
            }
            if constexpr (OP == CT_JAC) {
                float t1[3] = {1.0f, 0.0f, 0.0f}, t2[3] = {0.0f, 1.0f, 0.0f};   // the ground's friction directions
                if (lb >= 0) mi_contact_basis(n, t1, t2);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    pt[3 * t + q] = pc[q];
                    dir[9 * t + q] = n[q]; dir[9 * t + 3 + q] = t1[q]; dir[9 * t + 6 + q] = t2[q];
                }
                // columns of DOFs above the common ancestor (the root's among them) cancel
                const uint64_t ca = ct_cols(m, la), cb = lb >= 0 ? ct_cols(m, lb) : 0ull;
                cm[2 * t] = ca & ~cb; cm[2 * t + 1] = cb & ~ca;
            }
        };
        // the smallest gap of each requested link over this pass's candidates (min: any order, the same bits)
        auto clearance = [&](bool valid, int la, int lb, float gap) {
            if constexpr (OP == CT_SUMMARY) {
                for (int k = 0; k < K; ++k) {
                    const int lk = rq.link[k];
                    float v = valid && (la == lk || lb == lk) ? gap : INFINITY;
                    if (!__any(v < INFINITY)) continue;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
                    if (lane == 0) clr[e * K + k] = fminf(clr[e * K + k], v);
                }
            }
        };
        int ncon = 0;
        for (int c0 = 0; c0 < m.npts; c0 += 64) {
            const int c = c0 + lane;
            bool act = false;
            float pc[3] = {0.0f, 0.0f, 0.0f}, gap = 0.0f;
            int l = 0;
            if (c < m.npts) {
                const int g = m.pt_geom[c];
                l = m.geom_link[g];
                const float* pl = (m.pt_end[c] ? m.geom_p1 : m.geom_p0) + 3 * g;
                const float* f = F + 12 * l;
                float x[3];
                m3_vec(f, pl, x);
#pragma unroll
                for (int q = 0; q < 3; ++q) x[q] += f[9 + q];
                const float r = m.geom_radius[g];
                gap = s[2] + x[2] - r;
                act = gap < a.contact_offset;
                pc[0] = x[0]; pc[1] = x[1]; pc[2] = x[2] - r;
            }
            const unsigned long long mask = __ballot(act);
            if (act) {
                const float up[3] = {0.0f, 0.0f, 1.0f};
                file(ncon + __popcll(mask & below), l, -1, pc, up, gap);
            }
            ncon += __popcll(mask);
            clearance(c < m.npts, l, -1, gap);
        }
        int budget = (MI_MAX_ROWS - 3 * ncon - a.nlimc) / 3;
        for (int p0 = 0; p0 < a.npairs; p0 += 64) {
            const int pi = p0 + lane;
            bool act = false;
            float pc[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f}, gap = 0.0f;
            int la = 0, lb = 0;
            if (pi < a.npairs) {
                const int ga = a.pairs[2 * pi], gb = a.pairs[2 * pi + 1];
                la = m.geom_link[ga]; lb = m.geom_link[gb];
                float a0[3], a1[3], b0[3], b1[3];
                ct_segment(m, F + 12 * la, ga, a0, a1);
                ct_segment(m, F + 12 * lb, gb, b0, b1);
                gap = mi_pair_contact(a0, a1, m.geom_radius[ga], b0, b1, m.geom_radius[gb], pc, n);
                act = gap < a.contact_offset;
            }
            const unsigned long long mask = __ballot(act);
            const int rank = __popcll(mask & below);
            if (act && rank < budget) file(ncon + rank, la, lb, pc, n, gap);
            const int took = budget > 0 ? min(__popcll(mask), budget) : 0;
            ncon += took;
            budget -= took;
            clearance(pi < a.npairs, la, lb, gap);
        }
        if (lane == 0) cnt[e] = ncon;
    }
    __syncthreads();

    // ---- phase 4: the workgroup's output blocks
    if constexpr (OP == CT_DATA) {
        const size_t r0 = (size_t)e0 * C;
        if (a.count) ct_block_store(a.count + e0, cnt, ne);
        if (a.links) ct_block_store(a.links + r0 * 2, lnk, ne * C * 2);
        if (a.point) ct_block_store(a.point + r0 * 3, pt, ne * C * 3);
        if (a.normal) ct_block_store(a.normal + r0 * 3, dir, ne * C * 3);
        if (a.gap) ct_block_store(a.gap + r0, gp, ne * C);
    }
    if constexpr (OP == CT_SUMMARY) {
        // kept contacts that involve link k (a self-contact counts for both of its links)
        for (int t = threadIdx.x; t < ne * K; t += kCtThreads) {
            const int e = t / K, lk = rq.link[t - e * K];
            int n = 0;
            for (int i = 0; i < cnt[e]; ++i) n += (lnk[2 * (e * C + i)] == lk || lnk[2 * (e * C + i) + 1] == lk) ? 1 : 0;
            tal[t] = n;
        }
        __syncthreads();
        if (a.lcount) ct_block_store(a.lcount + (size_t)e0 * K, tal, ne * K);
        if (a.clearance) ct_block_store(a.clearance + (size_t)e0 * K, clr, ne * K);
    }
    if constexpr (OP == CT_JAC) {
        const int per = C * 3 * nv, n = ne * per;
        float* __restrict__ dst = a.jac + (size_t)e0 * per;
        // output element i of the block -> (env, slot, row, column)
        struct Pos { int e, k, r, c; };
        auto locate = [&](int i) {
            Pos p;
            p.e = i / per;
            const int x = i - p.e * per;
            p.k = x / (3 * nv);
            const int y = x - p.k * 3 * nv;
            p.r = y / nv;
            p.c = y - p.r * nv;
            return p;
        };
        // row r (normal, t1, t2) of slot k: direction . (velocity of A's point - B's) per unit of column c
        auto elem = [&](const Pos& p) {
            const int t = p.e * C + p.k, c = p.c;
            const bool ina = (cm[2 * t] >> c) & 1, inb = (cm[2 * t + 1] >> c) & 1;
            if (!ina && !inb) return 0.0f;            // moves neither body, or both alike; slots past the count
            const float* T = tab + p.e * 6 * nv;
            const float* d = dir + 9 * t + 3 * p.r;
            float v;
            if (!kind[c]) {                           // translation: d . a
                v = d[0] * T[c] + d[1] * T[nv + c] + d[2] * T[2 * nv + c];
            } else {                                  // rotation: d . (a x (p - o))
                const float* x = pt + 3 * t;
                const float ax[3] = {T[c], T[nv + c], T[2 * nv + c]};
                const float rr[3] = {x[0] - T[3 * nv + c], x[1] - T[4 * nv + c], x[2] - T[5 * nv + c]};
                float w[3];
                cross3(ax, rr, w);
                v = dot3(d, w);
            }
            return ina ? v : -v;
        };
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            const int n4 = n >> 2;
            for (int i = threadIdx.x; i < n4; i += kCtThreads) {
                Pos p = locate(4 * i);
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = elem(p);
                    if (++p.c == nv) { p.c = 0; if (++p.r == 3) { p.r = 0; if (++p.k == C) { p.k = 0; ++p.e; } } }
                }
                reinterpret_cast<float4*>(dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
            }
            done = n4 << 2;
        }
        for (int i = done + threadIdx.x; i < n; i += kCtThreads) dst[i] = elem(locate(i));
    }
}

}  // namespace mi
