// mi_link.hpp — link-frame view: poses, velocities and Jacobians of frames rigidly attached to
// links (include/mi_sim.h mi_get_link_state / mi_get_link_jacobian), gfx950.
//
// Both kernels are bound by their stores (13 K floats per env, 6 nv K for the Jacobian) and read
// almost nothing (13 + 2 D state floats per env), so the work is laid out around the output:
//   phase 0  the workgroup's envs' state -> LDS, in the state layout's contiguous direction
//            (field-major SoA: env fastest; per-env records: field fastest);
//   phase 1  forward kinematics, one lane per (env, frame): the lane walks its frame's ancestor
//            chain root -> leaf (parent[l] < l, so the chain is the set bits of a 64-bit mask in
//            ascending order) with R, o, quat, omega, v in registers — no per-link array, no
//            scratch; the chain repeats work of sibling frames, which is a few hundred FLOPs
//            against kilobytes of output per env;
//   phase 2  the workgroup's output block [envs, K, ...] is contiguous in global memory: every
//            lane stores 16 B of it per instruction, consecutive lanes consecutive addresses.
//            Link state: the rows are staged in LDS in output order and copied out. Jacobian:
//            staging the rows themselves (Humanoid, all links: 14 KB per env) would cap the
//            occupancy, so the per-env column table (world axis + origin per DOF, 6 nv floats)
//            and the frame origins are staged instead and each lane forms its four consecutive
//            output elements from them — one cross-product component each.
// A ragged last workgroup (N not a multiple of the env tile) loads, walks and stores only its
// ne < E envs.
#pragma once
#include "mi_device.hpp"

namespace mi {

constexpr int kLinkMaxK = MI_MAXA + 1;   // frames per call <= links of a model (mi_sim_create)
constexpr int kLinkThreads = 256;
constexpr int kLinkStateEnvs = 16;       // envs per workgroup, multiples of 4: a workgroup's
constexpr int kLinkJacEnvs = 4;          // output block starts on a 16-B boundary
constexpr int kLinkRootW = 13;           // root pos 3, quat 4, vel 6 ahead of q, qd in the LDS copy

// the request, by value in the kernel argument block
struct LinkReq {
    int K, has_off;
    int link[kLinkMaxK];
    float off[3 * kLinkMaxK];
};

MI_D int link_state_width(const DevModel& m) { return kLinkRootW + 2 * m.D; }   // odd: no bank conflicts across envs

// phase 0: se[e][f] <- state of env e0 + e; f: root pos 3, quat 4, vel 6, q D, qd D
MI_D void link_load_state(const DevModel& m, const DevState& st, int e0, int ne, int E, float* se) {
    const int SW = link_state_width(m), D = m.D;
    for (int t = threadIdx.x; t < E * SW; t += kLinkThreads) {
        int e, f;
        if (st.es == 1) { f = t / E; e = t - f * E; } else { e = t / SW; f = t - e * SW; }
        if (e >= ne) continue;
        const float* base;
        int k;
        if (f < 3) { base = st.root_pos; k = f; }
        else if (f < 7) { base = st.root_quat; k = f - 3; }
        else if (f < kLinkRootW) { base = st.root_vel; k = f - 7; }
        else if (f < kLinkRootW + D) { base = st.q; k = f - kLinkRootW; }
        else { base = st.qd; k = f - kLinkRootW - D; }
        se[e * SW + f] = base[sx(st, k, e0 + e)];
    }
}

MI_D void quat_mul(const float* a, const float* b, float* o) {
    const float w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    const float x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    const float y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    const float z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
    o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}

// ancestors of `link` (itself included, the root excluded) as a bit set
MI_D uint64_t link_chain(const DevModel& m, int link) {
    uint64_t mask = 0;
    for (int l = link; l > 0; l = m.parent[l]) mask |= 1ull << l;
    return mask;
}

// World frame of a link, origin relative to the root origin; a = world joint axis of the link.
// kFull: also the orientation quaternion, the angular velocity w and the origin velocity v.
struct LinkFrame { float R[9], o[3], a[3], q[4], w[3], v[3]; };

template <bool kFull>
MI_D void link_walk(const DevModel& m, const float* se, int link, LinkFrame& f) {
    const int D = m.D;
    m3_from_quat(se + 3, f.R);
#pragma unroll
    for (int c = 0; c < 3; ++c) { f.o[c] = 0.0f; f.a[c] = 0.0f; }
    if constexpr (kFull) {
#pragma unroll
        for (int c = 0; c < 4; ++c) f.q[c] = se[3 + c];
        // a fixed base has no root velocity (its generalized velocity is qd alone)
#pragma unroll
        for (int c = 0; c < 3; ++c) { f.v[c] = m.root_free ? se[7 + c] : 0.0f; f.w[c] = m.root_free ? se[10 + c] : 0.0f; }
    }
    uint64_t mask = link_chain(m, link);
    while (mask) {
        const int l = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        // f holds the parent's frame
        float Rq[9], Rj[9], d[3];
        const float* ql = m.quat + 4 * l;
        const float* al = m.axis + 3 * l;
        m3_from_quat(ql, Rq);
        m3_mul(f.R, Rq, Rj);
        m3_vec(Rj, al, f.a);
        m3_vec(f.R, m.pos + 3 * l, d);
        const float qj = se[kLinkRootW + l - 1], qdj = se[kLinkRootW + D + l - 1];
        const bool hinge = m.jtype[l] == MI_JOINT_HINGE;
        if (!hinge) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += f.a[c] * qj;
        }
        if constexpr (kFull) {
            float wd[3], t[4];
            cross3(f.w, d, wd);       // the origin rides on the parent: v_l = v_P + w_P x (o_l - o_P) [+ a qd]
            quat_mul(f.q, ql, t);
            if (hinge) {
                float s, c;
                sincosf(0.5f * qj, &s, &c);
                const float qa[4] = {c, al[0] * s, al[1] * s, al[2] * s};
                quat_mul(t, qa, f.q);
#pragma unroll
                for (int k = 0; k < 3; ++k) { f.v[k] += wd[k]; f.w[k] += f.a[k] * qdj; }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) f.q[k] = t[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) f.v[k] += wd[k] + f.a[k] * qdj;
            }
        }
        if (hinge) {
            float Ra[9];
            m3_axis_angle(al, qj, Ra);
            m3_mul(Rj, Ra, f.R);
        } else {
#pragma unroll
            for (int c = 0; c < 9; ++c) f.R[c] = Rj[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) f.o[c] += d[c];
    }
}

// phase 2 of the link state: n floats of the workgroup's contiguous output block, LDS -> global
MI_D void link_block_store(float* __restrict__ dst, const float* src, int n) {
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {     // every caller with 16-B aligned buffers
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += kLinkThreads)
            reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += kLinkThreads) dst[i] = src[i];
}

// LDS floats of k_link_state: state, then pos / quat / vel rows in output order
static inline size_t link_state_lds(int D, int K) {
    const int E = kLinkStateEnvs;
    return sizeof(float) * (size_t)(((E * (kLinkRootW + 2 * D) + 3) & ~3) + E * K * 13);
}

__global__ __launch_bounds__(kLinkThreads) void k_link_state(DevModel m, DevState st, LinkReq rq,
                                                            float* __restrict__ pos, float* __restrict__ quat,
                                                            float* __restrict__ vel) {
    extern __shared__ float4 link_smem[];
    constexpr int E = kLinkStateEnvs;
    const int K = rq.K, SW = link_state_width(m);
    const int e0 = blockIdx.x * E, ne = min(E, st.N - e0);
    float* se = reinterpret_cast<float*>(link_smem);
    float* sp = se + ((E * SW + 3) & ~3);
    float* sq = sp + E * K * 3;
    float* sv = sq + E * K * 4;
    link_load_state(m, st, e0, ne, E, se);
    __syncthreads();
    for (int t = threadIdx.x; t < E * K; t += kLinkThreads) {
        const int k = t / E, e = t - k * E;
        if (e >= ne) continue;
        const float* s = se + e * SW;
        const int link = rq.link[k];
        LinkFrame f;
        link_walk<true>(m, s, link, f);
        float r[3] = {0.0f, 0.0f, 0.0f};
        if (rq.has_off) {
            const float off[3] = {rq.off[3 * k], rq.off[3 * k + 1], rq.off[3 * k + 2]};
            float wr[3];
            m3_vec(f.R, off, r);
            cross3(f.w, r, wr);
#pragma unroll
            for (int c = 0; c < 3; ++c) f.v[c] += wr[c];
        }
        const bool is_root = link == 0 && !rq.has_off;    // the root state itself, bit for bit
        const int row = e * K + k;
#pragma unroll
        for (int c = 0; c < 3; ++c) sp[row * 3 + c] = is_root ? s[c] : s[c] + (f.o[c] + r[c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) sq[row * 4 + c] = f.q[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) { sv[row * 6 + c] = f.v[c]; sv[row * 6 + 3 + c] = f.w[c]; }
    }
    __syncthreads();
    const size_t r0 = (size_t)e0 * K;
    if (pos) link_block_store(pos + r0 * 3, sp, ne * K * 3);
    if (quat) link_block_store(quat + r0 * 4, sq, ne * K * 4);
    if (vel) link_block_store(vel + r0 * 6, sv, ne * K * 6);
}

// LDS of k_link_jacobian: frame column masks (8-B aligned first), state, column table
// [E][6][nv] (axis 3, origin 3; component-major so that consecutive columns are consecutive
// words), frame origins [E][K][3], column kinds [nv]
static inline size_t link_jac_lds(int D, int nv, int K) {
    const int E = kLinkJacEnvs;
    return sizeof(uint64_t) * (size_t)K + sizeof(float) * (size_t)(E * (kLinkRootW + 2 * D) + E * 6 * nv + E * K * 3 + nv);
}

// element (row r of frame k, column c) of env e's Jacobian from the staged tables
MI_D float link_jac_elem(const float* T, const float* p, const int* kind, uint64_t cols, int nv, int r, int c) {
    if (!((cols >> c) & 1)) return 0.0f;             // not an ancestor DOF
    if (!kind[c]) return r < 3 ? T[r * nv + c] : 0.0f;   // translation: (a, 0)
    if (r >= 3) return T[(r - 3) * nv + c];          // rotation: (a x (p - o), a)
    const int r1 = r == 2 ? 0 : r + 1, r2 = r == 0 ? 2 : r - 1;
    const float d1 = p[r1] - T[(3 + r1) * nv + c], d2 = p[r2] - T[(3 + r2) * nv + c];
    return T[r1 * nv + c] * d2 - T[r2 * nv + c] * d1;
}

__global__ __launch_bounds__(kLinkThreads) void k_link_jacobian(DevModel m, DevState st, LinkReq rq,
                                                               float* __restrict__ jac) {
    extern __shared__ float4 link_smem[];
    constexpr int E = kLinkJacEnvs;
    const int K = rq.K, L = m.L, nv = m.nv, nr = m.nr, SW = link_state_width(m);
    const int e0 = blockIdx.x * E, ne = min(E, st.N - e0);
    uint64_t* cm = reinterpret_cast<uint64_t*>(link_smem);
    float* se = reinterpret_cast<float*>(cm + K);
    float* tab = se + E * SW;
    float* sp = tab + E * 6 * nv;
    int* kind = reinterpret_cast<int*>(sp + E * K * 3);
    link_load_state(m, st, e0, ne, E, se);
    for (int k = threadIdx.x; k < K; k += kLinkThreads)    // columns: the root's nr, then link l at nr + l - 1
        cm[k] = ((1ull << nr) - 1) | ((link_chain(m, rq.link[k]) >> 1) << nr);
    for (int c = threadIdx.x; c < nv; c += kLinkThreads)
        kind[c] = c < nr ? (c >= 3) : (m.jtype[c - nr + 1] == MI_JOINT_HINGE);
    __syncthreads();
    for (int t = threadIdx.x; t < E * (L + K); t += kLinkThreads) {
        const int j = t / E, e = t - j * E;
        if (e >= ne) continue;
        const float* s = se + e * SW;
        float* T = tab + e * 6 * nv;
        LinkFrame f;
        if (j >= L) {               // frame j - L: its origin
            const int k = j - L;
            link_walk<false>(m, s, rq.link[k], f);
            float r[3] = {0.0f, 0.0f, 0.0f};
            if (rq.has_off) {
                const float off[3] = {rq.off[3 * k], rq.off[3 * k + 1], rq.off[3 * k + 2]};
                m3_vec(f.R, off, r);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) sp[(e * K + k) * 3 + c] = f.o[c] + r[c];
        } else if (j > 0) {         // link j: the column of its DOF
            link_walk<false>(m, s, j, f);
            // a hinge turns about its own origin; a slide's column has no origin term
            const int c = nr + j - 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) { T[k * nv + c] = f.a[k]; T[(3 + k) * nv + c] = f.o[k]; }
        } else {                    // the root's columns: unit translations, unit rotations about its origin
            for (int c = 0; c < nr; ++c)
#pragma unroll
                for (int k = 0; k < 3; ++k) { T[k * nv + c] = (c % 3 == k) ? 1.0f : 0.0f; T[(3 + k) * nv + c] = 0.0f; }
        }
    }
    __syncthreads();
    const int per = K * 6 * nv, n = ne * per;
    float* __restrict__ dst = jac + (size_t)e0 * per;
    // output element i of the block -> (env, frame, row, column)
    struct Pos { int e, k, r, c; };
    auto locate = [&](int i) {
        Pos p;
        p.e = i / per;
        const int x = i - p.e * per;
        p.k = x / (6 * nv);
        const int y = x - p.k * 6 * nv;
        p.r = y / nv;
        p.c = y - p.r * nv;
        return p;
    };
    auto elem = [&](const Pos& p) {
        return link_jac_elem(tab + p.e * 6 * nv, sp + (p.e * K + p.k) * 3, kind, cm[p.k], nv, p.r, p.c);
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
                if (++p.c == nv) { p.c = 0; if (++p.r == 6) { p.r = 0; if (++p.k == K) { p.k = 0; ++p.e; } } }
            }
            reinterpret_cast<float4*>(dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += kLinkThreads) dst[i] = elem(locate(i));
}

}  // namespace mi
