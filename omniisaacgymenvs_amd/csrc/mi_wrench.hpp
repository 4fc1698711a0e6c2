// mi_wrench.hpp — body wrenches: forces and torques on frames rigidly attached to links, turned
// into the generalized force Q = sum_k J_k^T (f_k, tau_k) that the EnvP step kernels add to their
// bias (include/mi_sim.h mi_apply_link_wrenches), gfx950.
//
// The frames are mi_link.hpp's (LinkReq, link_walk) and J_k is mi_get_link_jacobian's frame
// Jacobian, formed on the chip from the same column table (world axis + origin per DOF); nothing
// is read back from a Jacobian in memory. A workgroup serves kWrenchEnvs rows of the call (a row
// names its env through idx, so the rows' envs need not be neighbours):
//   phase 0  the rows' env ids, then their state -> LDS in the state layout's contiguous direction;
//   phase 1  one lane per (row, link): the DOF's world axis and origin; one lane per (row, frame):
//            the frame origin and the wrench in world axes (is_global = 0: rotated by the link's
//            orientation here);
//   phase 2  one lane per (row, DOF): the frames in call order k = 0..K-1, each adding its column's
//            product if the DOF is on its ancestor chain — a fixed order and no atomics, so the
//            same bits on every run; a DOF that moves none of the frames gets exactly 0. The store
//            is Q[env][dof], dof fastest: the line P3 of the step reads with lane = DOF, next to
//            the effort line, as it reads the record's damping / armature.
#pragma once
#include "mi_link.hpp"

namespace mi {

constexpr int kWrenchEnvs = 8;           // rows per workgroup

struct WrenchArgs {
    int n, is_global, accumulate;
    const float* force;                  // [n,K,3] | nullptr
    const float* torque;                 // [n,K,3] | nullptr
    const int64_t* idx;                  // [n] | nullptr: rows 0..n-1
    float* Q;                            // [N,nv]
};

// LDS of k_apply_wrench: frame column masks (8-B aligned first), state [E][SW], column table
// [E][6][nv], frame origin + force + torque [E][K][9], column kinds [nv], env ids [E]
static inline size_t wrench_lds(int D, int nv, int K) {
    const int E = kWrenchEnvs;
    return sizeof(uint64_t) * (size_t)K + sizeof(float) * (size_t)(E * (kLinkRootW + 2 * D) + E * 6 * nv + E * K * 9 + nv + E);
}

__global__ __launch_bounds__(kLinkThreads) void k_apply_wrench(DevModel m, DevState st, LinkReq rq, WrenchArgs a) {
    extern __shared__ float4 link_smem[];
    constexpr int E = kWrenchEnvs;
    const int K = rq.K, L = m.L, nv = m.nv, nr = m.nr, SW = link_state_width(m);
    const int r0 = blockIdx.x * E;
    uint64_t* cm = reinterpret_cast<uint64_t*>(link_smem);
    float* se = reinterpret_cast<float*>(cm + K);
    float* tab = se + E * SW;
    float* sw = tab + E * 6 * nv;
    int* kind = reinterpret_cast<int*>(sw + E * K * 9);
    int* senv = kind + nv;
    if (threadIdx.x < E) {
        const int r = r0 + (int)threadIdx.x;
        int64_t i = -1;
        if (r < a.n) i = a.idx ? a.idx[r] : r;
        senv[threadIdx.x] = (i >= 0 && i < st.N) ? (int)i : -1;     // out-of-range ids are ignored
    }
    for (int k = threadIdx.x; k < K; k += kLinkThreads)    // columns: the root's nr, then link l at nr + l - 1
        cm[k] = ((1ull << nr) - 1) | ((link_chain(m, rq.link[k]) >> 1) << nr);
    for (int c = threadIdx.x; c < nv; c += kLinkThreads)
        kind[c] = c < nr ? (c >= 3) : (m.jtype[c - nr + 1] == MI_JOINT_HINGE);
    __syncthreads();
    // phase 0: link_load_state's fields for the rows' envs
    {
        const int D = m.D;
        for (int t = threadIdx.x; t < E * SW; t += kLinkThreads) {
            int e, f;
            if (st.es == 1) { f = t / E; e = t - f * E; } else { e = t / SW; f = t - e * SW; }
            const int i = senv[e];
            if (i < 0) continue;
            const float* base;
            int k;
            if (f < 3) { base = st.root_pos; k = f; }
            else if (f < 7) { base = st.root_quat; k = f - 3; }
            else if (f < kLinkRootW) { base = st.root_vel; k = f - 7; }
            else if (f < kLinkRootW + D) { base = st.q; k = f - kLinkRootW; }
            else { base = st.qd; k = f - kLinkRootW - D; }
            se[e * SW + f] = base[sx(st, k, i)];
        }
    }
    __syncthreads();
    // phase 1
    for (int t = threadIdx.x; t < E * (L - 1 + K); t += kLinkThreads) {
        const int j = t / E + 1, e = t - (j - 1) * E;
        if (senv[e] < 0) continue;
        const float* s = se + e * SW;
        LinkFrame f;
        if (j >= L) {               // frame j - L: origin and wrench, world axes
            const int k = j - L;
            link_walk<false>(m, s, rq.link[k], f);
            float r[3] = {0.0f, 0.0f, 0.0f};
            if (rq.has_off) {
                const float off[3] = {rq.off[3 * k], rq.off[3 * k + 1], rq.off[3 * k + 2]};
                m3_vec(f.R, off, r);
            }
            const size_t row = ((size_t)(r0 + e) * K + k) * 3;
            float fv[3] = {0.0f, 0.0f, 0.0f}, tv[3] = {0.0f, 0.0f, 0.0f};
            if (a.force) { fv[0] = a.force[row]; fv[1] = a.force[row + 1]; fv[2] = a.force[row + 2]; }
            if (a.torque) { tv[0] = a.torque[row]; tv[1] = a.torque[row + 1]; tv[2] = a.torque[row + 2]; }
            if (!a.is_global) {     // given in the link's axes at call time
                m3_vec(f.R, fv, fv);
                m3_vec(f.R, tv, tv);
            }
            float* w = sw + (e * K + k) * 9;
#pragma unroll
            for (int c = 0; c < 3; ++c) { w[c] = f.o[c] + r[c]; w[3 + c] = fv[c]; w[6 + c] = tv[c]; }
        } else {                    // link j: the column of its DOF (a hinge turns about its own origin)
            link_walk<false>(m, s, j, f);
            float* T = tab + e * 6 * nv;
            const int c = nr + j - 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) { T[k * nv + c] = f.a[k]; T[(3 + k) * nv + c] = f.o[k]; }
        }
    }
    __syncthreads();
    // phase 2: Q[c] = sum_k column c of J_k . (f_k, tau_k)
    for (int t = threadIdx.x; t < E * nv; t += kLinkThreads) {
        const int e = t / nv, c = t - e * nv;
        const int i = senv[e];
        if (i < 0) continue;
        const float* T = tab + e * 6 * nv;
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) {
            if (!((cm[k] >> c) & 1)) continue;      // not an ancestor DOF of frame k
            const float* w = sw + (e * K + k) * 9;
            const float* fv = w + 3;
            const float* tv = w + 6;
            float term;
            if (c < nr) {           // the root: unit translations, unit rotations about its origin
                if (c < 3) {
                    term = fv[c];
                } else {
                    const int x = c - 3, x1 = x == 2 ? 0 : x + 1, x2 = x == 0 ? 2 : x - 1;
                    term = (w[x1] * fv[x2] - w[x2] * fv[x1]) + tv[x];
                }
            } else {
                const float ax[3] = {T[c], T[nv + c], T[2 * nv + c]};
                if (kind[c]) {      // rotation: (a x (p - o), a)
                    const float d[3] = {w[0] - T[3 * nv + c], w[1] - T[4 * nv + c], w[2] - T[5 * nv + c]};
                    float ad[3];
                    cross3(ax, d, ad);
                    term = dot3(ad, fv) + dot3(ax, tv);
                } else {            // translation: (a, 0)
                    term = dot3(ax, fv);
                }
            }
            acc += term;
        }
        float* q = a.Q + (size_t)i * nv + c;
        *q = a.accumulate ? *q + acc : acc;
    }
}

// rows of Q <- 0 (idx nullptr: rows 0..n-1; out-of-range ids ignored)
__global__ __launch_bounds__(256) void k_wrench_clear(float* __restrict__ Q, int nv, const int64_t* __restrict__ idx,
                                                      int n, int N) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n * nv) return;
    const int r = (int)(t / nv), c = (int)(t - (int64_t)r * nv);
    const int64_t i = idx ? idx[r] : r;
    if (i < 0 || i >= N) return;
    Q[(size_t)i * nv + c] = 0.0f;
}

}  // namespace mi
