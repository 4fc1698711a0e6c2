// mi_phase.hpp — what the one-env-per-wave kernel (mi_wave.hpp, wave_artic_substep) and the
// two-envs-per-wave kernel (mi_pair.hpp, pair_artic_substep) run as ONE function: the P3 phase of
// the substep (bias and CRBA rows) and the pre-physics task layer. A change to either is made
// here, once, and reaches both kernels.
//
// A shared function is templated on the lane group G that owns one env — Grp64: the whole wave,
// Grp32: this lane's 32-lane half — and, where the topology matters, on TP. The group is a
// compile-time tag and nothing else; what really differs between the two kernels is an
// `if constexpr` on G or TP inside the one function. Two phases use it so far, and only for its
// width; it is meant to grow a member (ballot, popcount, lane-0 broadcast) with each phase that
// can join them. Statement order follows the pair kernel, the
// measured default, whose instruction streams a shared function must leave as they are
// (profiles/phase_share/isa_identity.txt; DESIGN.md section 2 lists the phases that are still
// written out in both kernels and why).
//
// Included by mi_wave.hpp after its helpers (MC, wave_lane, ...): not a header to include on
// its own.
#pragma once

namespace mi {

// ---- lane groups -------------------------------------------------------------------------
MI_D int pair_l64() { return (int)(threadIdx.x & 63u); }
// the whole wave: one env
struct Grp64 {
    static constexpr int kW = 64;
    static MI_D int lane() { return wave_lane(); }
};
// this lane's half of the wave: one of two envs
struct Grp32 {
    static constexpr int kW = 32;
    static MI_D int lane() { return pair_l64() & 31; }
};

#ifndef MI_PAIR_SDOF_PD
#define MI_PAIR_SDOF_PD 6   // DOF-loop prefetch depth (sdof_loop): 2 -> 0.1609 ms, 4 -> 0.1592 (A/B, round 3); 6: 0.1356 -> 0.1349 (round 4)
#endif
// Per-DOF loop over the motion subspaces S_c (6 floats per DOF in LDS, uniform per half) and,
// with R, the rhs entries R[c]: fn(c, S_c, R[c]) with the loads of DOF c + SP issued before DOF c's
// arithmetic, into a ring of SP + 1 buffers indexed at compile time. Each DOF's arithmetic is a
// handful of VALU ops, so with the loads in line every DOF exposed a full LDS round trip.
// S0: the first DOF whose S_c is read (the callers that know S_c of the free root's six DOFs
// at compile time pass TP::nr; fn then gets an unread sv for c < S0).
template <class TP, int SP, bool WITH_R, int S0 = 0, class F>
MI_D void sdof_loop(const float* Ss, const float* R, F&& fn) {
    constexpr int NB = SP + 1;
    float sb[NB][6], rb[NB];
    auto load = [&](auto C) {
        constexpr int c = C;
        if constexpr (c >= S0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) sb[c % NB][q] = Ss[6 * c + q];
        }
        if constexpr (WITH_R) rb[c % NB] = R[c];
    };
    sfor<0, (SP < TP::nv ? SP : TP::nv)>([&](auto C) { load(C); });
    sfor<0, TP::nv>([&](auto C) {
        constexpr int c = C;
        if constexpr (c + SP < TP::nv) load(std::integral_constant<int, c + SP>{});
        fn(C, sb[c % NB], WITH_R ? rb[c % NB] : 0.0f);
    });
}
// S_c . f for DOF c: the free root's six DOFs have unit subspaces (linear x, y, z then angular
// x, y, z: the substeps' state load), so their dot product is one component of f (what dot6 with a
// unit vector returns, up to the sign of a zero); the joint DOFs' from S_c in LDS
template <class TP, int c>
MI_D float sdot(const float (&sv)[6], const float (&f)[6]) {
    if constexpr (TP::nr == 6 && c < 6) return f[c < 3 ? 3 + c : c - 3];
    else return dot6(sv, f);
}
constexpr int sdof_first_loaded(int nr) { return nr == 6 ? 6 : 0; }

// ---- P3: bias + CRBA (lane k = dof k)
// ep (TP::kEnvP only): the env's record of the per-env parameter table, damping and armature
// read where the state's effort line is (lane = DOF, coalesced)
// wq (TP::kEnvP only, may be null): the body wrenches' generalized forces [N][nv]
// (mi_wrench.hpp), env i's line read the same way and added to every DOF's bias, the root's
// included; null (no wrench was ever applied): no add at all
// drv (TP::kEnvP only, may be null): the joint drives' records [N][4][D] (include/mi_drive.h: lines
// kp, kd, q*, qd*, lane = DOF like the effort line) and qs, the substep's own joint positions in
// LDS: damping and effort of a joint DOF become mi_drive_damping / mi_drive_effort. The four values
// are combined at once and dead before the CRBA rows; null (no drive call yet): no read at all
template <class G, class TP>
MI_D void phase_p3_bias_crba(int lane, int i, int D, int nv, int nr, float dt, const float* us, float* rhs,
                             float* Mx, const float* Ss, const MC& mc, const WaveTabs& t,
                             const DevState& st, const float* aux, const float* ep,
                             const float* wq = nullptr, const float* drv = nullptr,
                             const float* qs = nullptr) {
    if (lane < nv) {
        const int k = lane, l = k < nr ? 0 : k - nr + 1;
        float s[6], I[10], f[6], F[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) s[q] = Ss[6 * k + q];
        {
            const float4* rec = reinterpret_cast<const float4*>(aux) + 4 * l;
            const float4 a0 = rec[0], a1 = rec[1], a2 = rec[2], a3 = rec[3];
            I[0] = a0.x; I[1] = a0.y; I[2] = a0.z; I[3] = a0.w;
            I[4] = a1.x; I[5] = a1.y; I[6] = a1.z; I[7] = a1.w;
            I[8] = a2.x; I[9] = a2.y; F[0] = a2.z; F[1] = a2.w;
            F[2] = a3.x; F[3] = a3.y; F[4] = a3.z; F[5] = a3.w;
        }
        inertia_mul(I, s, f);
        float diag = dot6(s, f);
        float r = -dot6(s, F);
        if (k >= nr) {
            float damp, arm;
            if constexpr (TP::kEnvP) {
                damp = ep[kEnvpDamping + k - nr];
                arm = ep[kEnvpDamping + D + k - nr];
            } else {
                damp = mc.lf(MC_DAMP, l);
                arm = mc.lf(MC_ARM, l);
            }
            float eff = st.eff[sx(st, k - nr, i)];
            if constexpr (TP::kEnvP) {
                if (drv) {
                    const float* dl = drv + (size_t)i * MI_DRIVE_LINES * D + (k - nr);
                    const float kp = dl[MI_DRIVE_KP * D], kd = dl[MI_DRIVE_KD * D];
                    eff = mi_drive_effort(eff, kp, kd, qs[k - nr], dl[MI_DRIVE_QT * D], dl[MI_DRIVE_QDT * D]);
                    damp = mi_drive_damping(damp, kp, kd, dt);
                }
            }
            diag += arm + dt * damp;
            r += eff - damp * us[k];
        }
        if constexpr (TP::kEnvP) {
            if (wq) r += wq[(size_t)i * nv + k];
        }
        rhs[k] = r;
        if constexpr (TP::kCT) {
            // row k of M~: S_j . f for every j, branch-free (uniform j: the S_j reads are LDS
            // broadcasts). Only the ancestors of k are ever read (ct_load_columns masks the rest),
            // so the other entries are written but dead; a lane-varying ancestor branch per j cost
            // more than the 6 FMAs it skipped.
            if constexpr (G::kW == 32) {
                // the pair kernel: S_j prefetched ahead of its dot product, the free root's by component
                sdof_loop<TP, MI_PAIR_SDOF_PD, false, sdof_first_loaded(TP::nr)>(Ss, nullptr, [&](auto J, const float (&sj)[6], float) {
                    constexpr int j = J;
                    Mx[k * nv + j] = sdot<TP, j>(sj, f);
                });
            } else {
                sfor<0, TP::nv>([&](auto J) {
                    constexpr int j = J;
                    float sj[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) sj[q] = Ss[6 * j + q];
                    Mx[k * nv + j] = dot6(sj, f);
                });
            }
        } else {
            // runtime tables: only the ancestors of k, from the runtime list
            for (int a = t.anc_start[k]; a < t.anc_start[k + 1]; ++a) {
                const int j = t.anc_list[a];
                float sj[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) sj[q] = Ss[6 * j + q];
                Mx[k * nv + j] = dot6(sj, f);
            }
        }
        // The diagonal goes last on every path. (Stored first on the runtime path, as the wave
        // kernel's own text had it, the TGS runtime kernels took one VGPR more through this
        // function; last, they are back at the parent's count. Other addresses: same result.)
        Mx[k * nv + k] = diag;
    }
}

// ---------------------------------------------------------------------------------------
// Group-cooperative task layer of the fused env step (locomotion tasks). Same formulas, same
// evaluation order and the same Philox streams as the one-lane versions in mi_task.hpp; the
// work is spread over the group's lanes (lane j = DOF j) and reads the LDS-resident physics state.
// ---------------------------------------------------------------------------------------

// VecEnvRLGames.step's clamp + action noise DR (vec_env_rlgames.py:57-60), then
// pre_physics_step (locomotion.py:103-145): mask-driven reset_idx, efforts. Returns lane j's
// action as pre_physics_step received it (task.actions[i, j]; 0 on lanes >= A).
template <class G>
MI_D float task_pre(const DevModel& m, const DevState& st, const DevTask& tp, int i,
                    const float* actions, int64_t* reset_buf, int64_t* progress_buf,
                    float* potentials, float* prev_potentials, float* actions_out) {
#pragma clang fp contract(off)
    const int lane = G::lane(), N = st.N, D = m.D, A = tp.A;
    const bool flagged = reset_buf[i] != 0;      // group-uniform
    mi_dr_env dre{};
    if (tp.dr_act) dre = dr_begin(st, tp, 1, i, flagged);
    if (flagged) {
        const uint64_t gid = (uint64_t)(st.off + i);
        const uint32_t cnt = st.reset_count[i];
        const float pn = tp.dof_pos_noise, vn = tp.dof_vel_noise;
        const float pw = (float)((double)pn - (double)(-pn));
        const float vw = (float)((double)vn - (double)(-vn));
        if (lane < D) {
            const int j = lane;
            float u[4];
            uniform4(st.seed, gid, cnt, (uint32_t)(j >> 2), 0, u);
            float v = tp.init_dof[j] + (pw * u[j & 3] + (-pn));
            const float lo = m.lower[j + 1], hi = m.upper[j + 1];
            if (lo < hi) { v = v < hi ? v : hi; v = v > lo ? v : lo; }
            st.q[sx(st, j, i)] = v;
            const int s = D + j;
            uniform4(st.seed, gid, cnt, (uint32_t)(s >> 2), 0, u);
            st.qd[sx(st, j, i)] = vw * u[s & 3] + (-vn);
        }
        if (lane < 3) st.root_pos[sx(st, lane, i)] = st.origins[(size_t)lane * N + i] + tp.init_root_pos[lane];
        if (lane < 4) st.root_quat[sx(st, lane, i)] = tp.init_root_quat[lane];
        if (lane < 6) st.root_vel[sx(st, lane, i)] = 0.0f;
        if (lane == 0) {
            float rp[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) rp[k] = st.origins[(size_t)k * N + i] + tp.init_root_pos[k];
            float tx = tp.target[0] - rp[0], ty = tp.target[1] - rp[1];
            float pot = -sqrtf(tx * tx + ty * ty + 0.0f * 0.0f) / tp.task_dt;
            prev_potentials[i] = pot;
            potentials[i] = pot;
            st.reset_count[i] = cnt + 1;
            reset_buf[i] = 0;
            progress_buf[i] = 0;
        }
    }
    float a = 0.0f;
    if (lane < A) {
        const int j = lane;
        a = clampf(actions[(size_t)A * i + j], -tp.clip_actions, tp.clip_actions);
        if (tp.dr_act) a = dr_col(st, tp, 1, dre, i, j, a);
        if (actions_out) actions_out[(size_t)A * i + j] = a;
        st.eff[sx(st, j, i)] = a * tp.gears[j] * tp.power_scale;
    }
    if (tp.dr_act && lane == 0) dr_store(st, 1, i, dre);
    return a;
}

}  // namespace mi
