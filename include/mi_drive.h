/* mi_drive.h — implicit PD joint drives: the two combinations every device site and every view
 * uses, shared as source by the HIP kernels and by host tests (like mi_dr_phys.h: plain C, FP
 * contraction off, one fixed evaluation order).
 *
 * ArticulationView.set_gains / set_joint_position_targets / set_joint_velocity_targets of the
 * reference (tasks/anymal.py:187, franka_cabinet.py:254,285, ball_balance.py:188) ask the solver
 * for the joint torque tau_d = kp (q* - q+) + kd (qd* - u+), evaluated at the END of the substep.
 * With q+ = q + dt u+ the substep's equation
 *     (M + arm + dt B) (u+ - u) / dt = S^T tau + Q - c - g - B u
 * keeps its form, with the damping and the effort of every joint DOF replaced by
 *     B_E = (B + kd) + dt kp                       mi_drive_damping
 *     tau + F_d = (tau + kp (q* - q)) + kd qd*     mi_drive_effort   (q of THIS substep)
 * so a sim whose damping record holds B_E and whose efforts hold tau + F_d, both formed by these
 * two functions, steps to the same bits as a sim with the drive set. (clang honours the pragma
 * below; build with -ffp-contract=off under another compiler.)
 */
#ifndef MI_DRIVE_H
#define MI_DRIVE_H

#if defined(__HIPCC__)
#define MI_DRIVE_FN static inline __host__ __device__
#else
#define MI_DRIVE_FN static inline
#endif

#if defined(__clang__)
#define MI_DRIVE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MI_DRIVE_NO_CONTRACT
#endif

/* lines of an env's drive record, D floats each (include/mi_sim.h mi_set_drive_gains) */
#define MI_DRIVE_KP 0
#define MI_DRIVE_KD 1
#define MI_DRIVE_QT 2
#define MI_DRIVE_QDT 3
#define MI_DRIVE_LINES 4

/* effective damping of a driven joint DOF: (damp + kd) + dt*kp */
MI_DRIVE_FN float mi_drive_damping(float damp, float kp, float kd, float dt) {
    MI_DRIVE_NO_CONTRACT
    const float a = damp + kd;
    const float b = dt * kp;
    return a + b;
}

/* effective effort of a driven joint DOF: (eff + kp*(qt - q)) + kd*qdt */
MI_DRIVE_FN float mi_drive_effort(float eff, float kp, float kd, float q, float qt, float qdt) {
    MI_DRIVE_NO_CONTRACT
    const float e = qt - q;
    const float s = kp * e;
    const float a = eff + s;
    const float d = kd * qdt;
    return a + d;
}

#endif /* MI_DRIVE_H */
