/*
 * mi_sim.h — C ABI of libmi_sim.so, the MI355X-native replacement for the closed
 * PhysX GPU articulation pipeline + the task-layer TorchScript kernels that sit behind
 * OmniIsaacGymEnvs' VecEnvBase / RLTask for the Humanoid, Ant and Cartpole tasks.
 *
 * Every entry point replaces one call site of the reference (file:line under
 * tzmhuang/OmniIsaacGymEnvs v1.1.0, omniisaacgymenvs/...). The reference binds these from
 * Python; the binding a maintainer would add is the ctypes stub in INTEGRATION.md
 * (our own binding: omniisaacgymenvs_amd/native.py).
 *
 * Conventions
 *  - Return 0 (MI_OK) on success, a negative MI_E_* code on failure; the message is in
 *    mi_last_error() (thread-local). No C++ exception crosses this ABI.
 *  - Ownership: an mi_sim owns ALL physics state (struct-of-arrays in device memory).
 *    Every other buffer is caller-owned (PyTorch tensors); the library never frees or
 *    retains them past the call.
 *  - Pointers: tensor arguments are DEVICE pointers on the sim's device, row-major
 *    [N, ...] exactly like the reference's torch buffers. `model`, `params`, `env_origins`,
 *    `dof_limits` and task parameter structs are HOST pointers.
 *  - Dtypes are those of the reference buffers: f32 state/obs/reward, int64 reset_buf /
 *    progress_buf / reset indices, int32 effort indices.
 *  - Streams: `stream` is a hipStream_t passed as void* (torch's current stream); every
 *    call is stream-ordered and none blocks the host except create/destroy/info.
 *  - A handle is not re-entrant: one host thread at a time.
 */
#ifndef MI_SIM_H
#define MI_SIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ABI_VERSION 4

enum {
    MI_OK = 0,
    MI_E_NULL = -1,    /* null pointer where a buffer is required            */
    MI_E_SHAPE = -2,   /* size / count out of range                          */
    MI_E_HIP = -3,     /* HIP runtime error                                  */
    MI_E_MODEL = -4,   /* model description rejected                         */
    MI_E_ARG = -5,     /* bad enum / parameter value                         */
    MI_E_NODEV = -6,   /* no GPU / bad device id                             */
    MI_E_STATE = -7    /* call out of order (e.g. task not configured)       */
};

/* Task kinds: which fused task kernels run on top of the physics. */
enum { MI_TASK_CARTPOLE = 0, MI_TASK_ANT = 1, MI_TASK_HUMANOID = 2 };

/* Dynamics kinds. */
enum {
    MI_DYN_ARTICULATION = 0, /* floating/fixed-base tree, CRBA + tree-LTDL + PGS contacts  */
    MI_DYN_CARTPOLE = 1      /* analytic 2-DOF cart-pole (prismatic cart + hinge pole)      */
};

enum { MI_JOINT_HINGE = 0, MI_JOINT_SLIDE = 1 };
enum { MI_GEOM_SPHERE = 0, MI_GEOM_CAPSULE = 1 };

/*
 * Compiled model description (host arrays). Produced from an MJCF-subset file by
 * omniisaacgymenvs_amd/robots/model.py; replaces the USD articulation the reference
 * pulls from Nucleus (robots/articulations/humanoid.py:57, ant.py:57, cartpole.py:56).
 *
 * Links: link 0 is the root. For a floating root (root_free=1) its 6 DOFs are the root
 * linear (x,y,z, world) and angular (x,y,z, world) velocities; they are NOT part of the
 * joint DOF vector the task sees. Links 1..L-1 each carry exactly ONE joint DOF
 * (multi-DOF MJCF bodies are chains of massless 1-DOF links) in BFS order, and
 * parent[l] < l. Joint DOF j belongs to link j+1.
 */
typedef struct mi_model_desc {
    int32_t dyn_kind;        /* MI_DYN_*                                             */
    int32_t root_free;       /* 1: floating base (free joint), 0: fixed base         */
    int32_t num_links;       /* L, incl. root link 0                                 */
    int32_t num_geoms;       /* G contact geoms                                      */
    int32_t num_sensors;     /* S force sensors                                      */
    int32_t num_pairs;       /* self-collision geom pairs (may be 0)                 */
    const int32_t* parent;   /* [L]   parent link (-1 for root)                      */
    const int32_t* jtype;    /* [L]   MI_JOINT_* (ignored for link 0)                */
    const float* axis;       /* [L,3] joint axis in the link's joint frame (unit)    */
    const float* pos;        /* [L,3] joint-frame origin in the parent link frame    */
    const float* quat;       /* [L,4] joint-frame rotation wrt parent frame (wxyz)   */
    const float* mass;       /* [L]                                                  */
    const float* com;        /* [L,3] centre of mass in link frame                   */
    const float* inertia;    /* [L,6] about com, link frame: xx yy zz xy xz yz       */
    const float* lower;      /* [L]   joint limits (rad or m); lower>=upper: unlimited */
    const float* upper;      /* [L]                                                  */
    const float* damping;    /* [L]   joint viscous damping (implicit)               */
    const float* armature;   /* [L]   joint armature (added to M diagonal)           */
    const int32_t* geom_link;/* [G]                                                  */
    const int32_t* geom_type;/* [G]   MI_GEOM_*                                      */
    const float* geom_p0;    /* [G,3] sphere centre / capsule end 0, link frame      */
    const float* geom_p1;    /* [G,3] capsule end 1 (ignored for spheres)            */
    const float* geom_radius;/* [G]                                                  */
    const int32_t* sensor_link; /* [S] force sensor body                              */
    const float* sensor_pos; /* [S,3] sensor site in link frame (wrench reference)   */
    const int32_t* pairs;    /* [P,2] self-collision geom pairs                      */
    /* analytic cart-pole parameters (dyn_kind == MI_DYN_CARTPOLE)                   */
    float cart_mass, pole_mass, pole_com, pole_inertia, cart_damping, pole_damping;
} mi_model_desc;

/* Scene / solver parameters — the task YAML `sim:` + `physx:` surface
 * (cfg/task/Humanoid.yaml:34-63, utils/config_utils/default_scene_params.py:30-112). */
typedef struct mi_sim_params {
    float dt;                       /* sim.dt                                         */
    float gravity[3];               /* sim.gravity                                    */
    int32_t solver_iterations;      /* PGS: position + velocity iteration counts;     */
                                    /* TGS: solver_position_iteration_count          */
    float contact_offset;           /* physx.contact_offset                           */
    float rest_offset;              /* physx.rest_offset                              */
    float friction;                 /* default_physics_material.dynamic_friction      */
    float max_depenetration_velocity;
    float erp;                      /* position-error reduction per substep (0..1)    */
    int32_t enable_self_collisions; /* <Actor>.enable_self_collisions                 */
    float max_angular_velocity;     /* rad/s, PhysX default 5729.58 deg/s             */
    float angular_damping;          /* 1/s, per-link angular velocity damping, PhysX  */
                                    /* default 0.05 (docs/transfering_policies_...:74) */
    int32_t solver_type;            /* physx.solver_type (cfg/config.yaml:31): 0 PGS, */
                                    /* 1 TGS (MI_SOLVER_*); anything else is refused  */
    int32_t velocity_iterations;    /* TGS: solver_velocity_iteration_count (PGS: 0)  */
} mi_sim_params;

/* Contact / limit solvers. Both build the same constraint rows from the same
 * state, with the rows' separation d (contact gap - rest_offset, or the joint's distance inside
 * its limit).
 *   MI_SOLVER_PGS: solver_iterations velocity-level Gauss-Seidel sweeps over the whole substep,
 *     bias b = d >= 0 ? -d / dt : -erp d / dt (capped at max_depenetration_velocity); positions
 *     integrated with the final velocity.
 *   MI_SOLVER_TGS (PhysX's default, solver_type 1): solver_iterations position iterations, each a
 *     sub-step h = dt / solver_iterations: one sweep with the bias of the row's CURRENT separation
 *     d + J (sum of h u over the earlier sub-steps) over h; then velocity_iterations sweeps with
 *     the speculative bias only (no position correction). Positions advance by the sub-steps'
 *     velocities (dt x their mean), the velocity state is the last sweep's. */
#define MI_SOLVER_PGS 0
#define MI_SOLVER_TGS 1

/* Task-layer parameters (cfg/task/{Humanoid,Ant,Cartpole}.yaml `env:` + task
 * constants from tasks/shared/locomotion.py:147-171, tasks/humanoid.py:81-112,
 * tasks/ant.py:79-86, tasks/cartpole.py:54-62). */
typedef struct mi_task_params {
    int32_t task_kind;              /* MI_TASK_*                                      */
    int32_t num_obs;                /* O                                              */
    int32_t num_actions;            /* A                                              */
    float clip_actions, clip_obs;   /* env.clipActions / env.clipObservations (inf)   */
    float max_episode_length;       /* env.episodeLength (cartpole: 500)              */
    /* locomotion */
    float power_scale, heading_weight, up_weight, actions_cost, energy_cost;
    float dof_vel_scale, angular_velocity_scale, contact_force_scale;
    float joints_at_limit_cost, death_cost, termination_height, alive_reward_scale;
    float task_dt;                  /* locomotion.py:163, 1/60                         */
    float target[3];                /* locomotion.py:161, (1000,0,0)                   */
    float init_root_pos[3];         /* spawn translation, env frame                   */
    float init_root_quat[4];        /* wxyz                                           */
    float dof_pos_noise, dof_vel_noise; /* locomotion.py:120,124: 0.2, 0.1            */
    const float* joint_gears;       /* [A] host                                       */
    const float* motor_effort_ratio;/* [A] host                                       */
    const float* init_dof_pos;      /* [D] host                                       */
    /* cartpole */
    float reset_dist, max_push_effort;
} mi_task_params;

/* Constraint-row budget per env-substep (every path, and the oracle): ground contact and joint-
 * limit rows always fit (3 * candidate points + D <= MI_MAX_ROWS is required); self-contacts
 * take what is left, (MI_MAX_ROWS - 3 * ground_contacts - limited_joints) / 3 of them, in pair
 * order. */
#define MI_MAX_ROWS 128

typedef struct mi_sim mi_sim;

/* --- lifecycle: replaces World/SimulationContext + GridCloner + ArticulationView init
 *     (tasks/base/rl_task.py:109-131, utils/task_util.py:70) ---------------------------- */
int mi_sim_create(const mi_model_desc* model, const mi_sim_params* params, int32_t num_envs,
                  int64_t env_id_offset, int32_t device_id, const float* env_origins /*[N,3]*/,
                  uint64_t seed, mi_sim** out);
/* Issues any deferred substeps, waits for the device, frees everything. */
int mi_sim_destroy(mi_sim* sim);
/* ArticulationView.num_dof / count / get_dof_limits (humanoid.py:110, ant.py:81) */
int mi_sim_info(const mi_sim* sim, int32_t* num_envs, int32_t* num_dof, int32_t* num_links,
                int32_t* num_sensors, float* dof_limits /*[D,2] host or NULL*/);

/* --- ArticulationView tensor API (call sites locomotion.py:81-89,114,130-134) -------- */
int mi_get_root_state(mi_sim* sim, float* pos /*[N,3]*/, float* quat /*[N,4] wxyz*/,
                      float* vel /*[N,6] lin,ang*/, void* stream);
int mi_get_dof_state(mi_sim* sim, float* q /*[N,D]*/, float* qd /*[N,D]*/, void* stream);
int mi_get_sensor_wrench(mi_sim* sim, float* out /*[N,S,6]*/, void* stream);
int mi_set_dof_efforts(mi_sim* sim, const float* eff /*[n,D]*/, const int32_t* idx /*[n]|NULL*/,
                       int32_t n, void* stream);
int mi_set_dof_state(mi_sim* sim, const float* q /*[n,D]|NULL*/, const float* qd /*[n,D]|NULL*/,
                     const int64_t* idx /*[n]|NULL*/, int32_t n, void* stream);
int mi_set_root_state(mi_sim* sim, const float* pos /*[n,3]|NULL*/, const float* quat /*[n,4]|NULL*/,
                      const float* vel /*[n,6]|NULL*/, const int64_t* idx /*[n]|NULL*/, int32_t n,
                      void* stream);
/* The same two setters with int32 env ids: the Cartpole task's reset passes int32 indices
 * (tasks/cartpole.py:129-130, set_joint_positions / set_joint_velocities), so the view forwards
 * them without an int64 conversion launch per call. */
int mi_set_dof_state_i32(mi_sim* sim, const float* q /*[n,D]|NULL*/, const float* qd /*[n,D]|NULL*/,
                         const int32_t* idx /*[n]|NULL*/, int32_t n, void* stream);
int mi_set_root_state_i32(mi_sim* sim, const float* pos /*[n,3]|NULL*/, const float* quat /*[n,4]|NULL*/,
                          const float* vel /*[n,6]|NULL*/, const int32_t* idx /*[n]|NULL*/, int32_t n,
                          void* stream);
/* --- link-frame view: RigidPrimView over the articulation's bodies (knees and feet,
 *     tasks/anymal_terrain.py:293-307; hand and finger frames, tasks/franka_cabinet.py:197-217) ---
 * K frames, each rigidly attached to a link: frame k sits at link_ids[k] with origin offsets[k]
 * (link frame; NULL = link origins) and the link's orientation. Outputs row-major, any may be NULL:
 * pos [N,K,3] world, quat [N,K,4] wxyz, vel [N,K,6] = linear velocity of the frame origin, angular
 * velocity (world axes) — root_state's conventions, so frame (link 0, offset 0) IS mi_get_root_state
 * (a fixed base has no root velocity: its frames' velocities come from qd alone).
 * Both calls issue deferred substeps like the other getters, are stream-ordered, do not block the
 * host and do not allocate (capturable); link_ids and offsets are HOST arrays that travel by value
 * in the kernel argument block. They only read the state. 1 <= K <= L, else MI_E_SHAPE; an id
 * outside [0, L) is MI_E_ARG. */
int mi_get_link_state(mi_sim* sim, const int32_t* link_ids /*host [K]*/, const float* offsets /*host [K,3]|NULL*/,
                      int32_t K, float* pos, float* quat, float* vel, void* stream);
/* jac [N,K,6,nv]: rows lin(3), ang(3) of the same frames; columns = the generalized velocity
 * u = (root lin, root ang (world), qd[D]) for a floating root (nv = D+6), qd[D] for a fixed one.
 * vel[n,k] == jac[n,k] @ u[n]. Columns of DOFs that do not move the frame are exactly 0. */
int mi_get_link_jacobian(mi_sim* sim, const int32_t* link_ids, const float* offsets, int32_t K,
                         float* jac, void* stream);
/* --- dynamics view: ArticulationView.get_mass_matrices / get_coriolis_and_centrifugal_forces /
 *     get_generalized_gravity_forces, the terms a task-layer controller needs next to
 *     mi_get_link_jacobian (gravity compensation, computed torque, operational space) ---
 * Any output may be NULL, not all three (MI_E_NULL). Row-major:
 *   M    [N,nv,nv]  joint-space inertia of the rigid-body tree
 *   cor  [N,nv]     velocity-product (Coriolis / centrifugal) forces c(q,u)
 *   grav [N,nv]     generalized gravity forces g(q)
 * with  M u' + c + g = tau  for u = (root lin, root ang (world), qd[D]) (floating root,
 * nv = D+6) or qd[D] (fixed root): the generalized velocity of mi_get_link_jacobian.
 * M is the pure rigid-body inertia, sum_l J_l^T diag(m_l, I_l^world) J_l with J_l =
 * mi_get_link_jacobian of link l at offset com[l]: no armature and no dt * damping (the stepper
 * adds both to its own M; read them with mi_get_env_params / the model). Massless links contribute
 * nothing. M[j][k] is exactly 0 when neither DOF is an ancestor of the other, and M[j][k],
 * M[k][j] are the same bits.
 * c is the generalized force that holds u' = 0 at gravity 0: sum_l J_l^T (m_l a_l, I_l w'_l +
 * w_l x I_l w_l) with a_l / w'_l the centre-of-mass and angular accelerations the links have
 * while u is held constant. The per-link angular damping (mi_sim_params.angular_damping) and the
 * joint damping are NOT part of c.
 * g = -sum_l m_l J_lin,l^T gravity: for gravity (0,0,-9.81) the root's z entry is +9.81 * total
 * mass. With a per-env parameter table (mi_set_env_params, MI_ENVP_GRAVITY) g uses the gravity of
 * each env's record, else mi_sim_params.gravity; M and c never depend on the table.
 * Like the other getters the call issues deferred substeps, is stream-ordered, does not block the
 * host and does not allocate (capturable; a captured call keeps reading the parameter table it
 * was captured with). It only reads the state. Every model mi_sim_create accepts, both state
 * layouts; the analytic cart-pole is computed from its link tree like any other fixed-base model.
 * No atomics: the outputs are the same bits on every run. */
int mi_get_dynamics(mi_sim* sim, float* M, float* cor, float* grav, void* stream);
/* --- mass-matrix solve view: ArticulationView.solve_mass_matrices / get_forward_dynamics /
 *     get_task_space_inertias — products with the inverse of the joint-space inertia, the operation
 *     computed torque (Mt^-1 (tau - c - g)) and operational-space control (J Mt^-1 J^T) need on top
 *     of mi_get_dynamics and mi_get_link_jacobian ---
 * Mt is M of mi_get_dynamics (the same statements) plus the diagonal of the chosen mode on the joint
 * DOFs; it is factorised on the chip by the stepper's own tree LTDL (Mt = L^T D L over the DOF
 * tree, no fill-in) and never written to memory. Armature and damping come from each env's record
 * of the per-env parameter table (mi_set_env_params) when it exists, else from the model.
 * A bare-M mode is deliberately not offered: the rigid-body M of a model whose 3-DOF joints are
 * chains of massless links is nearly singular (Humanoid: condition number up to 4.7e7, smallest
 * eigenvalue ~1e-6, so a float32 solve is off by 1e-3 relative), while the matrices below have
 * condition numbers of 6.9e3 / 3.3e3 and solve to 4e-6 relative in float32.
 * u, nv as for mi_get_link_jacobian. Like the other getters the calls issue deferred substeps, are
 * stream-ordered, do not block the host and do not allocate (capturable; a captured call keeps
 * reading the parameter table it was captured with). They only read the state (and the efforts).
 * Every model mi_sim_create accepts, both state layouts; the analytic cart-pole goes through its
 * link tree (its own stepper treats damping explicitly, so there MI_MASS_STEPPER differs from the
 * matrix it inverts by dt * damping). Fixed summation order, no atomics: the same bits on every
 * run and every graph replay. Errors: MI_E_NULL; MI_E_SHAPE for R < 1 or K outside [1, L];
 * MI_E_ARG for a bad `which` or link id. */
enum { MI_MASS_ARMATURE = 0,  /* M + diag(armature)               : continuous-time inertia   */
       MI_MASS_STEPPER  = 1 };/* M + diag(armature + dt * damping): the matrix mi_sim_step inverts */

/* out[n,r,:] = Mt^-1 rhs[n,r,:];  rhs, out [N,R,nv] device, R >= 1; out may alias rhs. */
int mi_solve_mass(mi_sim* sim, int32_t which, const float* rhs, int32_t R, float* out, void* stream);

/* acc [N,nv] = Mt^-1 (S^T tau - c - g - B u): tau [N,D] device, NULL = the efforts last set.
 * B = joint damping (0 on root DOFs). With MI_MASS_STEPPER, u + dt*acc is the velocity one
 * contact-free, limit-free substep produces (mi_sim_params.angular_damping aside). While a body
 * wrench buffer exists (mi_apply_link_wrenches) its generalized force Q is part of the right-hand
 * side, as in the step: Mt^-1 (S^T tau + Q - c - g - B u); without one the result is unchanged.
 * While joint drive records exist (mi_set_drive_gains) the three calls see the drive as the step does
 * (include/mi_drive.h): MI_MASS_STEPPER's diagonal is armature + dt * B_E, B_E = (B + kd) + dt kp, and
 * forward dynamics uses B_E u and adds F_d = kp (q* - q) + kd qd* to tau, so the sentence above on
 * u + dt*acc stays true under a drive. MI_MASS_ARMATURE is continuous time: its matrix is unchanged
 * (the same bits), its forward dynamics uses B + kd and adds F_d. Without records: unchanged bits. */
int mi_get_forward_dynamics(mi_sim* sim, int32_t which, const float* tau, float* acc, void* stream);

/* Frames as mi_get_link_jacobian (host link_ids[K], offsets[K,3]|NULL). Either output may be
 * NULL, not both.  minv_jt [N,6K,nv] = rows Mt^-1 J_r^T;  lam_inv [N,6K,6K] = J Mt^-1 J^T
 * (the inverse task-space inertia; [i][j] and [j][i] the same bits). The Jacobian rows are formed
 * on the chip; nothing is read back from memory. */
int mi_get_link_task_inertia(mi_sim* sim, int32_t which, const int32_t* link_ids, const float* offsets,
                             int32_t K, float* minv_jt, float* lam_inv, void* stream);
/* --- inverse-dynamics view: ArticulationView.get_inverse_dynamics / get_joint_reaction_wrenches,
 *     RigidPrimView.get_accelerations, ArticulationView.get_coms / get_momenta /
 *     get_centroidal_momentum_matrices / get_energies — the other direction of the two views above:
 *     computed torque (tau = Mt acc + c + g + B u) by one recursive Newton-Euler pass that never
 *     forms M, the frame bias acceleration Jdot u of operational-space control, and the whole-body
 *     quantities balance controllers and imitation rewards are written in ---
 * The three calls follow mi_get_dynamics' contract: they issue deferred substeps, are stream-ordered,
 * do not block the host and do not allocate (capturable; a captured call keeps reading the parameter
 * table it was captured with). They only read the state. Gravity, armature and damping come from each
 * env's record of the per-env parameter table (mi_set_env_params) when it exists, else from
 * mi_sim_params / the model. Every model mi_sim_create accepts, both state layouts; the analytic
 * cart-pole goes through its link tree. Fixed summation order, no atomics: the same bits on every
 * run and every graph replay. Any output may be NULL, not all of a call's (MI_E_NULL). u, nv as for
 * mi_get_link_jacobian. */
enum { MI_MASS_RIGID = 2 };   /* M alone: inverse dynamics only (harmless to multiply, unsafe to invert) */

/* tau [N,nv] = Mt acc + c + g + B u   (acc [N,nv] device, NULL = 0)
 *   MI_MASS_RIGID   : Mt = M, B = 0            -> M acc + cor + grav of mi_get_dynamics
 *   MI_MASS_ARMATURE: Mt = M + diag(armature), B = joint damping
 *   MI_MASS_STEPPER : Mt = M + diag(armature + dt damping), B = joint damping
 * so mi_get_forward_dynamics(which, tau[:,joint dofs]) returns acc when the root entries of tau are 0.
 * Root entries (floating base) are the wrench the world must apply at the root origin. acc = NULL
 * gives the bits an all-zero acc gives. MI_E_ARG for any other `which`.
 * Joint drives (mi_set_drive_gains), like the body wrenches' Q, are NOT part of it: the call answers
 * which efforts a motion needs, whatever supplies them (with a drive or a wrench in effect, forward
 * dynamics of the returned tau is that motion plus what they add).
 * joint_wrench [N,L,6]|NULL: (force, torque about link l's origin), world axes, that link l's
 * parent (the world for link 0) transmits to link l for that motion under MI_MASS_RIGID terms
 * (inertial + velocity-product - gravity forces of l's subtree; no armature, no damping):
 * S_l . joint_wrench[l] == tau_rigid[dof of l]; joint_wrench[0] == tau_rigid[root] for a floating
 * base, and is the base reaction for a fixed one. */
int mi_get_inverse_dynamics(mi_sim* sim, int32_t which, const float* acc, float* tau, float* joint_wrench,
                            void* stream);

/* out [N,K,6] = J acc + Jdot u: time derivative of mi_get_link_state's vel for the same frames
 * (classical linear acceleration of the frame origin, angular acceleration, world axes).
 * acc NULL: the bias term Jdot u alone. Gravity does not enter. The frame (link 0, offset 0) of a
 * floating root is acc[:, 0:6] itself. Errors as mi_get_link_state (host link_ids[K],
 * offsets[K,3]|NULL; MI_E_SHAPE for K outside [1, L], MI_E_ARG for a bad link id); out NULL is
 * MI_E_NULL. */
int mi_get_link_acceleration(mi_sim* sim, const int32_t* link_ids, const float* offsets, int32_t K,
                             const float* acc, float* out, void* stream);

/* com [N,3] world; mom [N,6] = (total linear momentum, angular momentum about com), world axes;
 * cmm [N,6,nv] with mom == cmm @ u (rows 0..2 / total mass == Jacobian of com);
 * energy [N,2] = (1/2 u^T M u, -sum_l m_l gravity . com_l  [per-env gravity]). mom, cmm and the
 * kinetic energy do not depend on where the env stands or on the parameter table. */
int mi_get_momentum(mi_sim* sim, float* com, float* mom, float* cmm, float* energy, void* stream);
/* --- contact view: RigidContactView over the articulation's bodies (foot-contact rewards, "knee
 *     touched the ground" terminations, clearance shaping) and the contact Jacobian J_c a controller
 *     needs next to mi_solve_mass (J_c Mt^-1 J_c^T) ---
 * The contact set mi_sim_step would build from the CURRENT state, by the stepper's own definitions:
 *  - ground candidates: the model's contact points, one per sphere and two per capsule, in geom
 *    order; gap = root z + point z - radius against the plane z = 0, contact point (x, y, z -
 *    radius), normal +z, friction directions +x, +y, second link -1;
 *  - self candidates (enable_self_collisions and a model with pairs): the geom pairs in table
 *    order through mi_pair_contact / mi_contact_basis of mi_geom.h; normal from B to A;
 *  - a candidate is active when gap < contact_offset; `gap` is the surface gap (rest_offset not
 *    subtracted); active ground candidates come first in candidate order, active pairs follow in
 *    pair order, cut at (MI_MAX_ROWS - 3 ground - limited joints) / 3 (the budget above).
 * The set differs from the one the stepper builds from the same state only for candidates whose gap
 * is within rounding of contact_offset. Contact forces are not part of this view.
 * C = max_contacts = min(candidates, MI_MAX_ROWS / 3) slots per env; slots at or above count[n] are
 * written too: 0.0 in the float outputs, -1 in links. A model without geoms (Cartpole) has C = 0:
 * only count (zeros) and clearance (+inf) are written.
 * The three device calls follow the other views' contract: they issue deferred substeps, are
 * stream-ordered, do not block the host and do not allocate (capturable). They only read the
 * state. Every model mi_sim_create accepts, both state layouts. Compaction by ballot and prefix
 * count in candidate order, no atomics: the same bits on every run and every graph replay. */
int mi_get_contact_capacity(const mi_sim* sim, int32_t* max_contacts, int32_t* num_ground_candidates,
                            int32_t* num_pairs);
/* Any output may be NULL (skipped). count [N]; links [N,C,2] = (link of A, link of B or -1 for the
 * ground); point [N,C,3] world; normal [N,C,3]; gap [N,C]. */
int mi_get_contacts(mi_sim* sim, int32_t* count, int32_t* links, float* point, float* normal, float* gap,
                    void* stream);
/* J [N,C,3,nv]: rows (normal, t1, t2) of each slot; row . u = velocity of A's material point at the
 * contact point minus B's, along that direction (the ground is B and at rest); u, nv as for
 * mi_get_link_jacobian. Columns of DOFs above the common ancestor of A and B (the root's, for a
 * self-contact) cancel and are exactly 0.0f, like those of DOFs that move neither body. J NULL is
 * MI_E_NULL (with C = 0 there is nothing to write and the call returns 0). */
int mi_get_contact_jacobian(mi_sim* sim, float* J, void* stream);
/* Per link (host link_ids[K], 0 <= K <= L, else MI_E_SHAPE; an id outside [0, L) is MI_E_ARG):
 * count [N,K] = kept contacts that involve the link (a self-contact counts for both of its links);
 * clearance [N,K] = the smallest gap of any of the link's geoms, to the ground and to every geom it
 * is paired with, active or not; +inf for a link without geoms. Either output may be NULL. */
int mi_get_link_contact_summary(mi_sim* sim, const int32_t* link_ids, int32_t K, int32_t* count,
                                float* clearance, void* stream);
/* --- body wrenches: RigidPrimView.apply_forces / apply_forces_and_torques_at_pos over the
 *     articulation's bodies (rotor thrusts, tasks/quadcopter.py:159, crazyflie.py:261,
 *     ingenuity.py:172; push perturbations; the `rigid_prim_views: force` randomization group) ---
 * K frames as mi_get_link_state (HOST link_ids[K], offsets[K,3]|NULL = link origins). force, torque:
 * DEVICE [n,K,3], either may be NULL (not both: MI_E_NULL); idx: device int64 [n]|NULL (rows 0..n-1;
 * out-of-range ids are ignored, as mi_set_env_params; an id named twice in one call is undefined).
 * is_global 1: world axes; 0: the link's axes at call time. accumulate 0: the envs named REPLACE
 * their generalized force; 1: add to it.
 * The call turns the wrenches into the generalized force Q[n] = sum_k J_k(n)^T (f_k, tau_k), J_k
 * exactly mi_get_link_jacobian's frame Jacobian at the current state (its u and nv), formed on the
 * chip, summed in call order k = 0..K-1 (no atomics: the same bits on every run), and stores it in a
 * sim-owned [N,nv] buffer. Entries of DOFs that move none of the frames are exactly 0 (accumulate 0).
 * From then on Q acts in EVERY substep as a constant generalized force, root DOFs included, like an
 * effort: M~ (u+ - u) / dt = S^T tau + Q - c - g - B u. It is frozen in generalized coordinates at the
 * configuration of the call and stays until it is replaced or cleared; a reset does not clear it
 * (PhysX holds the world-frame force over the step and drops it afterwards; a
 * task that re-applies every pre_physics_step, as the three above do, sees no difference beyond
 * O(dt) per step).
 * The first call allocates the buffer (zeros) and, if absent, the per-env parameter table with the
 * nominal values (mi_set_env_params): the force is added by the kernel variants that read the
 * table, so the physics is otherwise unchanged and the plain kernels know nothing of it. Hence the
 * table's limits: MI_E_STATE on the wavefront-per-env path and for a first call inside a stream
 * capture; MI_E_ARG for MI_DYN_CARTPOLE (the analytic cart-pole takes efforts only).
 * mi_sim_clear_env_params drops the wrench buffer with the table.
 * Like the other entry points the three calls issue deferred substeps first (those ran under the
 * force of their request), are stream-ordered, do not block the host and allocate nothing after the
 * first use (capturable). They do not write the state: the mirrors stay valid. Every articulated
 * model mi_sim_create accepts, both state layouts. Errors: MI_E_SHAPE for K outside [1, L] or n < 0
 * (n > N without idx); MI_E_ARG for a bad link id. */
int mi_apply_link_wrenches(mi_sim* sim, const int32_t* link_ids, const float* offsets, int32_t K,
                           const float* force, const float* torque, const int64_t* idx, int32_t n,
                           int32_t is_global, int32_t accumulate, void* stream);
/* Q rows of the envs named <- exact zeros (idx NULL, n = N: all). A no-op before the first wrench. */
int mi_clear_link_wrenches(mi_sim* sim, const int64_t* idx, int32_t n, void* stream);
/* Q [N,nv] device <- the generalized force in effect (zeros before any wrench was applied). */
int mi_get_applied_generalized_forces(mi_sim* sim, float* Q, void* stream);
/* --- implicit PD joint drives: ArticulationView.set_gains / set_joint_position_targets /
 *     set_joint_velocity_targets (tasks/anymal.py:187, franka_cabinet.py:254,285, ball_balance.py:188,
 *     quadcopter.py:158, shared/in_hand_manipulation.py:267,329) ---
 * Per env and joint DOF a stiffness kp, a damping kd, a position target q* and a velocity target qd*.
 * Every substep applies the joint torque tau_d = kp (q* - q+) + kd (qd* - u+) at its END state
 * (q+ = q + dt u+), solved with the velocities: with
 *     B_E = (B + kd) + dt kp        F_d = kp (q* - q) + kd qd*      (include/mi_drive.h)
 * the substep solves (M + arm + dt B_E) (u+ - u) / dt = S^T (tau + F_d) + Q - c - g - B_E u, q the
 * substep's own positions, so F_d follows the joint within one mi_sim_step(k) or mi_env_step, which
 * an effort set from outside cannot. The contact and joint-limit rows see the drive's stiffness
 * through that matrix. tau is the effort in force (mi_set_dof_efforts, or actions * gear in the
 * fused env step): the drive adds to it. There is no effort cap (PhysX's maxForce) and the
 * mask-driven reset keeps gains and targets: a task sets targets in its own reset.
 * Storage: a sim-owned buffer of four lines of D floats per env (kp, kd, q*, qd*), absent until the
 * first setter call; all zeros is no drive. kd is NOT written into the table's MI_ENVP_DAMPING slot:
 * mi_set_env_params / mi_get_env_params and the physics DR schedules keep their meaning, and B above
 * is that slot. The first setter call allocates the buffer (zeros) and, if absent, the per-env
 * parameter table with the nominal values: only the kernel variants that read the table read the
 * drive, and the plain kernels know nothing of it. Hence the table's limits: MI_E_STATE on the
 * wavefront-per-env path and for a first call inside a stream capture; MI_E_ARG for
 * MI_DYN_CARTPOLE. mi_sim_clear_env_params drops the buffer with the table.
 * kp, kd / q_target, qd_target: DEVICE [n,D], either may be NULL (that line keeps its values), not
 * both (MI_E_NULL); idx: device int64 [n]|NULL (rows 0..n-1; out-of-range ids are ignored; an id
 * named twice in one call is undefined). MI_E_SHAPE for n < 0 (n > N without idx). The values are
 * stored as given: negative or non-finite gains, and targets outside the joint limits, are the
 * caller's responsibility.
 * Like the other entry points the calls issue deferred substeps first (those ran under the drive of
 * their request), are stream-ordered, do not block the host and allocate nothing after the first use
 * (capturable). They do not write the state: the mirrors stay valid. */
int mi_set_drive_gains(mi_sim* sim, const float* kp, const float* kd, const int64_t* idx, int32_t n,
                       void* stream);
int mi_set_drive_targets(mi_sim* sim, const float* q_target, const float* qd_target, const int64_t* idx,
                         int32_t n, void* stream);
/* Each [N,D] device, any may be NULL: the values in effect, the bits that were set (zeros before any
 * setter call). */
int mi_get_drives(mi_sim* sim, float* kp, float* kd, float* q_target, float* qd_target, void* stream);
/* All four lines of the envs named <- exact zeros (idx NULL, n = N: all): from the next substep on
 * they step to the bits of a sim that never had a drive. A no-op before the first setter call. */
int mi_clear_drives(mi_sim* sim, const int64_t* idx, int32_t n, void* stream);
/* State mirrors: row-major copies of the articulation state in caller-owned device buffers, the
 * tensors ArticulationView getters hand out with clone=False (get_world_poses, get_velocities,
 * get_joint_positions / velocities, _physics_view.get_force_sensor_forces: locomotion.py:81-89;
 * Isaac returns views of its own buffers there too). Register all six (or all NULL to stop);
 * mi_get_state_mirror issues any deferred substeps and refreshes every stale mirror in ONE launch
 * (none when nothing wrote the state since the last refresh), so the five getter calls of one
 * get_observations cost at most one gather launch. Every entry point that writes the state marks
 * the mirrors stale; mi_set_dof_efforts does not (efforts are not mirrored). A call on another
 * stream than the last refresh's waits for that refresh (stream-ordered, no host sync).
 * Contract: the mirrors are the library's copies — a caller must not write them (an in-place
 * edit would persist into later getters until the state changes; the reference's task code only
 * reads them, locomotion.py:81-89). */
int mi_sim_set_mirror(mi_sim* sim, float* pos /*[N,3]*/, float* quat /*[N,4]*/, float* vel /*[N,6]*/,
                      float* q /*[N,D]*/, float* qd /*[N,D]*/, float* sens /*[N,S,6]*/);
int mi_get_state_mirror(mi_sim* sim, void* stream);

/* --- physics step: World.step x controlFrequencyInv (envs/vec_env_rlgames.py:64-66) --- */
/* Substeps are deferred and coalesced: consecutive mi_sim_step calls on one stream with no
 * other call touching the state in between (the reference's controlFrequencyInv x World.step
 * loop) run as ONE launch, issued by the next entry point that reads or writes the state (or by
 * mi_sim_flush); results are identical to separate launches. Inside a stream capture, and with
 * the environment variable MI_SIM_DEFER=0, every call launches at once. substeps in [0, 64];
 * one launch never carries more than 64 (a call that would pass 64 issues the pending ones first). */
int mi_sim_step(mi_sim* sim, int32_t substeps, void* stream);
/* Issue any deferred substeps now (stream-ordered; no host sync). */
int mi_sim_flush(mi_sim* sim, void* stream);

/* --- fused task kernels ---------------------------------------------------------------- */
int mi_task_configure(mi_sim* sim, const mi_task_params* tp);
/* LocomotionTask.pre_physics_step / CartpoleTask.pre_physics_step
 * (locomotion.py:103-145, cartpole.py:101-134): mask-driven reset_idx for every env with
 * reset_buf != 0 (no host sync), actions_out = actions, efforts = actions*gear*power. */
int mi_task_pre_step(mi_sim* sim, const float* actions /*[N,A]*/, int64_t* reset_buf,
                     int64_t* progress_buf, float* potentials, float* prev_potentials,
                     float* actions_out /*[N,A]|NULL*/, void* stream);
/* reset_idx(env_ids) with explicit indices (locomotion.py:116-145, cartpole.py:114-134) */
int mi_task_reset_idx(mi_sim* sim, const int64_t* env_ids, int32_t n, int64_t* reset_buf,
                      int64_t* progress_buf, float* potentials, float* prev_potentials,
                      void* stream);
/* RLTask.post_physics_step (rl_task.py:231-251): progress += 1, get_observations,
 * calculate_metrics, is_done — one kernel (locomotion.py:80-101,173-321,
 * humanoid.py:116-127, ant.py:88-95, cartpole.py:80-99,143-162). */
int mi_task_post_step(mi_sim* sim, const float* actions /*[N,A]*/, float* obs /*[N,O]*/,
                      float* rew /*[N]*/, int64_t* reset_buf, int64_t* progress_buf,
                      float* potentials, float* prev_potentials, void* stream);
/* Which kernel the last mi_task_post_step launched and its grid (diagnostics, no reference
 * counterpart): 2 k_loco_post_tiled (one 32-env tile per workgroup), 4 k_loco_post_pipe (32-env
 * tiles), 5 k_post_step (one lane per env), 6 k_loco_post_pipe with 16-env tiles; -1 before the
 * first launch. The environment variable MI_POST_TILE (read per launch) asks for one of them:
 * 32p (code 4, the default), 16p (6) or 32s (2); any other value selects the default, as an unset
 * one does. Codes 0, 1 and 3 (MI_POST_TILE=64s, 64d, 32d: 64-env and unstaged variants of the
 * one-tile kernel) are retired: those values now select the default too. */
int mi_task_post_kernel(const mi_sim* sim, int32_t* kernel, int32_t* grid);
/* The three task methods RLTask.post_physics_step calls, as separate kernels
 * (rl_task.py:244-250) for tasks that override some of them in torch:
 * get_observations (locomotion.py:80-101 / cartpole.py:80-99) writes obs + potentials,
 * calculate_metrics (locomotion.py:173-178 / cartpole.py:143-153) reads obs,
 * is_done (locomotion.py:180-183 / cartpole.py:155-162) reads obs[:,0] and progress_buf. */
int mi_task_observations(mi_sim* sim, const float* actions /*[N,A]*/, float* obs /*[N,O]*/,
                         float* potentials, float* prev_potentials, void* stream);
int mi_task_metrics(mi_sim* sim, const float* actions, const float* obs, float* rew,
                    const float* potentials, const float* prev_potentials, void* stream);
int mi_task_is_done(mi_sim* sim, const float* obs, int64_t* reset_buf, const int64_t* progress_buf,
                    void* stream);
/* VecEnvRLGames.step (vec_env_rlgames.py:56-78) minus the Python: clamp actions,
 * pre_physics_step, `substeps` physics steps, post_physics_step and _process_data's obs
 * clamp, in ONE kernel launch. obs_task (unclamped task.obs_buf) may be NULL. */
int mi_env_step(mi_sim* sim, const float* actions /*[N,A]*/, int32_t substeps,
                float* obs_out /*[N,O] clamped*/, float* obs_task /*[N,O]|NULL*/,
                float* rew /*[N]*/, int64_t* reset_buf, int64_t* progress_buf,
                float* potentials, float* prev_potentials, float* actions_out /*[N,A]|NULL*/,
                float* rew_out /*[N]|NULL*/, int64_t* reset_out /*[N]|NULL*/, void* stream);
/* rew_out / reset_out: the fresh copies VecEnvRLGames._process_data returns
 * (vec_env_rlgames.py:41-46), written by the same launch instead of two clone kernels. */
/* Launch timing (measurement only, no reference counterpart; bench.py's roofline): from now on
 * every `every`-th mi_env_step / mi_task_post_step launch (up to `capacity` of them) carries a HIP start / stop event
 * pair on its own dispatch (hipExtLaunchKernelGGL), so the recorded interval is the kernel alone
 * and no marker packets are queued between launches. every <= 0 turns it off. Launches made while
 * the stream captures a graph are not timed. */
int mi_sim_time_launches(mi_sim* sim, int32_t every, int32_t capacity);
/* Durations (ms) of the launches timed since mi_sim_time_launches, in launch order: waits for
 * each one's stop event, writes min(recorded, max_out) values, *n_out = number recorded. */
int mi_sim_launch_times(mi_sim* sim, float* ms_out, int32_t max_out, int32_t* n_out);

/* --- observation / action noise DR (utils/domain_randomization/randomize.py:176-306) ------
 * The `domain_randomization.randomization_params.{observations,actions}` block of a task YAML.
 * Noise math and per-env schedule state: include/mi_dr.h. */
enum { MI_DR_OP_ADDITIVE = 0, MI_DR_OP_SCALING = 1 };
enum { MI_DR_DIST_GAUSSIAN = 0, MI_DR_DIST_UNIFORM = 1, MI_DR_DIST_LOGUNIFORM = 2 };
typedef struct mi_dr_noise {
    int32_t enabled;            /* 0: schedule absent                                  */
    int32_t operation;          /* MI_DR_OP_*          (randomize.py:277-282,298-303)  */
    int32_t distribution;       /* MI_DR_DIST_*        (randomize.py:270-275,290-296)  */
    int32_t frequency_interval; /* on_interval only    (randomize.py:228,252)          */
    float params[2];            /* distribution_parameters: (mean, std) | (lo, hi)     */
} mi_dr_noise;
typedef struct mi_dr_params {
    mi_dr_noise obs_on_reset, obs_on_interval, act_on_reset, act_on_interval;
} mi_dr_params;
/* Randomizer._set_up_{observations,actions}_randomization (randomize.py:176-210): configures
 * the schedules and zeroes the per-env state (counters, correlated-noise epochs). NULL or all
 * disabled turns DR off. Once on, mi_env_step applies the action noise after its clamp and the
 * observation noise before _process_data's clamp, in the same launch (vec_env_rlgames.py:59-71),
 * and requires actions_out (task.actions) for locomotion tasks. */
int mi_task_set_dr(mi_sim* sim, const mi_dr_params* dr /*host|NULL*/);
/* apply_actions_randomization / apply_observations_randomization (randomize.py:212-260) for the
 * method-by-method step: in place on [N,A] actions / [N,O] obs, with the step's reset_buf. */
int mi_dr_apply_actions(mi_sim* sim, float* actions /*[N,A]*/, const int64_t* reset_buf, void* stream);
int mi_dr_apply_observations(mi_sim* sim, float* obs /*[N,O]*/, const int64_t* reset_buf,
                             void* stream);
/* Per-env DR schedule state -> host [N,6] uint32: obs (counter, epoch, draws), act (same). */
int mi_get_dr_state(mi_sim* sim, uint32_t* out /*[N,6] host*/);

/* --- per-env physics parameters + physics DR (randomize.py:308-430) -----------------------
 * The `simulation`, `articulation_views` and `rigid_prim_views` groups of
 * `domain_randomization.randomization_params` (docs/domain_randomization.md:147-167), which the
 * reference hands to omni.replicator.isaac.physics_view. An mi_sim has an OPTIONAL device table
 * with one record per env, a whole number of 128-byte lines:
 *     gravity[3], friction, damping[D], armature[D], padding
 * Absent (the default), every kernel is the same code as without this feature and reads the
 * sim-wide mi_sim_params / mi_model_desc values. The first mi_set_env_params or
 * mi_sim_set_phys_dr allocates it (filled with the nominal values) and from then on mi_sim_step,
 * mi_env_step and the task path launch kernel variants that read gravity, ground / self-contact
 * friction, joint damping and armature from the record of the env they simulate. Covered: the
 * two-envs-per-wavefront kernels (both solvers) and the one-lane-per-env kernels (incl. the
 * analytic cart-pole, which takes gravity and damping = (cart, pole); armature and friction are
 * MI_E_ARG there). The wavefront-per-env path (MI_WAVE_PAIR=0, runtime tables) refuses the table
 * with MI_E_STATE. */
enum { MI_ENVP_GRAVITY = 0,   /* dim 3: SimulationContext gravity (randomize.py:308-342)        */
       MI_ENVP_FRICTION = 1,  /* dim 1: material_properties' dynamic friction (:344-430)        */
       MI_ENVP_DAMPING = 2,   /* dim D: ArticulationView.set_gains kds / `damping`              */
       MI_ENVP_ARMATURE = 3   /* dim D: ArticulationView.set_armatures / `joint_armatures`      */ };
/* ArticulationView-style indexed setter / getter of one attribute (stream-ordered, no host
 * block once the table exists). idx NULL: rows 0..n-1; out-of-range ids are ignored. */
int mi_set_env_params(mi_sim* sim, int32_t attr, const float* values /*[n,dim] device*/,
                      const int64_t* idx /*[n] device|NULL*/, int32_t n, void* stream);
/* Before the table exists: the nominal values broadcast over the envs. */
int mi_get_env_params(mi_sim* sim, int32_t attr, float* out /*[N,dim] device*/, void* stream);
/* Drops the table (and leaves the physics DR schedules off): back to the nominal physics and to
 * the kernels that know no table. The body wrench buffer (mi_apply_link_wrenches) rides on the
 * table's kernels and is dropped with it: no generalized force is in effect afterwards. So are
 * the joint drive records (mi_set_drive_gains): no drive is in effect afterwards. Waits for the
 * device. */
int mi_sim_clear_env_params(mi_sim* sim);

/* Physics DR schedules (include/mi_dr_phys.h): per attribute an optional on_reset and an optional
 * on_interval schedule (randomize.py:313-342,393-428). */
enum { MI_DR_OP_DIRECT = 2 };   /* docs/domain_randomization.md:85-89 */
typedef struct mi_dr_phys_sched {
    int32_t enabled;            /* 0: schedule absent                                  */
    int32_t operation;          /* MI_DR_OP_* incl. MI_DR_OP_DIRECT                    */
    int32_t distribution;       /* MI_DR_DIST_*                                        */
    int32_t frequency_interval; /* on_interval only; all on_interval schedules of one  */
                                /* sim share one value (one interval counter per env)  */
    const float* p0;            /* host [dim]: mean | lower, per component             */
    const float* p1;            /* host [dim]: std | upper                             */
} mi_dr_phys_sched;
typedef struct mi_dr_phys_params {
    mi_dr_phys_sched on_reset[4], on_interval[4];   /* indexed by MI_ENVP_*            */
    int32_t min_frequency;      /* docs/domain_randomization.md:120-128                */
} mi_dr_phys_params;
/* Randomizer.set_up_domain_randomization's physics groups (randomize.py:85-110). The first call
 * that turns a schedule on allocates the table and zeroes the per-env schedule state; later
 * calls (set_dr_distribution_parameters, randomize.py:461-488) replace the schedules and keep
 * that state. NULL (or nothing enabled) turns the schedules off; the table stays. A configuration
 * call: waits for the device before it replaces the schedules (not inside a stream capture). */
int mi_sim_set_phys_dr(mi_sim* sim, const mi_dr_phys_params* dr /*host|NULL*/);
/* dr.physics_view.step_randomization(reset_inds) (docs/domain_randomization.md:251-260,
 * in_hand_manipulation.py:226,271-275) as a mask: one launch, no allocation, no host sync
 * (capturable). mi_env_step issues it itself, before its fused launch, with the incoming
 * reset_buf; the method-by-method path calls it before mi_task_pre_step consumes the mask.
 * A no-op while no schedule is on. */
int mi_dr_phys_step(mi_sim* sim, const int64_t* reset_buf /*[N] device*/, void* stream);
/* Per-env schedule state -> host [N,4] uint32: since, counter, epoch, draws (zeros while off). */
int mi_get_phys_dr_state(mi_sim* sim, uint32_t* out /*[N,4] host*/);

/* --- utilities --------------------------------------------------------------------- */
/* U(lo,hi) Philox4x32-10 actions for the random-policy driver (scripts/random_policy.py:57),
 * keyed on (seed, env_id_offset + env, step). */
int mi_fill_uniform(mi_sim* sim, float* out /*[N,cols]*/, int32_t cols, uint64_t seed,
                    uint64_t step, float lo, float hi, void* stream);
/* Per-env reset counters (the Philox counter of the reset noise stream) -> host [N]. */
int mi_get_reset_count(mi_sim* sim, uint32_t* out /*[N] host*/);
/* Host [N] -> the per-env reset counters (restores a recorded state, e.g. a golden fixture's,
 * so the next reset draws the same Philox noise; no reference counterpart: torch's global
 * generator state plays this role there, locomotion.py:120-124). Blocks the host. */
int mi_set_reset_count(mi_sim* sim, const uint32_t* in /*[N] host*/);
/* Pairing by load of the two-envs-per-wavefront kernels (no reference counterpart: tests and
 * diagnostics). Each 16-env workgroup ranks its envs by a per-env load key — the most constraint
 * rows of any substep in the env's last fused env-step — and pairs ranks w and 15 - w in wave w.
 * out: host [N] <- the keys; in: host [N] -> the keys (either may be NULL; in after out);
 * pairing: 0 index pairing (envs 2w, 2w + 1), 1 by load, -1 unchanged. Blocks the host. */
int mi_sim_pair_load(mi_sim* sim, int32_t* out /*[N] host|NULL*/, const int32_t* in /*[N] host|NULL*/,
                     int32_t pairing);
/* Number of env-steps whose physics produced a non-finite state and were forced to reset
 * (issues deferred substeps first and waits for them: blocks the host). */
int mi_sim_nan_count(mi_sim* sim, int64_t* count);
/* Diagnostics: which physics kernel runs. path: 0 one-lane-per-env, 1 wavefront-per-env,
 * 2 two envs per wavefront (the compiled topologies' default; MI_WAVE_PAIR=0 selects path 1);
 * topology: id of the compile-time (model-specialised) topology, 0 = runtime tables;
 * lds_bytes: LDS per env (= per workgroup) of the wave path. Any output may be NULL. */
int mi_sim_kernel_path(const mi_sim* sim, int32_t* path, int32_t* topology, int32_t* lds_bytes);
/* Diagnostics: rows of an env's W matrix (one per constraint row of a substep) that the wave
 * paths keep in LDS; a substep with more rows puts the rest in the env's global slab. 0 on the
 * one-lane-per-env path. */
int mi_sim_w_rows_lds(const mi_sim* sim, int32_t* rows);
/* Diagnostics (host only, no device): how the compiled wave kernels spread the composite sums of
 * a substep (P2) over a group of `lanes` (32 or 64) lanes. The work items are the (link, slot)
 * pairs, slot = one of the four float4 of a link's record; links ranked by descendant count,
 * longest first, the items dealt to the lanes in passes. items[pass * lanes + lane] <- 4 link +
 * slot, or -1 where the lane idles; passes <- the number of passes. items may be NULL (passes
 * only); cap: entries items holds. link_parent as mi_model_desc.parent (root first, parent -1). */
int mi_p2_item_table(const int32_t* link_parent, int32_t L, int32_t lanes, int32_t* items, int32_t cap,
                     int32_t* passes);
int mi_abi_version(void);
/* SHA-256 (hex) of the sources this library was compiled from: csrc/mi_sim.hip, the csrc .hpp headers and
 * the include headers in name order (__graft_entry__.source_hash); "unknown" when built without it. A
 * stale binary shows up as a mismatch against the tree (smoke(), tests/test_host.py). */
const char* mi_build_id(void);
const char* mi_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MI_SIM_H */
