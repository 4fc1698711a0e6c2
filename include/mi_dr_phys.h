/* mi_dr_phys.h — per-env physics domain randomization (gravity, friction, joint damping and
 * armature): the schedule decision and the value function, shared as source by the HIP schedule
 * kernel and by host tests (like mi_dr.h: plain C, FP contraction off).
 *
 * Restates the physics half of the reference's Randomizer
 * (utils/domain_randomization/randomize.py:308-430, stepped by
 * omni.replicator.isaac.physics_view.step_randomization(reset_inds),
 * docs/domain_randomization.md:251-260, tasks/shared/in_hand_manipulation.py:226,271-275):
 *
 *   step_randomization(reset_inds), per env:
 *     r = reset_buf != 0 && since >= min_frequency        (docs/domain_randomization.md:120-128)
 *     if r: since = 0, epoch += 1;   since += 1
 *     interval counter: mi_dr_begin(counter, ., draws, reset := r, ., frequency_interval)
 *     component c of attribute a:
 *       v = nominal[c]
 *       on_reset    schedule, epoch > 0:  v = op(v, draw(stream_reset(a),    epoch, c))
 *       on_interval schedule, draws > 0:  v = op(v, draw(stream_interval(a), draws, c))
 *
 * MI355X-first storage, like mi_dr.h: no per-env sample buffers. A draw is a pure function of
 * (seed, stream, global env id, epoch | draws, component), so the record of an env is recomputed
 * from four uint32 (since, counter, epoch, draws) whenever one of its schedules fires and is
 * independent of sharding.
 *
 * Operations (docs/domain_randomization.md:85-89): additive v + x, scaling v * x, direct x.
 */
#ifndef MI_DR_PHYS_H
#define MI_DR_PHYS_H

#include "mi_dr.h"

/* attributes of an env's parameter record (include/mi_sim.h MI_ENVP_*) */
#define MI_DR_PHYS_ATTRS 4
/* Philox stream ids: 6 + 2 a (on_reset) and 7 + 2 a (on_interval) of attribute a (0..5 are
 * taken: mi_dr.h); the stream id occupies 4 bits of the counter block */
#define MI_DR_STREAM_PHYS_RESET(a) (6u + 2u * (uint32_t)(a))
#define MI_DR_STREAM_PHYS_INTERVAL(a) (7u + 2u * (uint32_t)(a))

#define MI_DR_PHYS_OP_DIRECT 2

MI_DR_FN float mi_dr_phys_op(int32_t operation, float x, float draw) {
    MI_DR_NO_CONTRACT
    return operation == MI_DR_PHYS_OP_DIRECT ? draw : mi_dr_op(operation, x, draw);
}

/* Per-env schedule decision of one step_randomization call. */
typedef struct mi_dr_phys_env {
    uint32_t since, counter, epoch, draws;
    int reset;       /* on_reset schedules fire this call    */
    int fire;        /* on_interval schedules fire this call */
} mi_dr_phys_env;

MI_DR_FN mi_dr_phys_env mi_dr_phys_begin(uint32_t since, uint32_t counter, uint32_t epoch,
                                         uint32_t draws, int reset_buf, int min_frequency,
                                         int on_interval, int frequency_interval) {
    mi_dr_phys_env e;
    const int r = reset_buf && (int64_t)since >= (int64_t)min_frequency;
    const mi_dr_env b = mi_dr_begin(counter, epoch, draws, r, 1, on_interval, frequency_interval);
    e.since = (r ? 0u : since) + 1u;
    e.counter = b.counter;
    e.epoch = b.epoch;
    e.draws = b.draws;
    e.reset = r;
    e.fire = b.fire;
    return e;
}

/* Component value after both schedules. ur / ui: the four uniforms of Philox block
 * (component >> 1) of the on_reset stream keyed on epoch / of the on_interval stream keyed on
 * draws (read only when that schedule is on and has fired at least once). */
MI_DR_FN float mi_dr_phys_value(float nominal, int component,
                                int r_on, int32_t r_op, int32_t r_dist, float r_p0, float r_p1,
                                uint32_t epoch, const float ur[4],
                                int i_on, int32_t i_op, int32_t i_dist, float i_p0, float i_p1,
                                uint32_t draws, const float ui[4]) {
    MI_DR_NO_CONTRACT
    float v = nominal;
    if (r_on && epoch) v = mi_dr_phys_op(r_op, v, mi_dr_value(r_dist, r_p0, r_p1, ur, component));
    if (i_on && draws) v = mi_dr_phys_op(i_op, v, mi_dr_value(i_dist, i_p0, i_p1, ui, component));
    return v;
}

#endif /* MI_DR_PHYS_H */
