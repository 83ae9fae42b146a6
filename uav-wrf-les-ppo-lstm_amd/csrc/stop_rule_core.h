// stop_rule_core.h -- the "autonomous stop" rule of PPOV1.1/evaluate_model.py:25-37 for one environment.
//
// The reference keeps a Python list of {pos (f32 pair), conc} per step and, once it holds `window` entries, stops the
// episode when BOTH hold:
//     np.std(last `window` positions, axis=0).mean() < pos_std_max          ("the UAV has settled")
//     trajectory[-1]['conc'] * CONC_PEAK > conc_min                          ("in high concentration")
// with conc = info['concentration_reward'] * CONC_PEAK = (conc_coef * obs[2]) * conc_peak, every product in f32 (a Python
// float times an np.float32 stays f32) -- the second scaling by CONC_PEAK is the reference's own and is kept.
//
// np.std over a [window][2] f32 array reduces along the outer axis, i.e. sequentially in time order, all in f32:
//     mean_k = (sum_i p_ik) / window;  var_k = (sum_i (p_ik - mean_k)^2) / window;  std_k = sqrt(var_k);  (std_0 + std_1) / 2
// stop_pos_std() below is that chain, operation for operation.  It is bit-exact only without FMA contraction: every
// translation unit that includes this header is built with -ffp-contract=off (csrc/Makefile; rollout, mlp_rollout, env).
// f32 division and sqrt are the correctly rounded ones (hipcc's default), as numpy's are.
//
// Window buffers of the entry points (include/uavppo.h: uav_greedy_episodes_stop, uav_stop_stability):
//     stop_win f32 [N][window][2]   the env's last stop_cnt[n] positions in TIME ORDER, oldest first, in rows 0 .. stop_cnt-1;
//                                   rows from stop_cnt[n] on are not read and not written
//     stop_cnt i32 [N]              number of valid rows, 0 .. window (it saturates at window)
// A kernel that runs many steps keeps the window as a ring (in LDS) and writes it back in time order, so the buffers do
// not depend on how the steps were cut into launches.
#pragma once
#include "common.h"

constexpr int STOP_WIN_MAX = 16;         // uav_stop_rule.window <= 16

struct StopRule {                        // kernel-argument copy of uav_stop_rule
    int window;
    float pos_std_max, conc_coef, conc_peak, conc_min;
};

// the record's concentration: evaluate_model.py:61 (`final_conc` of the CSV is this value at the last step)
__host__ __device__ inline float stop_conc(const StopRule& R, float obs2) { return (R.conc_coef * obs2) * R.conc_peak; }

// evaluate_model.py:35,37: current_conc = conc * CONC_PEAK > conc_threshold
__host__ __device__ inline bool stop_conc_high(const StopRule& R, float obs2) { return stop_conc(R, obs2) * R.conc_peak > R.conc_min; }

// at(i, x, y): sample i of the window, i = 0 the oldest
template <class At>
__host__ __device__ inline float stop_pos_std(int window, At&& at) {
    const float w = (float)window;
    float sx = 0.f, sy = 0.f;
    for (int i = 0; i < window; ++i) {
        float x, y;
        at(i, x, y);
        sx = sx + x;
        sy = sy + y;
    }
    const float mx = sx / w, my = sy / w;
    float qx = 0.f, qy = 0.f;
    for (int i = 0; i < window; ++i) {
        float x, y;
        at(i, x, y);
        const float dx = x - mx, dy = y - my;
        qx = qx + dx * dx;
        qy = qy + dy * dy;
    }
    const float sdx = sqrtf(qx / w), sdy = sqrtf(qy / w);
    return (sdx + sdy) / 2.0f;
}

// A ring of the last `window` positions: `ring` holds [STOP_WIN_MAX][2] floats of one env (LDS in the fused kernels),
// head = the slot the next push writes (= the oldest sample once the ring is full), fill = valid samples (<= window).
struct StopRing {
    int head, fill;
};

// rows 0 .. cnt-1 of the env's stop_win (time order) into the ring
__host__ __device__ inline StopRing stop_ring_load(float* ring, const float* win, int cnt, int window) {
    cnt = cnt < 0 ? 0 : (cnt > window ? window : cnt);
    for (int i = 0; i < cnt; ++i) {
        ring[2 * i] = win[2 * i];
        ring[2 * i + 1] = win[2 * i + 1];
    }
    return StopRing{cnt == window ? 0 : cnt, cnt};
}

// the ring back into stop_win, oldest first; returns stop_cnt
__host__ __device__ inline int stop_ring_store(const float* ring, const StopRing& r, float* win, int window) {
    const int first = r.fill == window ? r.head : 0;
    for (int i = 0; i < r.fill; ++i) {
        int s = first + i;
        if (s >= window) s -= window;
        win[2 * i] = ring[2 * s];
        win[2 * i + 1] = ring[2 * s + 1];
    }
    return r.fill;
}

// One step of the rule for one env: push agent_pos, then evaluate.  `value` receives pos_std, or NaN while the window is
// not full; with want_value = false the std is only formed when the concentration half already holds (the decision is the
// same: it is the conjunction).  Returns the stop decision.
__host__ __device__ inline bool stop_rule_step(const StopRule& R, float* ring, StopRing& r, float px, float py, float obs2,
                                               bool want_value, float& value) {
    ring[2 * r.head] = px;
    ring[2 * r.head + 1] = py;
    r.head = r.head + 1 == R.window ? 0 : r.head + 1;
    if (r.fill < R.window) r.fill += 1;
    value = __builtin_nanf("");
    if (r.fill < R.window) return false;
    const bool high = stop_conc_high(R, obs2);
    if (!want_value && !high) return false;
    const int head = r.head, window = R.window;
    value = stop_pos_std(window, [&](int i, float& x, float& y) {
        int s = head + i;
        if (s >= window) s -= window;
        x = ring[2 * s];
        y = ring[2 * s + 1];
    });
    return high && value < R.pos_std_max;
}
