// greedy_tail.hip -- the tail of ONE step of a step-wise greedy evaluation (evaluate_with_lstm.py's loop for the policies the
// fused greedy kernels of rollout.hip do not cover: stacked layers, h = 256, parameters beyond the fp16-split range) as one
// launch behind the per-layer LSTM step kernels: policy heads of the top layer's y, argmax, environment step WITHOUT reset,
// the optional stop rule, the step's record, the next observation and the env's `active` flag.  A step of such a policy is
// then L + 2 launches on the steppers (3 L + 1 on the uav_lstm_fwd layers) instead of the few dozen of the torch loop.
//
// A wave takes four envs: the heads by rows4_heads (rows_dot_core.h: rows_dot_kernel's sums, so the logits are bit for bit
// uav_gemm_f32's few-columns form), then lanes 0..3 each carry one env through argmax_first (loss_core.h), env_step (env_core.h)
// and stop_rule_step (stop_rule_core.h; the window in place in stop_win / stop_cnt, as stop_stability_kernel holds it).
// An env with active[i] = 0 only gets its "not stepped" record; its blob, cur_obs row and window are not touched.
// Built with the default -ffp-contract=off: it holds env and stop-rule arithmetic.
#include "internal_env.h"
#include "loss_core.h"
#include "rows_dot_core.h"

struct GreedyTailBufs {
    float* cur_obs;             // [N][od] in/out
    uint8_t* active;            // [N] in/out
    const double* noise;        // optional [N][2]: this step's standard normals
    int32_t* act; float* obs; float* pos; uint8_t* flags;      // records [N][steps](, od | 2), written at column t
    int32_t* nan_count;
    float* stop_win; int32_t* stop_cnt; float* rule_val;        // with a rule: window [N][window][2] + fill [N] in/out, optional [N][steps]
};

template <int A>
__global__ __launch_bounds__(256) void greedy_tail_kernel(EnvParams P, EnvBlob b, int n, const float* __restrict__ y, int64_t ldy,
                                                          int K, const float* __restrict__ w_head, const float* __restrict__ b_head,
                                                          int steps, int t, GreedyTailBufs B, bool has_rule, StopRule R) {
    const int lane = threadIdx.x & 63;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    if (m0 >= n) return;
    env_params_refresh(P);
    float z[A];
    rows4_heads<A>(w_head, b_head, y, ldy, m0, n, K, lane, z);
    const int64_t i64 = m0 + lane;
    if (lane >= 4 || i64 >= n) return;
    const int i = (int)i64;
    const int od = 6 + P.trend_k;
    const size_t col = (size_t)i * steps + t;
    const GreedyRec rec{B.act, B.obs, B.pos, B.flags, B.rule_val};
    if (B.active[i] == 0) {
        greedy_rec_idle(rec, col, od);
        return;
    }
    bool bad;
    const int a_sel = argmax_first<A>(z, bad);
    if (bad) atomicAdd(B.nan_count, 1);
    // ---- the env step without the reset: an ended env stays as its last step left it
    EnvState s = env_load(b, i);
    unsigned short* vis = b.visited + (size_t)i * NVIS;
    const int a_env = a_sel > 4 ? 4 : a_sel;        // uav_env_step's clamp (n_act = 6 only)
    StepOut o;
    env_step(P, P.env_offset + i, s, vis, a_env, B.noise, (size_t)i, o);
    env_store(b, i, s);
    // ---- the stop rule on this step's agent_pos and obs[2]
    bool hit = false;
    if (has_rule) {
        float ring[2 * STOP_WIN_MAX];
        float* win = B.stop_win + (size_t)i * R.window * 2;
        StopRing sr = stop_ring_load(ring, win, B.stop_cnt[i], R.window);
        float rv;
        hit = stop_rule_step(R, ring, sr, s.px, s.py, o.obs[2], B.rule_val != nullptr, rv);
        B.stop_cnt[i] = stop_ring_store(ring, sr, win, R.window);
        if (B.rule_val) B.rule_val[col] = rv;
    }
    // ---- the record, and what the next step starts from
    greedy_rec_stepped(rec, col, od, a_sel, o, s, hit);
    for (int k = 0; k < od; ++k) B.cur_obs[(size_t)i * od + k] = o.obs[k];
    if (o.done || hit) B.active[i] = 0;
}

extern "C" int uav_greedy_tail(uav_ctx* ctx, void* env_state, int n_env, const uav_env_cfg* cfg, const float* y, int64_t y_stride,
                               int hidden, const float* w_head, const float* b_head, int n_act, int steps, int t,
                               const double* noise_t, float* cur_obs, uint8_t* active, int32_t* act, float* obs, float* pos,
                               uint8_t* flags, int32_t* nan_count, const uav_stop_rule* rule, float* stop_win, int32_t* stop_cnt,
                               float* rule_val, uav_stream stream) {
    UAV_REQUIRE(ctx && env_state && y && w_head && b_head && cur_obs && active && act && obs && pos && flags && nan_count,
                "uav_greedy_tail: NULL argument");
    UAV_REQUIRE(n_env > 0 && steps > 0 && t >= 0 && t < steps, "uav_greedy_tail: n_env=%d steps=%d t=%d", n_env, steps, t);
    UAV_REQUIRE(hidden >= 4 && hidden <= 256 && hidden % 4 == 0 && y_stride % 4 == 0 && y_stride >= hidden &&
                (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (reinterpret_cast<uintptr_t>(w_head) & 15) == 0,
                "uav_greedy_tail: hidden %d (a multiple of 4 up to 256), y rows 16-byte aligned", hidden);
    StopRule R{};
    if (rule) {
        UAV_REQUIRE(rule->window >= 1 && rule->window <= STOP_WIN_MAX, "uav_greedy_tail: rule window=%d (1 .. %d)", rule->window,
                    STOP_WIN_MAX);
        UAV_REQUIRE(stop_win && stop_cnt, "uav_greedy_tail: NULL stop_win / stop_cnt (the rule's window buffers)");
        R = StopRule{rule->window, rule->pos_std_max, rule->conc_coef, rule->conc_peak, rule->conc_min};
    }
    EnvParams P;
    int rc = env_params_from_cfg(ctx, cfg, n_env, P);
    if (rc) return rc;
    UAV_REQUIRE((int64_t)n_env * steps * (6 + P.trend_k) < (1ll << 31), "uav_greedy_tail: n_env * steps too large");
    const GreedyTailBufs B{cur_obs, active, noise_t, act, obs, pos, flags, nan_count, stop_win, stop_cnt, rule ? rule_val : nullptr};
    const dim3 grid((unsigned)((n_env + 15) / 16));
#define LAUNCH_T(A_)                                                                                                             \
    hipLaunchKernelGGL(greedy_tail_kernel<A_>, grid, dim3(256), 0, as_stream(stream), P, env_blob_view(env_state, n_env), n_env, \
                       y, y_stride, hidden, w_head, b_head, steps, t, B, rule != nullptr, R)
    switch (n_act) {
        case 2: LAUNCH_T(2); break;
        case 3: LAUNCH_T(3); break;
        case 4: LAUNCH_T(4); break;
        case 5: LAUNCH_T(5); break;
        case 6: LAUNCH_T(6); break;
        default: UAV_REQUIRE(false, "uav_greedy_tail: n_act=%d unsupported (2..6)", n_act);
    }
#undef LAUNCH_T
    UAV_LAUNCH_CHECK();
    return 0;
}
