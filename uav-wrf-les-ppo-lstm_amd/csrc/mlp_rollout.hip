// mlp_rollout.hip -- R1 for the reference's OWN policy, the MLP of mlp_tile_core.h (train_ppo2.0.py:157-198 for N environments
// x T steps in ONE launch): rollout_mlp_kernel is a persistent kernel that runs policy forward -> Categorical sample -> env
// step -> store for 16 environments per workgroup and keeps every activation on chip.  Its GREEDY forms are the evaluation
// episodes (argmax, no auto-reset), with or without the stop rule.  The forward is mlp_tile_core.h's, shared with the update
// kernel (mlp_update.hip): the log-probabilities stored here are bit-identical to that kernel's first forward pass.
#include "internal_env.h"
#include "loss_core.h"
#include "mlp_tile_core.h"

namespace {

constexpr int WS2 = 260;                // row stride of the LDS image of wave 0's W2 rows (float4-aligned)

struct MlpRollBufs {
    float* cur_obs; float* obs; int32_t* act; float* rew; float* val; float* logp; float* done; uint8_t* flags;
    float* last_val; const int32_t* forced_act; const double* noise; int32_t* nan_count; float* info; float* heads;
    uint8_t* active; float* pos;    // greedy episodes only: active u8 [N] in/out, agent_pos record [N][T][2]
    // greedy episodes with the stop rule (STOP) only: window [N][window][2] + fill [N] in/out (stop_rule_core.h), optional pos_std [N][T]
    float* stop_win; int32_t* stop_cnt; float* rule_val; StopRule rule;
};

constexpr size_t ROLL_LDS = (size_t)(Tiles<1>::FLOATS + 16 * WS2) * sizeof(float);

// H3: the 256 x 128 layer on the fp16 matrix pipe (layer2_h3) -- the update kernel of the same arithmetic runs the same
// code, so the rollout's log-probabilities stay bit-identical to the update's first forward pass.
// GREEDY: greedy evaluation episodes (uav_greedy_episodes; the record is env_core.h's GreedyRec): argmax of the logits, no
// auto-reset, an ended or inactive env is never stepped.  GREEDY = false is the trainer's rollout.
// STOP (with GREEDY): evaluate_model.py's stop rule after every env step (flags bit3; a hit ends the episode as `done` does).
// STOP = false compiles to the kernels as they were.
template <bool H3, bool GREEDY = false, bool STOP = false, int INW = IN>
__global__ __launch_bounds__(512) void rollout_mlp_kernel(EnvParams P_arg, EnvBlob blob, int N, int T, uint64_t iter,
                                                            const float* __restrict__ params, MlpRollBufs B) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Tiles<1> L(smem);
    float* W2i = smem + Tiles<1>::FLOATS;                        // [16][WS2] rows 0..15 of W2: wave 0 (the env role) keeps no weight VGPRs
    __shared__ unsigned short vis[MT * NVIS];
    __shared__ EnvState es_s[MT];
    __shared__ double env_tab[ENV_LDS_TABLE_DOUBLES];            // pow(vc, 0.75) | ripple factors (env_core.h)
    static_assert(!STOP || GREEDY, "rollout_mlp_kernel: the stop rule belongs to the greedy episodes");
    constexpr size_t STOP_LDS = STOP ? MT * 2 * STOP_WIN_MAX * sizeof(float) : 0;      // the stop rule's position rings
    static_assert(ROLL_LDS + sizeof(vis) + sizeof(es_s) + sizeof(env_tab) + STOP_LDS <= 160 * 1024, "rollout_mlp_kernel: LDS over 160 KB per workgroup");
    float* ring = nullptr;                                       // STOP: this env lane's [STOP_WIN_MAX][2] ring
    StopRing sr{0, 0};
    if constexpr (STOP) {
        __shared__ float rings[MT * 2 * STOP_WIN_MAX];
        static_assert(sizeof(rings) == STOP_LDS, "stop rings");
        ring = rings + (threadIdx.x & 15) * 2 * STOP_WIN_MAX;
    }
    EnvParams P = P_arg;
    env_params_refresh(P);
    env_tables_to_lds(P, env_tab, threadIdx.x, 512);
    const int in = INW ? INW : 6 + P.trend_k;                    // observation features = row stride of cur_obs, obs and W1
    const MlpOff O(in);

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * MT;
    const int my_env = n0 + lane;
    const bool env_lane = (w == 0) && lane < MT && my_env < N;
    unsigned short* myvis = vis + (lane & 15) * NVIS;

    // ---- parameters
    stage_prm(L, params, O);
    unsigned short* W2p = reinterpret_cast<unsigned short*>(W2i);   // H3: rows 0..15 as piece fragments [8 slabs][2][64 lanes][8]
    if (H3) {
        for (int i = threadIdx.x; i < 16 * H1; i += 512) {
            const int row = i >> 8, k = i & 255, sl = k >> 5, q8 = (k >> 3) & 3, e = k & 7;
            _Float16 p0, p1;
            split2h(params[O.W2 + i], p0, p1);
            unsigned short* d = W2p + ((sl * 2) * 64 + q8 * 16 + row) * 8 + e;
            d[0] = h_bits(p0);
            d[64 * 8] = h_bits(p1);
        }
    } else {
        for (int i = threadIdx.x; i < 16 * H1; i += 512) W2i[(i >> 8) * WS2 + (i & 255)] = params[O.W2 + i];
    }
    float w1a[2][2], wh[4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k = 4 * s + kq;
            w1a[t][s] = k < in ? params[O.W1 + (32 * w + 16 * t + j) * in + k] : 0.f;
        }
#pragma unroll
    for (int s = 0; s < 4; ++s) wh[s] = j < NH ? params[O.WH + j * H2 + 16 * w + 4 * s + kq] : 0.f;
    const float* bh = params + O.BH;

    bool on = true, ran = true;                                  // GREEDY, wave 0: env active now / at entry
    if (w == 0 && lane < MT) {
        const int n = min(my_env, N - 1);
        es_s[lane] = env_load(blob, n);
        for (int k = 0; k < NVIS; ++k) myvis[k] = blob.visited[(size_t)n * NVIS + k];
#pragma unroll
        for (int f = 0; f < 8; ++f) L.X[lane * 8 + f] = f < in ? B.cur_obs[(size_t)n * in + f] : 0.f;
        if constexpr (GREEDY) on = ran = my_env < N && B.active[n] != 0;
        if constexpr (STOP) sr = stop_ring_load(ring, B.stop_win + (size_t)n * B.rule.window * 2, B.stop_cnt[n], B.rule.window);
    }
    lds_barrier();

    const float* w2row = W2i + j * WS2 + 4 * kq;
    const int steps = T + (B.last_val ? 1 : 0);              // one extra value-only pass for V(s_T)
    if (w != 0) {
        // ------------------------------------------------------------------ waves 1..7: their rows of W2 in registers
        f32x4 wA[H3 ? 1 : H1 / 16];
        f16x8 wP[H3 ? H1 / 32 : 1][2];
        if (H3) {
#pragma unroll
            for (int sl = 0; sl < H1 / 32; ++sl) {
                const float* src = params + O.W2 + (16 * w + j) * H1 + 32 * sl + 8 * kq;
                const f32x4 v0 = ld4(src), v1 = ld4(src + 4);
                const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    _Float16 p0, p1;
                    split2h(v[e], p0, p1);
                    wP[sl][0][e] = p0; wP[sl][1][e] = p1;
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < H1 / 16; ++s) wA[s] = ld4(params + O.W2 + (16 * w + j) * H1 + 16 * s + 4 * kq);
        }
        for (int t = 0; t < steps; ++t) {
            f32x4 xh1[1][2], xh2[1];
            float r1[1], r2[1];
            layer1<1, H3>(L, w1a, w, j, kq, xh1, r1);
            lds_barrier();                                   // a1 visible
            if constexpr (H3) layer2_h3<1>(L, [&](int sl, int pc) { return wP[sl][pc]; }, w, j, kq, xh2, r2);
            else layer2<1>(L, [&](int s) { return wA[s]; }, w, j, kq, xh2, r2);
            lds_barrier();                                   // a2 visible
            heads_fwd<1>(L, wh, bh, w, lane);
            lds_barrier();                                   // wave 0 has stepped the environments: next observations visible
        }
    } else {
        // ------------------------------------------------------------------ wave 0: its rows from LDS + the env role
        for (int t = 0; t < steps; ++t) {
            const bool value_only = (t == T);
            f32x4 xh1[1][2], xh2[1];
            float r1[1], r2[1];
            layer1<1, H3>(L, w1a, w, j, kq, xh1, r1);
            lds_barrier();                                       // a1 visible
            if constexpr (H3) layer2_h3<1>(L, [&](int sl, int pc) { return *reinterpret_cast<const f16x8*>(W2p + ((sl * 2 + pc) * 64 + lane) * 8); },
                                           w, j, kq, xh2, r2);
            else layer2<1>(L, [&](int s) { return ld4(w2row + 16 * s); }, w, j, kq, xh2, r2);
            lds_barrier();                                       // a2 visible
            heads_fwd<1>(L, wh, bh, w, lane);
            if (w == 0) {
                __builtin_amdgcn_s_waitcnt(0xc07f);              // lgkmcnt(0): HD written (single wave)
                __builtin_amdgcn_wave_barrier();
                if (lane < MT) {
                    float z[NA];
#pragma unroll
                    for (int a = 0; a < NA; ++a) z[a] = L.HD[lane * 8 + a];
                    const float V = L.HD[lane * 8 + NA];
                    if (value_only) {
                        if (env_lane) B.last_val[my_env] = V;
                    } else if constexpr (GREEDY) {
                        // argmax of the logits, then the environment step without reset
                        bool bad;
                        const int a_sel = argmax_first<NA>(z, bad);
                        if (bad && env_lane && on) atomicAdd(B.nan_count, 1);
                        const size_t row = (size_t)min(my_env, N - 1) * T + t;
                        const GreedyRec rec{B.act, B.obs, B.pos, B.flags, STOP ? B.rule_val : nullptr};
                        if (on) {
                            EnvState es = es_s[lane];
                            StepOut so;
                            env_step(P, P.env_offset + my_env, es, myvis, a_sel, B.noise, row, so);
                            bool hit = false;                    // STOP: the rule fires on this step
                            if constexpr (STOP) {
                                float rv;
                                hit = stop_rule_step(B.rule, ring, sr, es.px, es.py, so.obs[2], B.rule_val != nullptr, rv);
                                if (B.rule_val && env_lane) B.rule_val[row] = rv;
                            }
                            if (env_lane) greedy_rec_stepped(rec, row, in, a_sel, so, es, hit);
#pragma unroll
                            for (int f = 0; f < IN_MAX; ++f) if (f < in) L.X[lane * 8 + f] = so.obs[f];
                            es_s[lane] = es;
                            if (so.done || hit) on = false;
                        } else if (env_lane) {
                            greedy_rec_idle(rec, row, in);
                        }
                        (void)V;
                    } else {
                        const int eg = P.env_offset + my_env;
                        const size_t row = (size_t)min(my_env, N - 1) * T + t;
                        float lp;
                        bool bad;
                        const int a_sel = rollout_draw<NA>(z, B.forced_act, row, [&]() {
                            return philox4x32_10(P.seed, (uint32_t)t, (uint32_t)eg, (uint32_t)iter, RNG_ACTION).x; }, lp, bad);
                        if (bad && env_lane) atomicAdd(B.nan_count, 1);
                        // environment step (f64, env_core.h) + auto reset
                        EnvState es = es_s[lane];
                        StepOut so;
                        env_step(P, eg, es, myvis, a_sel, B.noise, row, so);
                        if (env_lane) {
#pragma unroll
                            for (int f = 0; f < IN_MAX; ++f) if (f < in) B.obs[row * in + f] = L.X[lane * 8 + f];
                            B.act[row] = a_sel;
                            B.rew[row] = (float)so.reward;
                            B.val[row] = V;
                            B.logp[row] = lp;
                            B.done[row] = so.done ? 1.f : 0.f;
                            B.flags[row] = (uint8_t)step_flags(so);
                            if (B.heads) {
#pragma unroll
                                for (int a = 0; a < NA; ++a) B.heads[row * NH + a] = z[a];
                                B.heads[row * NH + NA] = V;
                            }
                            if (B.info) {
#pragma unroll
                                for (int f = 0; f < 5; ++f) B.info[row * 10 + f] = (float)so.info[f];
                                B.info[row * 10 + 5] = so.obs[2];
                                B.info[row * 10 + 6] = es.px;    // agent_pos after the move (before any auto-reset)
                                B.info[row * 10 + 7] = es.py;
                                B.info[row * 10 + 8] = (float)es.sx;
                                B.info[row * 10 + 9] = (float)es.sy;
                            }
                        }
                        env_auto_reset(P, eg, es, myvis, so);
#pragma unroll
                        for (int f = 0; f < IN_MAX; ++f) if (f < in) L.X[lane * 8 + f] = so.obs[f];
                        es_s[lane] = es;
                    }
                }
            }
            lds_barrier();                                       // next observations visible; HD / HP free again
        }
    }
    if (GREEDY && env_lane) B.active[my_env] = on ? 1 : 0;
    if (env_lane && ran) {
        env_store(blob, my_env, es_s[lane]);
        for (int k = 0; k < NVIS; ++k) blob.visited[(size_t)my_env * NVIS + k] = myvis[k];
#pragma unroll
        for (int f = 0; f < IN_MAX; ++f) if (f < in) B.cur_obs[(size_t)my_env * in + f] = L.X[lane * 8 + f];
        if constexpr (STOP)
            B.stop_cnt[my_env] = stop_ring_store(ring, sr, B.stop_win + (size_t)my_env * B.rule.window * 2, B.rule.window);
    }
}
}  // namespace

// one rollout_mlp_kernel launch in the width the env asks for: 6 inputs = the instantiation with compile-time offsets,
// 7 / 8 = the run-time-width one
template <bool H3, bool GREEDY, bool STOP>
static int launch_rollout_mlp_form(const EnvParams& P, const EnvBlob& blob, int n_env, int steps, uint64_t iter, const float* params,
                                   const MlpRollBufs& B, hipStream_t st) {
    const dim3 grid((n_env + MT - 1) / MT);
    if (P.trend_k == 0) {
        UAV_CHECK_HIP(uav_dyn_lds(reinterpret_cast<const void*>(&rollout_mlp_kernel<H3, GREEDY, STOP>), (int)ROLL_LDS));
        hipLaunchKernelGGL((rollout_mlp_kernel<H3, GREEDY, STOP>), grid, dim3(512), ROLL_LDS, st, P, blob, n_env, steps, iter, params, B);
    } else {
        UAV_CHECK_HIP(uav_dyn_lds(reinterpret_cast<const void*>(&rollout_mlp_kernel<H3, GREEDY, STOP, 0>), (int)ROLL_LDS));
        hipLaunchKernelGGL((rollout_mlp_kernel<H3, GREEDY, STOP, 0>), grid, dim3(512), ROLL_LDS, st, P, blob, n_env, steps, iter, params, B);
    }
    UAV_LAUNCH_CHECK();
    return 0;
}

// ---- entry used by uav_rollout (rollout.hip) for policy_kind 0 (`trend` false: 6 inputs only) and 2 (6 + trend_k inputs)
int launch_rollout_mlp(uav_ctx* ctx, void* env_state, int n_env, const uav_env_cfg* cfg, const float* params, int horizon,
                       uint64_t iter, float* cur_obs, float* obs, int32_t* act, float* rew, float* val, float* logp,
                       float* done, uint8_t* flags, float* last_val, const int32_t* forced_act, const double* noise,
                       int32_t* nan_count, float* info, float* heads, bool trend, hipStream_t st) {
    EnvParams P;
    int rc = env_params_from_cfg(ctx, cfg, n_env, P);
    if (rc) return rc;
    UAV_REQUIRE(trend || P.trend_k == 0, "uav_rollout: the fused MLP rollout has 6 observation features (trend_k = 0)");
    UAV_REQUIRE(P.trend_k >= 0 && 6 + P.trend_k <= IN_MAX, "uav_rollout: trend_k=%d (0 .. 2)", P.trend_k);
    MlpRollBufs B{cur_obs, obs, act, rew, val, logp, done, flags, last_val, forced_act, noise, nan_count, info, heads};
    EnvBlob blob = env_blob_view(env_state, n_env);
    // the handle's arithmetic (uav_set_lstm_arith): FP16X3 = the 256 x 128 layer on the fp16 matrix pipe (max |param| < 2048);
    // anything else = exact-f32 MFMA
    return ctx->mode.arith == UAV_ARITH_FP16X3 ? launch_rollout_mlp_form<true, false, false>(P, blob, n_env, horizon, iter, params, B, st)
                                               : launch_rollout_mlp_form<false, false, false>(P, blob, n_env, horizon, iter, params, B, st);
}

// ---- entry used by uav_greedy_episodes (rollout.hip) for policy_kind 0 and 2 (the caller checked kind against P.trend_k): the
// fp16-split form only (the caller checked the mode)
int launch_greedy_mlp(const EnvParams& P, void* env_state, int n_env, const float* params, int steps, float* cur_obs,
                      uint8_t* active, const double* noise, int32_t* act, float* obs, float* pos, uint8_t* flags,
                      int32_t* nan_count, hipStream_t st) {
    UAV_REQUIRE(P.trend_k >= 0 && 6 + P.trend_k <= IN_MAX, "uav_greedy_episodes: trend_k=%d (0 .. 2)", P.trend_k);
    MlpRollBufs B{cur_obs, obs, act, nullptr, nullptr, nullptr, nullptr, flags, nullptr, nullptr, noise, nan_count, nullptr, nullptr,
                  active, pos};
    return launch_rollout_mlp_form<true, true, false>(P, env_blob_view(env_state, n_env), n_env, steps, 0, params, B, st);
}

// ---- the same with the stop rule (uav_greedy_episodes_stop; the caller checked the rule and its buffers)
int launch_greedy_mlp_stop(const EnvParams& P, void* env_state, int n_env, const float* params, int steps, float* cur_obs,
                           uint8_t* active, const double* noise, int32_t* act, float* obs, float* pos, uint8_t* flags,
                           int32_t* nan_count, const StopRule& rule, float* stop_win, int32_t* stop_cnt, float* rule_val,
                           hipStream_t st) {
    UAV_REQUIRE(P.trend_k >= 0 && 6 + P.trend_k <= IN_MAX, "uav_greedy_episodes_stop: trend_k=%d (0 .. 2)", P.trend_k);
    MlpRollBufs B{cur_obs, obs, act, nullptr, nullptr, nullptr, nullptr, flags, nullptr, nullptr, noise, nan_count, nullptr, nullptr,
                  active, pos, stop_win, stop_cnt, rule_val, rule};
    return launch_rollout_mlp_form<true, true, true>(P, env_blob_view(env_state, n_env), n_env, steps, 0, params, B, st);
}
