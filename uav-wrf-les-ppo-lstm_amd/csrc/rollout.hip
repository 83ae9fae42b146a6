// rollout.hip -- R1: fused persistent rollout for the LSTM actor-critic.
//
// Reference loop body: PPOV2.0/train_ppo2.0.py:157-198 (policy forward -> Categorical sample ->
// env.step -> buffer.store), here for N environments x T steps in ONE launch.
//
// One workgroup owns 16 environments for the whole horizon:
//   * H/16 "gate" waves keep the two fp16 pieces of their W_hh slice in VGPRs (as lstm_fwd_h3_kernel) and the
//     cell state in registers; h_t lives in two fp16 LDS planes;
//   * wave 0 additionally plays the "env" role: it computes the actor/critic heads of h_t with one
//     MFMA chain (head-weight pieces as A-fragments from LDS), then lanes 0..15 each sample an action
//     (counter RNG, torch Categorical(probs) semantics), step their environment (env_core.h, f64)
//     and store the transition into the (env, T, feat) buffers;
//   * that VALU/f64 work for step t overlaps the other waves' recurrent MFMAs for step t+1 (both
//     only need h_t; wave 0's SIMD partner fills the matrix pipe meanwhile); two workgroup
//     barriers per step, no inter-workgroup communication.
// (Tried and measured: spreading the env role over all waves with opposite [env|MFMA] order between SIMD
//  partners.  Correct, but two inlined copies of the f64 env chain beside 128 weight VGPRs spill ~90 VGPRs
//  in every wave: 1.9 ms vs 1.2 ms.  The env role stays on wave 0.)
// Procedural fields make the whole rollout HBM-write-only apart from the policy parameters:
// 44 B per env-step (obs 24, act 4, rew 4, val 4, logp 4, done 4) + 5 B (keep, flags).
#include "internal_env.h"
#include "loss_core.h"
#include "phase_prof.h"
#include "rows_dot_core.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RMT = 16;

// phase timing of wave 0: cycles summed over the rollout by workgroup 0 (phase_prof.h)
PROF_TABLE(g_roll_prof, [8], uav_roll_prof_read)

// (the activations are common.h's plain fast_sigmoid / fast_tanh: the update's sequence kernels use fast_tanh_fma)

// LDS geometry of the split-fp16 rollout (dynamic part; the env role's small arrays are static)
template <int H>
struct RGeom {
    static constexpr int NW = H / 16;
    static constexpr int NS = H / 32;                 // K = 32 slabs over the hidden dimension
    static constexpr int RS = H + 8;                  // padded plane row (fp16): conflict-free ds_read_b128
    static constexpr int PLANE = RMT * RS;
    static constexpr int W0 = 4 * NS * 2 * 64 * 8;    // fp16: BOTH weight pieces of wave 0 (its VGPRs belong to the env role)
    static constexpr size_t LDS = (2 * PLANE /*h*/ + 2 * PLANE /*head weights*/ + W0) * sizeof(unsigned short) +
                                  (NW * 8 * 64 /*W_ih fragments*/ + 4 * H /*bias*/) * sizeof(float);
};

struct RolloutBufs {
    float* cur_obs; float* h; float* c;
    float* obs; int32_t* act; float* rew; float* val; float* logp; float* done; uint8_t* flags; float* keep;
    float* last_val; const int32_t* forced_act; const double* noise; int32_t* nan_count;
    float* info;                // optional [N][T][10]: 5 reward parts of environment.py:161-167, obs[2], agent_pos, source_pos of the step
    float* heads;               // optional [N][T][NA+1]: logits | value of the step
    float* stash; float* y;     // optional: BPTT stash [N][T][6H] + y [N][T][H], so PPO epoch 0 skips its forward pass
    uint8_t* active; float* pos;  // greedy episodes only: active u8 [N] in/out, agent_pos record [N][T][2]
    // greedy episodes with the stop rule (STOP) only: window [N][window][2] + fill [N] in/out (stop_rule_core.h), optional pos_std [N][T]
    float* stop_win; int32_t* stop_cnt; float* rule_val; StopRule rule;
};

// The recurrent product h W_hh^T runs on the fp16 matrix pipe at f32 accuracy (two-piece operand split, three piece
// products into a main and a cross accumulator; common.h split2h, lstm.hip lstm_fwd_h3_kernel) in the weights-as-A
// orientation: lane (j, kq) owns env j and the four consecutive units uo..uo+3, so the stash leaves as dwordx4 stores and
// h_t is parked with one ds_write_b64 per piece.  Wave 0 (gate wave AND env role) keeps NO weights in registers -- both
// pieces of its slice sit in LDS and are read back as lane-contiguous b128 fragments -- so the f64 env chain has the
// register file to itself; the two roles run separate, barrier-matched time loops, which keeps the other waves' 128
// weight VGPRs out of wave 0's live set.
// GREEDY: one greedy evaluation episode per env (evaluate_with_lstm.py's loop) instead of a training rollout -- argmax of the
// logits instead of a sample, no auto-reset, and an env whose episode has ended (or that came in with active[n] = 0) is never
// stepped again: its blob, h and c keep the values of its last step.  kbuf holds the per-env active flag then.  The record
// per step is the action, the observation the step returned (the terminal one when done), agent_pos after the move, and flags
// (bit0 done, bit1 reached, bit2 not stepped: act -1, obs and pos 0).  GREEDY = false is the trainer's rollout, unchanged.
// STOP (with GREEDY): evaluate_model.py's stop rule after every env step (stop_rule_core.h) -- the env lane keeps its window as
// a ring in LDS, and a hit ends the episode as `done` does (flags bit3).  STOP = false compiles to the kernels as they were.
// TREND: the observation has od = 6 + P.trend_k features (od = 7 or 8 at run time, one instantiation for both).  The x rows
// were 8 wide all along (K = 8 in two f32 k-steps), so only what fills them changes: w_ih is [4H][od], xbuf / cur_obs / the obs
// record carry od features, and the parked transition keeps the whole 8-wide row -- the source position moves to the spare
// slots 5, 6 of the logits block, the greedy agent_pos to slots 1, 2 of the first block, so trs does not grow.  With a stash
// the kernel also fills the h_prev slot [.., 5H:6H] as uav_lstm_fwd does for I > 6 (uav_lstm_wgrad reads it there): the
// unmasked h_t goes to row t + 1 with the rest of the stash, and keep_fixup zeroes that row where step t ended the episode
// (the same lane, the same address: program order).  TREND = false compiles to the kernels as they were.
template <int H, int NA, bool GREEDY = false, bool STOP = false, bool TREND = false>
__global__ __launch_bounds__(H * 4) void rollout_lstm_kernel(EnvParams P_arg, EnvBlob blob, int N, int T,
                                                                        uint64_t iter, const float* __restrict__ params,
                                                                        RolloutBufs B) {
    using G = RGeom<H>;
    constexpr int NS = G::NS, RS = G::RS, PLANE = G::PLANE, W0 = G::W0, NW = G::NW;
    constexpr int NH = NA + 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned short* hpl = reinterpret_cast<unsigned short*>(smem);          // [2 pieces][RMT][RS] h_t
    unsigned short* whp = hpl + 2 * PLANE;                                  // [2 pieces][16 heads][RS] head weights
    unsigned short* w0p = whp + 2 * PLANE;                                  // [4 gates][NS][2 pieces][64 lanes][8]
    float* wxl = reinterpret_cast<float*>(w0p + W0);                        // [NW][4 gates][2 k-steps][64 lanes]
    float* bl = wxl + NW * 512;                                             // [4H] b_ih + b_hh
    __shared__ __attribute__((aligned(16))) float xbuf[RMT * 8];
    __shared__ float kbuf[RMT];
    __shared__ float hd[RMT * 16];
    __shared__ unsigned short vis[RMT * NVIS];
    __shared__ EnvState es_s[RMT];
    __shared__ float trs[4 * RMT * 8];                            // the step's transition, parked by wave 0, stored by the last gate wave
    __shared__ __attribute__((aligned(16))) f32x4 acc0[4 * 64];  // wave 0's next-step accumulators, computed by the gate waves
    __shared__ double env_tab[ENV_LDS_TABLE_DOUBLES];            // pow(vc, 0.75) | ripple factors (env_core.h)
    // one workgroup per CU at h = 128 (~145 KB with the 66 KB of env tables; h = 64: ~111 KB): any growth of a table or of the
    // geometry must fail HERE, not as a launch error on the GPU box
    static_assert(!STOP || GREEDY, "rollout_lstm_kernel: the stop rule belongs to the greedy episodes");
    constexpr size_t STOP_LDS = STOP ? RMT * 2 * STOP_WIN_MAX * sizeof(float) : 0;     // the stop rule's position rings
    static_assert(G::LDS + sizeof(xbuf) + sizeof(kbuf) + sizeof(hd) + sizeof(vis) + sizeof(es_s) + sizeof(trs) + sizeof(acc0) +
                      sizeof(env_tab) + STOP_LDS <= 160 * 1024, "rollout_lstm_kernel: LDS over 160 KB per workgroup");
    float* ring = nullptr;                                       // STOP: this env lane's [STOP_WIN_MAX][2] ring
    StopRing sr{0, 0};
    if constexpr (STOP) {
        __shared__ float rings[RMT * 2 * STOP_WIN_MAX];
        static_assert(sizeof(rings) == STOP_LDS, "stop rings");
        ring = rings + (threadIdx.x & 15) * 2 * STOP_WIN_MAX;
    }
    EnvParams P = P_arg;
    env_params_refresh(P);
    env_tables_to_lds(P, env_tab, threadIdx.x, H * 4);
    const int I = TREND ? 6 + P.trend_k : 6;   // observation features (TREND: 7 or 8, checked at launch)

    const float* w_ih = params;
    const float* w_hh = w_ih + 4 * H * I;
    const float* b_ih = w_hh + 4 * H * H;
    const float* b_hh = b_ih + 4 * H;
    const float* w_hd = b_hh + 4 * H;          // [NH][H]
    const float* b_hd = w_hd + NH * H;

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * RMT;
    const bool is_env_wave = (w == 0);   // wave 0: gate wave AND env role
    const int uw = 16 * w + j;                 // unit whose weight rows this lane holds / parks (A operand row)
    const int uo = 16 * w + 4 * kq;            // first of this lane's four units; its env is j
    const int nj = min(n0 + j, N - 1);
    const bool live = n0 + j < N;
    const int my_env = n0 + lane;              // env of lanes 0..15 of the env wave
    const bool env_lane = is_env_wave && lane < RMT && my_env < N;
    unsigned short* myvis = vis + (lane & 15) * NVIS;

    // ------------------------------------------------------------------ weights
    f16x8 wb[4][NS][2];                                                      // gate waves only
    f16x8* const w0f = reinterpret_cast<f16x8*>(w0p) + lane;                 // + ((q * NS + s) * 2 + piece) * 64
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float* src = w_hh + (size_t)(q * H + uw) * H + 32 * s + 8 * kq;
            const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 4);
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            f16x8 p0v, p1v;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                _Float16 p0, p1;
                split2h(v[i], p0, p1);
                p0v[i] = p0; p1v[i] = p1;
            }
            if (is_env_wave) {
                w0f[((q * NS + s) * 2 + 0) * 64] = p0v;
                w0f[((q * NS + s) * 2 + 1) * 64] = p1v;
            } else {
                wb[q][s][0] = p0v; wb[q][s][1] = p1v;
            }
        }
    float* const wxw = wxl + w * 512 + lane;                                 // this lane's W_ih fragments: + (2 q + s) * 64
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k = 2 * kq + s;
            wxw[(2 * q + s) * 64] = (k < I) ? w_ih[(size_t)(q * H + uw) * I + k] : 0.f;
        }
    for (int idx = threadIdx.x; idx < 4 * H; idx += H * 4) bl[idx] = b_ih[idx] + b_hh[idx];
    for (int idx = threadIdx.x; idx < 16 * H; idx += H * 4) {                // head weights as two fp16 planes
        const int hdx = idx / H, uu = idx % H;
        _Float16 p0, p1;
        split2h((hdx < NH) ? w_hd[(size_t)hdx * H + uu] : 0.f, p0, p1);
        unsigned short* d = whp + hdx * RS + uu;
        d[0] = h_bits(p0); d[PLANE] = h_bits(p1);
    }
    auto put_h = [&](const float (&hv)[4]) {                                 // split and park h[env j][uo .. uo+3]
        unsigned short b[2][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            _Float16 p0, p1;
            split2h(hv[r], p0, p1);
            b[0][r] = h_bits(p0); b[1][r] = h_bits(p1);
        }
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
            uint2 v;
            v.x = (unsigned)b[pc][0] | ((unsigned)b[pc][1] << 16);
            v.y = (unsigned)b[pc][2] | ((unsigned)b[pc][3] << 16);
            *reinterpret_cast<uint2*>(hpl + pc * PLANE + j * RS + uo) = v;
        }
    };
    float c_reg[4];
    {
        const float4 cv = *reinterpret_cast<const float4*>(B.c + (size_t)nj * H + uo);
        const float4 hv = *reinterpret_cast<const float4*>(B.h + (size_t)nj * H + uo);
        c_reg[0] = cv.x; c_reg[1] = cv.y; c_reg[2] = cv.z; c_reg[3] = cv.w;
        const float h_in[4] = {hv.x, hv.y, hv.z, hv.w};
        put_h(h_in);
        if constexpr (TREND && !GREEDY)                                      // h_prev of step 0: h comes in masked (keep[:, 0] = 1)
            if (B.stash && live) *reinterpret_cast<float4*>(B.stash + (size_t)(n0 + j) * T * (6 * H) + 5 * H + uo) = hv;
    }
    bool ran = true;                           // GREEDY: the env came in active (else its state is never written back)
    if (is_env_wave && lane < RMT) {
        const int n = min(my_env, N - 1);
        es_s[lane] = env_load(blob, n);
        for (int k = 0; k < NVIS; ++k) myvis[k] = blob.visited[(size_t)n * NVIS + k];
#pragma unroll
        for (int f = 0; f < 8; ++f) xbuf[lane * 8 + f] = f < I ? B.cur_obs[(size_t)n * I + f] : 0.f;
        if constexpr (GREEDY) {
            ran = my_env < N && B.active[n] != 0;
            kbuf[lane] = ran ? 1.f : 0.f;
            if constexpr (STOP)
                sr = stop_ring_load(ring, B.stop_win + (size_t)n * B.rule.window * 2, B.stop_cnt[n], B.rule.window);
        } else {
            kbuf[lane] = 1.f;
        }
    }
    lds_barrier();

    f32x4 acc[4];
    // One LDS address register for the four bias rows (+ q * H floats as the ds_read immediate): with a transparent lane offset
    // the compiler folds bl's > 64 KB offset into four separate address VGPRs, one of which the gate waves then spill and
    // reload inside the time loop -- and a scratch reload means s_waitcnt vmcnt(0), i.e. waiting for the stash stores.
    int bo = uo;
    asm volatile("" : "+v"(bo));
    const float* blu = bl + bo;
    auto bias_acc = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(blu + q * H);
            acc[q] = f32x4{v.x, v.y, v.z, v.w};
        }
    };
    // acc = bias + W_hh h^T of the step about to run: main products onto the bias, cross products apart, combined at the end
    auto recurrent = [&](auto&& wp0, auto&& wp1) {
        bias_acc();
        f32x4 acl[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acl[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned short* hrow = hpl + j * RS + 8 * kq;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const f16x8 a0 = *reinterpret_cast<const f16x8*>(hrow + 32 * s);
            const f16x8 a1 = *reinterpret_cast<const f16x8*>(hrow + PLANE + 32 * s);
#pragma unroll
            for (int q = 0; q < 4; ++q) acl[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wp1(q, s), a0, acl[q], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wp0(q, s), a0, acc[q], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) acl[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wp0(q, s), a1, acl[q], 0, 0, 0);
            asm volatile("" ::: "memory");               // one slab's h fragments at a time
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = acc[q] + acl[q] * H3_LO;
    };
    auto recurrent_regs = [&]() {
        recurrent([&](int q, int s) { return wb[q][s][0]; }, [&](int q, int s) { return wb[q][s][1]; });
    };
    // Wave 0's share of the recurrent product (units 0..15 of the four gates), computed by the gate waves from the
    // LDS copy of its weights while they would otherwise wait at barrier 2 for the env step.  Tile q goes to wave
    // 1 + q % (NW - 1), except that wave NW/2 -- wave 0's SIMD partner, whose MFMAs would serialise with the env chain's
    // VALU work (tools/simd_overlap_probe.hip) -- hands its tile to the next wave.  Same operand fragments and
    // accumulation order as recurrent(), so the bits do not change.
    auto recurrent_for_wave0 = [&]() {
        const f16x8* const wf = reinterpret_cast<const f16x8*>(w0p) + lane;
        const unsigned short* hrow = hpl + j * RS + 8 * kq;
        const int q0 = (NW == 8) ? (w < 4 ? w - 1 : (w == 5 ? 3 : 4)) : w - 1;
        for (int q = q0; q < 4; q += NW - 1) {
            const float4 bv = *reinterpret_cast<const float4*>(bl + q * H + 4 * kq);
            f32x4 e = {bv.x, bv.y, bv.z, bv.w}, el = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const f16x8 a0 = *reinterpret_cast<const f16x8*>(hrow + 32 * s);
                const f16x8 a1 = *reinterpret_cast<const f16x8*>(hrow + PLANE + 32 * s);
                const f16x8 p0 = wf[((q * NS + s) * 2 + 0) * 64], p1 = wf[((q * NS + s) * 2 + 1) * 64];
                el = __builtin_amdgcn_mfma_f32_16x16x32_f16(p1, a0, el, 0, 0, 0);
                e = __builtin_amdgcn_mfma_f32_16x16x32_f16(p0, a0, e, 0, 0, 0);
                el = __builtin_amdgcn_mfma_f32_16x16x32_f16(p0, a1, el, 0, 0, 0);
                asm volatile("" ::: "memory");
            }
            acc0[q * 64 + lane] = e + el * H3_LO;
        }
    };
    auto recurrent_lds = [&]() {
        recurrent([&](int q, int s) { return w0f[((q * NS + s) * 2 + 0) * 64]; },
                  [&](int q, int s) { return w0f[((q * NS + s) * 2 + 1) * 64]; });
    };
    // phase 1: input projection (two exact-f32 k-steps), gate pointwise, h_t parked, stash / y stored.
    // The recurrent state handed to the next rollout (B.h) is stored at the last real step; keep_fixup zeroes it
    // again if that step ended the episode.
    auto finish_cell = [&](int t, bool value_only) {
        const float2 ax = *reinterpret_cast<const float2*>(&xbuf[j * 8 + 2 * kq]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wxw[(2 * q) * 64], ax.x, acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wxw[(2 * q + 1) * 64], ax.y, acc[q], 0, 0, 0);
        }
        const bool st = !GREEDY && B.stash && !value_only && live;       // the update's first epoch reuses this forward pass
        const bool on = !GREEDY || kbuf[j] != 0.f;            // GREEDY: an ended env's h and c stay as they are
        const unsigned row = (unsigned)(n0 + j) * T + t;       // N*T*6H < 2^32 elements is checked at launch
        float* sp = B.stash + (size_t)row * (6 * H) + uo;
        float gi[4], gf[4], gg[4], cc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gi[r] = fast_sigmoid(acc[0][r]); gf[r] = fast_sigmoid(acc[1][r]); gg[r] = fast_tanh(acc[2][r]);
            cc[r] = gf[r] * c_reg[r] + gi[r] * gg[r];
        }
        if (st) {
            *reinterpret_cast<float4*>(sp) = float4{gi[0], gi[1], gi[2], gi[3]};
            *reinterpret_cast<float4*>(sp + H) = float4{gf[0], gf[1], gf[2], gf[3]};
            *reinterpret_cast<float4*>(sp + 2 * H) = float4{gg[0], gg[1], gg[2], gg[3]};
            *reinterpret_cast<float4*>(sp + 4 * H) = float4{c_reg[0], c_reg[1], c_reg[2], c_reg[3]};
        }
        float go[4], hh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            go[r] = fast_sigmoid(acc[3][r]);
            hh[r] = go[r] * fast_tanh(cc[r]);
            if (!value_only && on) c_reg[r] = cc[r];
        }
        if (on) put_h(hh);
        // GREEDY: h of every stepped step goes straight to B.h (4 more live VGPRs beside the gate waves' 128 weight registers spill)
        if (GREEDY && on && live)
            *reinterpret_cast<float4*>(B.h + (size_t)(n0 + j) * H + uo) = float4{hh[0], hh[1], hh[2], hh[3]};
        if (st) {
            *reinterpret_cast<float4*>(sp + 3 * H) = float4{go[0], go[1], go[2], go[3]};
            *reinterpret_cast<float4*>(B.y + (size_t)row * H + uo) = float4{hh[0], hh[1], hh[2], hh[3]};
            if constexpr (TREND)                                 // h_prev of step t + 1, unmasked (keep_fixup applies the mask)
                if (t + 1 < T) *reinterpret_cast<float4*>(sp + 6 * H + 5 * H) = float4{hh[0], hh[1], hh[2], hh[3]};
        }
        if (!GREEDY && t == T - 1 && live)
            *reinterpret_cast<float4*>(B.h + (size_t)(n0 + j) * H + uo) = float4{hh[0], hh[1], hh[2], hh[3]};
    };
    // episode ended at step t: the recurrent state restarts from zero (acc falls back to the bias)
    auto keep_fixup = [&](int t) {
        if (!GREEDY && kbuf[j] == 0.f) {
#pragma unroll
            for (int r = 0; r < 4; ++r) c_reg[r] = 0.f;
            bias_acc();
            if (t == T - 1 && live) *reinterpret_cast<float4*>(B.h + (size_t)(n0 + j) * H + uo) = float4{0.f, 0.f, 0.f, 0.f};
            if constexpr (TREND)                                 // h_prev of step t + 1 after the restart mask
                if (B.stash && t + 1 < T && live)
                    *reinterpret_cast<float4*>(B.stash + ((size_t)(n0 + j) * T + t + 1) * (6 * H) + 5 * H + uo) =
                        float4{0.f, 0.f, 0.f, 0.f};
        }
    };

    // The transition of step t leaves for HBM from the last gate wave, not from wave 0 (whose heads -> action -> env chain
    // paces the kernel): wave 0 parks it in trs ([action, reward, V, logp, done, flags, keep, -] | [obs 6, source x, y] |
    // [info 8] | [logits 5]) and the last gate wave stores it right after barrier 2.  trs is rewritten only after barrier 1
    // of the next step, which that wave passes after its reads have completed.  (Spreading the stores over three gate
    // waves measured slower, 792 vs 773 us per rollout.)
    auto store_transition = [&](int t) {
        if (GREEDY && lane < RMT && n0 + lane < N) {                   // [action, -, -, -, -, flags, -, -] | [obs 6, agent_pos 2]
            const size_t row = (size_t)(n0 + lane) * T + t;
            const float* to = trs + RMT * 8 + lane * 8;
            if constexpr (TREND) {                                      // [action, agent_pos 2, -, -, flags, -, -] | [obs 8]
#pragma unroll
                for (int f = 0; f < 8; ++f) if (f < I) B.obs[row * I + f] = to[f];
                B.pos[row * 2] = trs[lane * 8 + 1];
                B.pos[row * 2 + 1] = trs[lane * 8 + 2];
            } else {
#pragma unroll
                for (int f = 0; f < 6; ++f) B.obs[row * 6 + f] = to[f];
                B.pos[row * 2] = to[6];
                B.pos[row * 2 + 1] = to[7];
            }
            B.act[row] = __float_as_int(trs[lane * 8]);
            B.flags[row] = (uint8_t)__float_as_int(trs[lane * 8 + 5]);
        } else if (!GREEDY && lane < RMT && n0 + lane < N) {
            const size_t row = (size_t)(n0 + lane) * T + t;
            const float* tq = trs + lane * 8;
            if constexpr (TREND) {                                      // ... | [obs 8] | [info 8] | [logits 5, source x, y]
#pragma unroll
                for (int f = 0; f < 8; ++f) if (f < I) B.obs[row * I + f] = trs[RMT * 8 + lane * 8 + f];
            } else {
#pragma unroll
                for (int f = 0; f < 6; ++f) B.obs[row * 6 + f] = trs[RMT * 8 + lane * 8 + f];
            }
            B.act[row] = __float_as_int(tq[0]);
            B.rew[row] = tq[1];
            B.val[row] = tq[2];
            B.logp[row] = tq[3];
            B.done[row] = tq[4];
            B.flags[row] = (uint8_t)__float_as_int(tq[5]);
            B.keep[row] = tq[6];
            if (B.heads) {
#pragma unroll
                for (int a = 0; a < NA; ++a) B.heads[row * NH + a] = trs[3 * RMT * 8 + lane * 8 + a];
                B.heads[row * NH + NA] = tq[2];
            }
            if (B.info) {
#pragma unroll
                for (int f = 0; f < 8; ++f) B.info[row * 10 + f] = trs[2 * RMT * 8 + lane * 8 + f];
                constexpr int SRC = TREND ? 3 * RMT * 8 + 5 : RMT * 8 + 6;
                B.info[row * 10 + 8] = trs[SRC + lane * 8];
                B.info[row * 10 + 9] = trs[SRC + lane * 8 + 1];
            }
        }
    };

    const int steps = T + (B.last_val ? 1 : 0);   // one extra value-only pass for V(s_T)
    if (!is_env_wave) {
        // ------------------------------------------------------------------ gate waves
        recurrent_regs();
        lds_barrier();     // every wave has read h_{-1} before step 0 overwrites the planes
        for (int t = 0; t < steps; ++t) {
            const bool value_only = (t == T);
            finish_cell(t, value_only);
            lds_barrier();                       // barrier 1: h_t visible
            if (!value_only && t + 1 < steps) {
                recurrent_regs();                // bias + W_hh h_t for step t+1
                recurrent_for_wave0();
            }
            lds_barrier();                       // barrier 2: x_{t+1}, keep_{t+1} visible; reads of h_t done
            if (!value_only) {
                keep_fixup(t);
                if (w == NW - 1) store_transition(t);
            }
        }
    } else {
        // ------------------------------------------------------------------ wave 0: gate wave + env role
        recurrent_lds();
        lds_barrier();
        float bh[NH];                            // head biases: read once (a load inside the loop could not be hoisted past the stores)
#pragma unroll
        for (int a = 0; a < NH; ++a) bh[a] = b_hd[a];
        PROF_DECL(8);
        for (int t = 0; t < steps; ++t) {
            const bool value_only = (t == T);
            PROF_MARK(7);
            finish_cell(t, value_only);
            PROF_MARK(0);
            // the step's action-independent part (sampling uniform, the wind displacement from its two normals), computed
            // while the other waves finish their cells: off the heads -> action -> env chain that paces the kernel
            uint32_t u_act = 0;
            double wind_x = 0.0, wind_y = 0.0;
            if (lane < RMT && !value_only) {
                const int eg = P.env_offset + my_env;
                const size_t row = (size_t)min(my_env, N - 1) * T + t;
                if (!GREEDY && !B.forced_act) u_act = philox4x32_10(P.seed, (uint32_t)t, (uint32_t)eg, (uint32_t)iter, RNG_ACTION).x;
                env_step_draw_wind(P, eg, es_s[lane], B.noise, row, wind_x, wind_y);
            }
            PROF_MARK(6);
            lds_barrier();                       // barrier 1: h_t visible
            PROF_MARK(1);
            // heads of h_t: D[head 4 kq + r][env j] = W_head h_t^T, three piece products per slab
            f32x4 ha = {0.f, 0.f, 0.f, 0.f}, hb2 = ha;
            {
                const unsigned short* hrow = hpl + j * RS + 8 * kq;
                const unsigned short* wrow = whp + j * RS + 8 * kq;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    f16x8 a[2], bw[2];
#pragma unroll
                    for (int pc = 0; pc < 2; ++pc) {
                        a[pc] = *reinterpret_cast<const f16x8*>(hrow + pc * PLANE + 32 * s);
                        bw[pc] = *reinterpret_cast<const f16x8*>(wrow + pc * PLANE + 32 * s);
                    }
                    hb2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bw[1], a[0], hb2, 0, 0, 0);
                    ha = __builtin_amdgcn_mfma_f32_16x16x32_f16(bw[0], a[0], ha, 0, 0, 0);
                    hb2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bw[0], a[1], hb2, 0, 0, 0);
                }
                ha = ha + hb2 * H3_LO;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) hd[j * 16 + 4 * kq + r] = ha[r];
            __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): the hd tile is written (single wave)
            __builtin_amdgcn_wave_barrier();
            PROF_MARK(2);
            if (lane < RMT) {
                float z[NA];
#pragma unroll
                for (int a = 0; a < NA; ++a) z[a] = hd[lane * 16 + a] + bh[a];
                const float V = hd[lane * 16 + NA] + bh[NA];
                if (value_only) {
                    if (env_lane) B.last_val[my_env] = V;
                } else if constexpr (GREEDY) {
                    // argmax of the logits (torch.argmax: the first of equal maxima), then the environment step without reset.
                    // argmax_first (loss_core.h) written out: through the helper the h = 64 TREND form of this branch gains a
                    // VGPR and 47 SGPR-spill lane moves (profiles/step_core_static_table.md)
                    const bool on = kbuf[lane] != 0.f;
                    int a_sel = 0;
                    float m = z[0];
                    bool bad = (z[0] != z[0]);
#pragma unroll
                    for (int a = 1; a < NA; ++a) {
                        bad |= (z[a] != z[a]);
                        if (z[a] > m) { m = z[a]; a_sel = a; }
                    }
                    if (bad && env_lane && on) atomicAdd(B.nan_count, 1);
                    float* tr = trs + lane * 8;
                    float* to = trs + RMT * 8 + lane * 8;
                    if (on) {
                        EnvState es = es_s[lane];
                        StepOut so;
                        env_step_core(P, P.env_offset + my_env, es, myvis, a_sel, wind_x, wind_y, so);
                        bool hit = false;                       // STOP: the rule fires on this step
                        if constexpr (STOP) {
                            float rv;
                            hit = stop_rule_step(B.rule, ring, sr, es.px, es.py, so.obs[2], B.rule_val != nullptr, rv);
                            if (B.rule_val && env_lane) B.rule_val[(size_t)my_env * T + t] = rv;
                        }
                        tr[0] = __int_as_float(a_sel);
                        tr[5] = __int_as_float(step_flags(so, hit));
                        if constexpr (TREND) {
#pragma unroll
                            for (int f = 0; f < 8; ++f) {
                                const float v = f < I ? so.obs[f] : 0.f;
                                to[f] = v; xbuf[lane * 8 + f] = v;
                            }
                            tr[1] = es.px;
                            tr[2] = es.py;
                        } else {
#pragma unroll
                            for (int f = 0; f < 6; ++f) { to[f] = so.obs[f]; xbuf[lane * 8 + f] = so.obs[f]; }
                            to[6] = es.px;
                            to[7] = es.py;
                        }
                        es_s[lane] = es;
                        if (so.done || hit) kbuf[lane] = 0.f;
                    } else {
                        tr[0] = __int_as_float(-1);
                        tr[5] = __int_as_float(4);
#pragma unroll
                        for (int f = 0; f < 8; ++f) to[f] = 0.f;
                        if constexpr (TREND) tr[1] = tr[2] = 0.f;
                        if constexpr (STOP)
                            if (B.rule_val && env_lane) B.rule_val[(size_t)my_env * T + t] = __builtin_nanf("");
                    }
                    (void)V;
                } else {
                    const int eg = P.env_offset + my_env;
                    const size_t row = (size_t)min(my_env, N - 1) * T + t;
                    float lp;
                    bool bad;
                    const int a_sel = rollout_draw<NA>(z, B.forced_act, row, [&]() { return u_act; }, lp, bad);
                    if (bad && env_lane) atomicAdd(B.nan_count, 1);
                    PROF_MARK(3);
                    // environment step (f64, env_core.h) + auto reset
                    EnvState es = es_s[lane];
                    StepOut so;
                    env_step_core(P, eg, es, myvis, a_sel, wind_x, wind_y, so);
                    PROF_MARK(4);
                    // park the transition in LDS for store_transition()
                    float* tr = trs + lane * 8;
                    tr[0] = __int_as_float(a_sel);
                    tr[1] = (float)so.reward;
                    tr[2] = V;
                    tr[3] = lp;
                    tr[4] = so.done ? 1.f : 0.f;
                    tr[5] = __int_as_float(step_flags(so));
                    tr[6] = kbuf[lane];
                    if (B.heads) {
#pragma unroll
                        for (int a = 0; a < NA; ++a) trs[3 * RMT * 8 + lane * 8 + a] = z[a];
                    }
                    if (B.info) {
#pragma unroll
                        for (int f = 0; f < 5; ++f) trs[2 * RMT * 8 + lane * 8 + f] = (float)so.info[f];
                        trs[2 * RMT * 8 + lane * 8 + 5] = so.obs[2];
                        trs[2 * RMT * 8 + lane * 8 + 6] = es.px;          // agent_pos after the move (before any auto-reset)
                        trs[2 * RMT * 8 + lane * 8 + 7] = es.py;
                    }
                    constexpr int OW = TREND ? 8 : 6;                     // TREND: the whole x row, source beside the logits
                    constexpr int SRC = TREND ? 3 * RMT * 8 + 5 : RMT * 8 + 6;
                    float ob_old[OW];
#pragma unroll
                    for (int f = 0; f < OW; ++f) ob_old[f] = xbuf[lane * 8 + f];
#pragma unroll
                    for (int f = 0; f < OW; ++f) trs[RMT * 8 + lane * 8 + f] = ob_old[f];
                    trs[SRC + lane * 8] = (float)es.sx;                   // source of the episode this step belongs to
                    trs[SRC + lane * 8 + 1] = (float)es.sy;
                    env_auto_reset(P, eg, es, myvis, so);
#pragma unroll
                    for (int f = 0; f < OW; ++f) xbuf[lane * 8 + f] = f < I ? so.obs[f] : 0.f;
                    es_s[lane] = es;
                    kbuf[lane] = so.done ? 0.f : 1.f;
                }
            }
            PROF_MARK(5);
            lds_barrier();                       // barrier 2: the gate waves have left bias + W_hh h_t of this wave's units in acc0
            if (!value_only && t + 1 < steps) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = acc0[q * 64 + lane];
            }
            if (!value_only) keep_fixup(t);
        }
        PROF_FLUSH(g_roll_prof, 8, blockIdx.x == 0 && threadIdx.x == 0);
    }
    // ------------------------------------------------------------------ write back persistent state
    if (live) *reinterpret_cast<float4*>(B.c + (size_t)(n0 + j) * H + uo) = float4{c_reg[0], c_reg[1], c_reg[2], c_reg[3]};
    if (GREEDY && env_lane) B.active[my_env] = kbuf[lane] != 0.f ? 1 : 0;
    if (env_lane && ran) {
        env_store(blob, my_env, es_s[lane]);
        for (int k = 0; k < NVIS; ++k) blob.visited[(size_t)my_env * NVIS + k] = myvis[k];
#pragma unroll
        for (int f = 0; f < (TREND ? 8 : 6); ++f) if (f < I) B.cur_obs[(size_t)my_env * I + f] = xbuf[lane * 8 + f];
        if constexpr (STOP)
            B.stop_cnt[my_env] = stop_ring_store(ring, sr, B.stop_win + (size_t)my_env * B.rule.window * 2, B.rule.window);
    }
}

template <int H, bool GREEDY = false, bool STOP = false, bool TREND = false>
static int launch_rollout(const EnvParams& P, EnvBlob blob, int N, int T, uint64_t iter, const float* params,
                          const RolloutBufs& B, hipStream_t st) {
    const dim3 grid((N + RMT - 1) / RMT), block(H * 4);
    UAV_CHECK_HIP(uav_dyn_lds(reinterpret_cast<const void*>(&rollout_lstm_kernel<H, 5, GREEDY, STOP, TREND>), (int)RGeom<H>::LDS));
    hipLaunchKernelGGL((rollout_lstm_kernel<H, 5, GREEDY, STOP, TREND>), grid, block, RGeom<H>::LDS, st, P, blob, N, T, iter, params, B);
    UAV_LAUNCH_CHECK();
    return 0;
}

// ---- the tail of ONE step of a step-wise rollout (policies the fused rollout kernels do not cover: stacked layers, h = 256)
// as one launch: policy heads of the top layer's y_t, action sample, environment step, PPOBuffer.store, next observation into
// the sequence array -- five launches (rows-dot GEMM 14.3 us, uav_policy_sample_at 4.3, uav_env_step 8.6, uav_store_transition
// 2.9, a copy 3.4 at 4096 envs, each mostly launch and memory latency) that all sit on the step's dependency chain.
// A wave takes four envs: the heads by rows4_heads (rows_dot_core.h: rows_dot_kernel's sums, so heads[:, t] is bit for bit
// uav_gemm_f32's), then lanes 0..3 each carry one env through uav_policy_sample_at's draw (sample_categorical, loss_core.h)
// and env_step + env_auto_reset (env_core.h).  4096 envs = 1024 waves = one per SIMD.
template <int A>
__global__ __launch_bounds__(256) void rollout_tail_kernel(
    EnvParams P, EnvBlob b, int n, const float* __restrict__ y, int64_t ldy, int K, const float* __restrict__ w_head,
    const float* __restrict__ b_head, float* __restrict__ heads, int64_t ldh, int T, int t, uint64_t seed, uint64_t counter,
    int64_t index_offset, const int32_t* __restrict__ forced, const double* __restrict__ noise, int32_t* __restrict__ act_out,
    float* __restrict__ cur_obs, float* __restrict__ obs_seq, float* __restrict__ keep, int32_t* __restrict__ act_buf,
    float* __restrict__ val_buf, float* __restrict__ logp_buf, float* __restrict__ keep_buf, float* __restrict__ rew_buf,
    float* __restrict__ done_buf, uint8_t* __restrict__ flags_buf, int32_t* __restrict__ nan_count) {
    const int lane = threadIdx.x & 63;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    if (m0 >= n) return;
    env_params_refresh(P);
    float z[A + 1];
    rows4_heads<A + 1>(w_head, b_head, y, ldy, m0, n, K, lane, z);
    const int64_t i64 = m0 + lane;
    if (lane >= 4 || i64 >= n) return;
    const int i = (int)i64;
#pragma unroll
    for (int o = 0; o <= A; ++o) heads[i64 * ldh + o] = z[o];
    // ---- uav_policy_sample_at
    float p[A], qa;
    bool bad;
    int a = sample_categorical<A>(z, p, nullptr, seed, counter, index_offset + i, forced ? &forced[i] : nullptr, qa, bad);
    if (bad) atomicAdd(nan_count, 1);
    const int64_t col = i64 * T + t;
    act_out[i] = a;
    act_buf[col] = a;
    logp_buf[col] = logf(fminf(fmaxf(qa, F32_EPS), 1.0f - F32_EPS));
    val_buf[col] = z[A];
    // ---- uav_env_step
    EnvState s = env_load(b, i);
    unsigned short* vis = b.visited + (size_t)i * NVIS;
    const int eg = P.env_offset + i;
    a = a < 0 ? 0 : (a > 4 ? 4 : a);
    StepOut o;
    env_step(P, eg, s, vis, a, noise, (size_t)i, o);
    const float d = o.done ? 1.f : 0.f;
    const uint8_t fl = (uint8_t)step_flags(o);
    const float rw = (float)o.reward;
    env_auto_reset(P, eg, s, vis, o);
    env_store(b, i, s);
    // ---- uav_store_transition, and the observation step t + 1 starts from
    keep_buf[col] = keep[i];
    rew_buf[col] = rw;
    done_buf[col] = d;
    flags_buf[col] = fl;
    keep[i] = 1.0f - d;
    const int od = 6 + P.trend_k;
    for (int k = 0; k < od; ++k) {
        cur_obs[(size_t)i * od + k] = o.obs[k];
        if (t + 1 < T) obs_seq[((size_t)i * T + t + 1) * od + k] = o.obs[k];
    }
}

extern "C" int uav_rollout_tail(uav_ctx* ctx, void* env_state, int n_env, const uav_env_cfg* cfg, const float* y, int64_t y_stride,
                                int hidden, const float* w_head, const float* b_head, int n_act, float* heads, int64_t heads_stride,
                                int T, int t, uint64_t seed, uint64_t counter, int64_t index_offset, const int32_t* forced_act,
                                const double* noise, int32_t* act_out, float* cur_obs, float* obs_seq, float* keep,
                                int32_t* act_buf, float* val_buf, float* logp_buf, float* keep_buf, float* rew_buf, float* done_buf,
                                uint8_t* flags_buf, int32_t* nan_count, uav_stream stream) {
    UAV_REQUIRE(ctx && env_state && y && w_head && b_head && heads && act_out && cur_obs && obs_seq && keep && act_buf && val_buf &&
                logp_buf && keep_buf && rew_buf && done_buf && flags_buf && nan_count, "uav_rollout_tail: NULL argument");
    UAV_REQUIRE(n_env > 0 && T > 0 && t >= 0 && t < T, "uav_rollout_tail: n_env=%d T=%d t=%d", n_env, T, t);
    UAV_REQUIRE(hidden >= 4 && hidden <= 256 && hidden % 4 == 0 && y_stride % 4 == 0 && y_stride >= hidden &&
                (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (reinterpret_cast<uintptr_t>(w_head) & 15) == 0,
                "uav_rollout_tail: hidden %d (a multiple of 4 up to 256), y rows 16-byte aligned", hidden);
    UAV_REQUIRE(heads_stride > n_act, "uav_rollout_tail: heads_stride=%lld n_act=%d", (long long)heads_stride, n_act);
    EnvParams P;
    int rc = env_params_from_cfg(ctx, cfg, n_env, P);
    if (rc) return rc;
    const dim3 grid((unsigned)((n_env + 15) / 16));
#define LAUNCH_T(A_)                                                                                                              \
    hipLaunchKernelGGL(rollout_tail_kernel<A_>, grid, dim3(256), 0, as_stream(stream), P, env_blob_view(env_state, n_env), n_env, \
                       y, y_stride, hidden, w_head, b_head, heads, heads_stride, T, t, seed, counter, index_offset, forced_act,   \
                       noise, act_out, cur_obs, obs_seq, keep, act_buf, val_buf, logp_buf, keep_buf, rew_buf, done_buf,           \
                       flags_buf, nan_count)
    switch (n_act) {
        case 2: LAUNCH_T(2); break;
        case 3: LAUNCH_T(3); break;
        case 4: LAUNCH_T(4); break;
        case 5: LAUNCH_T(5); break;
        case 6: LAUNCH_T(6); break;
        default: UAV_REQUIRE(false, "uav_rollout_tail: n_act=%d unsupported (2..6)", n_act);
    }
#undef LAUNCH_T
    UAV_LAUNCH_CHECK();
    return 0;
}

extern "C" int uav_rollout(uav_ctx* ctx, void* env_state, int n_env, const uav_env_cfg* cfg, int policy_kind,
                           const float* params, int hidden, int horizon, uint64_t iter, float* cur_obs, float* h,
                           float* c, float* obs, int32_t* act, float* rew, float* val, float* logp, float* done,
                           uint8_t* flags, float* keep, float* last_val, const int32_t* forced_act,
                           const double* noise, int32_t* nan_count, float* stash, float* y_out, float* info,
                           float* heads, uav_stream stream) {
    UAV_REQUIRE(ctx && env_state && params && cur_obs && obs && act && rew && val && logp && done && flags && nan_count,
                "uav_rollout: NULL argument");
    UAV_REQUIRE(n_env > 0 && horizon > 0, "uav_rollout: n_env=%d horizon=%d", n_env, horizon);
    UAV_REQUIRE(policy_kind >= 0 && policy_kind <= 2, "uav_rollout: policy_kind %d (0 = MLP, 1 = LSTM, 2 = MLP with 6 + trend_k inputs)",
                policy_kind);
    if (policy_kind != 1) {      // the reference's MLP policy (2: with the trend channels as inputs): csrc/mlp_rollout.hip
        UAV_REQUIRE(!stash && !y_out, "uav_rollout: stash / y_out belong to the LSTM policy");
        return launch_rollout_mlp(ctx, env_state, n_env, cfg, params, horizon, iter, cur_obs, obs, act, rew, val, logp, done,
                                  flags, last_val, forced_act, noise, nan_count, info, heads, policy_kind == 2, as_stream(stream));
    }
    UAV_REQUIRE(h && c && keep, "uav_rollout: LSTM policy needs h, c, keep");
    EnvParams P;
    int rc = env_params_from_cfg(ctx, cfg, n_env, P);
    if (rc) return rc;
    UAV_REQUIRE((stash == nullptr) == (y_out == nullptr), "uav_rollout: stash and y_out go together");
    UAV_REQUIRE(!stash || (int64_t)n_env * horizon * 6 * hidden < (1ll << 32), "uav_rollout: stash rows exceed 32-bit offsets");
    RolloutBufs B{cur_obs, h, c, obs, act, rew, val, logp, done, flags, keep, last_val, forced_act, noise, nan_count, info, heads, stash, y_out};
    EnvBlob blob = env_blob_view(env_state, n_env);
    const bool trend = P.trend_k != 0;       // 6 + trend_k features in cur_obs, obs and w_ih: the TREND form of the kernel
    switch (hidden) {
        case 64: return trend ? launch_rollout<64, false, false, true>(P, blob, n_env, horizon, iter, params, B, as_stream(stream))
                              : launch_rollout<64>(P, blob, n_env, horizon, iter, params, B, as_stream(stream));
        case 128: return trend ? launch_rollout<128, false, false, true>(P, blob, n_env, horizon, iter, params, B, as_stream(stream))
                               : launch_rollout<128>(P, blob, n_env, horizon, iter, params, B, as_stream(stream));
    }
    UAV_REQUIRE(false, "uav_rollout: hidden=%d unsupported (64, 128)", hidden);
}

// uav_greedy_episodes and uav_greedy_episodes_stop: `rule` NULL = the plain greedy episodes
static int greedy_episodes_impl(const char* who, uav_ctx* ctx, void* env_state, int n_env, const uav_env_cfg* cfg, int policy_kind,
                                const float* params, int hidden, int steps, float* cur_obs, float* h, float* c, uint8_t* active,
                                const double* noise, int32_t* act, float* obs, float* pos, uint8_t* flags, int32_t* nan_count,
                                const uav_stop_rule* rule, float* stop_win, int32_t* stop_cnt, float* rule_val, hipStream_t st) {
    UAV_REQUIRE(ctx && env_state && params && cur_obs && active && act && obs && pos && flags && nan_count,
                "%s: NULL argument", who);
    UAV_REQUIRE(n_env > 0 && steps > 0, "%s: n_env=%d steps=%d", who, n_env, steps);
    UAV_REQUIRE(policy_kind >= 0 && policy_kind <= 2, "%s: policy_kind %d (0 = MLP, 1 = LSTM, 2 = MLP with 6 + trend_k inputs)", who,
                policy_kind);
    UAV_REQUIRE(ctx->mode.arith == UAV_ARITH_FP16X3,
                "%s: the fused greedy kernels exist in the fp16x3 arithmetic only (handle mode %d)", who, ctx->mode.arith);
    StopRule R{};
    if (rule) {
        UAV_REQUIRE(rule->window >= 1 && rule->window <= STOP_WIN_MAX, "%s: rule window=%d (1 .. %d)", who, rule->window,
                    STOP_WIN_MAX);
        UAV_REQUIRE(stop_win && stop_cnt, "%s: NULL stop_win / stop_cnt (the rule's window buffers)", who);
        R = StopRule{rule->window, rule->pos_std_max, rule->conc_coef, rule->conc_peak, rule->conc_min};
    }
    EnvParams P;
    int rc = env_params_from_cfg(ctx, cfg, n_env, P);
    if (rc) return rc;
    UAV_REQUIRE(policy_kind != 0 || P.trend_k == 0, "%s: trend_k=%d unsupported (the fused MLP kernels take 6 observation features)",
                who, P.trend_k);
    UAV_REQUIRE((int64_t)n_env * steps * (6 + P.trend_k) < (1ll << 31), "%s: n_env * steps too large", who);
    if (policy_kind != 1)
        return rule ? launch_greedy_mlp_stop(P, env_state, n_env, params, steps, cur_obs, active, noise, act, obs, pos, flags,
                                             nan_count, R, stop_win, stop_cnt, rule_val, st)
                    : launch_greedy_mlp(P, env_state, n_env, params, steps, cur_obs, active, noise, act, obs, pos, flags, nan_count, st);
    UAV_REQUIRE(h && c, "%s: LSTM policy needs h, c", who);
    RolloutBufs B{cur_obs, h, c, obs, act, nullptr, nullptr, nullptr, nullptr, flags, nullptr, nullptr, nullptr, noise, nan_count,
                  nullptr, nullptr, nullptr, nullptr, active, pos, stop_win, stop_cnt, rule_val, R};
    EnvBlob blob = env_blob_view(env_state, n_env);
#define LAUNCH_G(H_)                                                                                      \
    (P.trend_k ? (rule ? launch_rollout<H_, true, true, true>(P, blob, n_env, steps, 0, params, B, st)        \
                       : launch_rollout<H_, true, false, true>(P, blob, n_env, steps, 0, params, B, st))      \
               : (rule ? launch_rollout<H_, true, true>(P, blob, n_env, steps, 0, params, B, st)              \
                       : launch_rollout<H_, true>(P, blob, n_env, steps, 0, params, B, st)))
    switch (hidden) {
        case 64: return LAUNCH_G(64);
        case 128: return LAUNCH_G(128);
    }
#undef LAUNCH_G
    UAV_REQUIRE(false, "%s: hidden=%d unsupported by the fused kernel (64, 128)", who, hidden);
}

extern "C" int uav_greedy_episodes(uav_ctx* ctx, void* env_state, int n_env, const uav_env_cfg* cfg, int policy_kind,
                                   const float* params, int hidden, int steps, float* cur_obs, float* h, float* c,
                                   uint8_t* active, const double* noise, int32_t* act, float* obs, float* pos, uint8_t* flags,
                                   int32_t* nan_count, uav_stream stream) {
    return greedy_episodes_impl("uav_greedy_episodes", ctx, env_state, n_env, cfg, policy_kind, params, hidden, steps, cur_obs, h, c,
                                active, noise, act, obs, pos, flags, nan_count, nullptr, nullptr, nullptr, nullptr, as_stream(stream));
}

extern "C" int uav_greedy_episodes_stop(uav_ctx* ctx, void* env_state, int n_env, const uav_env_cfg* cfg, int policy_kind,
                                        const float* params, int hidden, int steps, float* cur_obs, float* h, float* c,
                                        uint8_t* active, const double* noise, int32_t* act, float* obs, float* pos, uint8_t* flags,
                                        int32_t* nan_count, const uav_stop_rule* rule, float* stop_win, int32_t* stop_cnt,
                                        float* rule_val, uav_stream stream) {
    UAV_REQUIRE(rule, "uav_greedy_episodes_stop: NULL rule");
    return greedy_episodes_impl("uav_greedy_episodes_stop", ctx, env_state, n_env, cfg, policy_kind, params, hidden, steps, cur_obs,
                                h, c, active, noise, act, obs, pos, flags, nan_count, rule, stop_win, stop_cnt, rule_val,
                                as_stream(stream));
}

// ---- the same rule, one step, for envs stepped by other means (uav_stop_stability): one thread per env, the window in place
__global__ __launch_bounds__(256) void stop_stability_kernel(StopRule R, int n, const float* __restrict__ pos,
                                                             const float* __restrict__ obs2, int64_t obs2_stride,
                                                             const uint8_t* __restrict__ active, float* __restrict__ stop_win,
                                                             int32_t* __restrict__ stop_cnt, uint8_t* __restrict__ stop,
                                                             float* __restrict__ value) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (active && active[i] == 0) {
        stop[i] = 0;
        value[i] = __builtin_nanf("");
        return;
    }
    float ring[2 * STOP_WIN_MAX];
    float* win = stop_win + (size_t)i * R.window * 2;
    StopRing sr = stop_ring_load(ring, win, stop_cnt[i], R.window);
    float v;
    const bool hit = stop_rule_step(R, ring, sr, pos[2 * (size_t)i], pos[2 * (size_t)i + 1], obs2[(size_t)i * obs2_stride], true, v);
    stop_cnt[i] = stop_ring_store(ring, sr, win, R.window);
    stop[i] = hit ? 1 : 0;
    value[i] = v;
}

extern "C" int uav_stop_stability(uav_ctx* ctx, int n, const uav_stop_rule* rule, const float* pos, const float* obs2,
                                  int64_t obs2_stride, const uint8_t* active, float* stop_win, int32_t* stop_cnt, uint8_t* stop,
                                  float* value, uav_stream stream) {
    UAV_REQUIRE(ctx && rule && pos && obs2 && stop && value, "uav_stop_stability: NULL argument");
    UAV_REQUIRE(n > 0 && obs2_stride >= 1, "uav_stop_stability: n=%d obs2_stride=%lld", n, (long long)obs2_stride);
    UAV_REQUIRE(rule->window >= 1 && rule->window <= STOP_WIN_MAX, "uav_stop_stability: rule window=%d (1 .. %d)", rule->window,
                STOP_WIN_MAX);
    UAV_REQUIRE(stop_win && stop_cnt, "uav_stop_stability: NULL stop_win / stop_cnt (the rule's window buffers)");
    const StopRule R{rule->window, rule->pos_std_max, rule->conc_coef, rule->conc_peak, rule->conc_min};
    hipLaunchKernelGGL(stop_stability_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), R, n, pos, obs2, obs2_stride,
                       active, stop_win, stop_cnt, stop, value);
    UAV_LAUNCH_CHECK();
    return 0;
}
