// loss_core.h -- the per-sample arithmetic of the clipped-PPO loss (train_ppo2.0.py:55-83), shared by the elementwise
// loss kernels (loss.hip) and the fused MLP update (mlp_update.hip), so every path rounds alike.
#pragma once
#include "common.h"
#include "philox.h"

constexpr float F32_EPS = 1.1920928955078125e-07f;

template <int A>
__device__ __forceinline__ void softmax_row(const float* z, float* p) {
    float m = z[0];
#pragma unroll
    for (int k = 1; k < A; ++k) m = fmaxf(m, z[k]);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        p[k] = expf(z[k] - m);
        s += p[k];
    }
#pragma unroll
    for (int k = 0; k < A; ++k) p[k] = p[k] / s;
}

// One Categorical(probs) draw from logits z[A] (train_ppo2.0.py:171-173; torch.multinomial's inverse-CDF semantics over the
// normalised probabilities): p[] = softmax(z), the action (forced, from a given uniform, or from the counter RNG keyed
// (seed; step-in-rollout, GLOBAL env index, iteration) like the fused rollout kernels, so a job draws the same actions however
// its envs are sharded over ranks and whichever rollout path runs it), qa = its normalised probability, bad = a NaN probability.
template <int A>
__device__ __forceinline__ int sample_categorical(const float* z, float* p, const float* u, uint64_t seed, uint64_t counter,
                                                  int64_t env_global, const int32_t* forced, float& qa, bool& bad) {
    softmax_row<A>(z, p);
    float psum = 0.f;
    bad = false;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        psum += p[k];
        bad |= (p[k] != p[k]);
    }
    int a;
    if (forced) {
        a = *forced;
    } else {
        float uu;
        if (u) uu = *u;
        else {
            const Philox4 r = philox4x32_10(seed, (uint32_t)counter, (uint32_t)env_global, (uint32_t)(counter >> 32), RNG_ACTION);
            uu = u01_f32(r.x);
        }
        float cdf = 0.f;
        a = A - 1;
        const float target = uu * psum;
#pragma unroll
        for (int k = 0; k < A; ++k) {
            cdf += p[k];
            if (target < cdf) { a = k; break; }
        }
    }
    qa = 0.f;
#pragma unroll
    for (int k = 0; k < A; ++k)
        if (k == a) qa = p[k] / psum;
    return a;
}

// ---- the fused rollouts' flavour (rollout_lstm_kernel, rollout_mlp_kernel).  Two flavours exist on purpose: the draw above
// uses libm's expf / logf and keys the counter RNG by (counter, env), because uav_policy_sample and the step-wise tail must
// agree with the loss kernels' softmax bit for bit; the fused kernels sit on the chain that paces a rollout and use the
// hardware __expf / __logf, with the word keyed (step, env, iteration) by the kernel.  Their log-probs differ in the last bits,
// and each route's update recomputes them with softmax_row either way.

// argmax of logits (torch.argmax: the first of equal maxima); bad = a NaN logit
template <int A>
__device__ __forceinline__ int argmax_first(const float (&z)[A], bool& bad) {
    int a_sel = 0;
    float m = z[0];
    bad = (z[0] != z[0]);
#pragma unroll
    for (int a = 1; a < A; ++a) {
        bad |= (z[a] != z[a]);
        if (z[a] > m) { m = z[a]; a_sel = a; }
    }
    return a_sel;
}

// softmax + Categorical(probs) sample / log_prob (train_ppo2.0.py:161-163,189).  forced: NULL, or the action is forced[row];
// u_word(): the step's 32-bit Philox word, called only when the action is drawn (a kernel that formed it earlier returns it).
// Returns the action in 0 .. A-1; lp = log of its normalised probability clamped to [eps, 1 - eps]; bad = a NaN probability.
template <int A, class U>
__device__ __forceinline__ int rollout_draw(const float (&z)[A], const int32_t* __restrict__ forced, size_t row, U&& u_word,
                                            float& lp, bool& bad) {
    float p[A];
    float m = z[0];
#pragma unroll
    for (int a = 1; a < A; ++a) m = fmaxf(m, z[a]);
    float ssum = 0.f;
#pragma unroll
    for (int a = 0; a < A; ++a) { p[a] = __expf(z[a] - m); ssum += p[a]; }
    float psum = 0.f;
    bad = false;
#pragma unroll
    for (int a = 0; a < A; ++a) { p[a] = p[a] / ssum; psum += p[a]; bad |= (p[a] != p[a]); }
    int a_sel;
    if (forced) {
        a_sel = forced[row];
    } else {
        const float target = u01_f32(u_word()) * psum;
        float cdf = 0.f;
        a_sel = A - 1;
        bool found = false;
#pragma unroll
        for (int a = 0; a < A; ++a) {                 // inverse CDF: first a with target < cdf
            cdf += p[a];
            if (!found && target < cdf) { a_sel = a; found = true; }
        }
    }
    a_sel = a_sel < 0 ? 0 : (a_sel > A - 1 ? A - 1 : a_sel);
    float psel = 0.f;
#pragma unroll
    for (int a = 0; a < A; ++a) if (a == a_sel) psel = p[a];
    lp = __logf(fminf(fmaxf(psel / psum, F32_EPS), 1.0f - F32_EPS));
    return a_sel;
}

constexpr int LOSS_BLOCKS = 1024;
constexpr int LOSS_PSTRIDE = 16;   // doubles per block partial: 4 loss sums + up to 9 head-bias sums

struct LossAcc { double pl, vl, en, nan; };

// Update diagnostics (uav_set_ppo_diag): UAV_PPO_DIAG_N f64 sums over a call's samples, by-products of the loss arithmetic.
// They exist in the DIAG = true instantiations only; DIAG = false is the loss code without them.
//   [UAV_PPO_DIAG_KL_K1]    logp_old - logp                      the k1 estimator of KL(old || new)
//   [UAV_PPO_DIAG_KL_K3]    expm1(lr) - lr, lr = logp - logp_old the k3 estimator (non-negative)
//   [UAV_PPO_DIAG_CLIPPED]  count of ratio < 1 - clip or ratio > 1 + clip
//   [UAV_PPO_DIAG_VCLIPPED] count of |V - v_old| > clip
//   [UAV_PPO_DIAG_VERR2]    (R - V)^2
//   [UAV_PPO_DIAG_RET]      R
//   [UAV_PPO_DIAG_RET2]     R^2
//   [UAV_PPO_DIAG_COUNT]    the sample count
// logp, ratio, V and lr are the f32 values the loss itself uses; the arithmetic on them is f64 (in f32 (ratio - 1) - lr cancels
// to nothing at the small lr that matters), expm1 included.  Samples with NaN probabilities are not special-cased: loss_sums[3]
// counts them as before and they make the sums they enter NaN; a ratio that overflows (lr > 88.7 in f32) puts more than 3.4e38
// into the k3 sum, and lr = +inf (logp_old = -inf) makes it infinite.
struct DiagAcc { double s[UAV_PPO_DIAG_N]; };

// expm1(x) - x in f64 for the k3 estimator, in a dozen registers: libm's expm1 inlined into mlp_ppo_grad_kernel (a kernel at
// its 256-VGPR limit) tripled that kernel's spills.  |x| <= 1/4: the series x^2 / 2! + x^3 / 3! + ... + x^14 / 14! by Horner
// -- no cancellation against x, truncation x^15 / 15! < 3e-18 of the leading term, every term of one sign or alternating and
// decreasing, so the result is >= 0.  Larger |x| (< 1024): y = x 2^-k with |y| <= 1/4, expm1(y) by the same series, then k
// times expm1(2 t) = E (E + 2) -- about one ulp per doubling, k <= 12 -- and x is subtracted; overflow past x = 709.8 gives
// +inf by itself.  |x| >= 1024, infinite or NaN: the limits (+inf, -1 - x, NaN).
__device__ __forceinline__ double diag_expm1_series(double y, bool minus_y) {      // expm1(y) (- y), |y| <= 1/4
    double p = 1.0 / 14.0;
#pragma unroll
    for (int n = 13; n >= 3; --n) p = __builtin_fma(p, y, 1.0) * (1.0 / n);       // ... (1 + y / (n + 1) (...)) / n
    p = __builtin_fma(p, y, 1.0) * 0.5 * y * y;                                     // y^2 / 2 + y^3 / 6 + ...
    return minus_y ? p : p + y;
}
__device__ __forceinline__ double diag_k3(double x) {
    const double ax = __builtin_fabs(x);
    if (ax <= 0.25) return diag_expm1_series(x, true);
    if (!(ax < 1024.0)) return x > 0.0 ? __builtin_inf() : (x < 0.0 ? -1.0 - x : x);
    const int k = (int)((__builtin_bit_cast(unsigned long long, ax) >> 52) & 0x7ff) - 1023 + 3;      // |x| < 2^(k - 2), so |y| < 1/4; k in 1 .. 12
    double E = diag_expm1_series(ldexp(x, -k), false);
    for (int i = 0; i < k; ++i) E = E * (E + 2.0);
    return E - x;
}
// block partials of the diagnostics: [gridDim.x][UAV_PPO_DIAG_N] doubles right behind the gridDim.x loss partials
__device__ __forceinline__ double* diag_partials(double* loss_partial) { return loss_partial + (size_t)LOSS_PSTRIDE * gridDim.x; }

// one sample: loss terms into `acc`, d(total)/d(logits) into dz[A], d(total)/dV returned; DIAG: the diagnostic terms into *dg
template <int A, bool DIAG = false>
__device__ __forceinline__ float ppo_sample(const float* z, float V, int a, float lpo, float Ad, float R, float vo,
                                            float inv_n, float clip, float beta, LossAcc& acc, float* dz, DiagAcc* dg = nullptr) {
    float p[A];
    softmax_row<A>(z, p);
    float psum = 0.f;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        psum += p[k];
        bad |= (p[k] != p[k]);
    }
    if (bad) acc.nan += 1.0;
    // Categorical(probs): q = p / sum p, clamped to [eps, 1-eps]
    float q[A];
    float qa = 0.f;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        q[k] = p[k] / psum;
        if (k == a) qa = q[k];
    }
    const bool clamp_open = (qa >= F32_EPS) && (qa <= 1.0f - F32_EPS);
    const float qc = fminf(fmaxf(qa, F32_EPS), 1.0f - F32_EPS);
    const float logp = logf(qc);
    const float ratio = expf(logp - lpo);
    const float lo = 1.0f - clip, hi = 1.0f + clip;
    const float rc = fminf(fmaxf(ratio, lo), hi);
    const float s1 = ratio * Ad, s2 = rc * Ad;
    acc.pl += (double)(-fminf(s1, s2));
    const bool in_rng = (ratio >= lo) && (ratio <= hi);
    // torch.min backward: ties split 1/2 - 1/2; clamp backward passes inside [lo,hi]
    float g_ratio;
    if (s1 < s2) g_ratio = Ad;
    else if (s1 == s2) g_ratio = 0.5f * Ad + (in_rng ? 0.5f * Ad : 0.f);
    else g_ratio = in_rng ? Ad : 0.f;
    // dL/dlogp.  A ratio that overflowed to +inf (logp_old far below anything a policy assigns) whose sample is clipped away or
    // has no advantage has the gradient 0, not 0 * inf = NaN; every other sample's bits are those of the plain product.
    const bool dead_inf = (g_ratio == 0.f) && (ratio == __builtin_inff());
    const float g_logp = (clamp_open && !dead_inf) ? (-inv_n * g_ratio * ratio) : 0.f;

    // value loss, train_ppo2.0.py:74-78
    const float dv = V - vo;
    const float vc = vo + fminf(fmaxf(dv, -clip), clip);
    const float e1 = (V - R) * (V - R), e2 = (vc - R) * (vc - R);
    acc.vl += (double)(0.5f * fmaxf(e1, e2));
    const float d1 = 2.0f * (V - R);
    const float d2 = (dv >= -clip && dv <= clip) ? 2.0f * (vc - R) : 0.f;
    const float gV = (e1 > e2) ? d1 : ((e1 < e2) ? d2 : 0.5f * (d1 + d2));

    // entropy, train_ppo2.0.py:81 :  H = -sum p log(p + 1e-8)
    float Hs = 0.f, hk[A], ph = 0.f;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float lg = logf(p[k] + 1e-8f);
        Hs -= p[k] * lg;
        hk[k] = -lg - p[k] / (p[k] + 1e-8f);      // dH/dp_k
        ph += p[k] * hk[k];
    }
    acc.en += (double)Hs;
    // through the softmax: d/dz_k = p_k (g_k - sum_j p_j g_j)
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float dpol = g_logp * ((k == a ? 1.0f : 0.0f) - q[k]);
        const float dent = -beta * inv_n * p[k] * (hk[k] - ph);
        dz[k] = dpol + dent;
    }
    if constexpr (DIAG) {
        const double lr = (double)(logp - lpo), Rd = (double)R, er = Rd - (double)V;      // lr: the f32 argument of the ratio's expf
        dg->s[UAV_PPO_DIAG_KL_K1] -= lr;
        dg->s[UAV_PPO_DIAG_KL_K3] += diag_k3(lr);          // f64: the f32 ratio's own rounding (6e-8) would swamp lr^2 / 2
        dg->s[UAV_PPO_DIAG_CLIPPED] += (ratio < lo || ratio > hi) ? 1.0 : 0.0;
        dg->s[UAV_PPO_DIAG_VCLIPPED] += (fabsf(dv) > clip) ? 1.0 : 0.0;
        dg->s[UAV_PPO_DIAG_VERR2] += er * er;
        dg->s[UAV_PPO_DIAG_RET] += Rd;
        dg->s[UAV_PPO_DIAG_RET2] += Rd * Rd;
        dg->s[UAV_PPO_DIAG_COUNT] += 1.0;
    }
    return 0.5f * inv_n * gV;
}

// ---- behaviour cloning (uav_bc_loss, uav_mlp_bc_grad): the supervised loss on the expert's action.  Softmax, normalisation,
// clamp and logf are ppo_sample's, so the log-probability formed here is bit for bit the one ppo_sample forms on the same logits.
struct BcAcc { double nll, vl, en, nan, agree, cnt; };

// one sample: loss terms into `acc`, d(total)/d(logits) into dz[A], d(total)/dV returned.  a outside 0 .. A-1 is a MASKED sample
// (a padded step of a ragged episode): dz = 0, dV = 0 and no sum, the NaN count included, sees it.  has_vt: R is a value target
// (vl = 0.5 (V - R)^2, dV = vcoef inv_n (V - R)); without one vl = 0 and dV = 0.
template <int A>
__device__ __forceinline__ float bc_sample(const float (&z)[A], float V, int a, bool has_vt, float R, float inv_n, float vcoef,
                                           float beta, BcAcc& acc, float* dz) {
    if (a < 0 || a >= A) {
#pragma unroll
        for (int k = 0; k < A; ++k) dz[k] = 0.f;
        return 0.f;
    }
    float p[A];
    softmax_row<A>(z, p);
    float psum = 0.f;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        psum += p[k];
        bad |= (p[k] != p[k]);
    }
    if (bad) acc.nan += 1.0;
    float q[A];
    float qa = 0.f;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        q[k] = p[k] / psum;
        if (k == a) qa = q[k];
    }
    const bool clamp_open = (qa >= F32_EPS) && (qa <= 1.0f - F32_EPS);
    const float qc = fminf(fmaxf(qa, F32_EPS), 1.0f - F32_EPS);
    acc.nll += (double)(-logf(qc));
    const float g_logp = clamp_open ? -inv_n : 0.f;       // dL/dlogp
    bool zbad;
    if (argmax_first<A>(z, zbad) == a) acc.agree += 1.0;
    acc.cnt += 1.0;

    float dV = 0.f;
    if (has_vt) {
        const float e = V - R;
        acc.vl += (double)(0.5f * e * e);
        dV = vcoef * inv_n * e;
    }
    // entropy: ppo_sample's
    float Hs = 0.f, hk[A], ph = 0.f;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float lg = logf(p[k] + 1e-8f);
        Hs -= p[k] * lg;
        hk[k] = -lg - p[k] / (p[k] + 1e-8f);
        ph += p[k] * hk[k];
    }
    acc.en += (double)Hs;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float dpol = g_logp * ((k == a ? 1.0f : 0.0f) - q[k]);
        const float dent = -beta * inv_n * p[k] * (hk[k] - ph);
        dz[k] = dpol + dent;
    }
    return dV;
}
