// reward_norm.hip -- running return-based reward normalisation (the reward half of "VecNormalize"), on the device.
//
//   N1  return trace + statistics   G[e][t] = r[e][t] + gamma * k[e][t-1] * G[e][t-1]  (f64), k = (done != 0) ? 0 : 1, the term in front
//                                   of t = 0 is gamma * carry[e]; on exit carry[e] = k[e][T-1] * G[e][T-1], so a rollout continues
//                                   the episodes the previous one left open.  stats3 = {sum G, sum G^2, n_env * T}.
//   N2  merge                       Chan's update of the running {mean, M2, count, skipped} by one thread; scale = 1 / sqrt(M2 / count + eps).
//   N3  scale                       out = clamp(rew * scale, -clip, clip), scale read from device memory.
//
// Nothing is read by the host between the three: ranks all-reduce stats3 between N1 and N2 (uavppo/reward_norm.py).
// Layout (env, T) as in gae.hip: one wavefront owns one env row, lane i <-> t = 64c + i, one coalesced wave access per chunk
// (256 B of rewards, 256 B of done flags; 512 B of the trace where it is asked for).
#include "common.h"

// G[t] = b_t + a_t * G[t-1] is an affine map of what stands to its left; the prefix composition over a 64-step chunk is a
// Hillis-Steele scan on (a, b) pairs with wave shuffles, (a2,b2) then (a1,b1) = (a1*a2, b1 + a1*b2): gae_scan_kernel's suffix
// scan mirrored.  a_t = gamma * k[t-1] is exact (k is 0 or 1), so against the sequential f64 evaluation the scan only
// reassociates products and sums.
// The sums: every lane adds up its own steps over the chunks, then wave tree, the block's 4 waves in order, one partial pair
// per block; return_stats_final adds the partials in a fixed order -- the same bits on every run of the same shape.
__global__ __launch_bounds__(256) void return_scan_kernel(const float* __restrict__ rew, const float* __restrict__ done,
                                                          double* __restrict__ carry, int n_env, int T, double gamma,
                                                          double* __restrict__ partial, double* __restrict__ trace) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63;
    const int env = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = env < n_env;            // wave-uniform; a dead wave still walks to the block sums below
    double s = 0.0, q = 0.0;
    if (live) {
        const size_t row = (size_t)env * T;
        const int nchunk = (T + 63) >> 6;
        double left = carry[env];             // k * G of the step to the left of the chunk
        for (int c = 0; c < nchunk; ++c) {
            const int t = c * 64 + lane;
            const bool in = t < T;
            const double r = in ? (double)rew[row + t] : 0.0;
            const double k = (in && done[row + t] != 0.f) ? 0.0 : 1.0;
            double k1 = __shfl_up(k, 1, 64);  // k of step t-1; lane 0 multiplies `left`, which carries its k already
            if (lane == 0) k1 = 1.0;
            double a = in ? gamma * k1 : 1.0, b = r;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double a2 = __shfl_up(a, o, 64);
                const double b2 = __shfl_up(b, o, 64);
                if (lane >= o) {
                    b = b + a * b2;
                    a = a * a2;
                }
            }
            const double G = b + a * left;
            if (in) {
                if (trace) trace[row + t] = G;
                s += G;
                q += G * G;
            }
            const int last = (T - c * 64 < 64 ? T - c * 64 : 64) - 1;     // last step of the row that lies in this chunk
            left = __shfl(k * G, last, 64);
        }
        if (lane == 0) carry[env] = left;
    }
    s = block256_sum(s, sm);
    q = block256_sum(q, sm);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = s;
        partial[2 * blockIdx.x + 1] = q;
    }
}

__global__ __launch_bounds__(256) void return_stats_final(const double* __restrict__ partial, int nb, double n,
                                                          double* __restrict__ stats3) {
    __shared__ double sm[4];
    double s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) {
        s += partial[2 * i];
        q += partial[2 * i + 1];
    }
    s = block256_sum(s, sm);
    q = block256_sum(q, sm);
    if (threadIdx.x == 0) {
        stats3[0] = s;
        stats3[1] = q;
        stats3[2] = n;
    }
}

// One thread, f64 (uavppo/reward_norm.py: merge_running states the same lines in numpy).  A batch whose sums are not finite
// (a NaN or inf reward), or that holds no samples, leaves the running estimate as it was and is counted.
__global__ void return_norm_merge_kernel(double* __restrict__ state, const double* __restrict__ stats3, double eps,
                                         float* __restrict__ scale) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double mean = state[0], M2 = state[1], count = state[2];
    const double s = stats3[0], q = stats3[1], nb = stats3[2];
    if (isfinite(s) && isfinite(q) && nb > 0.0) {
        const double mb = s / nb;
        const double M2b = fmax(q - s * s / nb, 0.0);
        const double d = mb - mean;
        const double tot = count + nb;
        mean += d * nb / tot;
        M2 += M2b + d * d * count * nb / tot;
        count = tot;
        state[0] = mean;
        state[1] = M2;
        state[2] = count;
    } else {
        state[3] += 1.0;
    }
    // no samples yet, or a constant history: the reward passes unscaled (never divided by sqrt(eps))
    float sc = 1.0f;
    if (count > 0.0) {
        const double var = M2 / count;
        if (var > 0.0) sc = (float)(1.0 / sqrt(var + eps));
    }
    scale[0] = sc;
}

// rew and out carry no __restrict__: out may be rew.  A NaN fails both comparisons and stays NaN.
__global__ __launch_bounds__(256) void reward_scale_kernel(const float* rew, int64_t n, const float* __restrict__ scale,
                                                           float clip, float* out) {
#pragma clang fp contract(off)
    const float sc = scale[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v = rew[i] * sc;
        if (clip > 0.f) v = v > clip ? clip : (v < -clip ? -clip : v);
        out[i] = v;
    }
}

extern "C" {

int uav_return_stats(uav_ctx* ctx, const float* rew, const float* done, double* carry, int n_env, int horizon,
                     double gamma, double* stats3, double* trace_out, uav_stream stream) {
    UAV_REQUIRE(ctx && rew && done && carry && stats3, "uav_return_stats: NULL argument");
    UAV_REQUIRE(n_env > 0 && horizon > 0, "uav_return_stats: n_env=%d horizon=%d", n_env, horizon);
    UAV_REQUIRE(gamma >= 0.0 && gamma <= 1.0, "uav_return_stats: gamma=%g outside [0, 1]", gamma);
    const int blocks = (n_env + 3) / 4;
    UAV_REQUIRE((size_t)blocks * 2 * sizeof(double) <= ctx->ws_bytes, "uav_return_stats: %d block partials do not fit the workspace", blocks);
    double* partial = (double*)ctx->ws;
    hipLaunchKernelGGL(return_scan_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), rew, done, carry, n_env, horizon,
                       gamma, partial, trace_out);
    hipLaunchKernelGGL(return_stats_final, dim3(1), dim3(256), 0, as_stream(stream), partial, blocks,
                       (double)n_env * (double)horizon, stats3);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_return_norm_merge(uav_ctx* ctx, double* state, const double* stats3, double eps, float* scale, uav_stream stream) {
    UAV_REQUIRE(ctx && state && stats3 && scale, "uav_return_norm_merge: NULL argument");
    UAV_REQUIRE(eps > 0.0, "uav_return_norm_merge: eps=%g must be positive", eps);
    hipLaunchKernelGGL(return_norm_merge_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, stats3, eps, scale);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_reward_scale(uav_ctx* ctx, const float* rew, int64_t n, const float* scale, float clip, float* out, uav_stream stream) {
    UAV_REQUIRE(ctx && rew && scale && out, "uav_reward_scale: NULL argument");
    UAV_REQUIRE(n > 0, "uav_reward_scale: n=%lld", (long long)n);
    int nb = (int)((n + 1023) / 1024);
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(reward_scale_kernel, dim3(nb), dim3(256), 0, as_stream(stream), rew, n, scale, clip, out);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
