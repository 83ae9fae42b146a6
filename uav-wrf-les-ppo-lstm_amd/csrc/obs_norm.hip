// obs_norm.hip -- running per-channel observation normalisation (the observation half of "VecNormalize"), folded into the
// policy's first affine layer instead of applied to the observations: every kernel that reads an observation runs unchanged.
//
//   O1  statistics   stats = {rows, sum_j x[.][j], sum_j x[.][j]^2} (f64) of obs f32 [rows][D], D = 6 .. 8, one launch
//   O2  merge        Chan's update of {count, skipped, mean_j, M2_j} per channel by one thread; mu_j, inv_sigma_j = 1 / sqrt(M2_j / count + eps)
//   O3  fold         w_eff[r][j] = w[r][j] * inv_sigma_j,  b_eff[r] = b[r] - sum_j w_eff[r][j] mu_j:  w_eff x + b_eff = w (x - mu) / sigma + b
//   O4  unfold grad  dw[r][j] = (dw_eff[r][j] - db[r] mu_j) inv_sigma_j  (the chain rule of O3; db is its own gradient)
//   O5  unfold       w = w_eff / inv_sigma_j, b = b_eff + sum_j w_eff[r][j] mu_j  (O3 inverted, for parameters written by someone else)
//
// Nothing is read by the host between them: ranks all-reduce `stats` between O1 and O2 (uavppo/obs_norm.py, which states every
// one of these in numpy).  The file is compiled without FMA contraction, so the f64 lines below round as numpy's do.
#include "common.h"

constexpr int OBS_VB = 256;                       // blocks of the statistics pass: a constant, so that the order of summation is one
constexpr int OBS_SLOTS = OBS_VB * 256;           // threads of the pass ("slots")

// Order of summation, the same for every shape: slot k = 256 * block + thread adds up the rows k, k + 65536, k + 2 * 65536, ... one
// after the other; then per block wave_sum's tree over the 64 lanes of a wave and ((w0 + w1) + w2) + w3 over its four waves
// (block256_sum); then the 256 block sums the same way once more, in the block that finishes last.  batch_stats (obs_norm.py)
// is this order in numpy.  The hand-over between the blocks is the ticket form: block sums stored, one agent-scope release, a
// relaxed ticket; the block that draws the last ticket acquires once and reads all of them.  `ticket` is zeroed ahead of the launch.
template <int D>
__global__ __launch_bounds__(256) void obs_stats_kernel(const float* __restrict__ obs, int64_t rows, int64_t row_stride,
                                                        double* __restrict__ partial, unsigned* __restrict__ ticket,
                                                        double* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double sm[5];                      // block256_sum's four slots | "this block is the last one"
    double s[D], q[D];
#pragma unroll
    for (int j = 0; j < D; ++j) s[j] = q[j] = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += OBS_SLOTS) {
        const float* x = obs + r * row_stride;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const double v = (double)x[j];
            s[j] += v;
            q[j] += v * v;
        }
    }
    double* mine = partial + (size_t)blockIdx.x * 2 * D;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const double a = block256_sum(s[j], sm), b = block256_sum(q[j], sm);
        if (threadIdx.x == 0) {
            mine[j] = a;
            mine[D + j] = b;
        }
    }
    if (threadIdx.x == 0) {                       // the only thread of the block that stored anything
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == (unsigned)(OBS_VB - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        sm[4] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    if (sm[4] == 0.0) return;                     // block-uniform
    // thread 0 acquired; the others read the block sums with agent-scope loads, which no cache of this CU answers
    const double* p = partial + (size_t)threadIdx.x * 2 * D;      // thread i holds block i's sums: OBS_VB == 256 threads
#pragma unroll
    for (int j = 0; j < 2 * D; ++j) {
        const double v = __hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double a = block256_sum(v, sm);
        if (threadIdx.x == 0) stats[1 + j] = a;
    }
    if (threadIdx.x == 0) stats[0] = (double)rows;
}

// One thread, f64, channel after channel (obs_norm.py: merge_running states the same lines in numpy).  A batch with a sum that
// is not finite, or without rows, leaves the running estimate as it was and is counted.  mask bit j clear: channel j passes as it is.
__global__ void obs_norm_merge_kernel(double* __restrict__ state, const double* __restrict__ stats, int D, unsigned mask,
                                      double eps, float* __restrict__ mu, float* __restrict__ inv_sigma) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double count = state[0];
    const double nb = stats[0];
    bool ok = nb > 0.0;
    for (int j = 0; j < 2 * D; ++j) ok = ok && isfinite(stats[1 + j]);
    if (ok) {
        const double tot = count + nb;
        for (int j = 0; j < D; ++j) {
            const double s = stats[1 + j], q = stats[1 + D + j];
            double mean = state[2 + j], M2 = state[2 + D + j];
            const double mb = s / nb;
            const double M2b = fmax(q - s * s / nb, 0.0);
            const double d = mb - mean;
            mean += d * nb / tot;
            M2 += M2b + d * d * count * nb / tot;
            state[2 + j] = mean;
            state[2 + D + j] = M2;
        }
        count = tot;
        state[0] = count;
    } else {
        state[1] += 1.0;
    }
    for (int j = 0; j < D; ++j) {
        float m = 0.f, is = 1.f;
        if (count > 0.0 && ((mask >> j) & 1u)) {
            m = (float)state[2 + j];
            is = (float)(1.0 / sqrt(state[2 + D + j] / count + eps));
        }
        mu[j] = m;
        inv_sigma[j] = is;
    }
}

// max |v| over the block -> *pmax_bits, raised only (bit patterns of non-negative floats order like the floats; a NaN counts as +inf)
__device__ __forceinline__ void raise_pmax(float amax, unsigned* __restrict__ pmax_bits, float* wmax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(pmax_bits, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}

__device__ __forceinline__ float abs_or_inf(float v) { return v == v ? fabsf(v) : __builtin_inff(); }

// one thread per row of the first layer (rows = 4H or h1: a few hundred)
__global__ __launch_bounds__(256) void obs_fold_kernel(const float* __restrict__ w, const float* __restrict__ b, int rows, int D,
                                                       const float* __restrict__ mu, const float* __restrict__ inv_sigma,
                                                       float* __restrict__ w_eff, float* __restrict__ b_eff,
                                                       unsigned* __restrict__ pmax_bits) {
#pragma clang fp contract(off)
    __shared__ float wmax[4];
    const int r = blockIdx.x * 256 + threadIdx.x;
    float amax = 0.f;
    if (r < rows) {
        double acc = (double)b[r];
        for (int j = 0; j < D; ++j) {
            const float we = w[(size_t)r * D + j] * inv_sigma[j];
            w_eff[(size_t)r * D + j] = we;
            acc = acc - (double)we * (double)mu[j];
            amax = fmaxf(amax, abs_or_inf(we));
        }
        const float be = (float)acc;
        b_eff[r] = be;
        amax = fmaxf(amax, abs_or_inf(be));
    }
    if (pmax_bits) raise_pmax(amax, pmax_bits, wmax);
}

__global__ __launch_bounds__(256) void obs_unfold_grad_kernel(float* __restrict__ dw, const float* __restrict__ db, int rows, int D,
                                                              const float* __restrict__ mu, const float* __restrict__ inv_sigma) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const double g = (double)db[r];
    for (int j = 0; j < D; ++j) {
        const double v = (double)dw[(size_t)r * D + j] - g * (double)mu[j];
        dw[(size_t)r * D + j] = (float)(v * (double)inv_sigma[j]);
    }
}

// w may be w_eff and b may be b_eff (every row is read before it is written, by its own thread)
__global__ __launch_bounds__(256) void obs_unfold_kernel(const float* w_eff, const float* b_eff, int rows, int D,
                                                         const float* __restrict__ mu, const float* __restrict__ inv_sigma,
                                                         float* w, float* b) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    double acc = (double)b_eff[r];
    for (int j = 0; j < D; ++j) {
        const float we = w_eff[(size_t)r * D + j];
        acc = acc + (double)we * (double)mu[j];
        w[(size_t)r * D + j] = we / inv_sigma[j];
    }
    b[r] = (float)acc;
}

#define OBS_REQUIRE_SHAPE(name, rows, D)                                             \
    UAV_REQUIRE((D) >= 6 && (D) <= 8, name ": D=%d outside 6..8", (int)(D));         \
    UAV_REQUIRE((rows) > 0, name ": rows=%lld", (long long)(rows))

extern "C" {

int uav_obs_stats(uav_ctx* ctx, const float* obs, int64_t rows, int D, int64_t row_stride, double* stats, uav_stream stream) {
    UAV_REQUIRE(ctx && obs && stats, "uav_obs_stats: NULL argument");
    OBS_REQUIRE_SHAPE("uav_obs_stats", rows, D);
    UAV_REQUIRE(row_stride >= D, "uav_obs_stats: row_stride=%lld is less than D=%d", (long long)row_stride, D);
    const size_t pbytes = (size_t)OBS_VB * 2 * 8 * sizeof(double);
    UAV_REQUIRE(pbytes + sizeof(unsigned) <= ctx->ws_bytes, "uav_obs_stats: the block sums do not fit the workspace");
    double* partial = (double*)ctx->ws;
    unsigned* ticket = (unsigned*)((char*)ctx->ws + pbytes);
    UAV_CHECK_HIP(hipMemsetAsync(ticket, 0, sizeof(unsigned), as_stream(stream)));
    if (D == 6)
        hipLaunchKernelGGL(obs_stats_kernel<6>, dim3(OBS_VB), dim3(256), 0, as_stream(stream), obs, rows, row_stride, partial, ticket, stats);
    else if (D == 7)
        hipLaunchKernelGGL(obs_stats_kernel<7>, dim3(OBS_VB), dim3(256), 0, as_stream(stream), obs, rows, row_stride, partial, ticket, stats);
    else
        hipLaunchKernelGGL(obs_stats_kernel<8>, dim3(OBS_VB), dim3(256), 0, as_stream(stream), obs, rows, row_stride, partial, ticket, stats);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_obs_norm_merge(uav_ctx* ctx, double* state, const double* stats, int D, unsigned mask, double eps, float* mu,
                       float* inv_sigma, uav_stream stream) {
    UAV_REQUIRE(ctx && state && stats && mu && inv_sigma, "uav_obs_norm_merge: NULL argument");
    UAV_REQUIRE(D >= 6 && D <= 8, "uav_obs_norm_merge: D=%d outside 6..8", D);
    UAV_REQUIRE(eps > 0.0, "uav_obs_norm_merge: eps=%g must be positive", eps);
    hipLaunchKernelGGL(obs_norm_merge_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, stats, D, mask, eps, mu, inv_sigma);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_obs_fold(uav_ctx* ctx, const float* w, const float* b, int rows, int D, const float* mu, const float* inv_sigma,
                 float* w_eff, float* b_eff, float* pmax_inout, uav_stream stream) {
    UAV_REQUIRE(ctx && w && b && mu && inv_sigma && w_eff && b_eff, "uav_obs_fold: NULL argument");
    OBS_REQUIRE_SHAPE("uav_obs_fold", rows, D);
    hipLaunchKernelGGL(obs_fold_kernel, dim3((rows + 255) / 256), dim3(256), 0, as_stream(stream), w, b, rows, D, mu, inv_sigma,
                       w_eff, b_eff, reinterpret_cast<unsigned*>(pmax_inout));
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_obs_unfold_grad(uav_ctx* ctx, float* dw, const float* db, int rows, int D, const float* mu, const float* inv_sigma,
                        uav_stream stream) {
    UAV_REQUIRE(ctx && dw && db && mu && inv_sigma, "uav_obs_unfold_grad: NULL argument");
    OBS_REQUIRE_SHAPE("uav_obs_unfold_grad", rows, D);
    hipLaunchKernelGGL(obs_unfold_grad_kernel, dim3((rows + 255) / 256), dim3(256), 0, as_stream(stream), dw, db, rows, D, mu, inv_sigma);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_obs_unfold(uav_ctx* ctx, const float* w_eff, const float* b_eff, int rows, int D, const float* mu, const float* inv_sigma,
                   float* w, float* b, uav_stream stream) {
    UAV_REQUIRE(ctx && w_eff && b_eff && mu && inv_sigma && w && b, "uav_obs_unfold: NULL argument");
    OBS_REQUIRE_SHAPE("uav_obs_unfold", rows, D);
    hipLaunchKernelGGL(obs_unfold_kernel, dim3((rows + 255) / 256), dim3(256), 0, as_stream(stream), w_eff, b_eff, rows, D, mu,
                       inv_sigma, w, b);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
