// eval_track.hip -- the bookkeeping of an in-training greedy evaluation, kept on the device (no counterpart in the reference,
// whose evaluate_with_lstm.py:67-101 does it per episode in Python; uavppo/eval_track.py states every line in numpy).
//
//   E1  reduce    one chunk of greedy records (uav_greedy_episodes / _stop / uav_greedy_tail) -> per env: the step, the position
//                 and the cause of its episode's end.  One wave per env row, byte loads of the flags coalesced along the row.
//   E2  summary   per env steps / deviation / success and the eight sums of an evaluation, in ONE order of summation
//   E3  keep best the decision "this evaluation is the best so far" by one thread, then the parameter copy under its flag in a
//                 SECOND launch: a block of the copy can never see a state that the same call is still deciding.
//
// Nothing is read by the host between them; ranks all-reduce the eight sums between E2 and E3 and so take the same decision.
#include "common.h"

constexpr int FLAG_DONE = 1, FLAG_SKIP = 4, FLAG_RULE = 8;      // record flags: bit0 done, bit2 not stepped, bit3 rule fired

__global__ __launch_bounds__(256) void greedy_reduce_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ obs,
                                                            const float* __restrict__ pos, int n, int k, int D, int t0,
                                                            int32_t* __restrict__ ep_steps, uint8_t* __restrict__ ep_state,
                                                            double* __restrict__ ep_pos) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);        // wave-uniform
    if (row >= n) return;
    if (ep_state[row] & 1) return;                              // ended in an earlier chunk: left alone to the bit
    const uint8_t* f = flags + (int64_t)row * k;
    int first = -1;
    uint8_t at = 0;
    for (int base = 0; base < k; base += 64) {                  // wave-uniform trip count
        const int i = base + lane;
        const uint8_t v = i < k ? f[i] : (uint8_t)FLAG_SKIP;
        const bool end = !(v & FLAG_SKIP) && (v & (FLAG_DONE | FLAG_RULE));
        const unsigned long long m = __ballot(end);
        if (m) {
            const int src = __builtin_ctzll(m);
            first = base + src;
            at = (uint8_t)__shfl((int)v, src, 64);
            break;
        }
    }
    if (lane != 0) return;
    if (first >= 0) {
        const int64_t rec = (int64_t)row * k + first;
        double x, y;
        if (at & FLAG_DONE) {                                   // the record holds the terminal observation
            x = (double)obs[rec * D] * 500.0;
            y = (double)obs[rec * D + 1] * 500.0;
        } else {
            x = (double)pos[rec * 2];
            y = (double)pos[rec * 2 + 1];
        }
        ep_steps[row] = t0 + first + 1;
        ep_state[row] = (uint8_t)(ep_state[row] | 1 | ((at & FLAG_RULE) ? 2 : 0));
        ep_pos[row * 2] = x;
        ep_pos[row * 2 + 1] = y;
    } else if (!(f[k - 1] & FLAG_SKIP)) {                       // still running: where a cut-off by the step limit would stand
        const int64_t rec = (int64_t)row * k + (k - 1);
        ep_pos[row * 2] = (double)pos[rec * 2];
        ep_pos[row * 2 + 1] = (double)pos[rec * 2 + 1];
    }
}

// Order of summation, the same for every n: thread j of ONE block of 256 adds up the envs j, j + 256, j + 512, ... one after the
// other; then block256_sum's tree (wave_sum over 64 lanes, ((w0 + w1) + w2) + w3).  summarise (eval_track.py) is this order.
__global__ __launch_bounds__(256) void greedy_summary_kernel(const int32_t* __restrict__ ep_steps, const uint8_t* __restrict__ ep_state,
                                                             const double* __restrict__ ep_pos, const double* __restrict__ src,
                                                             int n, int limit, double success_distance,
                                                             const int32_t* __restrict__ nan_count, double* __restrict__ deviation,
                                                             int32_t* __restrict__ steps, uint8_t* __restrict__ success,
                                                             double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    double s[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) {
        const bool ended = ep_state[e] & 1;
        const int st = ended ? ep_steps[e] : limit;
        const double dx = ep_pos[2 * e] - src[2 * e], dy = ep_pos[2 * e + 1] - src[2 * e + 1];
        const double dev = sqrt(dx * dx + dy * dy);
        const bool ok = dev <= success_distance;                // false for a NaN
        if (deviation) deviation[e] = dev;
        if (steps) steps[e] = st;
        if (success) success[e] = ok ? 1 : 0;
        s[0] += ok ? 1.0 : 0.0;
        s[1] += (double)st;
        s[2] += dev;
        s[3] += dev * dev;
        if (ok) s[4] += dev;
        s[5] += ended ? 0.0 : 1.0;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double a = block256_sum(s[j], sm);
        if (threadIdx.x == 0) sums[1 + j] = a;
    }
    if (threadIdx.x == 0) {
        sums[0] = (double)n;
        sums[7] = nan_count ? (double)nan_count[0] : 0.0;
    }
}

// One thread, f64: better_rule (eval_track.py) line by line.  state = {best successes, best step sum, best iteration, evaluations
// seen, improvements, skipped, this call took the row}; all zeros is the fresh state.
__global__ void keep_best_decide_kernel(double* __restrict__ state, const double* __restrict__ sums, double iteration) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    bool valid = sums[UAV_EVAL_SUM_EPISODES] > 0.0 && !(sums[UAV_EVAL_SUM_NAN] > 0.0);
    for (int j = 0; j < UAV_EVAL_SUM_N; ++j) valid = valid && sums[j] == sums[j];
    double took = 0.0;
    state[UAV_BEST_SEEN] += 1.0;
    if (!valid) {
        state[UAV_BEST_SKIPPED] += 1.0;
    } else {
        const double succ = sums[UAV_EVAL_SUM_SUCCESSES], st = sums[UAV_EVAL_SUM_STEPS];
        const bool better = state[UAV_BEST_IMPROVED] == 0.0 || succ > state[UAV_BEST_SUCCESSES] ||
                            (succ == state[UAV_BEST_SUCCESSES] && st < state[UAV_BEST_STEPS]);
        if (better) {
            state[UAV_BEST_SUCCESSES] = succ;
            state[UAV_BEST_STEPS] = st;
            state[UAV_BEST_ITERATION] = iteration;
            state[UAV_BEST_IMPROVED] += 1.0;
            took = 1.0;
        }
    }
    state[UAV_BEST_TOOK] = took;
}

__global__ __launch_bounds__(256) void keep_best_copy_kernel(const double* __restrict__ state, const float* __restrict__ cand,
                                                             float* __restrict__ best, int64_t n_params) {
    if (state[UAV_BEST_TOOK] != 1.0) return;                    // decided by the launch before this one: the same for every block
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_params; i += (int64_t)gridDim.x * 256) best[i] = cand[i];
}

extern "C" {

int uav_greedy_reduce(uav_ctx* ctx, const uint8_t* flags, const float* obs, const float* pos, int n, int k, int D, int t0,
                      int32_t* ep_steps, uint8_t* ep_state, double* ep_pos, uav_stream stream) {
    UAV_REQUIRE(ctx && flags && obs && pos && ep_steps && ep_state && ep_pos, "uav_greedy_reduce: NULL argument");
    UAV_REQUIRE(n >= 1 && k >= 1 && D >= 2, "uav_greedy_reduce: n=%d, k=%d must be at least 1 and D=%d at least 2", n, k, D);
    UAV_REQUIRE(t0 >= 0 && (int64_t)t0 + k < (int64_t)1 << 31, "uav_greedy_reduce: t0=%d outside 0 .. 2^31 - k", t0);
    UAV_REQUIRE((int64_t)n * k * D < (int64_t)1 << 31, "uav_greedy_reduce: n * k * D = %lld is 2^31 or more", (long long)n * k * D);
    hipLaunchKernelGGL(greedy_reduce_kernel, dim3((n + 3) / 4), dim3(256), 0, as_stream(stream), flags, obs, pos, n, k, D, t0,
                       ep_steps, ep_state, ep_pos);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_greedy_summary(uav_ctx* ctx, const int32_t* ep_steps, const uint8_t* ep_state, const double* ep_pos, const double* src, int n,
                       int limit, double success_distance, const int32_t* nan_count, double* deviation, int32_t* steps,
                       uint8_t* success, double* sums, uav_stream stream) {
    UAV_REQUIRE(ctx && ep_steps && ep_state && ep_pos && src && sums, "uav_greedy_summary: NULL argument");
    UAV_REQUIRE(n >= 1, "uav_greedy_summary: n=%d must be at least 1", n);
    UAV_REQUIRE(limit >= 1, "uav_greedy_summary: limit=%d must be at least 1", limit);
    UAV_REQUIRE(success_distance == success_distance, "uav_greedy_summary: success_distance is a NaN");
    hipLaunchKernelGGL(greedy_summary_kernel, dim3(1), dim3(256), 0, as_stream(stream), ep_steps, ep_state, ep_pos, src, n, limit,
                       success_distance, nan_count, deviation, steps, success, sums);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_keep_best(uav_ctx* ctx, double* state, const double* sums, int iteration, const float* cand, float* best, int64_t n_params,
                  uav_stream stream) {
    UAV_REQUIRE(ctx && state && sums && cand && best, "uav_keep_best: NULL argument");
    UAV_REQUIRE(n_params >= 1, "uav_keep_best: n_params=%lld must be at least 1", (long long)n_params);
    UAV_REQUIRE(cand != best, "uav_keep_best: cand and best are the same buffer");
    hipLaunchKernelGGL(keep_best_decide_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, sums, (double)iteration);
    UAV_LAUNCH_CHECK();
    const int64_t blocks = (n_params + 255) / 256;
    hipLaunchKernelGGL(keep_best_copy_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, as_stream(stream), state,
                       cand, best, n_params);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
