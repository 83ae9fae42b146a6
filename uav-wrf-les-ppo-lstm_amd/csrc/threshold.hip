// threshold.hip -- the PPOV2.0 threshold stop rule over a chunk of concentration records: the two small kernels around one batched
// call of the ConcentrationThresholdPredictor.
//
// Reference: PPOV2.0/evaluate_with_lstm.py:10-37 (ThresholdController) and :67-101 (the episode loop).  Every 10th step, once the
// trajectory holds 20 concentrations, the last 10 go through the MinMaxScaler and the predictor (3-layer LSTM from zero state ->
// fc), and 0.95 of its output becomes the threshold; every step from the 20th on stops the episode when the concentration, or the
// np.mean of the last 10, reaches the threshold.
//
// The rule is no recurrence over the predictor: its windows start from zero state, they sit at known steps (t % every == 0,
// t >= max(window, min_steps)) and the threshold is piecewise constant in between.  So a chunk is three stages:
//   threshold_windows_kernel   cuts the chunk's predictor windows out of (hist, series) and scales them: x f32 [n][S][window],
//                              S = ceil(steps / every) slots per env, zeros in the slots that hold no update step.  One thread per
//                              element of x; reads hist / step_cnt, writes neither.
//   (the host runs the predictor over the n * S rows: uav_lstm_fwd x 3, uav_gemm_f32, uav_ln_relu, uav_gemm_f32)
//   threshold_rule_kernel      one thread per env walks the chunk's steps in order: takes the slot's prediction on an update step,
//                              forms cur and the window mean, records the first hit; then shifts the env's history and advances
//                              step_cnt.  The window is read straight from hist / series at every step (n * steps * window loads in
//                              all; the whole kernel is a few thousand f64 adds per thread).
// Slots are per env: env e enters with step_cnt[e] steps behind it, step i of the call is its step t = step_cnt[e] + i + 1, and the
// update step t fills slot t / every - step_cnt[e] / every - 1.
// All arithmetic is f64 and this file is compiled with -ffp-contract=off: (f64(v) * conc_scale - lo) / scale is the host's
// ((window - lo) / scale).to(float32) operation for operation, and the mean adds in numpy's order (np_mean below), since the
// reference calls np.mean on a Python list.  No atomics; nothing depends on the launch shape.
#include "common.h"

constexpr int TH_WIN_MAX = 32;

__global__ __launch_bounds__(256) void threshold_windows_kernel(const float* __restrict__ series, int64_t row_stride,
                                                                int64_t elem_stride, int steps, int S,
                                                                const uint8_t* __restrict__ active, const float* __restrict__ hist,
                                                                const int32_t* __restrict__ step_cnt, int window, int every,
                                                                int min_steps, double lo, double scale, double conc_scale,
                                                                float* __restrict__ x, int64_t total) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int j = (int)(g % window);
    const int64_t row = g / window;
    const int s = (int)(row % S);
    const int64_t e = row / S;
    float out = 0.f;
    if (active == nullptr || active[e] != 0) {
        int cnt = step_cnt[e];
        cnt = cnt < 0 ? 0 : cnt;
        const int64_t t = ((int64_t)(cnt / every) + s + 1) * every;          // the update step of slot s, if the chunk reaches it
        const int64_t i = t - cnt - 1;
        const int64_t t_min = window > min_steps ? window : min_steps;
        if (i < steps && t >= t_min) {
            const int fill = cnt < window - 1 ? cnt : window - 1;
            const int64_t p = fill + i + 1 - window + j;                     // position in (hist rows 0 .. fill - 1, then series[0 .. i])
            const float v = p < fill ? hist[e * (window - 1) + p] : series[e * row_stride + (p - fill) * elem_stride];
            out = (float)(((double)v * conc_scale - lo) / scale);
        }
    }
    x[g] = out;
}

// np.mean of a(0) .. a(w - 1), f64: numpy's add.reduce sums a contiguous run of fewer than 8 elements one by one and a longer one
// (up to 128) in eight interleaved accumulators, combined pairwise, with the remainder added behind.
template <class A>
__device__ __forceinline__ double np_mean(int w, A a) {
    double res;
    if (w < 8) {
        res = 0.0;
        for (int k = 0; k < w; ++k) res += a(k);
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a(j);
        int k = 8;
        for (; k < w - w % 8; k += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += a(k + j);
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; k < w; ++k) res += a(k);
    }
    return res / (double)w;
}

__global__ __launch_bounds__(64) void threshold_rule_kernel(const float* __restrict__ series, int64_t row_stride, int64_t elem_stride,
                                                            int n, int steps, int S, const uint8_t* __restrict__ active,
                                                            float* __restrict__ hist, int32_t* __restrict__ step_cnt, int window,
                                                            int every, int min_steps, double conc_scale, double factor,
                                                            const float* __restrict__ pred, double* __restrict__ thr,
                                                            int32_t* __restrict__ first_hit, uint8_t* __restrict__ stop,
                                                            double* __restrict__ thr_out) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    uint8_t* stop_row = stop ? stop + (int64_t)e * steps : nullptr;
    double* thr_row = thr_out ? thr_out + (int64_t)e * steps : nullptr;
    double th = thr[e];
    if (active != nullptr && active[e] == 0) {
        first_hit[e] = -1;
        for (int i = 0; i < steps; ++i) {
            if (stop_row) stop_row[i] = 0;
            if (thr_row) thr_row[i] = th;
        }
        return;
    }
    int cnt = step_cnt[e];
    cnt = cnt < 0 ? 0 : cnt;
    const int fill = cnt < window - 1 ? cnt : window - 1;
    float* hr = hist + (int64_t)e * (window - 1);
    const float* sr = series + (int64_t)e * row_stride;
    const float* pr = pred + (int64_t)e * S;
    const int64_t t_min = window > min_steps ? window : min_steps;
    const int slot0 = cnt / every + 1;
    int first = -1;
    for (int i = 0; i < steps; ++i) {
        const int64_t t = (int64_t)cnt + i + 1;
        if (t % every == 0 && t >= t_min) th = (double)pr[(int)(t / every) - slot0] * factor;
        const double cur = (double)sr[(int64_t)i * elem_stride] * conc_scale;
        bool hit = false;
        if (t >= min_steps && !(th != th)) {
            hit = cur >= th;
            if (!hit && t >= window) {
                const int base = fill + i + 1 - window;          // >= 0 since t >= window
                const double mean = np_mean(window, [&](int k) -> double {
                    const int p = base + k;
                    const float v = p < fill ? hr[p] : sr[(int64_t)(p - fill) * elem_stride];
                    return (double)v * conc_scale;
                });
                hit = mean >= th;
            }
        }
        if (hit && first < 0) first = i;
        if (stop_row) stop_row[i] = hit ? 1 : 0;
        if (thr_row) thr_row[i] = th;
    }
    first_hit[e] = first;
    thr[e] = th;
    // the env's last window - 1 inputs in time order, oldest first (in place: slot q takes position shift + q >= q of the old
    // sequence, so ascending q never reads a slot it has already written)
    const int64_t total = (int64_t)fill + steps;
    const int nfill = total < window - 1 ? (int)total : window - 1;
    const int64_t shift = total - nfill;
    for (int q = 0; q < nfill; ++q) {
        const int64_t p = shift + q;
        hr[q] = p < fill ? hr[p] : sr[(p - fill) * elem_stride];
    }
    step_cnt[e] = cnt + steps;
}

static int th_check_common(const char* who, int window, int every, int n, int steps) {
    UAV_REQUIRE(window >= 1 && window <= TH_WIN_MAX, "%s: window=%d (1 .. %d)", who, window, TH_WIN_MAX);
    UAV_REQUIRE(every >= 1, "%s: every=%d (at least 1)", who, every);
    UAV_REQUIRE(n >= 1 && steps >= 1, "%s: n=%d steps=%d (both at least 1)", who, n, steps);
    return 0;
}

extern "C" {

int uav_threshold_windows(uav_ctx* ctx, const float* series, int64_t row_stride, int64_t elem_stride, int n, int steps,
                          const uint8_t* active, const float* hist, const int32_t* step_cnt, int window, int every, int min_steps,
                          double lo, double scale, double conc_scale, float* x, uav_stream stream) {
    if (int rc = th_check_common("uav_threshold_windows", window, every, n, steps)) return rc;
    UAV_REQUIRE(series, "uav_threshold_windows: NULL series");
    UAV_REQUIRE(hist && step_cnt, "uav_threshold_windows: NULL hist / step_cnt (the window's history buffers)");
    UAV_REQUIRE(x, "uav_threshold_windows: NULL x (the windows)");
    UAV_REQUIRE(ctx, "uav_threshold_windows: NULL handle");
    const int S = (int)(((int64_t)steps + every - 1) / every);
    const int64_t total = (int64_t)n * S * window, nb = (total + 255) / 256;
    UAV_REQUIRE(nb <= 0x7fffffffLL, "uav_threshold_windows: n * slots * window = %lld elements exceed one launch", (long long)total);
    hipLaunchKernelGGL(threshold_windows_kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), series, row_stride, elem_stride,
                       steps, S, active, hist, step_cnt, window, every, min_steps, lo, scale, conc_scale, x, total);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_threshold_rule(uav_ctx* ctx, const float* series, int64_t row_stride, int64_t elem_stride, int n, int steps,
                       const uint8_t* active, float* hist, int32_t* step_cnt, int window, int every, int min_steps, double conc_scale,
                       double factor, const float* pred, double* thr, int32_t* first_hit, uint8_t* stop, double* thr_out,
                       uav_stream stream) {
    if (int rc = th_check_common("uav_threshold_rule", window, every, n, steps)) return rc;
    UAV_REQUIRE(series, "uav_threshold_rule: NULL series");
    UAV_REQUIRE(hist && step_cnt, "uav_threshold_rule: NULL hist / step_cnt (the window's history buffers)");
    UAV_REQUIRE(pred, "uav_threshold_rule: NULL pred");
    UAV_REQUIRE(thr, "uav_threshold_rule: NULL thr");
    UAV_REQUIRE(first_hit, "uav_threshold_rule: NULL first_hit");
    UAV_REQUIRE(ctx, "uav_threshold_rule: NULL handle");
    const int S = (int)(((int64_t)steps + every - 1) / every);
    hipLaunchKernelGGL(threshold_rule_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, as_stream(stream), series, row_stride,
                       elem_stride, n, steps, S, active, hist, step_cnt, window, every, min_steps, conc_scale, factor, pred, thr,
                       first_hit, stop, thr_out);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
