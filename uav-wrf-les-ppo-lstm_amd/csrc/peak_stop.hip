// peak_stop.hip -- the PPOV2.1 peak-and-stop rule over every sliding window of a chunk of concentration records, in one scan.
//
// Reference: PPOV2.1/evaluate_with_lstm.py:11-27 (PeakAndStopPredictor: LSTM(1 -> 32, batch_first) -> h_n -> fc_peak, and
// fc_stop = Linear + Sigmoid) and :69-77 (once the trajectory holds 20 concentrations, feed the last 20, divided by 100, and
// stop when stop_prob > 0.8).  The host loop this replaces fed f32((f64(obs2) * 100) / 100); that round trip returns obs2 bit
// for bit (tests/test_peak_stop_host.py asserts it on millions of f32 values), so the kernel reads obs[2] of the records as is.
//
// Shape of the work.  Every window's pass starts from zero (h, c), so the n * steps windows of a call are independent; they
// are flattened as g = env * steps + step and one wave owns 16 of them at a time as the N columns of v_mfma_f32_16x16x4_f32
// (exact f32: a k-ordered fmaf chain).  With j = lane & 15 the window and kq = lane >> 4:
//   gates[4H x 16] = W_hh[4H x H] h[H x 16]: A = W_hh, 4H / 16 row tiles x H / 4 k-steps, held in registers for the whole launch
//             (64 VGPRs at H = 32); the result leaves lane (j, kq) with rows 16 mt + 4 kq + r of tile mt, r < 4.  Gate q of unit
//             16 s + 4 kq + r is row r of tile q H / 16 + s: a lane holds all four gates of its H / 4 units, so the cell update
//             is lane-local.
//   h as B    The sum over k may walk the units in any order as long as A and B walk it the same way.  k-step ks = 4 s + r
//             takes unit 16 s + 4 kq + r from lane (j, kq) -- exactly the units whose h that lane has just computed.  So h_t
//             goes from the C layout to the B layout with no lane movement and no LDS; the A fragments are loaded in that order.
//   W_ih x_t + b_ih + b_hh   a rank-1 term: the accumulators START at b_ih + b_hh (registers) and w_ih[row] x_t is added behind the
//             MFMAs with one fmaf per row, w_ih read from LDS (512 bytes per workgroup) while the MFMAs run.
//   heads     8 lane-local products per head, then a sum over the 4 lanes of a window (xor 16, 32): the same bits in all four.
// A window's bits depend on its own 20 inputs and on nothing else (not on its column, its wave or the launch's shape): column
// j of an MFMA result is a function of column j of B alone.  Hence k calls of steps / k equal one call bit for bit, and a NaN
// in one window's inputs stays in that window.
// A tile whose 16 windows are all invalid (the env's history is still short) or inactive runs no LSTM step: it only stores its
// NaNs.  In a mixed tile the invalid columns ride along on zeros for free.
// first_hit and hist.  The scan leaves one hit byte per window in the handle's workspace; peak_stop_finish_kernel (one thread
// per env, a second, tiny launch behind it) takes the first hit of every env and then shifts the env's history: the scan's early
// windows READ hist, so it cannot be rewritten while the scan runs.  No atomics anywhere.
// Arithmetic floor: 4H / 16 x H / 4 = 64 MFMAs per LSTM step and tile, 32 cycles each on one SIMD: 20 steps = 41 k cycles per
// tile; 1000 x 50 windows are 3,125 tiles over 1,024 SIMDs.  The gate activations (40 per lane and step) are VALU work of the
// same order, which is why two waves share a SIMD (launch bounds (256, 2): one's MFMAs under the other's activations).
// H is a template parameter; only 32 (the reference's value everywhere) is instantiated: at H = 64 the A fragments alone are
// 256 VGPRs and would have to live in LDS.
#include "common.h"

constexpr int PS_WIN_MAX = 32;

static inline size_t ps_params(int H) { return (size_t)4 * H + (size_t)4 * H * H + 4 * H + 4 * H + H + 1 + H + 1; }

template <int H>
struct PsW {                // a lane's share of the parameters
    static constexpr int S = H / 16, MT = 4 * S, KS = H / 4;
    float whh[MT][KS];      // W_hh[16 mt + j][16 s + 4 kq + r] at ks = 4 s + r
    f32x4 b[MT];            // rows 16 mt + 4 kq + r: bias_ih + bias_hh
    __device__ __forceinline__ void load(const float* __restrict__ p, int j, int kq) {
        const float* w_hh = p + 4 * H;
        const float* b_ih = w_hh + 4 * H * H;
        const float* b_hh = b_ih + 4 * H;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) whh[mt][ks] = w_hh[(16 * mt + j) * H + 16 * (ks >> 2) + 4 * kq + (ks & 3)];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mt + 4 * kq + r;
                b[mt][r] = b_ih[row] + b_hh[row];
            }
        }
    }
};

template <int H>
__global__ __launch_bounds__(256, 2) void peak_stop_scan_kernel(const float* __restrict__ params, int window,
                                                                const float* __restrict__ series, int64_t row_stride,
                                                                int64_t elem_stride, int n, int steps,
                                                                const uint8_t* __restrict__ active, const float* __restrict__ hist,
                                                                const int32_t* __restrict__ hist_cnt, float prob_min,
                                                                float* __restrict__ peak, float* __restrict__ prob,
                                                                uint8_t* __restrict__ hit, int64_t ntile) {
    typedef PsW<H> W_t;
    constexpr int S = W_t::S, MT = W_t::MT, KS = W_t::KS;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
    const int64_t ntot = (int64_t)n * steps;
    const float nanf_ = __builtin_nanf("");
    __shared__ float heads[2 * H + 2];       // fc_peak.weight, fc_peak.bias, fc_stop.0.weight, fc_stop.0.bias: read once per tile
    __shared__ f32x4 wih[H];                 // weight_ih_l0 as rows 4 q .. 4 q + 3: read under each step's MFMAs
    for (int i = threadIdx.x; i < 4 * H; i += 256) ((float*)wih)[i] = params[i];
    for (int i = threadIdx.x; i < 2 * H + 2; i += 256) heads[i] = params[4 * H + 4 * H * H + 8 * H + i];
    __syncthreads();
    W_t W;
    W.load(params, j, kq);
    for (int64_t tile = (int64_t)blockIdx.x * 4 + w; tile < ntile; tile += (int64_t)gridDim.x * 4) {
        const int64_t g = tile * 16 + j;
        // ---- the window of column j: positions p0 .. p0 + window - 1 of (hist rows 0 .. cnt - 1, then series[0 .. i])
        bool valid = false;
        int cnt = 0, p0 = 0;
        const float* hrow = hist;
        const float* srow = series;
        if (g < ntot) {
            const int e = (int)(g / steps), i = (int)(g - (int64_t)e * steps);
            cnt = hist_cnt[e];
            cnt = cnt < 0 ? 0 : (cnt > window - 1 ? window - 1 : cnt);
            p0 = cnt + i + 1 - window;
            valid = p0 >= 0 && (active == nullptr || active[e] != 0);
            hrow = hist + (int64_t)e * (window - 1);
            srow = series + (int64_t)e * row_stride;
        }
        float pk = nanf_, pr = nanf_;
        if (__any(valid)) {
            auto x_at = [&](int t) -> float {
                const int p = p0 + t;
                if (!valid) return 0.f;
                return p < cnt ? hrow[p] : srow[(int64_t)(p - cnt) * elem_stride];
            };
            float h[KS], c[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) h[ks] = c[ks] = 0.f;
            float xn = x_at(0);
            for (int t = 0; t < window; ++t) {
                const float x = xn;
                if (t + 1 < window) xn = x_at(t + 1);
                f32x4 acc[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = W.b[mt];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(W.whh[mt][ks], h[ks], acc[mt], 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const f32x4 wi = wih[4 * mt + kq];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[mt][r] = __builtin_fmaf(wi[r], x, acc[mt][r]);
                }
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {           // gate order i, f, g, o (nn.LSTM)
                        const float gi = fast_sigmoid(acc[s][r]), gf = fast_sigmoid(acc[S + s][r]);
                        const float gg = fast_tanh(acc[2 * S + s][r]), go = fast_sigmoid(acc[3 * S + s][r]);
                        const float cc = __builtin_fmaf(gf, c[4 * s + r], gi * gg);
                        c[4 * s + r] = cc;
                        h[4 * s + r] = go * fast_tanh(cc);
                    }
            }
            float sp = 0.f, ss = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int u = 16 * (ks >> 2) + 4 * kq + (ks & 3);
                sp = __builtin_fmaf(heads[u], h[ks], sp);
                ss = __builtin_fmaf(heads[H + 1 + u], h[ks], ss);
            }
            sp += __shfl_xor(sp, 16, 64);
            sp += __shfl_xor(sp, 32, 64);
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            if (valid) {
                pk = sp + heads[H];
                pr = fast_sigmoid(ss + heads[2 * H + 1]);
            }
        }
        if (kq == 0 && g < ntot) {
            if (peak) peak[g] = pk;
            if (prob) prob[g] = pr;
            hit[g] = (valid && pr > prob_min) ? 1 : 0;          // a NaN probability is no hit
        }
    }
}

// one thread per env: first hit of the chunk, then the env's last window - 1 inputs in time order, oldest first (in place: slot q
// takes position shift + q >= q of the old sequence, so ascending q never reads a slot it has already written)
__global__ __launch_bounds__(256) void peak_stop_finish_kernel(int window, const float* __restrict__ series, int64_t row_stride,
                                                               int64_t elem_stride, int n, int steps,
                                                               const uint8_t* __restrict__ active, float* __restrict__ hist,
                                                               int32_t* __restrict__ hist_cnt, const uint8_t* __restrict__ hit,
                                                               int32_t* __restrict__ first_hit) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (active != nullptr && active[e] == 0) {
        first_hit[e] = -1;
        return;
    }
    int first = -1;
    const uint8_t* hrow = hit + (int64_t)e * steps;
    for (int i = 0; i < steps; ++i)
        if (hrow[i]) {
            first = i;
            break;
        }
    first_hit[e] = first;
    int cnt = hist_cnt[e];
    cnt = cnt < 0 ? 0 : (cnt > window - 1 ? window - 1 : cnt);
    const int64_t total = (int64_t)cnt + steps;
    const int ncnt = total < window - 1 ? (int)total : window - 1;
    const int64_t shift = total - ncnt;
    float* hr = hist + (int64_t)e * (window - 1);
    const float* sr = series + (int64_t)e * row_stride;
    for (int q = 0; q < ncnt; ++q) {
        const int64_t p = shift + q;
        hr[q] = p < cnt ? hr[p] : sr[(p - cnt) * elem_stride];
    }
    hist_cnt[e] = ncnt;
}

static int ps_check_hidden(const char* who, int hidden) {
    UAV_REQUIRE(hidden == 32, "%s: hidden=%d unsupported (the peak-and-stop predictor's kernel is built for hidden 32)", who, hidden);
    return 0;
}

extern "C" {

size_t uav_peak_stop_param_count(int hidden) {
    if (ps_check_hidden("uav_peak_stop_param_count", hidden) != 0) return 0;
    return ps_params(hidden);
}

int uav_peak_stop_scan(uav_ctx* ctx, const float* params, int hidden, int window, const float* series, int64_t row_stride,
                       int64_t elem_stride, int n, int steps, const uint8_t* active, float* hist, int32_t* hist_cnt, float prob_min,
                       float* peak, float* prob, int32_t* first_hit, uav_stream stream) {
    if (int rc = ps_check_hidden("uav_peak_stop_scan", hidden)) return rc;
    UAV_REQUIRE(window >= 1 && window <= PS_WIN_MAX, "uav_peak_stop_scan: window=%d (1 .. %d)", window, PS_WIN_MAX);
    UAV_REQUIRE(n >= 1 && steps >= 1, "uav_peak_stop_scan: n=%d steps=%d (both at least 1)", n, steps);
    UAV_REQUIRE(params && series, "uav_peak_stop_scan: NULL params / series");
    UAV_REQUIRE(hist && hist_cnt, "uav_peak_stop_scan: NULL hist / hist_cnt (the window's history buffers)");
    UAV_REQUIRE(first_hit, "uav_peak_stop_scan: NULL first_hit");
    UAV_REQUIRE(ctx, "uav_peak_stop_scan: NULL handle");
    const int64_t ntot = (int64_t)n * steps, ntile = (ntot + 15) / 16;
    UAV_REQUIRE((size_t)ntot <= ctx->ws_bytes, "uav_peak_stop_scan: n * steps = %lld hit bytes do not fit the workspace of %zu bytes",
                (long long)ntot, ctx->ws_bytes);
    uint8_t* hit = (uint8_t*)ctx->ws;
    int64_t nb = (ntile + 3) / 4;
    if (nb > 2 * (int64_t)ctx->num_cu) nb = 2 * (int64_t)ctx->num_cu;
    hipLaunchKernelGGL(peak_stop_scan_kernel<32>, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), params, window, series,
                       row_stride, elem_stride, n, steps, active, (const float*)hist, (const int32_t*)hist_cnt, prob_min, peak, prob,
                       hit, ntile);
    hipLaunchKernelGGL(peak_stop_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), window, series,
                       row_stride, elem_stride, n, steps, active, hist, hist_cnt, (const uint8_t*)hit, first_hit);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
