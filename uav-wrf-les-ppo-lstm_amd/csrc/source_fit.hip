// source_fit.hip -- where the measurements of a greedy episode say the plume's source is, on the device (no counterpart in the
// reference, whose GaussianParamPredictor is an untrained regressor; uavppo/source_fit.py states every line in numpy).
//
// The field (env_core.h field_at) is 100 exp(-d^2 / 2 sigma^2) + tke clipped to 0 .. 100, and a record carries conc / 100 (obs[2])
// and tke / 9 (obs[3]) of the cell it was sampled in: the plume term b is known per record, and ln b is linear in (1, x, y, x^2 + y^2).
//
//   S1  moments   one chunk of greedy records -> per env the weighted normal equations A = sum w phi phi^T, g = sum w phi ln b
//                 (w = b^2, Guo's weighting), the count, the centre and the largest sample.  One wave per env, registers only.
//   S2  solve     per env: scaled Cholesky of A, a0 .. a3 -> mu, sigma, peak, strength and a status.  One thread per env, f64.
//   S3  summary   twelve sums of an evaluation against the true sources, in uav_greedy_summary's ONE order of summation.
//
// Nothing is read by the host between them.  The order of every sum and of every operation of S2 is fixed: S1's integers, centre, A
// and largest sample, S2's status, mu and sigma and all of S3 equal the numpy statement bit for bit; g goes through log, peak
// through exp.
#include "common.h"

constexpr int FLAG_DONE = 1, FLAG_SKIP = 4, FLAG_RULE = 8;      // record flags: bit0 done, bit2 not stepped, bit3 rule fired
constexpr int ST_COUNT = 0, ST_CX = 1, ST_CY = 2, ST_A = 3, ST_G = 13, ST_BMAX = 17, ST_XMAX = 18, ST_YMAX = 19;
constexpr int N_ACC = 15;                                       // count | A (10, upper triangle by rows) | g (4)
constexpr double CELL_SCALE = 32.0;                             // p = (x - cx) / 32: exact in f64, |p| < 16

// the cell field_at sampled: min(max((int)v, 0), 499), clamped as a float first so that a NaN or a huge v is defined (cell 0 / 499)
__device__ __forceinline__ int cell_of(float v) { return (int)fminf(fmaxf(v, 0.0f), 499.0f); }

__global__ __launch_bounds__(256) void source_moments_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ obs,
                                                             const float* __restrict__ pos, int n, int k, int D, int use_tke,
                                                             double background, double floor_b, const uint8_t* __restrict__ ended,
                                                             double* __restrict__ state) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);        // wave-uniform
    if (row >= n) return;
    if (ended && ended[row]) return;                            // ended in an earlier chunk: left alone to the bit
    double* st = state + (int64_t)row * UAV_SRC_STATE_N;
    bool have_c = st[ST_COUNT] > 0.0;                           // the centre is fixed by the first used record of the episode
    double cx = st[ST_CX], cy = st[ST_CY];
    double acc[N_ACC];
#pragma unroll
    for (int j = 0; j < N_ACC; ++j) acc[j] = 0.0;
    double bm = 0.0;                                            // this lane's largest b (a used b is > floor >= 0), its record, its cell
    int bi = -1, bx = 0, by = 0;
    const uint8_t* f = flags + (int64_t)row * k;
    for (int base = 0; base < k; base += 64) {                  // wave-uniform trip count
        const int i = base + lane;
        const uint8_t v = i < k ? f[i] : (uint8_t)FLAG_SKIP;
        const bool end = !(v & FLAG_SKIP) && (v & (FLAG_DONE | FLAG_RULE));
        const unsigned long long m = __ballot(end);
        const int last = m ? __builtin_ctzll(m) : 63;
        const bool take = !(v & FLAG_SKIP) && lane <= last;     // up to and including the ending record; a bit2 record is never read
        int x = 0, y = 0;
        double b = 0.0;
        bool used = false;
        if (take) {
            const int64_t rec = (int64_t)row * k + i;
            const float o2 = obs[rec * D + 2];
            const float2 xy = *reinterpret_cast<const float2*>(pos + rec * 2);
            x = cell_of(xy.x);
            y = cell_of(xy.y);
            if (use_tke) {
                const float o3 = obs[rec * D + 3];
                b = 100.0 * (double)o2 - 9.0 * (double)o3;
            } else {
                b = 100.0 * (double)o2 - background;
            }
            used = b > floor_b && o2 < 1.0f;                    // false for a NaN; obs[2] == 1: the cell was clipped at 100
        }
        const unsigned long long mu = __ballot(used);
        if (!have_c && mu) {                                    // wave-uniform
            const int src = __builtin_ctzll(mu);
            cx = (double)__shfl(x, src, 64);
            cy = (double)__shfl(y, src, 64);
            have_c = true;
        }
        if (used) {
            const double p = ((double)x - cx) / CELL_SCALE, q = ((double)y - cy) / CELL_SCALE;
            const double r = p * p + q * q;
            const double w = b * b, lb = log(b);
            const double wp = w * p, wq = w * q, wr = w * r;
            acc[0] += 1.0;
            acc[1] += w;
            acc[2] += wp;
            acc[3] += wq;
            acc[4] += wr;
            acc[5] += wp * p;
            acc[6] += wp * q;
            acc[7] += wp * r;
            acc[8] += wq * q;
            acc[9] += wq * r;
            acc[10] += wr * r;
            acc[11] += w * lb;
            acc[12] += wp * lb;
            acc[13] += wq * lb;
            acc[14] += wr * lb;
            if (b > bm) {                                       // strictly: the earliest record of the lane wins a tie
                bm = b;
                bi = i;
                bx = x;
                by = y;
            }
        }
        if (m) break;                                           // nothing behind the ending block is read
    }
#pragma unroll
    for (int j = 0; j < N_ACC; ++j) acc[j] = wave_sum(acc[j]);  // lane l += lane l + 32, 16, ... 1
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                          // the largest b; of equal ones the earliest record
        const double ob = __shfl_down(bm, o, 64);
        const int oi = __shfl_down(bi, o, 64);
        if (lane + o < 64 && oi >= 0 && (bi < 0 || ob > bm || (ob == bm && oi < bi))) {
            bm = ob;
            bi = oi;
        }
    }
    const int wi = __shfl(bi, 0, 64);                           // record i was lane i % 64's
    const int wl = wi >= 0 ? (wi & 63) : 0;
    const int wx = __shfl(bx, wl, 64), wy = __shfl(by, wl, 64);
    if (lane != 0) return;
    st[ST_COUNT] += acc[0];
    st[ST_CX] = cx;
    st[ST_CY] = cy;
#pragma unroll
    for (int j = 1; j < N_ACC; ++j) st[ST_A + j - 1] += acc[j];
    if (wi >= 0 && bm > st[ST_BMAX]) {                          // strictly: an earlier chunk's record wins a tie
        st[ST_BMAX] = bm;
        st[ST_XMAX] = (double)wx;
        st[ST_YMAX] = (double)wy;
    }
}

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

// One thread per env: source_fit.solve line by line.  A is held by rows of its upper triangle: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2)
// (1,3) (2,2) (2,3) (3,3).
__global__ __launch_bounds__(256) void source_solve_kernel(const double* __restrict__ state, int n, double min_samples,
                                                           double min_pivot, double* __restrict__ est, uint8_t* __restrict__ status) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double* st = state + (int64_t)e * UAV_SRC_STATE_N;
    double* out = est + (int64_t)e * UAV_SRC_EST_N;
    const double nan = __builtin_nan("");
    const double count = st[ST_COUNT];
#pragma unroll
    for (int j = 0; j < 5; ++j) out[j] = nan;
    const bool any = count > 0.0;
    out[5] = any ? st[ST_XMAX] : nan;
    out[6] = any ? st[ST_YMAX] : nan;
    out[7] = any ? st[ST_BMAX] : nan;
    if (!(count >= min_samples)) {
        status[e] = UAV_SRC_FEW;
        return;
    }
    constexpr int IDX[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
    double d[4], S[4][4], L[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = sqrt(st[ST_A + IDX[j][j]]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) S[i][j] = st[ST_A + IDX[i][j]] / (d[i] * d[j]);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double s = S[j][j];
#pragma unroll
        for (int c = 0; c < j; ++c) s = s - L[j][c] * L[j][c];
        ok = ok && finite_d(s) && s >= min_pivot;               // a NaN fails both
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double t = S[i][j];
#pragma unroll
            for (int c = 0; c < j; ++c) t = t - L[i][c] * L[j][c];
            L[i][j] = t / L[j][j];
        }
    }
    if (!ok) {
        status[e] = UAV_SRC_DEGENERATE;
        return;
    }
    double z[4], u[4], a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double t = st[ST_G + j] / d[j];
#pragma unroll
        for (int c = 0; c < j; ++c) t = t - L[j][c] * z[c];
        z[j] = t / L[j][j];
    }
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        double t = z[j];
#pragma unroll
        for (int c = j + 1; c < 4; ++c) t = t - L[c][j] * u[c];
        u[j] = t / L[j][j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = u[j] / d[j];
    const double s2 = -1.0 / (2.0 * a[3]);
    if (!(finite_d(a[0]) && finite_d(a[1]) && finite_d(a[2]) && finite_d(a[3]) && a[3] < 0.0 && finite_d(s2))) {
        status[e] = UAV_SRC_NOT_A_PEAK;
        return;
    }
    const double sigma = CELL_SCALE * sqrt(s2);
    const double peak = exp(a[0] + (a[1] * a[1] + a[2] * a[2]) * s2 / 2.0);
    out[0] = st[ST_CX] + CELL_SCALE * a[1] * s2;
    out[1] = st[ST_CY] + CELL_SCALE * a[2] * s2;
    out[2] = sigma;
    out[3] = peak;
    out[4] = 6.283185307179586 * (sigma * sigma) * peak;
    status[e] = UAV_SRC_FITTED;
}

// uav_greedy_summary's order of summation: thread j of ONE block of 256 adds the envs j, j + 256, ... one after the other, then
// block256_sum's tree.  source_fit.summarise is this order.
__global__ __launch_bounds__(256) void source_summary_kernel(const double* __restrict__ est, const uint8_t* __restrict__ status,
                                                             const double* __restrict__ src, int n, double sigma_true, double peak_true,
                                                             double loc_tol, double* __restrict__ loc_err, double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    double s[UAV_SRC_SUM_N - 1];
#pragma unroll
    for (int j = 0; j < UAV_SRC_SUM_N - 1; ++j) s[j] = 0.0;
    const bool sig_known = finite_d(sigma_true) && sigma_true > 0.0, peak_known = finite_d(peak_true) && peak_true > 0.0;
    for (int e = threadIdx.x; e < n; e += 256) {
        const double* o = est + (int64_t)e * UAV_SRC_EST_N;
        const int stt = status[e];
        const double sx = src[2 * e], sy = src[2 * e + 1];
        double err = __builtin_nan("");
        s[0] += stt == UAV_SRC_FITTED ? 1.0 : 0.0;
        s[1] += stt == UAV_SRC_FEW ? 1.0 : 0.0;
        s[2] += stt == UAV_SRC_DEGENERATE ? 1.0 : 0.0;
        s[3] += stt == UAV_SRC_NOT_A_PEAK ? 1.0 : 0.0;
        if (stt == UAV_SRC_FITTED) {
            const double dx = o[0] - sx, dy = o[1] - sy;
            err = sqrt(dx * dx + dy * dy);
            s[4] += err;
            s[5] += err * err;
            s[6] += err <= loc_tol ? 1.0 : 0.0;                 // false for a NaN
            if (sig_known) s[7] += fabs(o[2] - sigma_true) / sigma_true;
            if (peak_known) s[8] += fabs(o[3] - peak_true) / peak_true;
        }
        if (o[7] == o[7]) {                                     // the env has a largest sample
            const double dx = o[5] - sx, dy = o[6] - sy;
            s[9] += sqrt(dx * dx + dy * dy);
            s[10] += 1.0;
        }
        if (loc_err) loc_err[e] = err;
    }
#pragma unroll
    for (int j = 0; j < UAV_SRC_SUM_N - 1; ++j) {
        const double a = block256_sum(s[j], sm);
        if (threadIdx.x == 0) sums[1 + j] = a;
    }
    if (threadIdx.x == 0) sums[UAV_SRC_SUM_ENVS] = (double)n;
}

static int source_cfg_ok(const uav_source_fit_cfg* cfg, const char* who) {
    UAV_REQUIRE(cfg, "%s: NULL cfg", who);
    UAV_REQUIRE(cfg->use_tke == 0 || cfg->use_tke == 1, "%s: use_tke=%d must be 0 or 1", who, cfg->use_tke);
    UAV_REQUIRE(cfg->min_samples >= 4, "%s: min_samples=%d must be at least 4 (four parameters)", who, cfg->min_samples);
    UAV_REQUIRE(cfg->floor - cfg->floor == 0.0 && cfg->floor >= 0.0, "%s: floor=%g must be finite and not negative", who, cfg->floor);
    UAV_REQUIRE(cfg->background - cfg->background == 0.0, "%s: background=%g must be finite", who, cfg->background);
    UAV_REQUIRE(cfg->min_pivot - cfg->min_pivot == 0.0 && cfg->min_pivot > 0.0, "%s: min_pivot=%g must be finite and positive", who,
                cfg->min_pivot);
    return 0;
}

extern "C" {

int uav_source_moments(uav_ctx* ctx, const uint8_t* flags, const float* obs, const float* pos, int n, int k, int D,
                       const uav_source_fit_cfg* cfg, const uint8_t* ended, double* state, uav_stream stream) {
    UAV_REQUIRE(ctx && flags && obs && pos && state, "uav_source_moments: NULL argument");
    if (int rc = source_cfg_ok(cfg, "uav_source_moments")) return rc;
    UAV_REQUIRE(n >= 1 && k >= 1, "uav_source_moments: n=%d, k=%d must be at least 1", n, k);
    UAV_REQUIRE(D >= (cfg->use_tke ? 4 : 3), "uav_source_moments: D=%d must be at least %d (obs[2]%s)", D, cfg->use_tke ? 4 : 3,
                cfg->use_tke ? " and obs[3]" : "");
    UAV_REQUIRE((int64_t)n * k * D < (int64_t)1 << 31, "uav_source_moments: n * k * D = %lld is 2^31 or more", (long long)n * k * D);
    UAV_REQUIRE(((uintptr_t)pos & 7) == 0, "uav_source_moments: pos is not 8-byte aligned");
    hipLaunchKernelGGL(source_moments_kernel, dim3((n + 3) / 4), dim3(256), 0, as_stream(stream), flags, obs, pos, n, k, D,
                       (int)cfg->use_tke, cfg->background, cfg->floor, ended, state);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_source_solve(uav_ctx* ctx, const double* state, int n, const uav_source_fit_cfg* cfg, double* est, uint8_t* status,
                     uav_stream stream) {
    UAV_REQUIRE(ctx && state && est && status, "uav_source_solve: NULL argument");
    if (int rc = source_cfg_ok(cfg, "uav_source_solve")) return rc;
    UAV_REQUIRE(n >= 1, "uav_source_solve: n=%d must be at least 1", n);
    hipLaunchKernelGGL(source_solve_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), state, n, (double)cfg->min_samples,
                       cfg->min_pivot, est, status);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_source_summary(uav_ctx* ctx, const double* est, const uint8_t* status, const double* src, int n, double sigma_true,
                       double peak_true, double loc_tol, double* loc_err, double* sums, uav_stream stream) {
    UAV_REQUIRE(ctx && est && status && src && sums, "uav_source_summary: NULL argument");
    UAV_REQUIRE(n >= 1, "uav_source_summary: n=%d must be at least 1", n);
    UAV_REQUIRE(loc_tol == loc_tol, "uav_source_summary: loc_tol is a NaN");
    hipLaunchKernelGGL(source_summary_kernel, dim3(1), dim3(256), 0, as_stream(stream), est, status, src, n, sigma_true, peak_true,
                       loc_tol, loc_err, sums);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
