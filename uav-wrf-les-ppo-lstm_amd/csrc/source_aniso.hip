// source_aniso.hip -- anisotropic plumes: a field generator and the six-term source estimator (uavppo/source_aniso.py states every
// line in numpy).
//
// A plume stretched along the wind is an elliptical Gaussian centred on the source: with (u, v) the offset from the source in the
// ellipse's frame, base = peak exp(-(u^2 / 2 sigma_major^2 + v^2 / 2 sigma_minor^2)).  A record still carries conc / 100 and
// tke / 9 of its cell, so b is known per record and ln b is a full quadratic in the cell: linear in SIX parameters.
//
//   P1  plume bank  [F][500][500][2] (conc, tke) fields of such plumes with E3's turbulence: what materialised-field mode reads.
//   A1  moments6    source_fit.hip's S1 with phi = (1, p, q, p p, p q, q q): A (21), g (6).  One wave per env, registers only.
//   A2  solve6      scaled Cholesky of the 6 x 6 system, a0 .. a5 -> mu, both widths, the axis angle, peak, strength, a status.
//   A3  summary6    sixteen sums against the true sources and per-env truth, in uav_greedy_summary's ONE order of summation.
//
// Record eligibility, the centre, p and q, b and w, chunking, `ended` and the largest sample are S1's, restated here line by line
// (the kernels of source_fit.hip are not touched).  f64 throughout, no LDS beyond block256_sum's four slots, no atomics; nothing
// is read by the host.
#include "env_core.h"

namespace {

constexpr int FLAG_DONE = 1, FLAG_SKIP = 4, FLAG_RULE = 8;      // record flags: bit0 done, bit2 not stepped, bit3 rule fired
constexpr int N_PHI = 6, N_A = 21, N_ACC6 = 1 + N_A + N_PHI;    // count | A (upper triangle by rows) | g
constexpr int S6_COUNT = 0, S6_CX = 1, S6_CY = 2, S6_A = 3, S6_G = S6_A + N_A, S6_BMAX = S6_G + N_PHI, S6_XMAX = S6_BMAX + 1,
              S6_YMAX = S6_BMAX + 2;
static_assert(S6_YMAX + 1 == UAV_SRC6_STATE_N, "state layout");
constexpr double CELL_SCALE = 32.0;                             // p = (x - cx) / 32: exact in f64, |p| < 16
constexpr double PI_D = 3.141592653589793, TWO_PI_D = 6.283185307179586;

__device__ __forceinline__ int cell_of(float v) { return (int)fminf(fmaxf(v, 0.0f), 499.0f); }
__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }
// (i, j), i <= j, of the upper triangle by rows
__host__ __device__ constexpr int tri(int i, int j) { return i * N_PHI - i * (i - 1) / 2 + (j - i); }
static_assert(tri(0, 0) == 0 && tri(1, 1) == 6 && tri(5, 5) == 20, "triangle index");

// P1: one thread per cell, blockIdx.y = the field.  tke is field_at's procedural branch line by line (same key, same order).
// The parameters of up to PLUME_BATCH fields travel as kernel arguments (the caller's rows are host memory, checked on the host):
// no device buffer, no copy, nothing to wait for.
constexpr int PLUME_BATCH = 32;
struct PlumeBatch { double p[PLUME_BATCH][UAV_PLUME_PARAM_N]; };

__global__ __launch_bounds__(256) void plume_bank_kernel(PlumeBatch params, uint64_t seed, int index0,
                                                         const double* __restrict__ wave, const double* __restrict__ ftab,
                                                         double* __restrict__ bank) {
#pragma clang fp contract(off)
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= GRID * GRID) return;
    const int f = blockIdx.y;                                    // the field within this launch: index0 and bank are its first's
    const double* pr = params.p[f];                              // block-uniform
    const int x = cell / GRID, y = cell % GRID;
    const Philox4 r = philox4x32_10(seed, (uint32_t)(x * GRID + y), (uint32_t)(index0 + f), 0u, RNG_FIELD);
    double gs, gc;
    ft_sincos_u24(r.y >> 8, ftab, gs, gc);
    const double g = bm_radius(r.x, ftab) * gc;
    const double un = (double)r.w * (1.0 / 4294967296.0);
    const double wv = (0.3 * wave[x]) * wave[GRID + y];
    const double tke = 3.0 * ((fabs(g) + wv) + 0.2 * un);
    const double s1 = pr[2], s2 = pr[3], cs = pr[4], sn = pr[5];
    const double dx = (double)x - pr[0], dy = (double)y - pr[1];
    const double u = dx * cs + dy * sn;
    const double v = dy * cs - dx * sn;
    const double e = u * u / (2.0 * (s1 * s1)) + v * v / (2.0 * (s2 * s2));
    const double base = e <= 300.0 ? pr[6] * ft_exp_neg(-e, ftab) : 0.0;
    const double c = base + tke;
    double* out = bank + ((size_t)f * (GRID * GRID) + (size_t)cell) * 2;
    *reinterpret_cast<double2*>(out) = make_double2(c < 0.0 ? 0.0 : (c > 100.0 ? 100.0 : c), tke);
}

// A1: source_moments_kernel of source_fit.hip with six basis functions.
__global__ __launch_bounds__(256) void source_moments6_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ obs,
                                                              const float* __restrict__ pos, int n, int k, int D, int use_tke,
                                                              double background, double floor_b, const uint8_t* __restrict__ ended,
                                                              double* __restrict__ state) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);        // wave-uniform
    if (row >= n) return;
    if (ended && ended[row]) return;                            // ended in an earlier chunk: left alone to the bit
    double* st = state + (int64_t)row * UAV_SRC6_STATE_N;
    bool have_c = st[S6_COUNT] > 0.0;                           // the centre is fixed by the first used record of the episode
    double cx = st[S6_CX], cy = st[S6_CY];
    double acc[N_ACC6];
#pragma unroll
    for (int j = 0; j < N_ACC6; ++j) acc[j] = 0.0;
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
            const double w = b * b, lb = log(b);
            double phi[N_PHI], wphi[N_PHI];
            phi[0] = 1.0;
            phi[1] = p;
            phi[2] = q;
            phi[3] = p * p;
            phi[4] = p * q;
            phi[5] = q * q;
            wphi[0] = w;
#pragma unroll
            for (int j = 1; j < N_PHI; ++j) wphi[j] = w * phi[j];
            acc[0] += 1.0;
#pragma unroll
            for (int a = 0; a < N_PHI; ++a) {
#pragma unroll
                for (int c = a; c < N_PHI; ++c) acc[1 + tri(a, c)] += c == 0 ? wphi[0] : wphi[a] * phi[c];
                acc[1 + N_A + a] += wphi[a] * lb;
            }
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
    for (int j = 0; j < N_ACC6; ++j) acc[j] = wave_sum(acc[j]); // lane l += lane l + 32, 16, ... 1
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
    st[S6_COUNT] += acc[0];
    st[S6_CX] = cx;
    st[S6_CY] = cy;
#pragma unroll
    for (int j = 1; j < N_ACC6; ++j) st[S6_A + j - 1] += acc[j];
    if (wi >= 0 && bm > st[S6_BMAX]) {                          // strictly: an earlier chunk's record wins a tie
        st[S6_BMAX] = bm;
        st[S6_XMAX] = (double)wx;
        st[S6_YMAX] = (double)wy;
    }
}

// A2: source_aniso.solve6 line by line.  One thread per env.
__global__ __launch_bounds__(256) void source_solve6_kernel(const double* __restrict__ state, int n, double min_samples,
                                                            double min_pivot, double* __restrict__ est, uint8_t* __restrict__ status) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double* st = state + (int64_t)e * UAV_SRC6_STATE_N;
    double* out = est + (int64_t)e * UAV_SRC6_EST_N;
    const double nan = __builtin_nan("");
    const double count = st[S6_COUNT];
    const bool any = count > 0.0;
    double o7[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) o7[j] = nan;
    int code = UAV_SRC_FEW;
    if (count >= min_samples) {
        double d[N_PHI], L[N_PHI][N_PHI];
#pragma unroll
        for (int j = 0; j < N_PHI; ++j) d[j] = sqrt(st[S6_A + tri(j, j)]);
        bool ok = true;
#pragma unroll
        for (int j = 0; j < N_PHI; ++j) {
            double s = st[S6_A + tri(j, j)] / (d[j] * d[j]);
#pragma unroll
            for (int c = 0; c < j; ++c) s = s - L[j][c] * L[j][c];
            ok = ok && finite_d(s) && s >= min_pivot;           // a NaN fails both
            L[j][j] = sqrt(s);
#pragma unroll
            for (int i = j + 1; i < N_PHI; ++i) {
                double t = st[S6_A + tri(j, i)] / (d[i] * d[j]);
#pragma unroll
                for (int c = 0; c < j; ++c) t = t - L[i][c] * L[j][c];
                L[i][j] = t / L[j][j];
            }
        }
        code = UAV_SRC_DEGENERATE;
        if (ok) {
            double z[N_PHI], u[N_PHI], a[N_PHI];
#pragma unroll
            for (int j = 0; j < N_PHI; ++j) {
                double t = st[S6_G + j] / d[j];
#pragma unroll
                for (int c = 0; c < j; ++c) t = t - L[j][c] * z[c];
                z[j] = t / L[j][j];
            }
#pragma unroll
            for (int j = N_PHI - 1; j >= 0; --j) {
                double t = z[j];
#pragma unroll
                for (int c = j + 1; c < N_PHI; ++c) t = t - L[c][j] * u[c];
                u[j] = t / L[j][j];
            }
            bool fin = true;
#pragma unroll
            for (int j = 0; j < N_PHI; ++j) {
                a[j] = u[j] / d[j];
                fin = fin && finite_d(a[j]);
            }
            const double l11 = -(2.0 * a[3]), l12 = -a[4], l22 = -(2.0 * a[5]);   // Lambda: the inverse covariance / 32^2
            const double det = l11 * l22 - l12 * l12;
            const double trace = l11 + l22;
            const double m0 = (l22 * a[1] - l12 * a[2]) / det;
            const double m1 = (l11 * a[2] - l12 * a[1]) / det;
            const double hd = (l11 - l22) / 2.0;
            const double disc = sqrt(hd * hd + l12 * l12);
            const double big = trace / 2.0 + disc;
            const double small = det / big;
            double v[7];
            v[0] = st[S6_CX] + CELL_SCALE * m0;
            v[1] = st[S6_CY] + CELL_SCALE * m1;
            v[2] = CELL_SCALE / sqrt(small);
            v[3] = CELL_SCALE / sqrt(big);
            const double th = atan2(-(2.0 * l12), l22 - l11) / 2.0;
            v[4] = th < 0.0 ? th + PI_D : th;
            v[5] = exp(a[0] + (a[1] * m0 + a[2] * m1) / 2.0);
            v[6] = TWO_PI_D * (v[2] * v[3]) * v[5];
            bool peaked = fin && det > 0.0 && trace > 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) peaked = peaked && finite_d(v[j]);
            code = UAV_SRC_NOT_A_PEAK;
            if (peaked) {
                code = UAV_SRC_FITTED;
#pragma unroll
                for (int j = 0; j < 7; ++j) o7[j] = v[j];
            }
        }
    }
    status[e] = (uint8_t)code;
#pragma unroll
    for (int j = 0; j < 7; ++j) out[j] = o7[j];
    out[7] = any ? st[S6_XMAX] : nan;
    out[8] = any ? st[S6_YMAX] : nan;
    out[9] = any ? st[S6_BMAX] : nan;
}

// A3: source_summary_kernel's order (thread j of ONE block of 256 adds the envs j, j + 256, ... then block256_sum's tree) with the
// truth per env: truth f64 [n][4] = {sigma_major, sigma_minor, theta, peak} or NULL.
__global__ __launch_bounds__(256) void source_summary6_kernel(const double* __restrict__ est, const uint8_t* __restrict__ status,
                                                              const double* __restrict__ src, const double* __restrict__ truth, int n,
                                                              double loc_tol, double* __restrict__ loc_err, double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    double s[UAV_SRC6_SUM_N - 1];
#pragma unroll
    for (int j = 0; j < UAV_SRC6_SUM_N - 1; ++j) s[j] = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) {
        const double* o = est + (int64_t)e * UAV_SRC6_EST_N;
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
            if (truth) {
                const double t1 = truth[4 * e], t2 = truth[4 * e + 1], ta = truth[4 * e + 2], tp = truth[4 * e + 3];
                if (finite_d(t1) && finite_d(t2) && finite_d(ta) && finite_d(tp)) {
                    s[7] += fabs(o[2] - t1) / t1;
                    s[8] += fabs(o[3] - t2) / t2;
                    double da = fmod(fabs(o[4] - ta), PI_D);
                    da = da > PI_D / 2.0 ? PI_D - da : da;
                    s[9] += da;
                    s[10] += fabs(o[5] - tp) / tp;
                    const double ts = TWO_PI_D * (t1 * t2) * tp;
                    s[11] += fabs(o[6] - ts) / ts;
                    s[14] += 1.0;
                }
            }
        }
        if (o[9] == o[9]) {                                     // the env has a largest sample
            const double dx = o[7] - sx, dy = o[8] - sy;
            s[12] += sqrt(dx * dx + dy * dy);
            s[13] += 1.0;
        }
        if (loc_err) loc_err[e] = err;
    }
#pragma unroll
    for (int j = 0; j < UAV_SRC6_SUM_N - 1; ++j) {
        const double a = block256_sum(s[j], sm);
        if (threadIdx.x == 0) sums[1 + j] = a;
    }
    if (threadIdx.x == 0) sums[UAV_SRC_SUM_ENVS] = (double)n;
}

int source6_cfg_ok(const uav_source_fit_cfg* cfg, const char* who) {
    UAV_REQUIRE(cfg, "%s: NULL cfg", who);
    UAV_REQUIRE(cfg->use_tke == 0 || cfg->use_tke == 1, "%s: use_tke=%d must be 0 or 1", who, cfg->use_tke);
    UAV_REQUIRE(cfg->min_samples >= 6, "%s: min_samples=%d must be at least 6 (six parameters)", who, cfg->min_samples);
    UAV_REQUIRE(cfg->floor - cfg->floor == 0.0 && cfg->floor >= 0.0, "%s: floor=%g must be finite and not negative", who, cfg->floor);
    UAV_REQUIRE(cfg->background - cfg->background == 0.0, "%s: background=%g must be finite", who, cfg->background);
    UAV_REQUIRE(cfg->min_pivot - cfg->min_pivot == 0.0 && cfg->min_pivot > 0.0, "%s: min_pivot=%g must be finite and positive", who,
                cfg->min_pivot);
    return 0;
}

}  // namespace

extern "C" {

int uav_plume_bank(uav_ctx* ctx, const double* params, int F, uint64_t seed, int index0, double* bank, uav_stream stream) {
    UAV_REQUIRE(ctx && params && bank, "uav_plume_bank: NULL argument");
    UAV_REQUIRE(F >= 1, "uav_plume_bank: F=%d must be at least 1", F);
    UAV_REQUIRE(index0 >= 0 && (int64_t)index0 + F < (int64_t)1 << 31, "uav_plume_bank: index0=%d must not be negative, index0 + F below 2^31",
                index0);
    UAV_REQUIRE(((uintptr_t)bank & 15) == 0, "uav_plume_bank: bank is not 16-byte aligned");
    for (int f = 0; f < F; ++f) {                               // params is HOST memory: the refusals are host arithmetic
        const double* p = params + (size_t)f * UAV_PLUME_PARAM_N;
        for (int j = 0; j < UAV_PLUME_PARAM_N; ++j)
            UAV_REQUIRE(p[j] - p[j] == 0.0, "uav_plume_bank: field %d: parameter %d is not finite", f, j);
        UAV_REQUIRE(p[2] > 0.0 && p[3] > 0.0, "uav_plume_bank: field %d: widths %g, %g must be positive", f, p[2], p[3]);
        UAV_REQUIRE(p[6] > 0.0, "uav_plume_bank: field %d: peak=%g must be positive", f, p[6]);
        UAV_REQUIRE(fabs(p[4] * p[4] + p[5] * p[5] - 1.0) <= 1e-12, "uav_plume_bank: field %d: cos^2 + sin^2 differs from 1 by more than 1e-12",
                    f);
    }
    for (int f0 = 0; f0 < F; f0 += PLUME_BATCH) {
        const int nf = F - f0 < PLUME_BATCH ? F - f0 : PLUME_BATCH;
        PlumeBatch b;
        memset(&b, 0, sizeof(b));
        memcpy(b.p, params + (size_t)f0 * UAV_PLUME_PARAM_N, sizeof(double) * UAV_PLUME_PARAM_N * nf);
        hipLaunchKernelGGL(plume_bank_kernel, dim3((GRID * GRID + 255) / 256, nf), dim3(256), 0, as_stream(stream), b, seed, index0 + f0,
                           ctx->wave, ctx->ftab, bank + (size_t)f0 * GRID * GRID * 2);
        UAV_LAUNCH_CHECK();
    }
    return 0;
}

int uav_source_moments6(uav_ctx* ctx, const uint8_t* flags, const float* obs, const float* pos, int n, int k, int D,
                        const uav_source_fit_cfg* cfg, const uint8_t* ended, double* state, uav_stream stream) {
    UAV_REQUIRE(ctx && flags && obs && pos && state, "uav_source_moments6: NULL argument");
    if (int rc = source6_cfg_ok(cfg, "uav_source_moments6")) return rc;
    UAV_REQUIRE(n >= 1 && k >= 1, "uav_source_moments6: n=%d, k=%d must be at least 1", n, k);
    UAV_REQUIRE(D >= (cfg->use_tke ? 4 : 3), "uav_source_moments6: D=%d must be at least %d (obs[2]%s)", D, cfg->use_tke ? 4 : 3,
                cfg->use_tke ? " and obs[3]" : "");
    UAV_REQUIRE((int64_t)n * k * D < (int64_t)1 << 31, "uav_source_moments6: n * k * D = %lld is 2^31 or more", (long long)n * k * D);
    UAV_REQUIRE(((uintptr_t)pos & 7) == 0, "uav_source_moments6: pos is not 8-byte aligned");
    hipLaunchKernelGGL(source_moments6_kernel, dim3((n + 3) / 4), dim3(256), 0, as_stream(stream), flags, obs, pos, n, k, D,
                       (int)cfg->use_tke, cfg->background, cfg->floor, ended, state);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_source_solve6(uav_ctx* ctx, const double* state, int n, const uav_source_fit_cfg* cfg, double* est, uint8_t* status,
                      uav_stream stream) {
    UAV_REQUIRE(ctx && state && est && status, "uav_source_solve6: NULL argument");
    if (int rc = source6_cfg_ok(cfg, "uav_source_solve6")) return rc;
    UAV_REQUIRE(n >= 1, "uav_source_solve6: n=%d must be at least 1", n);
    hipLaunchKernelGGL(source_solve6_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), state, n, (double)cfg->min_samples,
                       cfg->min_pivot, est, status);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_source_summary6(uav_ctx* ctx, const double* est, const uint8_t* status, const double* src, const double* truth, int n,
                        double loc_tol, double* loc_err, double* sums, uav_stream stream) {
    UAV_REQUIRE(ctx && est && status && src && sums, "uav_source_summary6: NULL argument");
    UAV_REQUIRE(n >= 1, "uav_source_summary6: n=%d must be at least 1", n);
    UAV_REQUIRE(loc_tol == loc_tol, "uav_source_summary6: loc_tol is a NaN");
    hipLaunchKernelGGL(source_summary6_kernel, dim3(1), dim3(256), 0, as_stream(stream), est, status, src, truth, n, loc_tol, loc_err,
                       sums);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
