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
// Record eligibility, the centre, p and q, b and w, chunking, `ended`, the largest sample and the Cholesky are S1's and S2's: one
// body in source_core.h / source_solve.h, instantiated here with AnisoBasis.  f64 throughout, no LDS beyond block256_sum's four
// slots, no atomics; nothing is read by the host.
#include "env_core.h"
#include "source_core.h"

namespace {

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

using Aniso = AnisoBasis;

__global__ __launch_bounds__(256) void source_moments6_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ obs,
                                                              const float* __restrict__ pos, int n, int k, int D, int use_tke,
                                                              double background, double floor_b, const uint8_t* __restrict__ ended,
                                                              double* __restrict__ state) {
    moments_body<Aniso>(flags, obs, pos, n, k, D, use_tke, background, floor_b, ended, state);
}

__global__ __launch_bounds__(256) void source_solve6_kernel(const double* __restrict__ state, int n, double min_samples,
                                                            double min_pivot, double* __restrict__ est, uint8_t* __restrict__ status) {
    solve_body<Aniso>(state, n, min_samples, min_pivot, est, status);
}

// The truth is per env: truth f64 [n][4] = {sigma_major, sigma_minor, theta, peak} or NULL; a row with a non-finite entry adds nothing.
__global__ __launch_bounds__(256) void source_summary6_kernel(const double* __restrict__ est, const uint8_t* __restrict__ status,
                                                              const double* __restrict__ src, const double* __restrict__ truth, int n,
                                                              double loc_tol, double* __restrict__ loc_err, double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    double s[Aniso::SUM_N - 1];
#pragma unroll
    for (int j = 0; j < Aniso::SUM_N - 1; ++j) s[j] = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) {
        const double* o = est + (int64_t)e * Aniso::EST_N;
        const int stt = status[e];
        const double sx = src[2 * e], sy = src[2 * e + 1];
        const double err = summary_head(stt, o, sx, sy, loc_tol, s);
        if (stt == UAV_SRC_FITTED && truth) {
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
        summary_tail<Aniso>(o, sx, sy, s);
        if (loc_err) loc_err[e] = err;
    }
    summary_write<Aniso>(s, sm, n, sums);
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
    if (int rc = source_cfg_ok(cfg, "uav_source_moments6", Aniso::N)) return rc;
    if (int rc = source_records_ok(cfg, "uav_source_moments6", n, k, D, 0, pos)) return rc;
    hipLaunchKernelGGL(source_moments6_kernel, dim3((n + 3) / 4), dim3(256), 0, as_stream(stream), flags, obs, pos, n, k, D,
                       (int)cfg->use_tke, cfg->background, cfg->floor, ended, state);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_source_solve6(uav_ctx* ctx, const double* state, int n, const uav_source_fit_cfg* cfg, double* est, uint8_t* status,
                      uav_stream stream) {
    UAV_REQUIRE(ctx && state && est && status, "uav_source_solve6: NULL argument");
    if (int rc = source_cfg_ok(cfg, "uav_source_solve6", Aniso::N)) return rc;
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
