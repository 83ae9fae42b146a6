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
//   S4  stop scan the estimator as a stop rule: S1's contributions scanned over the lanes, S2's solve after every record, the first
//                 record at which the estimate has settled ends the episode (uavppo/source_stop.py states it).
//
// S1 .. S3 are source_core.h's bodies (record reader, contributions, moments, summary head and tail) and source_solve.h's solve with
// IsoBasis; source_aniso.hip instantiates the same bodies with six basis functions.  S4 keeps its scan, run-length and hit logic
// and takes its records, contributions and per-lane solve from there.
// Nothing is read by the host between them.  The order of every sum and of every operation of S2 is fixed: S1's integers, centre, A
// and largest sample, S2's status, mu and sigma and all of S3 equal the numpy statement bit for bit; g goes through log, peak
// through exp.
#include "source_core.h"

using Iso = IsoBasis;

__global__ __launch_bounds__(256) void source_moments_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ obs,
                                                             const float* __restrict__ pos, int n, int k, int D, int use_tke,
                                                             double background, double floor_b, const uint8_t* __restrict__ ended,
                                                             double* __restrict__ state) {
    moments_body<Iso>(flags, obs, pos, n, k, D, use_tke, background, floor_b, ended, state);
}

__global__ __launch_bounds__(256) void source_solve_kernel(const double* __restrict__ state, int n, double min_samples,
                                                           double min_pivot, double* __restrict__ est, uint8_t* __restrict__ status) {
    solve_body<Iso>(state, n, min_samples, min_pivot, est, status);
}

// The truth is one sigma and one peak for every env; a truth that is not finite and positive leaves its sum 0.
__global__ __launch_bounds__(256) void source_summary_kernel(const double* __restrict__ est, const uint8_t* __restrict__ status,
                                                             const double* __restrict__ src, int n, double sigma_true, double peak_true,
                                                             double loc_tol, double* __restrict__ loc_err, double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    double s[Iso::SUM_N - 1];
#pragma unroll
    for (int j = 0; j < Iso::SUM_N - 1; ++j) s[j] = 0.0;
    const bool sig_known = finite_d(sigma_true) && sigma_true > 0.0, peak_known = finite_d(peak_true) && peak_true > 0.0;
    for (int e = threadIdx.x; e < n; e += 256) {
        const double* o = est + (int64_t)e * Iso::EST_N;
        const int stt = status[e];
        const double sx = src[2 * e], sy = src[2 * e + 1];
        const double err = summary_head(stt, o, sx, sy, loc_tol, s);
        if (stt == UAV_SRC_FITTED) {
            if (sig_known) s[7] += fabs(o[2] - sigma_true) / sigma_true;
            if (peak_known) s[8] += fabs(o[3] - peak_true) / peak_true;
        }
        summary_tail<Iso>(o, sx, sy, s);
        if (loc_err) loc_err[e] = err;
    }
    summary_write<Iso>(s, sm, n, sums);
}

// S4  stop scan: the estimator as a stop rule (source_stop.stop_scan_chunk line by line).  One wave per env, registers only.  Per
// block of 64 records: the 15 contributions as in S1, an inclusive Hillis-Steele scan over the lanes (offsets 1 .. 32, lane l adds
// lane l - o's old value), prefix = carry + scan, every eligible lane solves its own prefix system, the previous eligible record's
// estimate comes by shuffle (the state's for the block's first), run lengths from the ballot of the unsettled lanes, the first hit
// from the ballot of the hits.  The carry into the next block is the prefix at the block's last eligible lane.
constexpr int N_ACC = Iso::N_ACC, SS_ACC = 0, SS_CX = 1, SS_CY = 2, SS_PREV = UAV_SRC_STOP_PREV_X, SS_PFIT = UAV_SRC_STOP_PREV_FITTED,
              SS_RUN = UAV_SRC_STOP_RUN, SS_HIT = UAV_SRC_STOP_HIT_STEP, SS_EST = UAV_SRC_STOP_EST;

__device__ __forceinline__ unsigned long long lanes_upto(int l) { return l >= 63 ? ~0ull : (2ull << l) - 1ull; }   // bits 0 .. l

__global__ __launch_bounds__(256) void source_stop_kernel(uint8_t* flags, const float* __restrict__ obs, const float* __restrict__ pos,
                                                          int n, int k, int D, int t0, int use_tke, double background, double floor_b,
                                                          double min_samples, double min_pivot, double tol2, double near2,
                                                          int patience, int min_steps, const uint8_t* __restrict__ ended,
                                                          uint8_t* active, double* __restrict__ state, int32_t* __restrict__ first_hit,
                                                          double* __restrict__ mu_steps, uint8_t* __restrict__ status_steps, int mark) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);        // wave-uniform
    if (row >= n) return;
    double* st = state + (int64_t)row * UAV_SRC_STOP_STATE_N;
    uint8_t* f = flags + (int64_t)row * k;
    const double nan = __builtin_nan("");
    const bool idle = (ended && ended[row]) || st[SS_HIT] > 0.0;  // ended earlier, or already stopped: left alone to the bit
    int hit_at = -1, filled = 0;                                // the hit's record; records below `filled` have their per-record outputs
    if (!idle) {
        double carry[N_ACC];
        carry[0] = st[SS_ACC];
#pragma unroll
        for (int j = 1; j < N_ACC; ++j) carry[j] = st[Iso::A + j - 1];
        SourceCentre ce = {carry[0] > 0.0, {st[SS_CX], st[SS_CY]}};
        double pmx = st[SS_PREV], pmy = st[SS_PREV + 1];
        int pfit = st[SS_PFIT] != 0.0, run_in = (int)st[SS_RUN];
        bool any = false;
        for (int base = 0; base < k; base += 64) {              // wave-uniform trip count
            const int i = base + lane;
            SourceRecord r;                                     // r.take: eligible
            const unsigned long long m = read_records(f, obs, pos, row, k, D, i, lane, use_tke, background, floor_b, r, ce);
            const bool take = r.take;
            const double px = (double)r.xy.x, py = (double)r.xy.y;
            double c[N_ACC];
#pragma unroll
            for (int j = 0; j < N_ACC; ++j) c[j] = 0.0;
            if (r.used) contributions<Iso>(r, ce, c);
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {                  // inclusive scan: lane l += lane l - o's old value
#pragma unroll
                for (int j = 0; j < N_ACC; ++j) {
                    const double t = __shfl_up(c[j], o, 64);
                    if (lane >= o) c[j] = c[j] + t;
                }
            }
#pragma unroll
            for (int j = 0; j < N_ACC; ++j) c[j] = carry[j] + c[j];   // this lane's prefix system
            const unsigned long long el = __ballot(take);
            double e5[Iso::FIT_N] = {0.0, 0.0, 0.0, 0.0, 0.0};
            int status = 255;
            if (take) status = solve_core<Iso>(c[0], c + 1, c + 1 + Iso::N_A, ce.xy, min_samples, min_pivot, e5);
            const bool fit = status == UAV_SRC_FITTED;          // e5 stays 0 unless fitted: no NaN goes into the state
            const unsigned long long below = el & (lanes_upto(lane) >> 1);
            const int pl = below ? 63 - __builtin_clzll(below) : 0;
            double qx = __shfl(e5[0], pl, 64), qy = __shfl(e5[1], pl, 64);
            int qf = __shfl((int)fit, pl, 64);
            if (!below) {                                       // the block's first eligible record: the state's
                qx = pmx;
                qy = pmy;
                qf = pfit;
            }
            const double mvx = e5[0] - qx, mvy = e5[1] - qy;
            const bool settled = fit && qf && mvx * mvx + mvy * mvy <= tol2;
            const unsigned long long zb = __ballot(take && !settled) & lanes_upto(lane);
            const unsigned long long upto = el & lanes_upto(lane);
            const int run = zb ? __builtin_popcountll(upto & ~lanes_upto(63 - __builtin_clzll(zb))) : __builtin_popcountll(upto) + run_in;
            const double ndx = px - e5[0], ndy = py - e5[1];
            const bool hit = fit && run >= patience && ndx * ndx + ndy * ndy <= near2 && t0 + i + 1 >= min_steps;
            const unsigned long long hb = __ballot(hit);
            const int hl = hb ? __builtin_ctzll(hb) : 63;
            if (i < k) {
                const bool shown = take && lane <= hl;          // nothing behind the hit has an estimate
                if (status_steps) status_steps[(int64_t)row * k + i] = shown ? (uint8_t)status : (uint8_t)255;
                if (mu_steps) {
                    double* o = mu_steps + ((int64_t)row * k + i) * 2;
                    o[0] = shown && fit ? e5[0] : nan;
                    o[1] = shown && fit ? e5[1] : nan;
                }
            }
            filled = base + 64;
            if (hb) {                                           // wave-uniform: the state is the prefix at the hit
                hit_at = base + hl;
                if (lane == hl) {
                    st[SS_ACC] = c[0];
                    st[SS_CX] = ce.xy[0];
                    st[SS_CY] = ce.xy[1];
#pragma unroll
                    for (int j = 1; j < N_ACC; ++j) st[Iso::A + j - 1] = c[j];
                    st[SS_PREV] = e5[0];
                    st[SS_PREV + 1] = e5[1];
                    st[SS_PFIT] = 1.0;
                    st[SS_RUN] = (double)run;
                    st[SS_HIT] = (double)(t0 + i + 1);
#pragma unroll
                    for (int j = 0; j < 5; ++j) st[SS_EST + j] = e5[j];
                }
                break;
            }
            if (el) {                                           // wave-uniform: carry on from the last eligible lane
                const int le = 63 - __builtin_clzll(el);
#pragma unroll
                for (int j = 0; j < N_ACC; ++j) carry[j] = __shfl(c[j], le, 64);
                pmx = __shfl(e5[0], le, 64);
                pmy = __shfl(e5[1], le, 64);
                pfit = __shfl((int)fit, le, 64);
                run_in = __shfl(run, le, 64);
                any = true;
            }
            if (m) break;                                       // nothing behind the ending block is read
        }
        if (hit_at < 0 && any && lane == 0) {
            st[SS_ACC] = carry[0];
            st[SS_CX] = ce.xy[0];
            st[SS_CY] = ce.xy[1];
#pragma unroll
            for (int j = 1; j < N_ACC; ++j) st[Iso::A + j - 1] = carry[j];
            st[SS_PREV] = pmx;
            st[SS_PREV + 1] = pmy;
            st[SS_PFIT] = pfit ? 1.0 : 0.0;
            st[SS_RUN] = (double)run_in;
        }
    }
    for (int i = filled + lane; i < k; i += 64) {               // records the scan did not reach: no estimate
        if (status_steps) status_steps[(int64_t)row * k + i] = (uint8_t)255;
        if (mu_steps) {
            mu_steps[((int64_t)row * k + i) * 2] = nan;
            mu_steps[((int64_t)row * k + i) * 2 + 1] = nan;
        }
    }
    if (hit_at >= 0 && mark) {                                  // the flags now say where the episode ended
        for (int i = hit_at + 1 + lane; i < k; i += 64) f[i] = (uint8_t)(f[i] | FLAG_SKIP);
        if (lane == 0) {
            f[hit_at] = (uint8_t)(f[hit_at] | FLAG_RULE);
            if (active) active[row] = 0;
        }
    }
    if (lane == 0) first_hit[row] = hit_at;
}

extern "C" {

int uav_source_moments(uav_ctx* ctx, const uint8_t* flags, const float* obs, const float* pos, int n, int k, int D,
                       const uav_source_fit_cfg* cfg, const uint8_t* ended, double* state, uav_stream stream) {
    UAV_REQUIRE(ctx && flags && obs && pos && state, "uav_source_moments: NULL argument");
    if (int rc = source_cfg_ok(cfg, "uav_source_moments", Iso::N)) return rc;
    if (int rc = source_records_ok(cfg, "uav_source_moments", n, k, D, 0, pos)) return rc;
    hipLaunchKernelGGL(source_moments_kernel, dim3((n + 3) / 4), dim3(256), 0, as_stream(stream), flags, obs, pos, n, k, D,
                       (int)cfg->use_tke, cfg->background, cfg->floor, ended, state);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_source_solve(uav_ctx* ctx, const double* state, int n, const uav_source_fit_cfg* cfg, double* est, uint8_t* status,
                     uav_stream stream) {
    UAV_REQUIRE(ctx && state && est && status, "uav_source_solve: NULL argument");
    if (int rc = source_cfg_ok(cfg, "uav_source_solve", Iso::N)) return rc;
    UAV_REQUIRE(n >= 1, "uav_source_solve: n=%d must be at least 1", n);
    hipLaunchKernelGGL(source_solve_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), state, n, (double)cfg->min_samples,
                       cfg->min_pivot, est, status);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_source_stop_scan(uav_ctx* ctx, uint8_t* flags, const float* obs, const float* pos, int n, int k, int D, int t0,
                         const uav_source_fit_cfg* cfg, const uav_source_stop_cfg* stop, const uint8_t* ended, uint8_t* active,
                         double* state, int32_t* first_hit, double* mu_steps, uint8_t* status_steps, int mark, uav_stream stream) {
    UAV_REQUIRE(ctx && flags && obs && pos && state && first_hit, "uav_source_stop_scan: NULL argument");
    if (int rc = source_cfg_ok(cfg, "uav_source_stop_scan", Iso::N)) return rc;
    UAV_REQUIRE(stop, "uav_source_stop_scan: NULL stop cfg");
    UAV_REQUIRE(stop->settle_tol - stop->settle_tol == 0.0 && stop->settle_tol >= 0.0,
                "uav_source_stop_scan: settle_tol=%g must be finite and not negative", stop->settle_tol);
    UAV_REQUIRE(stop->near == stop->near && stop->near >= 0.0, "uav_source_stop_scan: near=%g must be a distance (inf: anywhere)",
                stop->near);
    UAV_REQUIRE(stop->patience >= 1, "uav_source_stop_scan: patience=%d must be at least 1", stop->patience);
    UAV_REQUIRE(stop->min_steps >= 0, "uav_source_stop_scan: min_steps=%d must not be negative", stop->min_steps);
    if (int rc = source_records_ok(cfg, "uav_source_stop_scan", n, k, D, t0, pos)) return rc;
    hipLaunchKernelGGL(source_stop_kernel, dim3((n + 3) / 4), dim3(256), 0, as_stream(stream), flags, obs, pos, n, k, D, t0,
                       (int)cfg->use_tke, cfg->background, cfg->floor, (double)cfg->min_samples, cfg->min_pivot,
                       stop->settle_tol * stop->settle_tol, stop->near * stop->near, (int)stop->patience, (int)stop->min_steps, ended,
                       active, state, first_hit, mu_steps, status_steps, mark);
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
