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

// source_fit.solve line by line on one system: the count, A (the upper triangle by rows: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3)
// (2,2) (2,3) (3,3)), g and the centre -> the status; o5 = {mu_x, mu_y, sigma, peak, strength} where FITTED, else untouched.  Both
// uav_source_solve and uav_source_stop_scan call it: one order of operations.
__device__ __forceinline__ int source_solve_core(double count, const double* A, const double* g, double cx, double cy,
                                                 double min_samples, double min_pivot, double* o5) {
#pragma clang fp contract(off)
    if (!(count >= min_samples)) return UAV_SRC_FEW;
    constexpr int IDX[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
    double d[4], S[4][4], L[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = sqrt(A[IDX[j][j]]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) S[i][j] = A[IDX[i][j]] / (d[i] * d[j]);
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
    if (!ok) return UAV_SRC_DEGENERATE;
    double z[4], u[4], a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double t = g[j] / d[j];
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
    if (!(finite_d(a[0]) && finite_d(a[1]) && finite_d(a[2]) && finite_d(a[3]) && a[3] < 0.0 && finite_d(s2))) return UAV_SRC_NOT_A_PEAK;
    const double sigma = CELL_SCALE * sqrt(s2);
    const double peak = exp(a[0] + (a[1] * a[1] + a[2] * a[2]) * s2 / 2.0);
    o5[0] = cx + CELL_SCALE * a[1] * s2;
    o5[1] = cy + CELL_SCALE * a[2] * s2;
    o5[2] = sigma;
    o5[3] = peak;
    o5[4] = 6.283185307179586 * (sigma * sigma) * peak;
    return UAV_SRC_FITTED;
}

// One thread per env: source_solve_core on the env's state.
__global__ __launch_bounds__(256) void source_solve_kernel(const double* __restrict__ state, int n, double min_samples,
                                                           double min_pivot, double* __restrict__ est, uint8_t* __restrict__ status) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double* st = state + (int64_t)e * UAV_SRC_STATE_N;
    double* out = est + (int64_t)e * UAV_SRC_EST_N;
    const double nan = __builtin_nan("");
    const double count = st[ST_COUNT];
    const bool any = count > 0.0;
    double A[10], g[4], o5[5];
#pragma unroll
    for (int j = 0; j < 10; ++j) A[j] = st[ST_A + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = st[ST_G + j];
#pragma unroll
    for (int j = 0; j < 5; ++j) o5[j] = nan;
    status[e] = (uint8_t)source_solve_core(count, A, g, st[ST_CX], st[ST_CY], min_samples, min_pivot, o5);
#pragma unroll
    for (int j = 0; j < 5; ++j) out[j] = o5[j];
    out[5] = any ? st[ST_XMAX] : nan;
    out[6] = any ? st[ST_YMAX] : nan;
    out[7] = any ? st[ST_BMAX] : nan;
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

// S4  stop scan: the estimator as a stop rule (source_stop.stop_scan_chunk line by line).  One wave per env, registers only.  Per
// block of 64 records: the 15 contributions as in S1, an inclusive Hillis-Steele scan over the lanes (offsets 1 .. 32, lane l adds
// lane l - o's old value), prefix = carry + scan, every eligible lane solves its own prefix system, the previous eligible record's
// estimate comes by shuffle (the state's for the block's first), run lengths from the ballot of the unsettled lanes, the first hit
// from the ballot of the hits.  The carry into the next block is the prefix at the block's last eligible lane.
constexpr int SS_ACC = 0, SS_CX = 1, SS_CY = 2, SS_PREV = UAV_SRC_STOP_PREV_X, SS_PFIT = UAV_SRC_STOP_PREV_FITTED,
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
        for (int j = 1; j < N_ACC; ++j) carry[j] = st[ST_A + j - 1];
        bool have_c = carry[0] > 0.0;
        double cx = st[SS_CX], cy = st[SS_CY];
        double pmx = st[SS_PREV], pmy = st[SS_PREV + 1];
        int pfit = st[SS_PFIT] != 0.0, run_in = (int)st[SS_RUN];
        bool any = false;
        for (int base = 0; base < k; base += 64) {              // wave-uniform trip count
            const int i = base + lane;
            const uint8_t v = i < k ? f[i] : (uint8_t)FLAG_SKIP;
            const bool end = !(v & FLAG_SKIP) && (v & (FLAG_DONE | FLAG_RULE));
            const unsigned long long m = __ballot(end);
            const int last = m ? __builtin_ctzll(m) : 63;
            const bool take = !(v & FLAG_SKIP) && lane <= last;  // eligible; a bit2 record is never read
            int x = 0, y = 0;
            double b = 0.0, px = 0.0, py = 0.0;
            bool used = false;
            if (take) {
                const int64_t rec = (int64_t)row * k + i;
                const float o2 = obs[rec * D + 2];
                const float2 xy = *reinterpret_cast<const float2*>(pos + rec * 2);
                px = (double)xy.x;
                py = (double)xy.y;
                x = cell_of(xy.x);
                y = cell_of(xy.y);
                if (use_tke) {
                    const float o3 = obs[rec * D + 3];
                    b = 100.0 * (double)o2 - 9.0 * (double)o3;
                } else {
                    b = 100.0 * (double)o2 - background;
                }
                used = b > floor_b && o2 < 1.0f;
            }
            const unsigned long long mu = __ballot(used);
            if (!have_c && mu) {                                // wave-uniform
                const int src = __builtin_ctzll(mu);
                cx = (double)__shfl(x, src, 64);
                cy = (double)__shfl(y, src, 64);
                have_c = true;
            }
            double c[N_ACC];
#pragma unroll
            for (int j = 0; j < N_ACC; ++j) c[j] = 0.0;
            if (used) {
                const double p = ((double)x - cx) / CELL_SCALE, q = ((double)y - cy) / CELL_SCALE;
                const double r = p * p + q * q;
                const double w = b * b, lb = log(b);
                const double wp = w * p, wq = w * q, wr = w * r;
                c[0] = 1.0;
                c[1] = w;
                c[2] = wp;
                c[3] = wq;
                c[4] = wr;
                c[5] = wp * p;
                c[6] = wp * q;
                c[7] = wp * r;
                c[8] = wq * q;
                c[9] = wq * r;
                c[10] = wr * r;
                c[11] = w * lb;
                c[12] = wp * lb;
                c[13] = wq * lb;
                c[14] = wr * lb;
            }
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
            double e5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            int status = 255;
            if (take) status = source_solve_core(c[0], c + 1, c + 11, cx, cy, min_samples, min_pivot, e5);
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
                    st[SS_CX] = cx;
                    st[SS_CY] = cy;
#pragma unroll
                    for (int j = 1; j < N_ACC; ++j) st[ST_A + j - 1] = c[j];
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
            st[SS_CX] = cx;
            st[SS_CY] = cy;
#pragma unroll
            for (int j = 1; j < N_ACC; ++j) st[ST_A + j - 1] = carry[j];
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

int uav_source_stop_scan(uav_ctx* ctx, uint8_t* flags, const float* obs, const float* pos, int n, int k, int D, int t0,
                         const uav_source_fit_cfg* cfg, const uav_source_stop_cfg* stop, const uint8_t* ended, uint8_t* active,
                         double* state, int32_t* first_hit, double* mu_steps, uint8_t* status_steps, int mark, uav_stream stream) {
    UAV_REQUIRE(ctx && flags && obs && pos && state && first_hit, "uav_source_stop_scan: NULL argument");
    if (int rc = source_cfg_ok(cfg, "uav_source_stop_scan")) return rc;
    UAV_REQUIRE(stop, "uav_source_stop_scan: NULL stop cfg");
    UAV_REQUIRE(stop->settle_tol - stop->settle_tol == 0.0 && stop->settle_tol >= 0.0,
                "uav_source_stop_scan: settle_tol=%g must be finite and not negative", stop->settle_tol);
    UAV_REQUIRE(stop->near == stop->near && stop->near >= 0.0, "uav_source_stop_scan: near=%g must be a distance (inf: anywhere)",
                stop->near);
    UAV_REQUIRE(stop->patience >= 1, "uav_source_stop_scan: patience=%d must be at least 1", stop->patience);
    UAV_REQUIRE(stop->min_steps >= 0, "uav_source_stop_scan: min_steps=%d must not be negative", stop->min_steps);
    UAV_REQUIRE(n >= 1 && k >= 1, "uav_source_stop_scan: n=%d, k=%d must be at least 1", n, k);
    UAV_REQUIRE(t0 >= 0 && (int64_t)t0 + k < (int64_t)1 << 31, "uav_source_stop_scan: t0=%d must not be negative, t0 + k below 2^31", t0);
    UAV_REQUIRE(D >= (cfg->use_tke ? 4 : 3), "uav_source_stop_scan: D=%d must be at least %d (obs[2]%s)", D, cfg->use_tke ? 4 : 3,
                cfg->use_tke ? " and obs[3]" : "");
    UAV_REQUIRE((int64_t)n * k * D < (int64_t)1 << 31, "uav_source_stop_scan: n * k * D = %lld is 2^31 or more", (long long)n * k * D);
    UAV_REQUIRE(((uintptr_t)pos & 7) == 0, "uav_source_stop_scan: pos is not 8-byte aligned");
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
