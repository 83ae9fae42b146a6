// source_core.h -- what the four-term kernels (source_fit.hip), the six-term kernels (source_aniso.hip) and the stop scan share: the
// record reader, a record's contributions, the moments kernel's body, the summary kernels' head and tail and the entry points'
// argument checks.  The solve and the two bases are in source_solve.h (no HIP in there).  uavppo/source_fit.py states every line in
// numpy (used_records, contributions, moments_chunk, summary_sums).
//
// Tie rules: of equal largest samples the earliest record of a lane wins, then the earliest record of the wave, then the earlier
// chunk.  log(b) is called once per record.  Row 0 of A is w itself and then w * phi[c].
#pragma once
#include "common.h"
#include "source_solve.h"

constexpr int FLAG_DONE = 1, FLAG_SKIP = 4, FLAG_RULE = 8;      // record flags: bit0 done, bit2 not stepped, bit3 rule fired
static_assert(SRC_FITTED == UAV_SRC_FITTED && SRC_FEW == UAV_SRC_FEW && SRC_DEGENERATE == UAV_SRC_DEGENERATE &&
              SRC_NOT_A_PEAK == UAV_SRC_NOT_A_PEAK, "status codes");
static_assert(IsoBasis::STATE_N == UAV_SRC_STATE_N && IsoBasis::EST_N == UAV_SRC_EST_N && IsoBasis::SUM_N == UAV_SRC_SUM_N &&
              IsoBasis::SUM_MAX_ERR == UAV_SRC_SUM_MAX_ERR && IsoBasis::BMAX == UAV_SRC_STOP_PREV_X && UAV_SRC_STOP_PREV_X == 17,
              "four-term layout: the stop scan's own fields begin where the largest sample lies in uav_source_moments' state");
static_assert(AnisoBasis::STATE_N == UAV_SRC6_STATE_N && AnisoBasis::EST_N == UAV_SRC6_EST_N && AnisoBasis::SUM_N == UAV_SRC6_SUM_N &&
              AnisoBasis::SUM_MAX_ERR == UAV_SRC6_SUM_MAX_ERR, "six-term layout");

// the cell field_at sampled: min(max((int)v, 0), 499), clamped as a float first so that a NaN or a huge v is defined (cell 0 / 499)
__device__ __forceinline__ int cell_of(float v) { return (int)fminf(fmaxf(v, 0.0f), 499.0f); }

// One block of 64 records of env `row`, record i = base + lane per lane.  A record is taken up to and including the block's first
// with bit0 or bit3, never one with bit2 (it is not read); it is used iff b > floor and its cell was not clipped.  The centre is
// fixed by the episode's first used record.  Returns the ballot of the ending records: callers read nothing behind such a block.
struct SourceRecord {
    bool take, used;
    int x, y;                                                   // the cell
    double b;
    float2 xy;                                                  // the position as recorded
};
struct SourceCentre {
    bool have;
    double xy[2];                                               // cx, cy: solve_core's centre
};
__device__ __forceinline__ unsigned long long read_records(const uint8_t* f, const float* __restrict__ obs, const float* __restrict__ pos,
                                                           int row, int k, int D, int i, int lane, int use_tke, double background,
                                                           double floor_b, SourceRecord& r, SourceCentre& c) {
#pragma clang fp contract(off)
    const uint8_t v = i < k ? f[i] : (uint8_t)FLAG_SKIP;
    const bool end = !(v & FLAG_SKIP) && (v & (FLAG_DONE | FLAG_RULE));
    const unsigned long long m = __ballot(end);
    const int last = m ? __builtin_ctzll(m) : 63;
    r.take = !(v & FLAG_SKIP) && lane <= last;
    r.x = r.y = 0;
    r.b = 0.0;
    r.xy = make_float2(0.0f, 0.0f);
    r.used = false;
    if (r.take) {
        const int64_t rec = (int64_t)row * k + i;
        const float o2 = obs[rec * D + 2];
        r.xy = *reinterpret_cast<const float2*>(pos + rec * 2);
        r.x = cell_of(r.xy.x);
        r.y = cell_of(r.xy.y);
        const double conc = 100.0 * (double)o2;                 // obs[3] is read only where the cfg says it is there
        r.b = use_tke ? conc - 9.0 * (double)obs[rec * D + 3] : conc - background;
        r.used = r.b > floor_b && o2 < 1.0f;                    // false for a NaN; obs[2] == 1: the cell was clipped at 100
    }
    const unsigned long long mu = __ballot(r.used);
    if (!c.have && mu) {                                        // wave-uniform
        const int src = __builtin_ctzll(mu);
        c.xy[0] = (double)__shfl(r.x, src, 64);
        c.xy[1] = (double)__shfl(r.y, src, 64);
        c.have = true;
    }
    return m;
}

// c[B::N_ACC] of one used record: 1 | (w phi_i) phi_j for i <= j by rows | (w phi_i) ln b, with w = b^2 (Guo's weighting)
template <class B>
__device__ __forceinline__ void contributions(const SourceRecord& r, const SourceCentre& ce, double* c) {
#pragma clang fp contract(off)
    const double p = ((double)r.x - ce.xy[0]) / CELL_SCALE, q = ((double)r.y - ce.xy[1]) / CELL_SCALE;
    const double w = r.b * r.b, lb = log(r.b);
    double phi[B::N], wphi[B::N];
    B::phi(p, q, phi);
    wphi[0] = w;
#pragma unroll
    for (int j = 1; j < B::N; ++j) wphi[j] = w * phi[j];
    c[0] = 1.0;
#pragma unroll
    for (int a = 0; a < B::N; ++a) {
#pragma unroll
        for (int j = a; j < B::N; ++j) c[1 + tri<B::N>(a, j)] = j == 0 ? wphi[0] : wphi[a] * phi[j];
        c[1 + B::N_A + a] = wphi[a] * lb;
    }
}

// One chunk of records -> per env the normal equations, the count, the centre and the largest sample.  One wave per env (blocks
// of 256 = four envs), registers only.
template <class B>
__device__ __forceinline__ void moments_body(const uint8_t* __restrict__ flags, const float* __restrict__ obs, const float* __restrict__ pos,
                                             int n, int k, int D, int use_tke, double background, double floor_b,
                                             const uint8_t* __restrict__ ended, double* __restrict__ state) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);        // wave-uniform
    if (row >= n) return;
    if (ended && ended[row]) return;                            // ended in an earlier chunk: left alone to the bit
    double* st = state + (int64_t)row * B::STATE_N;
    SourceCentre ce = {st[B::COUNT] > 0.0, {st[B::CX], st[B::CY]}};
    double acc[B::N_ACC];
#pragma unroll
    for (int j = 0; j < B::N_ACC; ++j) acc[j] = 0.0;
    double bm = 0.0;                                            // this lane's largest b (a used b is > floor >= 0), its record, its cell
    int bi = -1, bx = 0, by = 0;
    const uint8_t* f = flags + (int64_t)row * k;
    for (int base = 0; base < k; base += 64) {                  // wave-uniform trip count
        const int i = base + lane;
        SourceRecord r;
        const unsigned long long m = read_records(f, obs, pos, row, k, D, i, lane, use_tke, background, floor_b, r, ce);
        if (r.used) {
            double c[B::N_ACC];
            contributions<B>(r, ce, c);
#pragma unroll
            for (int j = 0; j < B::N_ACC; ++j) acc[j] += c[j];
            if (r.b > bm) {                                     // strictly: the earliest record of the lane wins a tie
                bm = r.b;
                bi = i;
                bx = r.x;
                by = r.y;
            }
        }
        if (m) break;                                           // nothing behind the ending block is read
    }
#pragma unroll
    for (int j = 0; j < B::N_ACC; ++j) acc[j] = wave_sum(acc[j]);   // lane l += lane l + 32, 16, ... 1
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
    st[B::COUNT] += acc[0];
    st[B::CX] = ce.xy[0];
    st[B::CY] = ce.xy[1];
#pragma unroll
    for (int j = 1; j < B::N_ACC; ++j) st[B::A + j - 1] += acc[j];
    if (wi >= 0 && bm > st[B::BMAX]) {                          // strictly: an earlier chunk's record wins a tie
        st[B::BMAX] = bm;
        st[B::XMAX] = (double)wx;
        st[B::YMAX] = (double)wy;
    }
}

// One thread per env: solve_core on the env's state -> est = {fit (NaN unless FITTED) | the largest sample's x, y, b (NaN for a
// count of 0)} and the status.  The pointers are the kernel's own __restrict__ arguments: restating the qualifier here costs
// source_solve6_kernel an occupancy step.
template <class B>
__device__ __forceinline__ void solve_body(const double* state, int n, double min_samples, double min_pivot,
                                           double* est, uint8_t* status) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double* st = state + (int64_t)e * B::STATE_N;
    double* out = est + (int64_t)e * B::EST_N;
    const double nan = __builtin_nan("");
    const bool any = st[B::COUNT] > 0.0;
    double fit[B::FIT_N];
#pragma unroll
    for (int j = 0; j < B::FIT_N; ++j) fit[j] = nan;
    status[e] = (uint8_t)solve_core<B>(st[B::COUNT], st + B::A, st + B::G, st + B::CX, min_samples, min_pivot, fit);
#pragma unroll
    for (int j = 0; j < B::FIT_N; ++j) out[j] = fit[j];
    out[B::FIT_N] = any ? st[B::XMAX] : nan;
    out[B::FIT_N + 1] = any ? st[B::YMAX] : nan;
    out[B::FIT_N + 2] = any ? st[B::BMAX] : nan;
}

// The summary kernels: thread j of ONE block of 256 adds the envs j, j + 256, ... one after the other into s[] (sums[1 + j] is
// s[j]), then block256_sum's tree: uav_greedy_summary's order of summation.  Between head and tail each model adds its truth columns.
// head: the four status counts, the fitted env's error, its square, whether it is within loc_tol; returns the error (NaN unless fitted)
__device__ __forceinline__ double summary_head(int stt, const double* o, double sx, double sy, double loc_tol, double* s) {
#pragma clang fp contract(off)
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
        s[6] += err <= loc_tol ? 1.0 : 0.0;                     // false for a NaN
    }
    return err;
}
// tail: the largest sample's distance to the source and how many envs have one, at the basis's own sums
template <class B>
__device__ __forceinline__ void summary_tail(const double* o, double sx, double sy, double* s) {
#pragma clang fp contract(off)
    if (o[B::FIT_N + 2] == o[B::FIT_N + 2]) {                   // the env has a largest sample
        const double dx = o[B::FIT_N] - sx, dy = o[B::FIT_N + 1] - sy;
        s[B::SUM_MAX_ERR - 1] += sqrt(dx * dx + dy * dy);
        s[B::SUM_MAX_ERR] += 1.0;
    }
}
template <class B>
__device__ __forceinline__ void summary_write(const double* s, double* sm, int n, double* __restrict__ sums) {
#pragma unroll
    for (int j = 0; j < B::SUM_N - 1; ++j) {
        const double a = block256_sum(s[j], sm);
        if (threadIdx.x == 0) sums[1 + j] = a;
    }
    if (threadIdx.x == 0) sums[UAV_SRC_SUM_ENVS] = (double)n;
}

// ---- the entry points' refusals
static inline int source_cfg_ok(const uav_source_fit_cfg* cfg, const char* who, int least) {
    UAV_REQUIRE(cfg, "%s: NULL cfg", who);
    UAV_REQUIRE(cfg->use_tke == 0 || cfg->use_tke == 1, "%s: use_tke=%d must be 0 or 1", who, cfg->use_tke);
    UAV_REQUIRE(cfg->min_samples >= least, "%s: min_samples=%d must be at least %d (%s parameters)", who, cfg->min_samples, least,
                least == 4 ? "four" : "six");
    UAV_REQUIRE(cfg->floor - cfg->floor == 0.0 && cfg->floor >= 0.0, "%s: floor=%g must be finite and not negative", who, cfg->floor);
    UAV_REQUIRE(cfg->background - cfg->background == 0.0, "%s: background=%g must be finite", who, cfg->background);
    UAV_REQUIRE(cfg->min_pivot - cfg->min_pivot == 0.0 && cfg->min_pivot > 0.0, "%s: min_pivot=%g must be finite and positive", who,
                cfg->min_pivot);
    return 0;
}

// the records of a chunk as the moments kernels and the stop scan (after t0 earlier steps) index them
static inline int source_records_ok(const uav_source_fit_cfg* cfg, const char* who, int n, int k, int D, int t0, const float* pos) {
    UAV_REQUIRE(n >= 1 && k >= 1, "%s: n=%d, k=%d must be at least 1", who, n, k);
    UAV_REQUIRE(t0 >= 0 && (int64_t)t0 + k < (int64_t)1 << 31, "%s: t0=%d must not be negative, t0 + k below 2^31", who, t0);
    UAV_REQUIRE(D >= (cfg->use_tke ? 4 : 3), "%s: D=%d must be at least %d (obs[2]%s)", who, D, cfg->use_tke ? 4 : 3,
                cfg->use_tke ? " and obs[3]" : "");
    UAV_REQUIRE((int64_t)n * k * D < (int64_t)1 << 31, "%s: n * k * D = %lld is 2^31 or more", who, (long long)n * k * D);
    UAV_REQUIRE(((uintptr_t)pos & 7) == 0, "%s: pos is not 8-byte aligned", who);
    return 0;
}
