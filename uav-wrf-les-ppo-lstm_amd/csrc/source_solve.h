// source_solve.h -- the source estimator's solve, for any number of basis functions: the state layout, the two bases, the scaled
// Cholesky and each basis's closed form (uavppo/source_fit.py states every line in numpy: coefficients, ISO / ANISO .closed_form).
// Nothing but <cmath>: the kernels of source_fit.hip / source_aniso.hip include it through source_core.h, and
// tests/host/source_core_check.cpp compiles it for the CPU.  Every operation is written out in its order and nothing contracts
// into an FMA (the pragma is per scope and an inlined body does not inherit its caller's), so host and device agree bit for bit in
// everything that goes through + - * / sqrt alone; peak and strength go through exp, theta through atan2.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define SRC_HD __host__ __device__ __forceinline__
#else
#define SRC_HD inline
#endif

constexpr int SRC_FITTED = 0, SRC_FEW = 1, SRC_DEGENERATE = 2, SRC_NOT_A_PEAK = 3;      // UAV_SRC_* of include/uavppo.h
constexpr double CELL_SCALE = 32.0;                             // p = (x - cx) / 32: exact in f64, |p| < 16
constexpr double PI_D = 3.141592653589793, TWO_PI_D = 6.283185307179586;

SRC_HD bool finite_d(double v) { return v - v == 0.0; }
// (i, j), i <= j, of an N x N upper triangle by rows
template <int N>
SRC_HD constexpr int tri(int i, int j) { return i * N - i * (i - 1) / 2 + (j - i); }
static_assert(tri<4>(1, 1) == 4 && tri<4>(3, 3) == 9 && tri<6>(1, 1) == 6 && tri<6>(5, 5) == 20, "triangle index");

// state f64 [STATE_N] of a fit with N_ basis functions: count, centre | A (upper triangle by rows) | g | the largest b, its cell.
// The accumulators of one record or one chunk are count | A | g (N_ACC).
template <int N_>
struct SourceLayout {
    static constexpr int N = N_, N_A = N_ * (N_ + 1) / 2, N_ACC = 1 + N_A + N_;
    static constexpr int COUNT = 0, CX = 1, CY = 2, A = 3, G = A + N_A, BMAX = G + N_, XMAX = BMAX + 1, YMAX = BMAX + 2, STATE_N = BMAX + 3;
};

// A round plume: ln b = a0 + a1 p + a2 q + a3 (p^2 + q^2).  fit = {mu_x, mu_y, sigma, peak, strength}.
struct IsoBasis : SourceLayout<4> {
    static constexpr int FIT_N = 5, EST_N = FIT_N + 3, SUM_N = 12, SUM_MAX_ERR = 10;
    SRC_HD static void phi(double p, double q, double* f) {
#pragma clang fp contract(off)
        f[0] = 1.0;
        f[1] = p;
        f[2] = q;
        f[3] = p * p + q * q;
    }
    // a0 .. a3 and centre = {cx, cy} -> fit, where the coefficients are a peak's; else untouched.  The centre comes by pointer: read
    // where it is used, it is not held in registers across the Cholesky (by value source_solve6_kernel loses an occupancy step).
    SRC_HD static bool finish(const double* a, const double* centre, double* fit) {
#pragma clang fp contract(off)
        const double s2 = -1.0 / (2.0 * a[3]);
        if (!(finite_d(a[0]) && finite_d(a[1]) && finite_d(a[2]) && finite_d(a[3]) && a[3] < 0.0 && finite_d(s2))) return false;
        const double sigma = CELL_SCALE * sqrt(s2);
        const double peak = exp(a[0] + (a[1] * a[1] + a[2] * a[2]) * s2 / 2.0);
        fit[0] = centre[0] + CELL_SCALE * a[1] * s2;
        fit[1] = centre[1] + CELL_SCALE * a[2] * s2;
        fit[2] = sigma;
        fit[3] = peak;
        fit[4] = TWO_PI_D * (sigma * sigma) * peak;
        return true;
    }
};

// A plume stretched along an axis: ln b = a0 + a1 p + a2 q + a3 p^2 + a4 p q + a5 q^2.  fit = {mu_x, mu_y, sigma_major,
// sigma_minor, theta, peak, strength}.
struct AnisoBasis : SourceLayout<6> {
    static constexpr int FIT_N = 7, EST_N = FIT_N + 3, SUM_N = 16, SUM_MAX_ERR = 13;
    SRC_HD static void phi(double p, double q, double* f) {
#pragma clang fp contract(off)
        f[0] = 1.0;
        f[1] = p;
        f[2] = q;
        f[3] = p * p;
        f[4] = p * q;
        f[5] = q * q;
    }
    SRC_HD static bool finish(const double* a, const double* centre, double* fit) {
#pragma clang fp contract(off)
        bool fin = true;
#pragma unroll
        for (int j = 0; j < N; ++j) fin = fin && finite_d(a[j]);
        const double l11 = -(2.0 * a[3]), l12 = -a[4], l22 = -(2.0 * a[5]);   // Lambda: the inverse covariance / 32^2
        const double det = l11 * l22 - l12 * l12;
        const double trace = l11 + l22;
        const double m0 = (l22 * a[1] - l12 * a[2]) / det;
        const double m1 = (l11 * a[2] - l12 * a[1]) / det;
        const double hd = (l11 - l22) / 2.0;
        const double disc = sqrt(hd * hd + l12 * l12);
        const double big = trace / 2.0 + disc;
        const double small = det / big;
        double v[FIT_N];
        v[0] = centre[0] + CELL_SCALE * m0;
        v[1] = centre[1] + CELL_SCALE * m1;
        v[2] = CELL_SCALE / sqrt(small);
        v[3] = CELL_SCALE / sqrt(big);
        const double th = atan2(-(2.0 * l12), l22 - l11) / 2.0;
        v[4] = th < 0.0 ? th + PI_D : th;
        v[5] = exp(a[0] + (a[1] * m0 + a[2] * m1) / 2.0);
        v[6] = TWO_PI_D * (v[2] * v[3]) * v[5];
        bool peaked = fin && det > 0.0 && trace > 0.0;
#pragma unroll
        for (int j = 0; j < FIT_N; ++j) peaked = peaked && finite_d(v[j]);
        if (!peaked) return false;
#pragma unroll
        for (int j = 0; j < FIT_N; ++j) fit[j] = v[j];
        return true;
    }
};

// A (upper triangle by rows) scaled by d_j = sqrt(A_jj), Cholesky by columns, the two triangular solves, the unscaling: a[N], and
// whether every pivot (the diagonal before its square root) was finite and at least min_pivot -- a[] is written only then.  low: the
// smallest pivot, -inf once one is not finite (the host check reads it; the kernels pass none).
template <int N>
SRC_HD bool chol_solve(const double* A, const double* g, double min_pivot, double* a, double* low = nullptr) {
#pragma clang fp contract(off)
    double d[N], L[N][N];
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] = sqrt(A[tri<N>(j, j)]);
    bool ok = true;
    double lo = INFINITY;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double s = A[tri<N>(j, j)] / (d[j] * d[j]);
#pragma unroll
        for (int c = 0; c < j; ++c) s = s - L[j][c] * L[j][c];
        ok = ok && finite_d(s) && s >= min_pivot;               // a NaN fails both
        lo = finite_d(s) ? (s < lo ? s : lo) : -INFINITY;
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double t = A[tri<N>(j, i)] / (d[i] * d[j]);
#pragma unroll
            for (int c = 0; c < j; ++c) t = t - L[i][c] * L[j][c];
            L[i][j] = t / L[j][j];
        }
    }
    if (low) *low = lo;
    if (!ok) return false;
    double z[N], u[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double t = g[j] / d[j];
#pragma unroll
        for (int c = 0; c < j; ++c) t = t - L[j][c] * z[c];
        z[j] = t / L[j][j];
    }
#pragma unroll
    for (int j = N - 1; j >= 0; --j) {
        double t = z[j];
#pragma unroll
        for (int c = j + 1; c < N; ++c) t = t - L[c][j] * u[c];
        u[j] = t / L[j][j];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] = u[j] / d[j];
    return true;
}

// One system -> its status; fit[B::FIT_N] is written only where FITTED (the stop scan keeps zeros there, the solve kernels NaN).
template <class B>
SRC_HD int solve_core(double count, const double* A, const double* g, const double* centre, double min_samples, double min_pivot,
                      double* fit) {
    if (!(count >= min_samples)) return SRC_FEW;
    double a[B::N];
    if (!chol_solve<B::N>(A, g, min_pivot, a)) return SRC_DEGENERATE;
    return B::finish(a, centre, fit) ? SRC_FITTED : SRC_NOT_A_PEAK;
}
