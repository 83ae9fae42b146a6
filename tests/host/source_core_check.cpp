// The source estimator's solve (csrc/source_solve.h: chol_solve, the two closed forms, solve_core) on the CPU: plain C++17, no HIP
// header, no device.  Built and run by tests/test_source_core_host.py under AddressSanitizer + UBSan.
//   source_core_check SYSTEMS     reads "N M min_samples min_pivot", then M lines "count cx cy A[N (N + 1) / 2] g[N]" (hex floats),
//                                 N = 4 or 6; prints per system "status solved low a[N] fit[FIT_N]" (hex floats; a is 0 where the
//                                 Cholesky was refused, fit NaN unless FITTED as the solve kernels prefill it).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "source_solve.h"

template <class B>
static int run(FILE* f, int m, double min_samples, double min_pivot) {
    std::vector<double> v(3 + B::N_A + B::N);
    for (int s = 0; s < m; ++s) {
        for (double& x : v) {
            char word[64];
            if (fscanf(f, "%63s", word) != 1) return 2;
            x = strtod(word, nullptr);
        }
        const double *A = v.data() + 3, *g = A + B::N_A;
        double a[B::N] = {}, fit[B::FIT_N], low = 0.0;
        for (double& x : fit) x = NAN;
        const bool solved = chol_solve<B::N>(A, g, min_pivot, a, &low);
        const int status = solve_core<B>(v[0], A, g, v.data() + 1, min_samples, min_pivot, fit);
        printf("%d %d %a", status, (int)solved, low);
        for (double x : a) printf(" %a", x);
        for (double x : fit) printf(" %a", x);
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0, m = 0;
    char ms[64], mp[64];
    int rc = 2;
    if (fscanf(f, "%d %d %63s %63s", &n, &m, ms, mp) == 4) {
        const double min_samples = strtod(ms, nullptr), min_pivot = strtod(mp, nullptr);
        if (n == IsoBasis::N) rc = run<IsoBasis>(f, m, min_samples, min_pivot);
        if (n == AnisoBasis::N) rc = run<AnisoBasis>(f, m, min_samples, min_pivot);
    }
    fclose(f);
    return rc;
}
