// phase_prof.h -- phase timing of a kernel's main loop, instrumented build only (`make prof`, -DUAV_X6_PROFILE:
// tools/libuavppo_prof.so); in the product build every macro here expands to nothing.  A wave keeps one cycle sum per phase
// in registers (s_memtime deltas between consecutive marks) and the chosen lanes copy theirs to a __device__ table at the
// kernel's end; the tools/perf_*.py scripts fetch the table through its exported reader and name the phases.
//   PROF_TABLE(table, dims, reader)   file scope: `__device__ unsigned long long table dims` and `extern "C" int reader(out)`
//   PROF_DECL(n)                      kernel scope: n phase sums and the time of the last mark
//   PROF_MARK(i)                      the time since the last mark goes to phase i
//   PROF_DEP(v)                       pins register v as used here, so that the work producing it is not sunk past the next mark
//   PROF_FLUSH(row, n, who)           lanes for which `who` holds write their n sums to row[0 .. n)
#pragma once

#ifdef UAV_X6_PROFILE
#define PROF_TABLE(table, dims, reader)                                                                            \
    __device__ unsigned long long table dims;                                                                      \
    extern "C" int reader(unsigned long long* out) {                                                               \
        return hipMemcpyFromSymbol(out, HIP_SYMBOL(table), sizeof(table)) == hipSuccess ? 0 : 1;                   \
    }
#define PROF_DECL(n) unsigned long long pm_[n] = {}, pl_ = __builtin_readcyclecounter()
#define PROF_MARK(i) do { const unsigned long long n_ = __builtin_readcyclecounter(); pm_[i] += n_ - pl_; pl_ = n_; } while (0)
#define PROF_DEP(v) asm volatile("" ::"v"(v))
#define PROF_FLUSH(row, n, who) do { if (who) for (int i_ = 0; i_ < (n); ++i_) (row)[i_] = pm_[i_]; } while (0)
#else
#define PROF_TABLE(table, dims, reader)
#define PROF_DECL(n)
#define PROF_MARK(i)
#define PROF_DEP(v)
#define PROF_FLUSH(row, n, who)
#endif
