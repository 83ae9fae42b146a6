// gather.hip -- uav_gather_rows_multi: the selected rows (envs) of up to UAV_GATHER_MAX_SPECS arrays packed into contiguous
// buffers by ONE launch.  A shuffled minibatch of whole env sequences is then an ordinary contiguous minibatch: the LSTM
// sequence kernels (forward, BPTT, weight gradients) and the fused MLP kernel run on it unchanged.
//
// Work decomposition.  An array is cut into units of 16 bytes (row_bytes, bases and plane strides all multiples of 16) or of
// 4 bytes (anything else); its units are numbered plane-major, then selected row, then position in the row, so consecutive
// lanes hold consecutive units of one row (and run on into the next selected row where a row ends inside a wave).  A
// workgroup of 256 lanes takes UNITS_PER_BLOCK consecutive units of ONE array -- every array gets its own whole number of
// workgroups, so which array a workgroup serves is uniform and its descriptor is read with scalar loads.  Each lane issues
// its two loads before its two stores.  At the C3 minibatch (512 envs of T = 128, D = 6, h = 128: 3.6 MB) that is 448
// workgroups for 256 CUs.
#include "common.h"

namespace {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_PER_LANE = 2;
constexpr unsigned UNITS_PER_BLOCK = GATHER_THREADS * GATHER_PER_LANE;

struct GatherArray {
    const char* src;
    char* dst;
    long long src_plane, dst_plane;      // bytes between planes
    long long row_bytes;
    unsigned units_per_row;              // row_bytes / (vec ? 16 : 4)
    unsigned n_units;                    // planes * n_sel * units_per_row
    unsigned block_end;                  // first workgroup index past this array's
    unsigned vec;                        // 1: 16-byte units, 0: 4-byte units
};
struct GatherArgs {
    GatherArray a[UAV_GATHER_MAX_SPECS];
    int n;
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// unit u of array g: byte offsets of its source and destination
template <typename V>
__device__ __forceinline__ void unit_offsets(const GatherArray& g, unsigned u, const int32_t* __restrict__ idx, unsigned n_sel, int n_rows,
                                             long long& from, long long& to) {
    const unsigned row = u / g.units_per_row;                        // plane * n_sel + j
    const unsigned c = u - row * g.units_per_row;
    const unsigned p = row / n_sel, j = row - p * n_sel;
    int i = idx[j];
    i = i < 0 ? 0 : (i >= n_rows ? n_rows - 1 : i);                  // a bad index reads a wrong row, never outside the array
    const long long within = (long long)c * (long long)sizeof(V);
    from = p * g.src_plane + i * g.row_bytes + within;
    to = p * g.dst_plane + j * g.row_bytes + within;
}

template <typename V>
__device__ __forceinline__ void gather_units(const GatherArray& g, unsigned u0, const int32_t* __restrict__ idx, unsigned n_sel,
                                             int n_rows) {
    static_assert(GATHER_PER_LANE == 2, "two units per lane");
    const unsigned u1 = u0 + GATHER_THREADS;
    const bool ok0 = u0 < g.n_units, ok1 = u1 < g.n_units;
    long long f0, t0, f1, t1;
    unit_offsets<V>(g, ok0 ? u0 : 0u, idx, n_sel, n_rows, f0, t0);   // a lane past the end loads unit 0 and stores nothing
    unit_offsets<V>(g, ok1 ? u1 : 0u, idx, n_sel, n_rows, f1, t1);
    const V v0 = *reinterpret_cast<const V*>(g.src + f0);
    const V v1 = *reinterpret_cast<const V*>(g.src + f1);
    if (ok0) *reinterpret_cast<V*>(g.dst + t0) = v0;
    if (ok1) *reinterpret_cast<V*>(g.dst + t1) = v1;
}

__global__ __launch_bounds__(GATHER_THREADS) void gather_rows_multi_kernel(GatherArgs args, const int32_t* __restrict__ idx,
                                                                          unsigned n_sel, int n_rows) {
    int s = 0;
    while (s + 1 < args.n && blockIdx.x >= args.a[s].block_end) ++s;
    const GatherArray& g = args.a[s];
    const unsigned first = s ? args.a[s - 1].block_end : 0u;
    const unsigned u0 = (blockIdx.x - first) * UNITS_PER_BLOCK + threadIdx.x;
    if (g.vec)
        gather_units<u32x4>(g, u0, idx, n_sel, n_rows);
    else
        gather_units<uint32_t>(g, u0, idx, n_sel, n_rows);
}

}  // namespace

extern "C" int uav_gather_rows_multi(uav_ctx* ctx, const int32_t* idx, int64_t n_sel, int64_t n_rows, const uav_gather_spec* specs,
                                     int n_specs, uav_stream stream) {
    UAV_REQUIRE(ctx && idx && specs, "uav_gather_rows_multi: NULL argument");
    UAV_REQUIRE(n_specs >= 1 && n_specs <= UAV_GATHER_MAX_SPECS, "uav_gather_rows_multi: n_specs=%d (1 .. %d)", n_specs,
                UAV_GATHER_MAX_SPECS);
    UAV_REQUIRE(n_sel > 0 && n_sel <= 0x7fffffffLL && n_rows > 0 && n_rows <= 0x7fffffffLL,
                "uav_gather_rows_multi: n_sel=%lld n_rows=%lld (1 .. 2^31 - 1)", (long long)n_sel, (long long)n_rows);
    GatherArgs args;
    memset(&args, 0, sizeof(args));
    args.n = n_specs;
    unsigned long long blocks = 0;
    for (int s = 0; s < n_specs; ++s) {
        const uav_gather_spec& sp = specs[s];
        UAV_REQUIRE(sp.src && sp.dst, "uav_gather_rows_multi: spec %d: NULL array", s);
        UAV_REQUIRE(sp.row_bytes > 0 && sp.row_bytes % 4 == 0, "uav_gather_rows_multi: spec %d: row_bytes=%lld (a positive multiple of 4)",
                    s, (long long)sp.row_bytes);
        UAV_REQUIRE(sp.planes >= 1, "uav_gather_rows_multi: spec %d: planes=%d", s, sp.planes);
        UAV_REQUIRE((uintptr_t)sp.src % 4 == 0 && (uintptr_t)sp.dst % 4 == 0, "uav_gather_rows_multi: spec %d: an array is not 4-byte aligned", s);
        const bool many = sp.planes > 1;
        UAV_REQUIRE(!many || (sp.src_plane_stride_bytes >= n_rows * sp.row_bytes && sp.dst_plane_stride_bytes >= n_sel * sp.row_bytes &&
                              sp.src_plane_stride_bytes % 4 == 0 && sp.dst_plane_stride_bytes % 4 == 0),
                    "uav_gather_rows_multi: spec %d: plane strides %lld / %lld do not cover %lld / %lld rows of %lld bytes", s,
                    (long long)sp.src_plane_stride_bytes, (long long)sp.dst_plane_stride_bytes, (long long)n_rows, (long long)n_sel,
                    (long long)sp.row_bytes);
        const unsigned long long words = (unsigned long long)sp.planes * (unsigned long long)n_sel * (unsigned long long)(sp.row_bytes / 4);
        UAV_REQUIRE(words < 0x80000000ULL, "uav_gather_rows_multi: spec %d: %llu 4-byte words to move (below 2^31)", s, words);
        const bool vec = sp.row_bytes % 16 == 0 && (uintptr_t)sp.src % 16 == 0 && (uintptr_t)sp.dst % 16 == 0 &&
                         (!many || (sp.src_plane_stride_bytes % 16 == 0 && sp.dst_plane_stride_bytes % 16 == 0));
        GatherArray& g = args.a[s];
        g.src = static_cast<const char*>(sp.src);
        g.dst = static_cast<char*>(sp.dst);
        g.src_plane = many ? sp.src_plane_stride_bytes : 0;
        g.dst_plane = many ? sp.dst_plane_stride_bytes : 0;
        g.row_bytes = sp.row_bytes;
        g.vec = vec ? 1u : 0u;
        g.units_per_row = (unsigned)(sp.row_bytes / (vec ? 16 : 4));
        g.n_units = (unsigned)(words / (vec ? 4 : 1));
        blocks += (g.n_units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK;
        g.block_end = (unsigned)blocks;
    }
    UAV_REQUIRE(blocks < 0x7fffffffULL, "uav_gather_rows_multi: %llu workgroups", blocks);
    hipLaunchKernelGGL(gather_rows_multi_kernel, dim3((unsigned)blocks), dim3(GATHER_THREADS), 0, as_stream(stream), args, idx,
                       (unsigned)n_sel, (int)n_rows);
    UAV_LAUNCH_CHECK();
    return 0;
}
