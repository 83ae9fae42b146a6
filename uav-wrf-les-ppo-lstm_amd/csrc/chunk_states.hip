// chunk_states.hip -- uav_lstm_chunk_states: the recurrent state entering every chunk of `chunk` consecutive steps, read out
// of ONE forward pass's y and stash.  Truncated BPTT (VecPPOTrainer(bptt_len=...)) views the [N][T] sample arrays as
// [N * C][chunk] with C = T / chunk and runs the sequence kernels on that view unchanged; what they need beside it is the
// state each chunk row starts from: this kernel's h_out, c_out [N * C][H].
//
// Row n * C + k is the state carried into step t0 = k * chunk, ALREADY multiplied by keep[n][t0]:
//   k = 0    h0[n] keep[n][0]                  c0[n] keep[n][0]
//   k > 0    y[n][t0 - 1] keep[n][t0]          stash[n][t0][4H:5H] keep[n][t0]      (the stash's c_prev slot)
// The slot holds the cell state entering step t in every forward form that fills a stash -- the h = 64 / 128 sequence kernels
// (lstm.hip: c_reg, masked by the step before), lstm_generic.hip's cell kernel (cs, masked), lstm_h3.hip's h = 256 step kernel (written
// unmasked by step t - 1 and rewritten masked by step t where the env restarts) and uav_rollout's stash with and without the
// trend channels (c_reg, zeroed by keep_fixup) -- and y holds the unmasked h_t in all of them; with keep in {0, 1} the
// product here is the same number whether or not the slot was masked before.
//
// Work decomposition.  A row of H floats is cut into units of 16 bytes (H % 4 == 0 and every base 16-byte aligned) or of
// 4 bytes; unit u belongs to row u / units_per_row, so consecutive lanes run along H.  One lane moves one unit of h and the
// same unit of c: two loads, then two plain vector stores.  No atomics, no workspace.
#include "common.h"

namespace {

constexpr int CHUNK_THREADS = 256;

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float scaled(float v, float k) { return v * k; }
__device__ __forceinline__ f32x4_t scaled(f32x4_t v, float k) { return f32x4_t{v.x * k, v.y * k, v.z * k, v.w * k}; }

template <typename V>
__global__ __launch_bounds__(CHUNK_THREADS) void chunk_states_kernel(const float* __restrict__ y, const float* __restrict__ stash,
                                                                     const float* __restrict__ keep, const float* __restrict__ h0,
                                                                     const float* __restrict__ c0, int T, int H, int chunk, int C,
                                                                     unsigned units_per_row, unsigned n_units,
                                                                     float* __restrict__ h_out, float* __restrict__ c_out) {
    const unsigned u = blockIdx.x * CHUNK_THREADS + threadIdx.x;
    if (u >= n_units) return;
    constexpr unsigned W = sizeof(V) / sizeof(float);
    const unsigned row = u / units_per_row;                    // n * C + k
    const unsigned e = (u - row * units_per_row) * W;          // first float of the unit within the row
    const unsigned n = row / (unsigned)C, k = row - n * (unsigned)C;
    const size_t t0 = (size_t)k * chunk, st = (size_t)n * T + t0;      // N * T * 6H < 2^31: every offset below fits
    const float kp = keep ? keep[st] : 1.f;
    const float* hs = k ? y + (st - 1) * H + e : h0 + (size_t)n * H + e;
    const float* cs = k ? stash + st * (6 * (size_t)H) + 4 * (size_t)H + e : c0 + (size_t)n * H + e;
    const V hv = *reinterpret_cast<const V*>(hs);
    const V cv = *reinterpret_cast<const V*>(cs);
    *reinterpret_cast<V*>(h_out + (size_t)row * H + e) = scaled(hv, kp);
    *reinterpret_cast<V*>(c_out + (size_t)row * H + e) = scaled(cv, kp);
}

}  // namespace

extern "C" int uav_lstm_chunk_states(uav_ctx* ctx, const float* y, const float* stash, const float* keep, const float* h0,
                                     const float* c0, int N, int T, int H, int chunk, float* h_out, float* c_out,
                                     uav_stream stream) {
    UAV_REQUIRE(ctx && y && stash && h0 && c0 && h_out && c_out, "uav_lstm_chunk_states: NULL argument (only keep may be NULL)");
    UAV_REQUIRE(N >= 1 && T >= 1, "uav_lstm_chunk_states: N=%d T=%d (positive)", N, T);
    UAV_REQUIRE(H >= 1, "uav_lstm_chunk_states: H=%d (positive)", H);
    UAV_REQUIRE(chunk >= 1, "uav_lstm_chunk_states: chunk=%d (at least 1)", chunk);
    UAV_REQUIRE(T % chunk == 0, "uav_lstm_chunk_states: T=%d is not a multiple of chunk=%d", T, chunk);
    const unsigned long long stash_floats = (unsigned long long)N * (unsigned long long)T * 6ULL * (unsigned long long)H;
    UAV_REQUIRE(stash_floats < 0x80000000ULL, "uav_lstm_chunk_states: N * T * 6H = %llu (below 2^31)", stash_floats);
    const uintptr_t bases = (uintptr_t)y | (uintptr_t)stash | (uintptr_t)h0 | (uintptr_t)c0 | (uintptr_t)h_out | (uintptr_t)c_out;
    UAV_REQUIRE((bases | (uintptr_t)keep) % 4 == 0, "uav_lstm_chunk_states: an array is not 4-byte aligned");
    const int C = T / chunk;
    const bool vec = H % 4 == 0 && bases % 16 == 0;
    const unsigned units_per_row = (unsigned)(vec ? H / 4 : H);
    const unsigned n_units = (unsigned)N * (unsigned)C * units_per_row;          // <= N * T * H < 2^31 / 6
    const unsigned blocks = (n_units + CHUNK_THREADS - 1) / CHUNK_THREADS;
    if (vec)
        hipLaunchKernelGGL(chunk_states_kernel<f32x4_t>, dim3(blocks), dim3(CHUNK_THREADS), 0, as_stream(stream), y, stash, keep, h0,
                           c0, T, H, chunk, C, units_per_row, n_units, h_out, c_out);
    else
        hipLaunchKernelGGL(chunk_states_kernel<float>, dim3(blocks), dim3(CHUNK_THREADS), 0, as_stream(stream), y, stash, keep, h0,
                           c0, T, H, chunk, C, units_per_row, n_units, h_out, c_out);
    UAV_LAUNCH_CHECK();
    return 0;
}
