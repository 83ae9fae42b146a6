// common.h -- shared device/host helpers for libuavppo (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/uavppo.h"
#include "lstm_forms.h"      // DgTile, DgPack, uav_lstm_forms, uav_lstm_mode
#include "scratch.h"         // uav_scratch

// One per uav_create, never copied: a helper that needs less than the whole handle takes the part as a value (the mode, a
// workspace slice).
struct uav_ctx {
    uav_ctx() = default;
    uav_ctx(const uav_ctx&) = delete;
    uav_ctx& operator=(const uav_ctx&) = delete;
    int device;
    int num_cu;
    void* ws;          // scratch for two-stage reductions / split-K slabs
    size_t ws_bytes;
    uav_scratch scratch() const { return uav_scratch{(char*)ws, ws_bytes, num_cu}; }      // the whole workspace
    double* pow075;    // device table pow(i, 0.75), i = 0..5000 (env_core.h)
    double* wave;      // device tables sin(0.05 x) | cos(0.07 y), x, y = 0..499 (env_core.h field_at)
    double* ftab;      // device tables of the table-driven f64 log / cos-sin / exp (env_core.h ft_*)
    // uav_set_lstm_arith / uav_set_debug_flags.  No getenv on any call path: the UAV_LSTM_BF16X6 / UAV_LSTM_F32_MFMA environment
    // variables are read ONCE, by uav_create, as the handle's initial mode.
    uav_lstm_mode mode;
    hipStream_t side[3];      // uav_lstm_bwd_stack: one stream per layer below the top (created on first use)
    hipEvent_t side_ev[8];    // fork / join + a small ring of per-step hand-off events per side stream
    void* comm;               // ncclComm_t of this process's rank (comm.hip: uav_comm_init), or NULL
    int comm_rank, comm_world;
    uav_lstm_forms forms;     // what the dgates / stash buffers of the LSTM update hold (lstm_forms.h; decided in lstm_api.hip)
    double* ppo_diag;  // device f64[UAV_PPO_DIAG_N] the loss-bearing entry points overwrite with their diagnostic sums, or NULL (uav_set_ppo_diag)
};

void uav_set_error(const char* fmt, ...);

// Opt a kernel in to `bytes` of dynamic LDS.  Function attributes are PER DEVICE, so the "already done" memo is keyed by
// (current device, kernel): a process that drives several devices through several handles gets the attribute on each.
hipError_t uav_dyn_lds(const void* kernel, int bytes);

#define UAV_CHECK_HIP(expr)                                                          \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) {                                                      \
            uav_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

#define UAV_REQUIRE(cond, ...)                                                       \
    do {                                                                             \
        if (!(cond)) {                                                               \
            uav_set_error(__VA_ARGS__);                                              \
            return 2;                                                                \
        }                                                                            \
    } while (0)

#define UAV_LAUNCH_CHECK() UAV_CHECK_HIP(hipGetLastError())

static inline hipStream_t as_stream(uav_stream s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int WAVE = 64;

// Workgroup barrier that orders LDS traffic ONLY.  __syncthreads() also waits vmcnt(0): in the
// persistent kernels that drained the software-prefetched global loads and every outstanding
// store at each time step (lstm_bwd: 0.84 -> 0.6 ms).  Waves of one workgroup never exchange data
// through global memory inside these kernels, so LDS ordering is all the barrier has to give.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// A global load at  uniform pointer + 32-bit byte offset + constant,  the scalar-base form
//   global_load v, v_off, s[base:base+1] offset:imm
// -- against a v_lshl_add_u64, and the integer VALU work in front of it, per load when a 64-bit address is built per lane.
// For the compiler to pick that form in a loop, `ubase` must be loop-invariant (a kernel argument) and `off_bytes` must
// change inside the loop: give it as  lane part (formed once) + uniform part of this iteration  -- one v_add_u32 with a
// scalar operand per distinct uniform part, everything in front of it scalar arithmetic.  (Of a loop-invariant offset the
// zero-extension is hoisted out of the loop as a VGPR pair, and the 64-bit adds are back.)  Keep imm_bytes inside the
// immediate field (gfx950: -4096 .. 4095).
template <class V>
__device__ __forceinline__ V ld_ubase(const void* ubase, unsigned off_bytes, int imm_bytes = 0) {
    return *reinterpret_cast<const V*>(static_cast<const char*>(ubase) + off_bytes + imm_bytes);
}

// LSTM gate activations: v_exp_f32 + v_rcp_f32 (1 ulp each).  A plain `1.0f / x` compiles to the
// ~10-instruction IEEE division sequence; with 20 activations per lane per step that sequence,
// not the MFMAs, paced the persistent kernels (tools/mfma_probe.hip).
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) {
    // |x| >= 1/4: tanh(x) = 1 - 2 / (exp(2x) + 1): exact limits at +-inf, absolute error <= 1.9e-7, i.e. relative <= 8e-7 there.
    // |x| <  1/4: that form cancels (its RELATIVE error is 1.9e-7 / |x|: 1e-3 at |x| = 1e-4), so the odd Taylor polynomial
    // x (1 - x^2/3 + 2 x^4/15 - 17 x^6/315 + 62 x^8/2835) takes over: truncation 8.9e-3 x^10 <= 8.5e-9 relative, rounding
    // ~2e-7 relative.  Both are evaluated and one selected (no branch): +8 VALU per call, which against the exp form
    // alone costs +1.4 % of a C3 iteration and +3.8 % of the fused rollout (profiles/r05_ab_tanh.txt; the compile-time switch that
    // built the exp-only library was last present at commit 27bad41).
    const float big = 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f);
    const float x2 = x * x;
    float p = __builtin_fmaf(x2, 62.0f / 2835.0f, -17.0f / 315.0f);
    p = __builtin_fmaf(p, x2, 2.0f / 15.0f);
    p = __builtin_fmaf(p, x2, -1.0f / 3.0f);
    p = __builtin_fmaf(p, x2, 1.0f);
    return __builtin_fabsf(x) < 0.25f ? x * p : big;
}
// The same function with `big` as ONE fma, 1 - 2 r rounded once: what the h = 64 / 128 sequence kernels of lstm.hip compute (forward
// and BPTT, every arithmetic).  The plain form above is everybody else's: the fused rollout, greedy and tail kernels (rollout.hip),
// the h = 256 step path (lstm_h3.hip), lstm_generic.hip and peak_stop.hip.  The two differ in the last bit of some results.
__device__ __forceinline__ float fast_tanh_fma(float x) {
    const float big = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f), 1.0f);
    const float x2 = x * x;
    float p = __builtin_fmaf(x2, 62.0f / 2835.0f, -17.0f / 315.0f);
    p = __builtin_fmaf(p, x2, 2.0f / 15.0f);
    p = __builtin_fmaf(p, x2, -1.0f / 3.0f);
    p = __builtin_fmaf(p, x2, 1.0f);
    return __builtin_fabsf(x) < 0.25f ? x * p : big;
}

// ---- split-bf16 ("x6") arithmetic: an f32 value as three bf16 pieces a = p0 + p1 + p2 (8 significand bits each, so
// the split is exact); products of two split operands keep the six piece products with i + j <= 2 and accumulate them
// in f32 (v_mfma_f32_16x16x32_bf16).  Error and rate: tools/bf16x6_probe.hip; the argument: lstm.hip, FwdSplitGeom.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split3(float a, __bf16& p0, __bf16& p1, __bf16& p2) {
    p0 = (__bf16)a;
    const float r1 = a - (float)p0;
    p1 = (__bf16)r1;
    p2 = (__bf16)(r1 - (float)p1);
}
__device__ __forceinline__ unsigned short bf_bits(__bf16 v) { return __builtin_bit_cast(unsigned short, v); }

// ---- split-fp16 ("h3") arithmetic: an f32 value as TWO fp16 pieces, a = p0 + 2^-11 p1 with p0 = fp16(a) and
// p1 = fp16((a - p0) * 2^11): the residual is scaled back into fp16's normal range, so a is carried to 2^-24 |a| (its last
// f32 bit).  a b = p0 q0 + 2^-11 (p0 q1 + p1 q0) + O(2^-24 |a b|): the main product and the two cross products go to two
// f32 accumulators (v_mfma_f32_16x16x32_f16), combined once per dot product as acc0 + 2^-11 acc1.  Three products
// instead of the bf16 split's six, two pieces instead of three (the weights keep their f32 register footprint), and on a
// K=128 dot product a SMALLER error against f64 than either the bf16 split or the exact-f32 MFMA chain (rms 1.06e-7 vs
// 1.50e-7 vs 2.05e-7 of the terms' rms sum: fewer accumulator roundings; tools/f16x3_probe.hip).  fp16's range is the
// caller's business: |a| < 65504, and operands with a wide dynamic range (gradients) are block-scaled by a power of two.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr float H3_LO = 1.0f / 2048.0f;          // weight of the cross-product accumulator
__device__ __forceinline__ void split2h(float a, _Float16& p0, _Float16& p1) {
    p0 = (_Float16)a;
    p1 = (_Float16)((a - (float)p0) * 2048.0f);
}
__device__ __forceinline__ unsigned short h_bits(_Float16 v) { return __builtin_bit_cast(unsigned short, v); }

// ---- the two splits as arithmetic policies of the persistent h = 64 / 128 sequence kernels (lstm.hip): the weights are
// the A operand of a 16x16x32 MFMA, h_t (forward) or the gate gradients (backward) the B operand.  A policy fixes the
// pieces, the order of the piece products of one K = 32 slab and the accumulator each product goes to -- and so the
// result bits.  w(q, p) / w(p) is piece p of a weight fragment, a / b / h(p) piece p of the other operand.
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct SplitF16x3 {          // UAV_ARITH_FP16X3 (the default): two fp16 pieces, three products
    typedef _Float16 piece;
    typedef f16x8 vec;
    static constexpr int NP = 2;
    // gate gradients span many binades, fp16 does not: the backward scales each env's by a power of two before the split
    static constexpr bool BLOCK_SCALE = true;
    // the backward's dG stores go behind the products (they drain under the partial-sum reduce, not ahead of the MFMAs)
    static constexpr bool DG_STORES_LATE = true;
    // the weight pieces take exactly the f32 weights' registers: nothing is parked in LDS
    static constexpr int fwd_park(int) { return 0; }
    static constexpr int bwd_park(int) { return 0; }
    __device__ __forceinline__ static void split(float a, piece (&p)[NP]) { split2h(a, p[0], p[1]); }
    __device__ __forceinline__ static unsigned short bits(piece v) { return h_bits(v); }
    __device__ __forceinline__ static f32x4 mma(vec a, vec b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    // forward, four gates: main products into acc, cross products into acl -- eight independent accumulators
    template <class W>
    __device__ __forceinline__ static void gates_slab(f32x4 (&acc)[4], f32x4 (&acl)[4], W w, const vec (&a)[NP]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acl[q] = mma(w(q, 1), a[0], acl[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mma(w(q, 0), a[0], acc[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acl[q] = mma(w(q, 0), a[1], acl[q]);
    }
    template <class W, class B>
    __device__ __forceinline__ static void head_slab(f32x4& ha, f32x4& hb, W w, B h) {
        hb = mma(w(1), h(0), hb);
        hb = mma(w(0), h(1), hb);
        ha = mma(w(0), h(0), ha);
    }
    // acc + 2^-11 acl as one fma, per element (only lstm.hip's kernels combine their accumulators through the policy)
    __device__ __forceinline__ static float sum(float acc, float acl) { return __builtin_fmaf(acl, H3_LO, acc); }
    __device__ __forceinline__ static f32x4 sum(f32x4 acc, f32x4 acl) {
        return __builtin_elementwise_fma(acl, f32x4{H3_LO, H3_LO, H3_LO, H3_LO}, acc);
    }
    // backward, one partial tile: the same three products over two accumulators
    template <class W>
    __device__ __forceinline__ static void tile_slab(f32x4& a0, f32x4& a1, W w, const vec (&b)[NP]) {
        a1 = mma(w(1), b[0], a1);
        a0 = mma(w(0), b[0], a0);
        a1 = mma(w(0), b[1], a1);
    }
    __device__ __forceinline__ static f32x4 tile_sum(f32x4 a0, f32x4 a1) { return sum(a0, a1); }
};

struct SplitBf16x6 {         // UAV_ARITH_BF16X6: three bf16 pieces, six products, f32's exponent range
    typedef __bf16 piece;
    typedef bf16x8 vec;
    static constexpr int NP = 3;
    static constexpr bool BLOCK_SCALE = false;
    static constexpr bool DG_STORES_LATE = false;
    // three bf16 pieces of W_hh are 1.5x its f32 size = 3/4 of the CU's register file at H = 128: there the smallest
    // piece of the first 3 gates (forward) / the first 6 (tile, slab) items (backward) lives in a wave-private LDS slab
    static constexpr int fwd_park(int H) { return H >= 128 ? 3 : 0; }
    static constexpr int bwd_park(int H) { return H >= 128 ? 6 : 0; }
    __device__ __forceinline__ static void split(float a, piece (&p)[NP]) { split3(a, p[0], p[1], p[2]); }
    __device__ __forceinline__ static unsigned short bits(piece v) { return bf_bits(v); }
    __device__ __forceinline__ static f32x4 mma(vec a, vec b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    // forward, four gates: the six products with i + j <= 2, smallest first, one accumulator per gate -- four
    // independent accumulators between dependent MFMAs
    template <class W>
    __device__ __forceinline__ static void gates_slab(f32x4 (&acc)[4], f32x4 (&)[4], W w, const vec (&a)[NP]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mma(w(q, 0), a[2], acc[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mma(w(q, 1), a[1], acc[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mma(w(q, 2), a[0], acc[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mma(w(q, 0), a[1], acc[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mma(w(q, 1), a[0], acc[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mma(w(q, 0), a[0], acc[q]);
    }
    template <class W, class B>
    __device__ __forceinline__ static void head_slab(f32x4& ha, f32x4&, W w, B h) {
        ha = mma(w(0), h(2), ha);
        ha = mma(w(1), h(1), ha);
        ha = mma(w(2), h(0), ha);
        ha = mma(w(0), h(1), ha);
        ha = mma(w(1), h(0), ha);
        ha = mma(w(0), h(0), ha);
    }
    template <class V> __device__ __forceinline__ static V sum(V acc, V) { return acc; }
    // backward, one partial tile: the same six products alternating between two accumulators
    template <class W>
    __device__ __forceinline__ static void tile_slab(f32x4& a0, f32x4& a1, W w, const vec (&b)[NP]) {
        a0 = mma(w(0), b[2], a0);
        a1 = mma(w(1), b[1], a1);
        a0 = mma(w(2), b[0], a0);
        a1 = mma(w(0), b[1], a1);
        a0 = mma(w(1), b[0], a0);
        a1 = mma(w(0), b[0], a1);
    }
    __device__ __forceinline__ static f32x4 tile_sum(f32x4 a0, f32x4 a1) { return a0 + a1; }
};

// ---- wave / block reductions (deterministic: fixed tree, no atomics) -------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // valid in lane 0
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_allsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over a 256-thread block; result valid in thread 0. `sm` has >= 4 slots.
template <typename T>
__device__ __forceinline__ T block256_sum(T v, T* sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sm[w] = v;
    __syncthreads();
    T r = T(0);
    if (threadIdx.x == 0) r = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    __syncthreads();
    return r;
}
