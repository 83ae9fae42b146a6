// lstm.hip -- L1: nn.LSTM-semantics sequence kernels (forward with BPTT stash, backward).
//
// Reference semantics: torch.nn.LSTM as the reference uses it (PPOV2.0/model.py:206-212,
// PPOV2.1/model.py:263,284,311,330): gates = x W_ih^T + b_ih + h W_hh^T + b_hh, chunk order
// i,f,g,o, c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c').
//
// MI355X design (persistent over time):
//   * one workgroup owns 16 env sequences for ALL T steps; grid = N/16 (256 WGs at N=4096);
//   * the recurrent weights stay on chip for the whole sequence (VGPRs, plus a wave-private LDS slab for the part
//     that does not fit): they are read from HBM once per launch, not once per step;
//   * the i,f,g,o pre-activations of one (env, unit) land in ONE lane's accumulators, so the gate pointwise and the
//     cell state never leave registers; h_t / the gate gradients are exchanged through LDS, one or two barriers a step.
// Kernel families in this file (dispatch: launch_fwd, lstm_bwd_seq):
//   SPLIT    one forward body (lstm_fwd_split) and one backward body (lstm_bwd_split), templated on the arithmetic of
//            their matrix products: the 16-bit matrix pipe at f32 accuracy with every operand split into pieces
//            (common.h: SplitF16x3, SplitBf16x6).  Weights-as-A orientation (a lane owns one env and four consecutive
//            units: dwordx4 stores), the head product fused into the forward, stash by LDS-DMA and the K split over the
//            waves in the backward.  Two arithmetics, each with its own entry points:
//              fp16 split (DEFAULT): lstm_fwd_h3_kernel, lstm_bwd_h3k_kernel -- two pieces, three products; the gate
//                gradients are block-scaled per env;
//              bf16 split: lstm_fwd_x6_kernel, lstm_bwd_x6k_kernel -- three pieces, six products (f32's exponent range:
//                no operand limits, twice the matrix work); uav_set_lstm_arith(UAV_ARITH_BF16X6);
//   EXACT-F32 lstm_fwd_kernel, lstm_bwd_kernel (also the plain-dy backward of stacked layers): v_mfma_f32_16x16x4_f32
//            with 128 weight VGPRs per lane; uav_set_lstm_arith(UAV_ARITH_F32_MFMA).
//   (Earlier generations -- an output-split bf16 backward exchanging dG through three LDS planes, an LDS-DMA form of
//    the exact-f32 backward -- were measured, superseded and removed in round 3; their numbers are in profiles/README.md.)
//   (A half-step stagger of waves 4-7 against 0-3 was built and measured on the exact-f32 forward: no gain,
//    tools/stagger_probe.hip; what paced the step was the IEEE division sequence inside the activations, now v_rcp_f32.)
//   * the K=I<=8 input projection rides along as two exact-f32 MFMA k-steps; wider inputs (stacked layers) use a
//     time-batched GEMM into the stash first.
#include <stdlib.h>
#include <type_traits>
#include "internal.h"
#include "phase_prof.h"

constexpr int MT = 16;      // env rows per workgroup (MFMA M)
constexpr int TC = 32;      // time steps staged per chunk

// Every tanh of this file is common.h's fast_tanh_fma, and every a b + c that is ONE rounding is written as an fma: the file is built
// without contraction, like the rest of the library, so the bits are the source's ("Contraction").  Where two
// instantiations round a quantity differently (the compiler once chose, and the recorded bits hold both), the site says so.
template <int H>
struct FwdGeom {
    static constexpr int NW = H / 16;          // waves per workgroup
    static constexpr int KS = H / 4;           // MFMA k-steps over the hidden dimension
    static constexpr int SEG = KS + 4;         // padded quarter-row (conflict-free ds_read_b128)
    static constexpr int S = 4 * SEG + 8;      // padded row stride of the h tile
    static constexpr size_t LDS = (2 * MT * S + TC * MT * 8 + (TC + 1) * MT) * sizeof(float);
};
// position of hidden unit u inside a padded h row
template <int H>
__device__ __forceinline__ int hpos(int u) { return (u / (H / 4)) * FwdGeom<H>::SEG + (u % (H / 4)); }

template <int H, bool FUSE_X>
__global__ __launch_bounds__(H * 4) void lstm_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ keep, const float* __restrict__ h0,
    const float* __restrict__ c0, const float* __restrict__ w_ih, const float* __restrict__ w_hh,
    const float* __restrict__ b_ih, const float* __restrict__ b_hh, int N, int T, int I,
    float* __restrict__ y, float* __restrict__ hn, float* __restrict__ cn, float* __restrict__ stash) {
    using G = FwdGeom<H>;
    constexpr int KS = G::KS, SEG = G::SEG, S = G::S;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* hbuf = smem;                        // [2][MT][S]
    float* xbuf = hbuf + 2 * MT * S;           // [TC][MT][8]
    float* kbuf = xbuf + TC * MT * 8;          // [TC+1][MT]

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int u = 16 * w + j;                  // hidden unit of this lane's accumulator column
    const int n0 = blockIdx.x * MT;

    // ---- this wave's slice of the weights, resident in VGPRs for the whole sequence
    float wh[4][KS];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float* src = w_hh + (size_t)(q * H + u) * H + kq * KS;
#pragma unroll
        for (int s = 0; s < KS; s += 4) {
            const float4 v = *reinterpret_cast<const float4*>(src + s);
            wh[q][s] = v.x; wh[q][s + 1] = v.y; wh[q][s + 2] = v.z; wh[q][s + 3] = v.w;
        }
    }
    float wx[4][2], bias[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bias[q] = FUSE_X ? (b_ih[q * H + u] + b_hh[q * H + u]) : 0.f;   // non-fused: bias is in `pre`
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k = 2 * kq + s;
            wx[q][s] = (FUSE_X && k < I) ? w_ih[(size_t)(q * H + u) * I + k] : 0.f;
        }
    }

    // ---- incoming state of this lane's (env row r, unit u) pairs: rows e = 4*kq + r
    float c_reg[4], hin[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = 4 * kq + r;
        const int n = min(n0 + e, N - 1);
        const float k0 = keep ? keep[(size_t)n * T] : 1.f;
        c_reg[r] = c0[(size_t)n * H + u] * k0;
        hin[r] = h0[(size_t)n * H + u] * k0;
        hbuf[e * S + hpos<H>(u)] = hin[r];
    }
    int cur = 0;
    float h_last[4] = {0.f, 0.f, 0.f, 0.f};

    for (int t0 = 0; t0 < T; t0 += TC) {
        const int tc = min(TC, T - t0);
        // ---- stage x[n0..n0+15][t0..t0+tc) (zero-padded to 8 features) and keep[..][t0..t0+tc]
        if (FUSE_X) {
            for (int idx = threadIdx.x; idx < MT * tc * 8; idx += blockDim.x) {
                const int e = idx / (tc * 8), rem = idx % (tc * 8), tt = rem >> 3, f = rem & 7;
                const int n = min(n0 + e, N - 1);
                xbuf[(tt * MT + e) * 8 + f] = (f < I) ? x[((size_t)n * T + t0 + tt) * I + f] : 0.f;
            }
        }
        for (int idx = threadIdx.x; idx < MT * (tc + 1); idx += blockDim.x) {
            const int e = idx / (tc + 1), tt = idx % (tc + 1);
            const int n = min(n0 + e, N - 1);
            kbuf[tt * MT + e] = (keep && t0 + tt < T) ? keep[(size_t)n * T + t0 + tt] : 1.f;
        }
        lds_barrier();

        for (int tt = 0; tt < tc; ++tt) {
            const int t = t0 + tt;
            f32x4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (FUSE_X) {
                    acc[q] = f32x4{bias[q], bias[q], bias[q], bias[q]};
                } else {
                    // pre-activations x W_ih^T + b from the time-batched GEMM (gates slot of the stash)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int n = min(n0 + 4 * kq + r, N - 1);
                        acc[q][r] = stash[((size_t)n * T + t) * (6 * H) + q * H + u];
                    }
                }
            }
            if (FUSE_X) {
                const float2 ax = *reinterpret_cast<const float2*>(&xbuf[(tt * MT + j) * 8 + 2 * kq]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax.x, wx[q][0], acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax.y, wx[q][1], acc[q], 0, 0, 0);
                }
            }
            // recurrent part: A = h_{t-1}[env j][k], k permuted so that lane (j,kq) reads a contiguous run
            const float* hrow = hbuf + cur * MT * S + j * S + kq * SEG;
#pragma unroll
            for (int s = 0; s < KS; s += 4) {
                const float4 a = *reinterpret_cast<const float4*>(hrow + s);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wh[q][s], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wh[q][s + 1], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wh[q][s + 2], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wh[q][s + 3], acc[q], 0, 0, 0);
            }
            // ---- gate pointwise, all in this lane's registers (C/D map: row = 4*kq + r, col = j)
            float* hnext = hbuf + (cur ^ 1) * MT * S;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 4 * kq + r;
                const int n = n0 + e;
                const float gi = fast_sigmoid(acc[0][r]), gf = fast_sigmoid(acc[1][r]);
                const float gg = fast_tanh_fma(acc[2][r]), go = fast_sigmoid(acc[3][r]);
                const float cp = c_reg[r];
                const float c = gf * cp + gi * gg;
                const float h = go * fast_tanh_fma(c);
                const float kn = kbuf[(tt + 1) * MT + e];     // keep of step t+1 (1 past the end)
                if (n < N) {
                    const size_t row = (size_t)n * T + t;
                    y[row * H + u] = h;
                    if (stash) {
                        float* sp = stash + row * (6 * H);
                        sp[u] = gi; sp[H + u] = gf; sp[2 * H + u] = gg; sp[3 * H + u] = go;
                        sp[4 * H + u] = cp;
                        if (I > 6) sp[5 * H + u] = hin[r];   // h_prev: only the generic wgrad path (I > 6) reads it
                    }
                }
                h_last[r] = h;
                if (t == T - 1) c_reg[r] = c;                 // cn is the unmasked final cell state
                else c_reg[r] = c * kn;
                hin[r] = h * kn;
                hnext[e * S + hpos<H>(u)] = hin[r];
            }
            cur ^= 1;
            lds_barrier();
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = n0 + 4 * kq + r;
        if (n < N) {
            hn[(size_t)n * H + u] = h_last[r];
            cn[(size_t)n * H + u] = c_reg[r];
        }
    }
}

// ---------------------------------------------------------------------------- forward, split MFMA (fp16 / bf16 pieces)
// Same recurrence, but the h W_hh^T product runs on the 16-bit matrix pipe at f32 accuracy: W_hh and h_t are carried as
// P::NP pieces each and the piece products accumulate in f32 (common.h: SplitF16x3, SplitBf16x6).  h_t is split once by
// the lane that produces it and exchanged through NP piece planes in LDS.
//   fp16 split (default): two pieces, three products per K = 32 slab; main and cross products accumulate separately and
//     are combined once per step.  Half the matrix instructions of the bf16 split, the weight pieces take exactly the f32
//     weights' 128 VGPRs (no LDS slab) -- and a smaller error (tools/f16x3_probe.hip).  h is in (-1, 1) and the weights
//     are O(1), far inside fp16's range; values below its normal range lose relative, not absolute, accuracy (absolute
//     error <= 2^-36), which is what a dot product needs.
//   bf16 split: three pieces (a = a0 + a1 + a2, 8 significand bits each, so the split is exact) and the six piece
//     products a_i b_j with i + j <= 2.  The dropped products are below 2^-24 |a b|, i.e. under the rounding of the f32
//     accumulation itself: measured error equals the exact-f32 MFMA chain's (tools/bf16x6_probe.hip: 2.69e-7 vs 2.75e-7
//     on a K=128 dot product) at 2.6x its rate (6 x 16 cycles per K=32 slab against 8 x 32).  W_hh pieces take 192 VGPRs
//     at H=128, so part of them is parked in LDS (SplitBf16x6::fwd_park).
template <class P, int H>
struct FwdSplitGeom {
    static constexpr int NS = H / 32;          // K = 32 slabs over the hidden dimension
    static constexpr int RS = H + 8;           // 16-bit elements per padded row: 16 lanes x ds_read_b128 conflict-free
    static constexpr int PLANE = MT * RS;
    static constexpr int QL = P::fwd_park(H);                            // gates whose smallest weight piece is in LDS
    static constexpr int WPARK = QL * NS * 64 * 8;                       // 16-bit elements per wave
    static constexpr int TCX = 8;                                        // steps of x / keep staged per chunk
    static constexpr int XPT = (MT * TCX * 8 + H * 4 - 1) / (H * 4);     // staged x elements per thread
    static constexpr int HPL = 8 * RS;                                   // one piece plane of the (<= 8) head weight rows
    static constexpr size_t LDS = (2 * P::NP * PLANE + (H / 16) * WPARK + P::NP * HPL) * sizeof(unsigned short) +
                                  (2 * TCX * MT * 8 + 2 * TCX * MT + (H / 16) * 8 * 64 + 4 * H + 8) * sizeof(float);
};
// phase timing of the split forward (four marks per step) and the BPTT (seven), summed over the sequence by wave 0 and the
// last wave of workgroup 0 (phase_prof.h)
PROF_TABLE(g_x6_prof, [2][8], uav_x6_prof_read)

// Orientation: gates^T = W h^T, i.e. the WEIGHTS are the MFMA A operand (16 units of one gate) and h^T the B
// operand (16 envs), so a lane's four accumulator rows are four CONSECUTIVE units of ONE env: y and the five
// stash values leave as dwordx4 stores (6 per step instead of 24 dword stores -- the vector-memory issue rate,
// 16 cycles per wave-instruction, paced the step as much as the MFMAs did), h_t is parked with one ds_write_b64
// per piece, and keep is one value per lane.
template <class P, int H, bool FUSE_X>
__device__ __forceinline__ void lstm_fwd_split(
    const float* __restrict__ x, const float* __restrict__ keep, const float* __restrict__ h0,
    const float* __restrict__ c0, const float* __restrict__ w_ih, const float* __restrict__ w_hh,
    const float* __restrict__ b_ih, const float* __restrict__ b_hh, int N, int T, int I,
    float* __restrict__ y, float* __restrict__ hn, float* __restrict__ cn, float* __restrict__ stash,
    const float* __restrict__ w_head, const float* __restrict__ b_head, int NHD, float* __restrict__ heads) {
    using G = FwdSplitGeom<P, H>;
    using vec = typename P::vec;
    using piece = typename P::piece;
    constexpr int NP = P::NP, NS = G::NS, RS = G::RS, PLANE = G::PLANE, QL = G::QL, WPARK = G::WPARK, TC = G::TCX;
    constexpr int XPT = G::XPT, NT = H * 4, HPL = G::HPL, NW = H / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned short* hpl = reinterpret_cast<unsigned short*>(smem);       // [2][NP pieces][MT][RS]
    unsigned short* wpark = hpl + 2 * NP * PLANE;                        // [waves][QL][NS][64 lanes][8]
    float* xbuf = reinterpret_cast<float*>(wpark + (H / 16) * WPARK);    // [2][TC][MT][8]
    float* kbuf = xbuf + 2 * TC * MT * 8;                                // [2][TC][MT]: keep[t + 1] of the chunk's steps
    float* wxl = kbuf + 2 * TC * MT;                                     // [waves][4 gates][2 k-steps][64 lanes]
    float* bl = wxl + (H / 16) * 512;                                    // [4H] b_ih + b_hh | [8] head bias
    unsigned short* whp = reinterpret_cast<unsigned short*>(bl + 4 * H + 8);   // [NP pieces][8 heads][RS]

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int uw = 16 * w + j;                 // unit whose weight row this lane holds (A operand row)
    const int uo = 16 * w + 4 * kq;            // first of this lane's four output units; its env is j
    const int n0 = blockIdx.x * MT;
    const int n = min(n0 + j, N - 1);
    const bool live = n0 + j < N;

    // A fragments of 16x16x32: lane (j, kq) holds k = 32 s + 8 kq .. + 7 of unit uw, per gate q and piece p; the
    // smallest piece of the first QL gates lives in this wave's LDS slab instead (read back as lane-contiguous b128)
    vec wb[4][NS][NP];
    vec* const wpk = reinterpret_cast<vec*>(wpark + w * WPARK) + lane;  // + (q * NS + s) * 64
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float* src = w_hh + (size_t)(q * H + uw) * H + 32 * s + 8 * kq;
            const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 4);
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                piece p[NP];
                P::split(v[i], p);
#pragma unroll
                for (int pc = 0; pc < NP; ++pc) wb[q][s][pc][i] = p[pc];
            }
            if (q < QL) wpk[(q * NS + s) * 64] = wb[q][s][NP - 1];
        }
    float* const wxw = wxl + w * 512 + lane;                             // this lane's W_ih fragments: + (2 q + s) * 64
    if (FUSE_X) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k = 2 * kq + s;
                wxw[(2 * q + s) * 64] = (k < I) ? w_ih[(size_t)(q * H + uw) * I + k] : 0.f;
            }
        for (int idx = threadIdx.x; idx < 4 * H; idx += NT) bl[idx] = b_ih[idx] + b_hh[idx];
    }
    if (heads) {                                                         // actor / critic head rows as piece planes
        for (int idx = threadIdx.x; idx < 8 * H; idx += NT) {
            const int hdx = idx / H, uu = idx % H;
            piece p[NP];
            P::split((hdx < NHD) ? w_head[(size_t)hdx * H + uu] : 0.f, p);
            unsigned short* d = whp + hdx * RS + uu;
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) d[pc * HPL] = P::bits(p[pc]);
        }
        if (threadIdx.x < 8) bl[4 * H + threadIdx.x] = (int)threadIdx.x < NHD ? b_head[threadIdx.x] : 0.f;
    }
    // heads of the h held in plane set `buf` (= h_t, UNMASKED): D[head 4kq + r][env j] = W_head h^T + b, stored to
    // heads[env][t][NHD].  One wave does it, beside its own recurrent MFMAs of the next step; the loss then reads
    // NHD floats per sample instead of the H floats of y.
    auto emit_heads = [&](int buf, int t) {
        f32x4 ha = {0.f, 0.f, 0.f, 0.f}, hb = ha;
        const unsigned short* hrow = hpl + buf * NP * PLANE + j * RS + 8 * kq;
        const unsigned short* wrow = whp + (j & 7) * RS + 8 * kq;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            P::head_slab(ha, hb, [&](int pc) { return *reinterpret_cast<const vec*>(wrow + pc * HPL + 32 * s); },
                         [&](int pc) { return *reinterpret_cast<const vec*>(hrow + pc * PLANE + 32 * s); });
            asm volatile("" ::: "memory");               // one slab's fragments at a time
        }
        if (live && kq < 2) {
            float* dst = heads + ((size_t)n * T + t) * NHD;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * kq + r < NHD) dst[4 * kq + r] = P::sum(ha[r], hb[r]) + bl[4 * H + 4 * kq + r];
        }
    };
    auto put_h = [&](unsigned short* plane0, const float (&hv)[4]) {     // split and park h[env j][uo .. uo+3]
        unsigned short b[NP][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            piece p[NP];
            P::split(hv[r], p);
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) b[pc][r] = P::bits(p[pc]);
        }
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) {
            uint2 v;
            v.x = (unsigned)b[pc][0] | ((unsigned)b[pc][1] << 16);
            v.y = (unsigned)b[pc][2] | ((unsigned)b[pc][3] << 16);
            *reinterpret_cast<uint2*>(plane0 + pc * PLANE + j * RS + uo) = v;
        }
    };

    // chunk staging through registers: chunk c + 1 is loaded while chunk c runs, committed to the other buffer
    float xr[XPT], kr = 1.f;
    auto stage_load = [&](int t0) {
        if (FUSE_X) {
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                const int idx = threadIdx.x + i * NT;                    // (e, tt, f) with f fastest
                const int e = min(idx / (TC * 8), MT - 1), tt = (idx >> 3) % TC, f = idx & 7;
                const int ne = min(n0 + e, N - 1), t = min(t0 + tt, T - 1);
                xr[i] = (f < I) ? x[((size_t)ne * T + t) * I + f] : 0.f;
            }
        }
        if (threadIdx.x < TC * MT) {
            const int e = threadIdx.x / TC, tt = threadIdx.x % TC;
            const int ne = min(n0 + e, N - 1), t = t0 + tt + 1;
            kr = (keep && t < T) ? keep[(size_t)ne * T + t] : 1.f;
        }
    };
    auto stage_commit = [&](int buf) {
        if (FUSE_X) {
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                const int idx = threadIdx.x + i * NT;
                const int e = idx / (TC * 8), tt = (idx >> 3) % TC, f = idx & 7;
                if (e < MT) xbuf[((buf * TC + tt) * MT + e) * 8 + f] = xr[i];
            }
        }
        if (threadIdx.x < TC * MT) kbuf[(buf * TC + threadIdx.x % TC) * MT + threadIdx.x / TC] = kr;
    };

    float c_reg[4];
    {
        const float k0 = keep ? keep[(size_t)n * T] : 1.f;
        const float4 cv = *reinterpret_cast<const float4*>(c0 + (size_t)n * H + uo);
        const float4 hv4 = *reinterpret_cast<const float4*>(h0 + (size_t)n * H + uo);
        c_reg[0] = cv.x * k0; c_reg[1] = cv.y * k0; c_reg[2] = cv.z * k0; c_reg[3] = cv.w * k0;
        const float hv[4] = {hv4.x * k0, hv4.y * k0, hv4.z * k0, hv4.w * k0};
        put_h(hpl, hv);
        if (stash && I > 6 && live)                                      // h_prev of step 0 (generic wgrad path)
            *reinterpret_cast<float4*>(stash + ((size_t)n * T) * (6 * H) + 5 * H + uo) = float4{hv[0], hv[1], hv[2], hv[3]};
    }
    stage_load(0);
    stage_commit(0);
    int cur = 0;
    float kcur = 1.f;            // keep of the step about to run (the mask on the incoming h); h0 is masked above
    PROF_DECL(8);
    lds_barrier();

    const int nchunk = (T + TC - 1) / TC;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int t0 = ch * TC, tc = min(TC, T - t0), xb = ch & 1;
        if (ch + 1 < nchunk) stage_load(t0 + TC);
        for (int tt = 0; tt < tc; ++tt) {
            const int t = t0 + tt;
            const size_t row = (size_t)n * T + t;
            PROF_MARK(0);
            if (heads && w == NW - 1 && t > 0) emit_heads(cur, t - 1);   // heads of h_{t-1}, while no accumulator is live
            // the planes hold h_{t-1} UNMASKED (the heads need it so); the episode mask k_t is a per-env scalar, so it
            // is applied to the finished h-part of the accumulator: acc = k_t (W_hh h_{t-1}) + bias + W_ih x_t
            f32x4 acc[4], acl[4];                                         // the policy's two accumulators per gate
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = acl[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            const unsigned short* hrow = hpl + cur * NP * PLANE + j * RS + 8 * kq;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                vec a[NP];
#pragma unroll
                for (int pc = 0; pc < NP; ++pc) a[pc] = *reinterpret_cast<const vec*>(hrow + pc * PLANE + 32 * s);
                auto wf = [&](int q, int p) { return (p == NP - 1 && q < QL) ? wpk[(q * NS + s) * 64] : wb[q][s][p]; };
                P::gates_slab(acc, acl, wf, a);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = FUSE_X ? *reinterpret_cast<const float4*>(bl + q * H + uo)
                                        : *reinterpret_cast<const float4*>(stash + row * (6 * H) + q * H + uo);
                acc[q] = __builtin_elementwise_fma(P::sum(acc[q], acl[q]), f32x4{kcur, kcur, kcur, kcur}, f32x4{v.x, v.y, v.z, v.w});
            }
            if (FUSE_X) {       // K = I <= 8 input projection: two exact-f32 k-steps
                const float2 ax = *reinterpret_cast<const float2*>(&xbuf[((xb * TC + tt) * MT + j) * 8 + 2 * kq]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wxw[(2 * q) * 64], ax.x, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wxw[(2 * q + 1) * 64], ax.y, acc[q], 0, 0, 0);
                }
            }
            PROF_DEP(acc[0][0]); PROF_DEP(acc[1][1]); PROF_DEP(acc[2][2]); PROF_DEP(acc[3][3]);
            PROF_MARK(1);
            const float kn = kbuf[(xb * TC + tt) * MT + j];              // keep of step t+1 (1 past the end)
            // the stash stores are issued as soon as their values exist, so the write stream starts under the rest of
            // the gate math instead of in one burst before the barrier.
            // c = f c_prev + i g fuses one of its two products into an fma.  Which one was once left to the compiler, and the
            // choice (it changes the last bit of c, and so the whole sequence) followed unrelated code around it; it is spelled
            // out as the compiler had made it (forward: by H; backward: f c_prev), like every other fma of this file.
            float gi[4], gf[4], gg[4], go[4], cp[4], hh[4], hm[4], cc[4];
            float* sp = stash + row * (6 * H) + uo;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                gi[r] = fast_sigmoid(acc[0][r]); gf[r] = fast_sigmoid(acc[1][r]); gg[r] = fast_tanh_fma(acc[2][r]);
                cp[r] = c_reg[r];
                cc[r] = H >= 128 ? __builtin_fmaf(gi[r], gg[r], gf[r] * cp[r])
                                 : __builtin_fmaf(gf[r], cp[r], gi[r] * gg[r]);
            }
            if (live && stash) {
                *reinterpret_cast<float4*>(sp) = float4{gi[0], gi[1], gi[2], gi[3]};
                *reinterpret_cast<float4*>(sp + H) = float4{gf[0], gf[1], gf[2], gf[3]};
                *reinterpret_cast<float4*>(sp + 2 * H) = float4{gg[0], gg[1], gg[2], gg[3]};
                *reinterpret_cast<float4*>(sp + 4 * H) = float4{cp[0], cp[1], cp[2], cp[3]};
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                go[r] = fast_sigmoid(acc[3][r]);
                hh[r] = go[r] * fast_tanh_fma(cc[r]);
                hm[r] = hh[r] * kn;
                c_reg[r] = (t == T - 1) ? cc[r] : cc[r] * kn;            // cn is the unmasked final cell state
            }
            put_h(hpl + (cur ^ 1) * NP * PLANE, hh);
            kcur = kn;
            if (live) {
                *reinterpret_cast<float4*>(y + row * H + uo) = float4{hh[0], hh[1], hh[2], hh[3]};
                if (stash) {
                    *reinterpret_cast<float4*>(sp + 3 * H) = float4{go[0], go[1], go[2], go[3]};
                    if (I > 6 && t + 1 < T)                              // h_prev of step t+1 (generic wgrad path)
                        *reinterpret_cast<float4*>(sp + 6 * H + 5 * H) = float4{hm[0], hm[1], hm[2], hm[3]};
                }
                if (t == T - 1) {
                    *reinterpret_cast<float4*>(hn + (size_t)n * H + uo) = float4{hh[0], hh[1], hh[2], hh[3]};
                    *reinterpret_cast<float4*>(cn + (size_t)n * H + uo) = float4{c_reg[0], c_reg[1], c_reg[2], c_reg[3]};
                }
            }
            cur ^= 1;
            PROF_MARK(2);
            lds_barrier();
            PROF_MARK(3);
        }
        if (ch + 1 < nchunk) {
            stage_commit(xb ^ 1);
            lds_barrier();
        }
    }
    if (heads && w == NW - 1) emit_heads(cur, T - 1);                     // planes `cur` hold h_{T-1}
    PROF_FLUSH(g_x6_prof[w ? 1 : 0], 4, blockIdx.x == 0 && lane == 0 && (w == 0 || w == H / 16 - 1));
}

// the entry points, one per arithmetic: profiles and bench.py find the kernels by these names in a kernel trace
template <int H, bool FUSE_X>
__global__ __launch_bounds__(H * 4) void lstm_fwd_h3_kernel(
    const float* __restrict__ x, const float* __restrict__ keep, const float* __restrict__ h0,
    const float* __restrict__ c0, const float* __restrict__ w_ih, const float* __restrict__ w_hh,
    const float* __restrict__ b_ih, const float* __restrict__ b_hh, int N, int T, int I,
    float* __restrict__ y, float* __restrict__ hn, float* __restrict__ cn, float* __restrict__ stash,
    const float* __restrict__ w_head, const float* __restrict__ b_head, int NHD, float* __restrict__ heads) {
    lstm_fwd_split<SplitF16x3, H, FUSE_X>(x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, N, T, I, y, hn, cn, stash, w_head,
                                          b_head, NHD, heads);
}
template <int H, bool FUSE_X>
__global__ __launch_bounds__(H * 4) void lstm_fwd_x6_kernel(
    const float* __restrict__ x, const float* __restrict__ keep, const float* __restrict__ h0,
    const float* __restrict__ c0, const float* __restrict__ w_ih, const float* __restrict__ w_hh,
    const float* __restrict__ b_ih, const float* __restrict__ b_hh, int N, int T, int I,
    float* __restrict__ y, float* __restrict__ hn, float* __restrict__ cn, float* __restrict__ stash,
    const float* __restrict__ w_head, const float* __restrict__ b_head, int NHD, float* __restrict__ heads) {
    lstm_fwd_split<SplitBf16x6, H, FUSE_X>(x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, N, T, I, y, hn, cn, stash, w_head,
                                           b_head, NHD, heads);
}

// ---------------------------------------------------------------------------------------- backward
template <int H>
struct BwdGeom {
    static constexpr int S = 4 * H + 4;        // padded row of the dgates tile (conflict-free b128)
    static constexpr size_t LDS = (2 * MT * S + TC * MT * 8 + (TC + 1) * MT) * sizeof(float);
};

// dy source: either dy[N][T][H] or (dheads[N][T][NH], w_head[NH][H]) with dy = dheads . w_head
template <int H>
__global__ __launch_bounds__(H * 4) void lstm_bwd_kernel(
    const float* __restrict__ keep, const float* __restrict__ stash, const float* __restrict__ w_hh,
    const float* __restrict__ dy, const float* __restrict__ dheads, const float* __restrict__ w_head, int NH,
    const float* __restrict__ dhn, const float* __restrict__ dcn, int N, int T, float* __restrict__ dgates,
    float* __restrict__ dh0, float* __restrict__ dc0) {
    using G = BwdGeom<H>;
    constexpr int S = G::S;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* dgbuf = smem;                       // [2][MT][S]
    float* dhbuf = dgbuf + 2 * MT * S;         // [TC][MT][8]   staged dheads
    float* kbuf = dhbuf + TC * MT * 8;         // [TC+1][MT]    keep[t0 .. t0+tc]

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int u = 16 * w + j;
    const int n0 = blockIdx.x * MT;

    // W_hh^T slice: B[k][col j] = W_hh[k][u]; lane group kq covers gate kq's rows (k = kq*H + s)
    float wt[H];
#pragma unroll
    for (int s = 0; s < H; ++s) wt[s] = w_hh[(size_t)(kq * H + s) * H + u];
    // head weights as MFMA B-fragments (k = head index): dy = dheads . W_head is two MFMA k-steps whose
    // result lands in the accumulator layout the pointwise needs (row = env, col = unit)
    float whb[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) whb[a] = (dheads && 4 * a + kq < NH) ? w_head[(size_t)(4 * a + kq) * H + u] : 0.f;

    float dh_rec[4], dc_next[4];
    size_t srow[4];                            // stash row base of this lane's 4 env rows at t = 0
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = min(n0 + 4 * kq + r, N - 1);
        dh_rec[r] = dhn ? dhn[(size_t)n * H + u] : 0.f;
        dc_next[r] = dcn ? dcn[(size_t)n * H + u] : 0.f;
        srow[r] = (size_t)n * T;
    }
    // software prefetch: the stash values (and dy) of step t-1 are loaded while step t's MFMAs run,
    // so the HBM latency never sits between two steps of the recurrence
    float pf[4][5], pdy[4];
    auto prefetch = [&](int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* sp = stash + (srow[r] + t) * (6 * H);
            pf[r][0] = sp[u]; pf[r][1] = sp[H + u]; pf[r][2] = sp[2 * H + u]; pf[r][3] = sp[3 * H + u];
            pf[r][4] = sp[4 * H + u];
            pdy[r] = dy ? dy[(srow[r] + t) * H + u] : 0.f;
        }
    };
    prefetch(T - 1);
    int cur = 0;
    const int nchunk = (T + TC - 1) / TC;
    for (int ch = nchunk - 1; ch >= 0; --ch) {
        const int t0 = ch * TC, tc = min(TC, T - t0);
        if (dheads) {
            for (int idx = threadIdx.x; idx < MT * tc * 8; idx += blockDim.x) {
                const int e = idx / (tc * 8), rem = idx % (tc * 8), tt = rem >> 3, f = rem & 7;
                const int n = min(n0 + e, N - 1);
                dhbuf[(tt * MT + e) * 8 + f] = (f < NH) ? dheads[((size_t)n * T + t0 + tt) * NH + f] : 0.f;
            }
        }
        for (int idx = threadIdx.x; idx < MT * tc; idx += blockDim.x) {
            const int e = idx / tc, tt = idx % tc;
            const int n = min(n0 + e, N - 1);
            kbuf[tt * MT + e] = keep ? keep[(size_t)n * T + t0 + tt] : 1.f;
        }
        lds_barrier();
        for (int tt = tc - 1; tt >= 0; --tt) {
            const int t = t0 + tt;
            float* dgw = dgbuf + cur * MT * S;
            f32x4 dyacc = {0.f, 0.f, 0.f, 0.f};
            if (dheads) {
                const float* dr = &dhbuf[(tt * MT + j) * 8];       // A-fragment: dheads[env j][head kq / 4+kq]
                dyacc = __builtin_amdgcn_mfma_f32_16x16x4f32(dr[kq], whb[0], dyacc, 0, 0, 0);
                dyacc = __builtin_amdgcn_mfma_f32_16x16x4f32(dr[4 + kq], whb[1], dyacc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 4 * kq + r;
                const float gi = pf[r][0], gf = pf[r][1], gg = pf[r][2], go = pf[r][3], cp = pf[r][4];
                const float dyv = dheads ? dyacc[r] : pdy[r];
                const float dh = dyv + dh_rec[r];
                const float c = gf * cp + gi * gg;              // both products rounded, unlike the split kernels' c
                const float tch = fast_tanh_fma(c);
                const float dc = __builtin_fmaf(dh * go, __builtin_fmaf(-tch, tch, 1.0f), dc_next[r]);
                const float dgi = dc * gg * gi * (1.0f - gi);
                const float dgf = dc * cp * gf * (1.0f - gf);
                const float dgg = dc * gi * __builtin_fmaf(-gg, gg, 1.0f);
                const float dgo = dh * tch * go * (1.0f - go);
                const float kp = kbuf[tt * MT + e];            // keep[t]: the incoming state was masked by it
                dc_next[r] = dc * gf * kp;
                dgw[e * S + 0 * H + u] = dgi;
                dgw[e * S + 1 * H + u] = dgf;
                dgw[e * S + 2 * H + u] = dgg;
                dgw[e * S + 3 * H + u] = dgo;
                if (n0 + e < N) {
                    float* gp = dgates + (srow[r] + t) * (4 * H);
                    gp[u] = dgi; gp[H + u] = dgf; gp[2 * H + u] = dgg; gp[3 * H + u] = dgo;
                }
            }
            if (t > 0) prefetch(t - 1);
            lds_barrier();
            // dh_{t-1}[env][u] = sum_k dgates[env][k] W_hh[k][u]; four independent accumulators
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
            const float* drow = dgw + j * S + kq * H;
#pragma unroll
            for (int s = 0; s < H; s += 4) {
                const float4 a = *reinterpret_cast<const float4*>(drow + s);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wt[s], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wt[s + 1], a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wt[s + 2], a2, 0, 0, 0);
                a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wt[s + 3], a3, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float kp = kbuf[tt * MT + 4 * kq + r];
                dh_rec[r] = ((a0[r] + a1[r]) + (a2[r] + a3[r])) * kp;
            }
            cur ^= 1;
        }
        lds_barrier();     // kbuf / dhbuf are restaged by the next chunk
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = n0 + 4 * kq + r;
        if (n < N) {
            if (dh0) dh0[(size_t)n * H + u] = dh_rec[r];
            if (dc0) dc0[(size_t)n * H + u] = dc_next[r];
        }
    }
}

// ---------------------------------------------------------------- backward, split MFMA, K split over the waves
// dh_{t-1}^T = W_hh^T dG_t^T on the 16-bit matrix pipe at f32 accuracy (the split of the forward pass, P), weights as
// the A operand: lane (j, kq) owns env j and the four consecutive units uo..uo+3.
// Giving every wave 16 OUTPUT units and the whole K = 4H of dG (the first form built, on the bf16 split) makes each wave
// read all three piece planes of the step's gate gradients back from LDS (48 b128 fragments, 384 KB per step and CU -- as
// many cycles of LDS bandwidth as the MFMAs take) behind a barrier: 0.52 of 0.62 ms with HBM taken out of the picture.
// Here the K dimension is split instead: wave w multiplies ONLY the 64 gate gradients it produced itself
// (gates x its 16 units -- they already sit in the right lanes: the MFMA's k order is free, so lane (j, kq)
// supplies k = (gate, unit 16w + 4kq + r) of its own env j) against W_hh[those 64 rows][all H units], and writes
// H/16 partial 16 x 16 tiles (f32) to LDS; after ONE barrier each wave sums the NW partials of its own tile in a
// fixed order.  LDS traffic per step drops from 384 + 48 KB to 64 + 64 KB, the gate gradients never go to LDS,
// and the MFMAs start right after the pointwise without waiting for anybody.  The stash ring needs a single
// slot: the refill for step t-1 is issued at the TOP of step t, right after the slot is read, a full step ahead.
// Stash by LDS-DMA (global_load_lds: no VGPR destination): each wave gathers exactly what its own lanes read back, so
// the only ordering needed is the wave's own counted s_waitcnt vmcnt(k) = "everything but the k ops issued last has
// landed" (loads, stores and LDS-DMA retire in issue order; the DMA ops of a step are issued unconditionally).
template <class P, int H>
struct BwdSplitGeom {
    static constexpr int NW = H / 16;
    static constexpr int SLOT = 5 * MT * 16;                         // floats per wave in the stash ring (one slot)
    static constexpr int SMALL = 128;                                // floats per small slot: dheads[16][6] | keep[16]
    static constexpr int PK = P::bwd_park(H);                        // (tile, slab) items whose smallest weight piece is in LDS
    static constexpr int WPARK = PK * 64 * 8;                        // 16-bit elements per wave
    static constexpr size_t LDS = (NW * NW * 64 * 4 /*partials*/ + NW * SLOT + 2 * SMALL) * sizeof(float) +
                                  NW * WPARK * sizeof(unsigned short);
};

template <class P, int H, bool TILE = false>
__device__ __forceinline__ void lstm_bwd_split(
    const float* __restrict__ keep, const float* __restrict__ stash, const float* __restrict__ w_hh,
    const float* __restrict__ dheads, const float* __restrict__ w_head, int NH, const float* __restrict__ dhn,
    const float* __restrict__ dcn, int N, int T, float* __restrict__ dgates, float* __restrict__ dh0,
    float* __restrict__ dc0) {
    using G = BwdSplitGeom<P, H>;
    using vec = typename P::vec;
    using piece = typename P::piece;
    constexpr int NP = P::NP, SLOT = G::SLOT, NW = G::NW, SMALL = G::SMALL, PK = G::PK, WPARK = G::WPARK;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4* part = reinterpret_cast<f32x4*>(smem);                           // [tile m][wave w][64 lanes]
    float* ring = smem + NW * NW * 64 * 4;                                  // [NW][SLOT]
    float* small = ring + NW * SLOT;                                        // [2 slots][SMALL]
    unsigned short* wpark = reinterpret_cast<unsigned short*>(small + 2 * SMALL);   // [NW][PK][64 lanes][8]

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, kq = lane >> 4;
    const int uw = 16 * w + j;                 // A row of the dy product (head weights of unit uw)
    const int uo = 16 * w + 4 * kq;            // first of this lane's four units; its env is j
    const int n0 = blockIdx.x * MT;
    const int n = min(n0 + j, N - 1);
    const bool live = n0 + j < N;

    // A fragments: tile m (units 16m..16m+15), slab sb (gates 2sb, 2sb+1): lane (i = j, kq), element e holds
    // W_hh[(2sb + e/4) H + 16w + 4kq + e%4][16m + j] -- the k order of this wave's own gate gradients.  The smallest
    // piece of the first PK items (item = 2m + sb) lives in this wave's LDS slab instead.
    vec wa[NW][2][NP];
    vec* const wpk = reinterpret_cast<vec*>(wpark + w * WPARK) + lane;      // + item * 64
#pragma unroll
    for (int m = 0; m < NW; ++m)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = (2 * sb + e / 4) * H + 16 * w + 4 * kq + (e % 4);
                piece p[NP];
                P::split(w_hh[(size_t)k * H + 16 * m + j], p);
#pragma unroll
                for (int pc = 0; pc < NP; ++pc) wa[m][sb][pc][e] = p[pc];
            }
            if (2 * m + sb < PK) wpk[(2 * m + sb) * 64] = wa[m][sb][NP - 1];
        }
    float whb[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) whb[a] = (4 * a + kq < NH) ? w_head[(size_t)(4 * a + kq) * H + uw] : 0.f;

    float dh_rec[4], dc_next[4];
    {
        const float4 a4 = dhn ? *reinterpret_cast<const float4*>(dhn + (size_t)n * H + uo) : float4{0.f, 0.f, 0.f, 0.f};
        const float4 c4 = dcn ? *reinterpret_cast<const float4*>(dcn + (size_t)n * H + uo) : float4{0.f, 0.f, 0.f, 0.f};
        dh_rec[0] = a4.x; dh_rec[1] = a4.y; dh_rec[2] = a4.z; dh_rec[3] = a4.w;
        dc_next[0] = c4.x; dc_next[1] = c4.y; dc_next[2] = c4.z; dc_next[3] = c4.w;
    }
    // gate-gradient row of (env j, step t): n T + t as f32 rows [N][T][4H], or -- tile form (lstm_forms.h: DgTile) -- the 16 rows
    // of this workgroup's step adjacent, (tile T + t) 16 + j.  Only live lanes store, so the padded rows of a ragged last tile stay unwritten.
    const size_t dg_row0 = TILE ? (size_t)blockIdx.x * T * MT + j : (size_t)n * T;
    constexpr int DG_STEP = TILE ? MT : 1;

    // ---- LDS-DMA (inline asm; ordering: comment above BwdSplitGeom): stash gather [q][env lane/4][units 4 (lane%4) ..]
    typedef __attribute__((address_space(3))) float lds_f;
    const int e_d = lane >> 2, g4 = lane & 3;
    const size_t drow = (size_t)min(n0 + e_d, N - 1) * T;
    const unsigned ring_base = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)((lds_f*)(ring + w * SLOT)));
    const unsigned small_base = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)((lds_f*)small));
    auto issue = [&](int t) {
        const float* src = stash + (drow + t) * (6 * H) + 16 * w + 4 * g4;
        unsigned m0save;
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
            "s_add_u32 m0, m0, 1024\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
            "s_add_u32 m0, m0, 1024\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, off\n\t"
            "s_add_u32 m0, m0, 1024\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, off\n\t"
            "s_add_u32 m0, m0, 1024\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, off\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(m0save)
            : "v"(src), "v"(src + H), "v"(src + 2 * H), "v"(src + 3 * H), "v"(src + 4 * H), "s"(ring_base)
            : "memory", "scc");
    };
    // waves 0 / 1: one 256-B piece each of the step's small image  [dheads(16 envs x NH, env-major) | keep(16)].
    // The lane's element of step 0 and its per-step stride are fixed: only `+ t * stride` is left in the loop
    // (the division by NH used to run every step on the two waves everybody waits for).
    const float* small_at0;
    unsigned small_stride;
    {
        const int e = w * 64 + lane;
        if (e < 16 * NH) { small_at0 = dheads + (size_t)min(n0 + e / NH, N - 1) * T * NH + e % NH; small_stride = (unsigned)NH; }
        else if (e >= 112 && keep) { small_at0 = keep + (size_t)min(n0 + e - 112, N - 1) * T; small_stride = 1u; }
        else { small_at0 = w_hh + (lane & 15); small_stride = 0u; }         // padding: any readable dwords
    }
    auto issue_small = [&](int t, int slot) {
        const float* src = small_at0 + (size_t)((unsigned)t * small_stride);
        const unsigned dst = small_base + (unsigned)((slot * SMALL + w * 64) * 4);
        unsigned m0save;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(m0save) : "v"(src), "s"(dst) : "memory");
    };
    const bool small_wave = w < 2;
    // vector-memory operations of this wave, in issue order (all retire in order):
    //   prologue  ring(T-1) [small(T-1)] [small(T-2)]
    //   step t    wait . ring(t-1) . 4 dG stores . [small(t-2)]
    // so at the top of step t everything but the 4 stores (and one small piece) of step t+1 must have landed
    issue(T - 1);
    if (small_wave) {
        issue_small(T - 1, (T - 1) & 1);
        issue_small(T >= 2 ? T - 2 : 0, (T - 2) & 1);
    }
    bool first = true;
    PROF_DECL(8);
    for (int t = T - 1; t >= 0; --t) {
        PROF_MARK(0);
        if (first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (small_wave) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        first = false;
        const float* sl = ring + w * SLOT + j * 16 + 4 * kq;
        float4 pf[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) pf[q] = *reinterpret_cast<const float4*>(sl + q * 256);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the slot is in registers: refill it with step t-1
        issue(t >= 1 ? t - 1 : 0);
        PROF_MARK(1);
        lds_barrier();           // b2: the partials of step t+1 have been summed by everyone; small image of step t landed
        PROF_MARK(2);
        const float* sm = small + (t & 1) * SMALL;
        f32x4 dyacc = {0.f, 0.f, 0.f, 0.f};
        {
            const float d0 = (kq < NH) ? sm[j * NH + kq] : 0.f;
            const float d1 = (4 + kq < NH) ? sm[j * NH + 4 + kq] : 0.f;
            dyacc = __builtin_amdgcn_mfma_f32_16x16x4f32(whb[0], d0, dyacc, 0, 0, 0);
            dyacc = __builtin_amdgcn_mfma_f32_16x16x4f32(whb[1], d1, dyacc, 0, 0, 0);
        }
        const float kp = keep ? sm[112 + j] : 1.f;                           // keep[env j][t]
        const float gi[4] = {pf[0].x, pf[0].y, pf[0].z, pf[0].w}, gf[4] = {pf[1].x, pf[1].y, pf[1].z, pf[1].w};
        const float gg[4] = {pf[2].x, pf[2].y, pf[2].z, pf[2].w}, go[4] = {pf[3].x, pf[3].y, pf[3].z, pf[3].w};
        const float cp[4] = {pf[4].x, pf[4].y, pf[4].z, pf[4].w};
        float dg[4][4];                                                      // [gate][unit r]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dh = dyacc[r] + dh_rec[r];
            const float c = __builtin_fmaf(gf[r], cp[r], gi[r] * gg[r]);    // the fused product: comment at lstm_fwd_split
            const float tch = fast_tanh_fma(c);
            const float dc = __builtin_fmaf(dh * go[r], __builtin_fmaf(-tch, tch, 1.0f), dc_next[r]);
            dg[0][r] = dc * gg[r] * gi[r] * (1.0f - gi[r]);
            dg[1][r] = dc * cp[r] * gf[r] * (1.0f - gf[r]);
            dg[2][r] = dc * gi[r] * __builtin_fmaf(-gg[r], gg[r], 1.0f);
            dg[3][r] = dh * tch * go[r] * (1.0f - go[r]);
            dc_next[r] = dc * gf[r] * kp;
        }
        int ex = 0;                  // the gate gradients enter the products as dG 2^ex, the partial tiles leave times 2^-ex
        float unscale = 1.f;
        if constexpr (P::BLOCK_SCALE) {
            // Gate gradients span many binades, fp16 does not: each env's 64 values of this wave are scaled by a power of
            // two that puts their largest magnitude in [2^13, 2^14) (exact), and the env's column of the partial tiles --
            // it sits in these same lanes -- is scaled back.  max over the lane's 16 values, then over the four kq rows of
            // env j with the two gfx950 row-swap instructions.
            float mx = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, fabsf(dg[q][r]));
            {
                const unsigned u = __builtin_bit_cast(unsigned, mx);
                const auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
                mx = fmaxf(__builtin_bit_cast(float, (unsigned)s16[0]), __builtin_bit_cast(float, (unsigned)s16[1]));
                const unsigned v = __builtin_bit_cast(unsigned, mx);
                const auto s32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
                mx = fmaxf(__builtin_bit_cast(float, (unsigned)s32[0]), __builtin_bit_cast(float, (unsigned)s32[1]));
            }
            ex = 14 - __builtin_amdgcn_frexp_expf(mx);                      // mx = f 2^e, f in [0.5, 1)  ->  mx 2^ex in [2^13, 2^14)
            ex = mx > 0.f ? min(max(ex, -100), 100) : 0;
            unscale = __builtin_amdgcn_ldexpf(1.0f, -ex);
        }
        // the step's four dG stores, between the ring DMA and the small piece in the wave's issue order (the counted waits
        // above rely on that): ahead of the products, or behind them where they drain under the partial-sum reduce
        // instead of queueing in front of the products of the slowest wave, which everybody then waits for at b1
        auto store_dg = [&](int q) {
            if (live) *reinterpret_cast<float4*>(dgates + (dg_row0 + (size_t)t * DG_STEP) * (4 * H) + q * H + uo) = float4{dg[q][0], dg[q][1], dg[q][2], dg[q][3]};
        };
        // this wave's 64 gate gradients as B fragments: slab sb = gates 2sb, 2sb+1; element e = (gate 2sb + e/4, unit e%4)
        vec bp[2][NP];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                piece p[NP];
                P::split(P::BLOCK_SCALE ? __builtin_amdgcn_ldexpf(dg[q][r], ex) : dg[q][r], p);
#pragma unroll
                for (int pc = 0; pc < NP; ++pc) bp[q >> 1][pc][4 * (q & 1) + r] = p[pc];
            }
            if constexpr (!P::DG_STORES_LATE) store_dg(q);
        }
        PROF_DEP(bp[1][NP - 1]); PROF_DEP(bp[0][0]);
        PROF_MARK(3);
        // partial dh^T tiles: D_m[unit 16m + 4kq + r][env j] over this wave's K range
#pragma unroll
        for (int m = 0; m < NW; ++m) {
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
                const int item = 2 * m + sb;
                P::tile_slab(a0, a1, [&](int p) { return (p == NP - 1 && item < PK) ? wpk[item * 64] : wa[m][sb][p]; }, bp[sb]);
            }
            part[(m * NW + w) * 64 + lane] = P::tile_sum(a0, a1) * unscale;
        }
        if constexpr (P::DG_STORES_LATE) {
#pragma unroll
            for (int q = 0; q < 4; ++q) store_dg(q);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        PROF_MARK(4);
        lds_barrier();           // b1: all partials written; nobody reads the small image of step t any more
        PROF_MARK(5);
        if (small_wave) issue_small(t >= 2 ? t - 2 : 0, t & 1);
        f32x4 sum = part[(w * NW) * 64 + lane];
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) sum += part[(w * NW + ww) * 64 + lane];      // fixed order: deterministic
#pragma unroll
        for (int r = 0; r < 4; ++r) dh_rec[r] = sum[r] * kp;
        PROF_DEP(dh_rec[3]);
        PROF_MARK(6);
    }
    PROF_FLUSH(g_x6_prof[w ? 1 : 0], 8, blockIdx.x == 0 && lane == 0 && (w == 0 || w == H / 16 - 1));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // retire the clamped tail DMAs before the LDS is released
    if (live) {
        if (dh0) *reinterpret_cast<float4*>(dh0 + (size_t)n * H + uo) = float4{dh_rec[0], dh_rec[1], dh_rec[2], dh_rec[3]};
        if (dc0) *reinterpret_cast<float4*>(dc0 + (size_t)n * H + uo) = float4{dc_next[0], dc_next[1], dc_next[2], dc_next[3]};
    }
}

template <int H>
__global__ __launch_bounds__(H * 4) void lstm_bwd_h3k_kernel(
    const float* __restrict__ keep, const float* __restrict__ stash, const float* __restrict__ w_hh,
    const float* __restrict__ dheads, const float* __restrict__ w_head, int NH, const float* __restrict__ dhn,
    const float* __restrict__ dcn, int N, int T, float* __restrict__ dgates, float* __restrict__ dh0,
    float* __restrict__ dc0) {
    lstm_bwd_split<SplitF16x3, H>(keep, stash, w_hh, dheads, w_head, NH, dhn, dcn, N, T, dgates, dh0, dc0);
}
template <int H>
__global__ __launch_bounds__(H * 4) void lstm_bwd_x6k_kernel(
    const float* __restrict__ keep, const float* __restrict__ stash, const float* __restrict__ w_hh,
    const float* __restrict__ dheads, const float* __restrict__ w_head, int NH, const float* __restrict__ dhn,
    const float* __restrict__ dcn, int N, int T, float* __restrict__ dgates, float* __restrict__ dh0,
    float* __restrict__ dc0) {
    lstm_bwd_split<SplitBf16x6, H>(keep, stash, w_hh, dheads, w_head, NH, dhn, dcn, N, T, dgates, dh0, dc0);
}
// the same two kernels writing dgates in tile form (lstm_forms.h: DgTile); a kernel trace still finds them by the names above as prefixes
template <int H>
__global__ __launch_bounds__(H * 4) void lstm_bwd_h3k_kernel_tile(
    const float* __restrict__ keep, const float* __restrict__ stash, const float* __restrict__ w_hh,
    const float* __restrict__ dheads, const float* __restrict__ w_head, int NH, const float* __restrict__ dhn,
    const float* __restrict__ dcn, int N, int T, float* __restrict__ dgates, float* __restrict__ dh0,
    float* __restrict__ dc0) {
    lstm_bwd_split<SplitF16x3, H, true>(keep, stash, w_hh, dheads, w_head, NH, dhn, dcn, N, T, dgates, dh0, dc0);
}
template <int H>
__global__ __launch_bounds__(H * 4) void lstm_bwd_x6k_kernel_tile(
    const float* __restrict__ keep, const float* __restrict__ stash, const float* __restrict__ w_hh,
    const float* __restrict__ dheads, const float* __restrict__ w_head, int NH, const float* __restrict__ dhn,
    const float* __restrict__ dcn, int N, int T, float* __restrict__ dgates, float* __restrict__ dh0,
    float* __restrict__ dc0) {
    lstm_bwd_split<SplitBf16x6, H, true>(keep, stash, w_hh, dheads, w_head, NH, dhn, dcn, N, T, dgates, dh0, dc0);
}

// the entry points of arithmetic P
template <class P, int H, bool FUSE_X>
static constexpr auto fwd_split_kernel() {
    if constexpr (std::is_same<P, SplitF16x3>::value) return &lstm_fwd_h3_kernel<H, FUSE_X>;
    else return &lstm_fwd_x6_kernel<H, FUSE_X>;
}
template <class P, int H, bool TILE>
static constexpr auto bwd_split_kernel() {
    if constexpr (std::is_same<P, SplitF16x3>::value) return TILE ? &lstm_bwd_h3k_kernel_tile<H> : &lstm_bwd_h3k_kernel<H>;
    else return TILE ? &lstm_bwd_x6k_kernel_tile<H> : &lstm_bwd_x6k_kernel<H>;
}

// f(P{}) with the split policy of mode m
template <class F>
static int with_split(const uav_lstm_mode& m, F&& f) {
    return m.bf16x6() ? f(SplitBf16x6{}) : f(SplitF16x3{});
}

template <class P, int H>
static int launch_bwd_split(const float* keep, const float* stash, const float* w_hh, const float* dheads,
                            const float* w_head, int NH, const float* dhn, const float* dcn, int N, int T, float* dgates,
                            bool tile, float* dh0, float* dc0, hipStream_t st) {
    const dim3 grid((N + MT - 1) / MT), block(H * 4);
    const size_t lx = BwdSplitGeom<P, H>::LDS;
    const auto kern = tile ? bwd_split_kernel<P, H, true>() : bwd_split_kernel<P, H, false>();
    UAV_CHECK_HIP(uav_dyn_lds(reinterpret_cast<const void*>(kern), (int)lx));
    hipLaunchKernelGGL(kern, grid, block, lx, st, keep, stash, w_hh, dheads, w_head, NH, dhn, dcn, N, T, dgates, dh0, dc0);
    UAV_LAUNCH_CHECK();
    return 0;
}

template <class P, int H>
static int launch_fwd_split(bool fuse, const float* x, const float* keep, const float* h0, const float* c0,
                            const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int N, int T, int I,
                            float* y, float* hn, float* cn, float* stash, const float* w_head, const float* b_head, int NHD,
                            float* heads, hipStream_t st) {
    const dim3 grid((N + MT - 1) / MT), block(H * 4);
    const size_t lx = FwdSplitGeom<P, H>::LDS;
    constexpr auto fused = fwd_split_kernel<P, H, true>(), unfused = fwd_split_kernel<P, H, false>();
    UAV_CHECK_HIP(uav_dyn_lds(reinterpret_cast<const void*>(fused), (int)lx));
    UAV_CHECK_HIP(uav_dyn_lds(reinterpret_cast<const void*>(unfused), (int)lx));
    hipLaunchKernelGGL(fuse ? fused : unfused, grid, block, lx, st, x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, N, T, I, y, hn,
                       cn, stash, w_head, b_head, NHD, heads);
    UAV_LAUNCH_CHECK();
    return 0;
}

template <int H>
static int launch_fwd(const uav_lstm_mode& m, bool fuse, const float* x, const float* keep, const float* h0, const float* c0,
                      const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int N, int T, int I,
                      float* y, float* hn, float* cn, float* stash, const float* w_head, const float* b_head, int NHD,
                      float* heads, bool* heads_done, hipStream_t st) {
    if (!m.f32_mfma()) {                 // the matrix products as 16-bit piece products at f32 accuracy, heads fused
        *heads_done = heads != nullptr;
        return with_split(m, [&](auto p) {
            return launch_fwd_split<decltype(p), H>(fuse, x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, N, T, I, y, hn, cn, stash,
                                                    w_head, b_head, NHD, heads, st);
        });
    }
    const dim3 grid((N + MT - 1) / MT), block(H * 4);
    const size_t lds = FwdGeom<H>::LDS;
    if (fuse)
        hipLaunchKernelGGL((lstm_fwd_kernel<H, true>), grid, block, lds, st, x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, N,
                           T, I, y, hn, cn, stash);
    else
        hipLaunchKernelGGL((lstm_fwd_kernel<H, false>), grid, block, lds, st, x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh,
                           N, T, I, y, hn, cn, stash);
    UAV_LAUNCH_CHECK();
    return 0;
}

template <int H>
static int launch_bwd(const float* keep, const float* stash, const float* w_hh, const float* dy, const float* dheads,
                      const float* w_head, int NH, const float* dhn, const float* dcn, int N, int T, float* dgates,
                      float* dh0, float* dc0, hipStream_t st) {
    const dim3 grid((N + MT - 1) / MT), block(H * 4);
    UAV_CHECK_HIP(uav_dyn_lds(reinterpret_cast<const void*>(&lstm_bwd_kernel<H>), (int)BwdGeom<H>::LDS));
    hipLaunchKernelGGL((lstm_bwd_kernel<H>), grid, block, BwdGeom<H>::LDS, st, keep, stash, w_hh, dy, dheads, w_head, NH,
                       dhn, dcn, N, T, dgates, dh0, dc0);
    UAV_LAUNCH_CHECK();
    return 0;
}

static_assert(MT == DgTile::MT, "a tile of the gate-gradient tile form is one BPTT workgroup's envs");

// ---- what this file gives the entry points (lstm_api.hip, through internal.h)
int lstm_fwd_seq(const uav_lstm_mode& m, bool fuse, const float* x, const float* keep, const float* h0, const float* c0, const float* w_ih,
                 const float* w_hh, const float* b_ih, const float* b_hh, int N, int T, int I, int H, float* y, float* hn, float* cn,
                 float* stash, const float* w_head, const float* b_head, int NHD, float* heads, bool* heads_done, hipStream_t st) {
    return H == 64 ? launch_fwd<64>(m, fuse, x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, N, T, I, y, hn, cn, stash, w_head, b_head, NHD, heads, heads_done, st)
                   : launch_fwd<128>(m, fuse, x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, N, T, I, y, hn, cn, stash, w_head, b_head, NHD, heads, heads_done, st);
}

int lstm_bwd_seq(const uav_lstm_mode& m, const float* keep, const float* stash, const float* w_hh, const float* dy, const float* dheads,
                 const float* w_head, int NH, const float* dhn, const float* dcn, int N, int T, int H, float* dgates, bool tile, float* dh0,
                 float* dc0, hipStream_t st) {
    if (dheads && NH <= 7 && !m.f32_mfma()) {   // the PPO path: split MFMA, K split over waves
        return with_split(m, [&](auto p) {
            using P = decltype(p);
            return H == 64 ? launch_bwd_split<P, 64>(keep, stash, w_hh, dheads, w_head, NH, dhn, dcn, N, T, dgates, tile, dh0, dc0, st)
                           : launch_bwd_split<P, 128>(keep, stash, w_hh, dheads, w_head, NH, dhn, dcn, N, T, dgates, tile, dh0, dc0, st);
        });
    }
    // exact-f32 MFMA (UAV_ARITH_F32_MFMA), plain dy (stacked layers), more than 7 heads: f32 rows only
    if (tile) {
        uav_set_error("uav_lstm_bwd: this dgates buffer is armed for tile form (uav_lstm_dgates_tile), which only the split kernels "
                      "driven by dheads (at most 7 heads) write; uav_lstm_dgates_forget returns it to f32 rows");
        return 2;
    }
    switch (H) {
        case 64: return launch_bwd<64>(keep, stash, w_hh, dy, dheads, w_head, NH, dhn, dcn, N, T, dgates, dh0, dc0, st);
        case 128: return launch_bwd<128>(keep, stash, w_hh, dy, dheads, w_head, NH, dhn, dcn, N, T, dgates, dh0, dc0, st);
    }
    uav_set_error("uav_lstm_bwd: H=%d unsupported (64, 128)", H);
    return 2;
}
