// mlp_tile_core.h -- the reference's OWN policy (PPOV2.0/model.py:17-53: Linear(6,256) -> LayerNorm -> ReLU ->
// Linear(256,128) -> LayerNorm -> ReLU -> actor Linear(128,5) | critic Linear(128,1)) on LDS tiles: what the two persistent
// kernels that keep every activation on chip -- rollout_mlp_kernel (mlp_rollout.hip) and mlp_ppo_grad_kernel (mlp_update.hip) --
// both run.  They run the same forward code in the same order: the rollout's log-probabilities are bit-identical to the
// update's first forward pass.
//
// Arithmetic: exact f32 (v_mfma_f32_16x16x4_f32 = a k-ordered fmaf chain), the reference's dtype; products are laid out
// "units on rows, samples on columns" (weights are the A operand), so the accumulator of a lane holds 4 consecutive units
// of ONE sample and LayerNorm's per-sample reductions are a 4-lane shuffle + one LDS exchange between the 8 waves.
//
// Input width: 6 (the reference's network), or 7 / 8 when the trend channels obs[6 + i] are inputs too (uav_rollout policy_kind 2,
// uav_mlp_ppo_grad_trend).  Layer 1 is a K = 8 product at every width (two MFMA k-steps, X rows of 8 floats): only the W1 row
// stride, the offsets behind W1, the observation copies and the place of db1 in the update depend on the width (MlpOff, INW).
#pragma once
#include "common.h"

namespace {

constexpr int MT = 16;                  // samples (environments) per tile = one MFMA column tile
constexpr int IN = 6, H1 = 256, H2 = 128, NA = 5, NH = 6;
constexpr int NWAVE = 8;
constexpr int AS1 = 260, AS2 = 132;     // row strides (floats) of the a1 / a2 tiles: float4-aligned rows
constexpr int RS1 = H1 + 8;             // row stride (halves) of the a1 piece planes: conflict-free ds_read_b128
constexpr float LN_EPS_F = 1e-5f;

// flat parameter layout of csrc/mlp.hip for `in` input features: W1[256][in] b1 g1 be1 W2 b2 g2 be2 Wh bh.  in = 6 is the
// reference's network; 7 and 8 carry the trend channels (obs[6 + i], uav_env_cfg::trend_k).  Every offset behind W1 moves
// with `in`; W2 stays 16-byte aligned at all three widths (256 in + 768 floats).
struct MlpOff {
    int W1, B1, G1, BE1, W2, B2, G2, BE2, WH, BH, N;
    __host__ __device__ constexpr explicit MlpOff(int in)
        : W1(0), B1(H1 * in), G1(B1 + H1), BE1(G1 + H1), W2(BE1 + H1), B2(W2 + H2 * H1), G2(B2 + H2), BE2(G2 + H2),
          WH(BE2 + H2), BH(WH + NH * H2), N(BH + NH) {}
};
static_assert(MlpOff(IN).N == 36230, "MLP parameter count (SURVEY 8a M1)");
static_assert(MlpOff(7).W2 % 4 == 0 && MlpOff(8).W2 % 4 == 0, "W2 rows are read as float4");
constexpr int IN_MAX = 8;               // the observation tile X and the W1 image are [.][8]
// Input width of a kernel instantiation: INW = 6 is the reference's network with every offset a compile-time constant (the
// kernels as they were); INW = 0 is ONE instantiation for 7 and 8 inputs with the width read at run time, as rollout.hip's
// TREND form.

// LDS regions common to both kernels (floats).  NC = column tiles (of 16 samples) a workgroup advances together: 1 in the
// rollout (16 environments per workgroup keep all 256 CUs busy at 4096 environments), 2 in the update (every weight
// fragment fetched from L2 then feeds two MFMAs, and the per-tile latencies -- barriers, the loss lanes -- are shared by 32
// samples).
template <int NC>
struct Tiles {
    static constexpr int MS = MT * NC;
    float* prm;      // b1 g1 be1 [256 each] | b2 g2 be2 [128 each]
    float* X;        // [MS][8]   observations of the tile, columns from the input width on zero
    float* A1;       // [MS][AS1] a1 = relu(LN1(z1)); later dz1
    float* A2;       // [MS][AS2] a2 = relu(LN2(z2)); later dz2
    double* red;     // [2][8 waves][MS] per-wave partial sums of the LayerNorm reductions
    f32x4* HP;       // [8 waves][NC][32] partial head tiles (K split over the waves; rows 0..7 = lanes with kq < 2)
    float* HD;       // [MS][8]   heads: logits | value
    unsigned short* P1;   // [2 pieces][MS][RS1] a1 as two fp16 planes (the B operand of the split layer-2 product)
    static constexpr int FLOATS = 3 * H1 + 3 * H2 + MS * 8 + MS * AS1 + MS * AS2 + 2 * (2 * NWAVE * MS) + NWAVE * NC * 32 * 4 + MS * 8 + MS * RS1;
    __device__ __forceinline__ explicit Tiles(float* base) {
        prm = base;
        X = prm + 3 * H1 + 3 * H2;
        A1 = X + MS * 8;
        A2 = A1 + MS * AS1;
        red = reinterpret_cast<double*>(A2 + MS * AS2);
        HP = reinterpret_cast<f32x4*>(red + 2 * NWAVE * MS);
        HD = reinterpret_cast<float*>(HP + NWAVE * NC * 32);
        P1 = reinterpret_cast<unsigned short*>(HD + MS * 8);
    }
};

__device__ __forceinline__ f32x4 ld4(const float* p) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    return f32x4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<float4*>(p) = float4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---------------------------------------------------------------------------------------------------- lane reductions
// sum over the 16 lanes of a row (the 16 samples lane & 15 = 0..15 that share lane >> 4): four DPP adds -- xor 1, xor 2,
// half-row mirror, row mirror -- every lane ends with the same total (a + b == b + a bitwise at every stage)
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));   // row_mirror
    return v;
}
__device__ __forceinline__ f32x4 row16_sum(f32x4 v) { return f32x4{row16_sum(v[0]), row16_sum(v[1]), row16_sum(v[2]), row16_sum(v[3])}; }

// max over the four lanes that hold the same sample (lane & 15) of a wave -- equally: over the wave, of a value every row of 16
// has already agreed on -- with the two gfx950 row swaps (quad_sum below); every lane gets the result
__device__ __forceinline__ float quad_max(float v) {
    const auto s16 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    v = fmaxf(__builtin_bit_cast(float, (unsigned)s16[0]), __builtin_bit_cast(float, (unsigned)s16[1]));
    const auto s32 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    return fmaxf(__builtin_bit_cast(float, (unsigned)s32[0]), __builtin_bit_cast(float, (unsigned)s32[1]));
}
// max over all 64 lanes of a wave (DPP within the rows of 16, then the two row swaps); every lane gets the result
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true)));
    return quad_max(v);
}

// sum over the four lanes that hold the same sample (lane & 15) of a wave
// (the two gfx950 row-swap instructions instead of ds_bpermute: v_permlane16_swap / v_permlane32_swap hand every lane its
//  xor-16 / xor-32 partner's dword without touching LDS; a + b == b + a bitwise, so the four lanes agree)
__device__ __forceinline__ float quad_sum(float v) {
    {
        const auto s = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
        v = __builtin_bit_cast(float, (unsigned)s[0]) + __builtin_bit_cast(float, (unsigned)s[1]);
    }
    {
        const auto s = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
        v = __builtin_bit_cast(float, (unsigned)s[0]) + __builtin_bit_cast(float, (unsigned)s[1]);
    }
    return v;
}
__device__ __forceinline__ double quad_sum(double v) {
    {
        const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
        const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
        const double x = __builtin_bit_cast(double, (unsigned long long)(unsigned)lo[0] | ((unsigned long long)(unsigned)hi[0] << 32));
        const double y = __builtin_bit_cast(double, (unsigned long long)(unsigned)lo[1] | ((unsigned long long)(unsigned)hi[1] << 32));
        v = x + y;
    }
    {
        const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
        const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
        const double x = __builtin_bit_cast(double, (unsigned long long)(unsigned)lo[0] | ((unsigned long long)(unsigned)hi[0] << 32));
        const double y = __builtin_bit_cast(double, (unsigned long long)(unsigned)lo[1] | ((unsigned long long)(unsigned)hi[1] << 32));
        v = x + y;
    }
    return v;
}

// One LayerNorm reduction round: every wave leaves (a, b) for its sample columns, then every lane reads the 8 partial
// pairs of ITS samples in a fixed order.  One barrier inside; the caller syncs before `red` is written again.
// T = double for the forward statistics (no cancellation at f32 data precision); T = float for the LayerNorm BACKWARD sums
// (mean of dxhat, mean of dxhat * xhat): they enter the result linearly, so there is no cancellation to protect and the
// reference's own backward accumulates them in f32.
template <int NC, class T>
__device__ __forceinline__ void ln_exchange(const Tiles<NC>& L, int w, int j, int kq, const T (&a)[NC], const T (&b)[NC], T (&A)[NC], T (&B)[NC]) {
    constexpr int MS = MT * NC;
    T* red = reinterpret_cast<T*>(L.red);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const T ta = quad_sum(a[c]), tb = quad_sum(b[c]);
        if (kq == 0) {
            red[w * MS + 16 * c + j] = ta;
            red[(NWAVE + w) * MS + 16 * c + j] = tb;
        }
    }
    lds_barrier();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        A[c] = T(0);
        B[c] = T(0);
#pragma unroll
        for (int i = 0; i < NWAVE; ++i) {
            A[c] += red[i * MS + 16 * c + j];
            B[c] += red[(NWAVE + i) * MS + 16 * c + j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- fp16 pieces
// Transposed LDS read (gfx950 ds_read_b64_tr_b16): an MFMA 16x16x32 fragment -- 8 consecutive K per lane -- from a plane
// stored [K rows][16+ columns of halves] with row stride `rs` halves: lane (i = lane & 15, kq) gets rows 8 kq .. 8 kq + 7 of
// column i.  Lane 4 q + p of a 16-lane group supplies the address of row q, columns 4 p .. 4 p + 3 of each 4-row block.
// EXEC must be all ones (the gather crosses lanes): only called from uniform code.
__device__ __forceinline__ f16x8 tr_frag(const unsigned short* plane, int rs, int lane) {
    typedef short v4s __attribute__((__vector_size__(4 * sizeof(short))));
    typedef __attribute__((address_space(3))) v4s lds_v4s;
    const int li = lane & 15, kq = lane >> 4;
    const unsigned short* a = plane + (8 * kq + (li >> 2)) * rs + 4 * (li & 3);
    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)a);
    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(a + 4 * rs));
    typedef short v8s __attribute__((__vector_size__(8 * sizeof(short))));
    const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(f16x8, r);
}

// Four consecutive values of one row as two fp16 pieces, one uint2 store per piece plane: `at` = the values' place in plane 0,
// plane 1 lies `plane` halves behind it.  SCALED = common.h's split2h (the residual times 2^11, back in fp16's normal range:
// the operand of a main + cross accumulator pair); !SCALED = the plain residual fp16(x - fp16(x)) of the update's dW2 product,
// which has ONE accumulator and folds the 2^-11 into the other operand instead.  The two round differently for residuals
// below fp16's normal range, so both forms stay.
template <bool SCALED>
__device__ __forceinline__ void st_pieces4(unsigned short* at, int plane, const f32x4& x) {
    unsigned short b[2][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        _Float16 p0, p1;
        if (SCALED) split2h(x[r], p0, p1);
        else {
            p0 = (_Float16)x[r];
            p1 = (_Float16)(x[r] - (float)p0);
        }
        b[0][r] = h_bits(p0); b[1][r] = h_bits(p1);
    }
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
        uint2 v;
        v.x = (unsigned)b[pc][0] | ((unsigned)b[pc][1] << 16);
        v.y = (unsigned)b[pc][2] | ((unsigned)b[pc][3] << 16);
        *reinterpret_cast<uint2*>(at + pc * plane) = v;
    }
}

// The power of two 2^e that puts the magnitude m into [2^13, 2^14), e clamped to +-100; `none` for m = 0, inf or NaN
__device__ __forceinline__ int pow2_to_2e13(float m, int none) {
    int e = none;
    if (m > 0.f && m < 3.0e38f) {
        e = 13 - (int)((__float_as_uint(m) >> 23) & 0xff) + 127;
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
    }
    return e;
}

// ---------------------------------------------------------------------------------------------------- forward
// the LayerNorm / bias vectors b1 g1 be1 | b2 g2 be2 into L.prm, by all 512 threads (the caller's barrier publishes them)
template <int NC>
__device__ __forceinline__ void stage_prm(const Tiles<NC>& L, const float* __restrict__ params, const MlpOff& O) {
    for (int i = threadIdx.x; i < H1; i += 512) {
        L.prm[i] = params[O.B1 + i];
        L.prm[H1 + i] = params[O.G1 + i];
        L.prm[2 * H1 + i] = params[O.BE1 + i];
    }
    for (int i = threadIdx.x; i < H2; i += 512) {
        L.prm[3 * H1 + i] = params[O.B2 + i];
        L.prm[3 * H1 + H2 + i] = params[O.G2 + i];
        L.prm[3 * H1 + 2 * H2 + i] = params[O.BE2 + i];
    }
}

// z1 -> LN1 -> a1 (to LDS).  Lane (j = lane & 15, kq = lane >> 4) of wave w holds units 32 w + 16 t + 4 kq + r, t < 2,
// r < 4 of samples 16 c + j.  Leaves xhat1 / rstd1 for the backward.  One barrier inside (ln_exchange); the caller's
// barrier after it publishes a1: as f32 rows (A1), or with PIECES as two fp16 piece planes (P1).
template <int NC, bool PIECES>
__device__ __forceinline__ void layer1(const Tiles<NC>& L, const float (&w1a)[2][2], int w, int j, int kq, f32x4 (&xh)[NC][2],
                                       float (&rstd)[NC]) {
    f32x4 z[NC][2];
    double s[NC], q[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float xb0 = L.X[(16 * c + j) * 8 + kq], xb1 = L.X[(16 * c + j) * 8 + 4 + kq];
        s[c] = 0.0;
        q[c] = 0.0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int u = 32 * w + 16 * t + 4 * kq;
            f32x4 acc = ld4(L.prm + u);                      // b1
            acc = mfma4(w1a[t][0], xb0, acc);
            acc = mfma4(w1a[t][1], xb1, acc);
            z[c][t] = acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[c] += (double)acc[r];
                q[c] += (double)acc[r] * (double)acc[r];
            }
        }
    }
    double S[NC], Q[NC];
    ln_exchange<NC>(L, w, j, kq, s, q, S, Q);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double mean = S[c] * (1.0 / H1);
        double var = Q[c] * (1.0 / H1) - mean * mean;        // f64: no cancellation at f32 data precision
        var = var > 0.0 ? var : 0.0;
        const float mf = (float)mean;
        rstd[c] = 1.0f / sqrtf((float)var + LN_EPS_F);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int u = 32 * w + 16 * t + 4 * kq;
            const f32x4 g = ld4(L.prm + H1 + u), be = ld4(L.prm + 2 * H1 + u);
            f32x4 a;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xh[c][t][r] = (z[c][t][r] - mf) * rstd[c];
                const float pre = xh[c][t][r] * g[r] + be[r];
                a[r] = pre < 0.f ? 0.f : pre;                // NaN propagates like torch.relu
            }
            if (PIECES) st_pieces4<true>(L.P1 + (16 * c + j) * RS1 + u, MT * NC * RS1, a);
            else st4(L.A1 + (16 * c + j) * AS1 + u, a);
        }
    }
}

// The tail of layer 2 in either arithmetic: LN2 statistics of z2 = acc, a2 = relu(LN2(z2)) to LDS, xhat2 / rstd2 for the backward
template <int NC>
__device__ __forceinline__ void layer2_ln_relu(const Tiles<NC>& L, const f32x4 (&acc)[NC], int w, int j, int kq, f32x4 (&xh)[NC],
                                               float (&rstd)[NC]) {
    const int u = 16 * w + 4 * kq;
    double s1[NC], q1[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        s1[c] = 0.0;
        q1[c] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s1[c] += (double)acc[c][r];
            q1[c] += (double)acc[c][r] * (double)acc[c][r];
        }
    }
    double S[NC], Q[NC];
    ln_exchange<NC>(L, w, j, kq, s1, q1, S, Q);
    const f32x4 g = ld4(L.prm + 3 * H1 + H2 + u), be = ld4(L.prm + 3 * H1 + 2 * H2 + u);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double mean = S[c] * (1.0 / H2);
        double var = Q[c] * (1.0 / H2) - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const float mf = (float)mean;
        rstd[c] = 1.0f / sqrtf((float)var + LN_EPS_F);
        f32x4 a;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xh[c][r] = (acc[c][r] - mf) * rstd[c];
            const float pre = xh[c][r] * g[r] + be[r];
            a[r] = pre < 0.f ? 0.f : pre;
        }
        st4(L.A2 + (16 * c + j) * AS2 + u, a);
    }
}

// z2 -> LN2 -> a2 (to LDS).  Lane holds units 16 w + 4 kq + r of samples 16 c + j.  The K = 256 sum runs in 16 slabs of 16:
// in slab s the lane group kq multiplies k = 16 s + 4 kq + i, i < 4 -- a permutation of the MFMA's natural k order (any
// order is a valid dot product as long as A and B agree) that makes BOTH operands four consecutive floats per lane:
// wa4(s) = W2[16 w + (lane & 15)][16 s + 4 kq .. + 3] is ONE dwordx4 load (registers, LDS or L2), the a1 fragment one
// ds_read_b128.
template <int NC, class WA>
__device__ __forceinline__ void layer2(const Tiles<NC>& L, WA&& wa4, int w, int j, int kq, f32x4 (&xh)[NC], float (&rstd)[NC]) {
    const int u = 16 * w + 4 * kq;
    f32x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = ld4(L.prm + 3 * H1 + u);       // b2
    const float* brow = L.A1 + j * AS1 + 4 * kq;
    // four slabs of weights in flight ahead of the MFMAs that use them (L2 latency), never all sixteen (registers)
    f32x4 wq[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wq[0][i] = wa4(i);
#pragma unroll
    for (int ch = 0; ch < H1 / 64; ++ch) {
        if (ch + 1 < H1 / 64) {
#pragma unroll
            for (int i = 0; i < 4; ++i) wq[(ch + 1) & 1][i] = wa4(4 * (ch + 1) + i);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 a = wq[ch & 1][i];
            f32x4 b[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) b[c] = ld4(brow + 16 * c * AS1 + 16 * (4 * ch + i));
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c] = mfma4(a[k], b[c][k], acc[c]);
        }
        asm volatile("" ::: "memory");
    }
    layer2_ln_relu<NC>(L, acc, w, j, kq, xh, rstd);
}

// The same layer on the fp16 matrix pipe at f32 accuracy (common.h split2h: two fp16 pieces per operand, three products per
// K = 32 slab into a main and a cross accumulator): 8 slabs x 3 x 16 cycles instead of 64 k-steps x 32.  wa8(s, piece) =
// the A fragment W2[16 w + (lane & 15)][32 s + 8 kq .. + 7] as fp16 piece `piece`; B fragments from the a1 piece planes.
// Operand ranges: |W2| < 65504 and a1 <= sqrt(255) |g1| + |be1| < 65504, i.e. max |param| < 2048 (the caller's guard).
template <int NC, class WA>
__device__ __forceinline__ void layer2_h3(const Tiles<NC>& L, WA&& wa8, int w, int j, int kq, f32x4 (&xh)[NC], float (&rstd)[NC]) {
    constexpr int MS = MT * NC;
    const int u = 16 * w + 4 * kq;
    f32x4 acc[NC], acl[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        acc[c] = ld4(L.prm + 3 * H1 + u);                    // b2
        acl[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const unsigned short* brow = L.P1 + j * RS1 + 8 * kq;
    // two slabs of weight fragments in flight ahead of the MFMAs that use them (L2 latency in the update kernel)
    f16x8 wq[2][2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { wq[0][i][0] = wa8(i, 0); wq[0][i][1] = wa8(i, 1); }
#pragma unroll
    for (int ch = 0; ch < H1 / 64; ++ch) {
        if (ch + 1 < H1 / 64) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { wq[(ch + 1) & 1][i][0] = wa8(2 * (ch + 1) + i, 0); wq[(ch + 1) & 1][i][1] = wa8(2 * (ch + 1) + i, 1); }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int s = 2 * ch + i;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const f16x8 b0 = *reinterpret_cast<const f16x8*>(brow + (16 * c) * RS1 + 32 * s);
                const f16x8 b1 = *reinterpret_cast<const f16x8*>(brow + (MS + 16 * c) * RS1 + 32 * s);
                acl[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[ch & 1][i][1], b0, acl[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[ch & 1][i][0], b0, acc[c], 0, 0, 0);
                acl[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[ch & 1][i][0], b1, acl[c], 0, 0, 0);
            }
        }
        asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = acc[c] + acl[c] * H3_LO;
    layer2_ln_relu<NC>(L, acc, w, j, kq, xh, rstd);
}

// heads = Wh a2 + bh with K = 128 split over the 8 waves (16 each); wave 0 adds the partial tiles in a fixed order and
// leaves heads[sample][0..5] in HD.  wh[s] = Wh[lane & 15][16 w + 4 s + kq] (0 for rows >= 6).  Barrier inside.
template <int NC>
__device__ __forceinline__ void heads_fwd(const Tiles<NC>& L, const float (&wh)[4], const float* __restrict__ bh, int w, int lane) {
    const int j = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        f32x4 hp = {0.f, 0.f, 0.f, 0.f};
        const float* brow = L.A2 + (16 * c + j) * AS2 + 16 * w + kq;
#pragma unroll
        for (int s = 0; s < 4; ++s) hp = mfma4(wh[s], brow[4 * s], hp);
        if (kq < 2) L.HP[(w * NC + c) * 32 + lane] = hp;
    }
    lds_barrier();
    if (w == 0 && kq < 2) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            f32x4 t = L.HP[c * 32 + lane];
#pragma unroll
            for (int i = 1; i < NWAVE; ++i) t = t + L.HP[(i * NC + c) * 32 + lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int hd = 4 * kq + r;
                L.HD[(16 * c + j) * 8 + hd] = t[r] + (hd < NH ? bh[hd] : 0.f);
            }
        }
    }
}

}  // namespace
