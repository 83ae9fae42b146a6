// mlp_update.hip -- U1-U3 up to the gradient for the reference's OWN policy, the MLP of mlp_tile_core.h (train_ppo2.0.py:55-86):
// mlp_ppo_grad_kernel is a persistent kernel that runs forward, clipped-PPO loss and backward through the whole network for
// tiles of 32 samples; LayerNorm statistics, activations and their gradients never leave the CU, weight gradients accumulate
// in registers over all of a workgroup's tiles and leave as one slab per workgroup.  HBM traffic = the 44 algorithmic bytes
// per sample.  The forward is mlp_tile_core.h's, shared with the rollout (mlp_rollout.hip).  The tile loop's ten
// phases (PROF_MARK 0 .. 9, the names tools/perf_mlp_fused.py prints) stay written out in the kernel body: at 256 VGPRs
// every phase tried as a function of its own -- and the LDS pointers gathered in a struct -- raised the scratch of some of
// the 16 forms (profiles/mlp_split_static_table.md).
#include <type_traits>

#include "internal.h"
#include "loss_core.h"
#include "mlp_tile_core.h"
#include "phase_prof.h"

// phase timing: cycles per phase summed over the tiles of workgroup 0, waves 0 (loss wave) and 1 (phase_prof.h)
PROF_TABLE(g_mlp_prof, [2][16], uav_mlp_prof_read)

namespace {

constexpr int RS2 = H2 + 8;             // row stride (halves) of the dz2 piece planes

// LDS of the update kernel: the tiles + the per-unit accumulators of the LayerNorm / bias gradients
//   ACC1 [2][256] (dg1, dbe1)   ACC2 [3][128] (dg2, dbe2, db2)   DH [MS][8] dheads
// (each tile's contribution is summed over its 16 sample lanes by row16_sum first; db1 rides on the dW1 product as a
//  ones column of X.  Round 2 kept one slot per (sample lane, unit): 74 KB of LDS and 18 LDS read-modify-writes per tile.)
constexpr int UNC = 2;                  // column tiles per workgroup step: 32 samples
constexpr int UMS = MT * UNC;
constexpr int LS_STRIDE = 10;             // doubles per loss lane: policy / value / entropy / NaN sums + 6 head-bias sums
// + (H3) P2 [2 pieces][MS][RS2] dz2 as scaled fp16 planes, MX [8 waves][MS] per-sample maxima for their scale
constexpr int UPD_FLOATS = Tiles<UNC>::FLOATS + 2 * H1 + 3 * H2 + UMS * 8 + 2 * UMS * LS_STRIDE + H1 * 8 + 8 * H2 + UMS * RS2 + NWAVE * UMS + UMS * RS2;
constexpr size_t UPD_LDS = (size_t)UPD_FLOATS * sizeof(float);
// DIAG (uav_set_ppo_diag): + DLS [MS][UAV_PPO_DIAG_N] doubles, the loss lanes' running diagnostic sums, behind everything else
constexpr size_t UPD_LDS_DIAG = UPD_LDS + (size_t)UMS * UAV_PPO_DIAG_N * sizeof(double);
// BC (uav_mlp_bc_grad): + BLS [MS][2] doubles, the loss lanes' agreement and sample counts, in the same place (there is no BC + DIAG form)
constexpr size_t UPD_LDS_BC = UPD_LDS + (size_t)UMS * 2 * sizeof(double);
static_assert(UAV_BC_SUMS_N == 6 && UAV_BC_SUMS_N + NH <= LOSS_PSTRIDE, "mlp_ppo_grad_kernel<BC>: 4 sums in LS + 2 in BLS + the head-bias sums per partial");
static_assert(UPD_LDS % sizeof(double) == 0 && UPD_LDS_DIAG <= 160 * 1024, "mlp_ppo_grad_kernel: LDS over 160 KB per workgroup");
// one gradient slab per workgroup, flat parameter layout: MlpOff(in).N floats

// H3: the two K = 256 / K = 128 products (layer 2 forward, da1 = W2^T dz2) on the fp16 matrix pipe at f32 accuracy; `w2t`
// is then the pre-split weights in MFMA fragment order (mlp_w2_pieces_kernel) instead of the f32 transpose.  dW2 (K = the
// tile's 32 samples) stays on exact-f32 MFMA: its operands would need a second, transposed set of piece planes.
// INW = 0 (7 or 8 inputs, `in_rt`): db1 can no longer ride in a spare column of X -- at 8 inputs the 8-float row has none --
// so X holds the observations only and the dW1 product's B operand takes its column j == 8 from the sample-valid predicate
// instead of from LDS (the MFMA's B tile has 16 columns, only the LDS row is 8 wide).  The same k-ordered fmaf chain over
// the tile's samples as the ones column of the 6-input form, so db1 rounds the same way at every width.
// ROWS (uav_mlp_ppo_grad_rows): sample s of the launch is row rows[s] of the Bt-row buffers -- the observation row and the five
// per-sample scalars are gathered, everything behind the staging is the contiguous form's.  The index of the NEXT tile is
// fetched with this tile's loads, so a tile's gathers never wait for their index; an index outside [0, Bt) is clamped.
// DIAG: the loss lanes also keep the update diagnostics (loss_core.h: DiagAcc), in LDS like their loss sums, and lane 0 leaves
// the workgroup's eight sums behind the loss partials.  DIAG = false compiles to the kernels as they were.
// BC (uav_mlp_bc_grad): the behaviour-cloning loss on the loss lanes (loss_core.h: bc_sample) -- they load act and, when `ret`
// is not NULL, the value target from it; logp_old, adv and val_old are never read and `clip` carries value_coef.  The workgroup's
// partial is UAV_BC_SUMS_N sums + the head-bias sums.  Everything but the loss lanes is the PPO forms' code; BC = false compiles to
// the kernels as they were, and there is no BC + DIAG form.
template <bool H3, int INW = IN, bool ROWS = false, bool DIAG = false, bool BC = false>
__global__ __launch_bounds__(512) void mlp_ppo_grad_kernel(
    const float* __restrict__ params, const float* __restrict__ obs, const int32_t* __restrict__ act,
    const float* __restrict__ logp_old, const float* __restrict__ adv, const float* __restrict__ ret,
    const float* __restrict__ val_old, int64_t Bn, float inv_n, float clip, float beta, double* __restrict__ loss_partial,
    float* __restrict__ slabs, const float* __restrict__ w2t, int in_rt, const int32_t* __restrict__ rows, int64_t Bt) {
    constexpr int NC = UNC, MS = UMS;
    const int in = INW ? INW : in_rt;
    const MlpOff O(in);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Tiles<NC> L(smem);
    float* ACC1 = smem + Tiles<NC>::FLOATS;
    float* ACC2 = ACC1 + 2 * H1;
    float* DH = ACC2 + 3 * H2;
    // the loss lanes' running sums live in LDS, not in registers: only wave 0 touches them, once per tile, but as registers
    // they were live in EVERY wave across the whole tile loop (14 VGPRs of a kernel that spills)
    double* LS = reinterpret_cast<double*>(DH + MS * 8);
    // W1 [256][8] (columns 6, 7 zero) and the head weights [8][128] (rows 6, 7 zero): their per-lane MFMA fragments are
    // re-read from here where they are used instead of living in 10 VGPRs across the whole tile loop
    float* W1L = reinterpret_cast<float*>(LS + MS * LS_STRIDE);
    float* WHL = W1L + H1 * 8;
    unsigned short* P2 = reinterpret_cast<unsigned short*>(WHL + 8 * H2);
    float* MX = reinterpret_cast<float*>(P2 + 2 * MS * RS2);
    // dz2 once more for dW2 = dz2^T a1 (K = the tile's samples, so the scale must not depend on the sample): plane 0 =
    // fp16(x), plane 1 = fp16(x - plane 0) with x = dz2 * 2^e_run, e_run the WAVE's running power of two (below)
    unsigned short* P2w = reinterpret_cast<unsigned short*>(MX + NWAVE * MS);
    double* DLS = reinterpret_cast<double*>(smem + UPD_FLOATS);     // DIAG only
    double* BLS = DLS;                                              // BC only
    static_assert(!(BC && DIAG), "mlp_ppo_grad_kernel: no diagnostics for the cloning loss");

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, kq = lane >> 4;

    // ---- parameters: LayerNorm / bias vectors in LDS, the small weight fragments in registers
    stage_prm(L, params, O);
    for (int i = threadIdx.x; i < 2 * H1 + 3 * H2; i += 512) ACC1[i] = 0.f;
    for (int i = threadIdx.x; i < H1 * 8; i += 512) W1L[i] = (i & 7) < in ? params[O.W1 + (i >> 3) * in + (i & 7)] : 0.f;
    for (int i = threadIdx.x; i < 8 * H2; i += 512) WHL[i] = (i / H2) < NH ? params[O.WH + i] : 0.f;
    // W2 is NOT held in registers: the 64 + 64 VGPRs of its two orientations beside the 64 of the dW2 accumulators spill
    // (measured: 85 VGPRs to scratch).  Both orientations are streamed from L2 instead -- 256 KB per 32 samples and CU,
    // dwordx4 per lane thanks to the permuted k order -- W2 row-major for the forward, its transpose (w2t, made once per
    // call) for da1 = W2^T dz2.
    const float* wfw = params + O.W2 + (16 * w + j) * H1 + 4 * kq;           // forward:  W2[16 w + j][16 s + 4 kq ..]
    const float* wbw0 = w2t + (32 * w + j) * H2 + 4 * kq;                    // backward: W2^T[32 w + 16 t + j][16 s + 4 kq ..]
    const float* wbw1 = wbw0 + 16 * H2;
    // H3: fragment-ordered pieces.  forward: [row tile w][8 slabs][2 pieces][64 lanes][8]; backward (after the 64 K halves of
    // the forward set): [row tile 2 w + t][4 slabs][2][64][8]
    const unsigned short* w2f = reinterpret_cast<const unsigned short*>(w2t) + (size_t)w * 8 * 2 * 512 + lane * 8;
    const unsigned short* w2b = reinterpret_cast<const unsigned short*>(w2t) + (size_t)H1 * H2 * 2 + (size_t)(2 * w) * 4 * 2 * 512 + lane * 8;
    const float* bh = params + O.BH;

    f32x4 dW2[16], dW1[2], dWh;
#pragma unroll
    for (int i = 0; i < 16; ++i) dW2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    dW1[0] = dW1[1] = dWh = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < MS * LS_STRIDE; i += 512) LS[i] = 0.0;
    if constexpr (DIAG)
        for (int i = threadIdx.x; i < MS * UAV_PPO_DIAG_N; i += 512) DLS[i] = 0.0;
    if constexpr (BC)
        for (int i = threadIdx.x; i < MS * 2; i += 512) BLS[i] = 0.0;

    // H3: the dW2 accumulators of this wave hold dW2 * 2^e_run: dz2 rows of this wave's 16 units enter the fp16 product
    // scaled by a power of two that puts the largest magnitude seen SO FAR in [2^13, 2^14); when a tile brings a larger one
    // the exponent drops and the accumulators are rescaled (exact)
    int e_run = 100;
    const int64_t ntile = (Bn + MS - 1) / MS;
    PROF_DECL(16);
    // ROWS: the buffer row of launch sample s (0 past the end: never used), and the rows of this thread's X element / loss sample
    auto row_of = [&](int64_t s) {
        int r = s < Bn ? rows[s] : 0;
        r = r < 0 ? 0 : r;
        return (int64_t)r < Bt ? r : (int)(Bt - 1);
    };
    int rx_next = 0, rl_next = 0;
    if constexpr (ROWS) {
        if (threadIdx.x < MS * 8) rx_next = row_of((int64_t)blockIdx.x * MS + (threadIdx.x >> 3));
        if (w == 0 && lane < MS) rl_next = row_of((int64_t)blockIdx.x * MS + lane);
    }
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t s0 = tile * MS;
        // ---- stage the tile's observations; the loss lanes fetch their per-sample scalars early
        if (threadIdx.x < MS * 8) {
            const int sj = threadIdx.x >> 3, f = threadIdx.x & 7;
            // column 6 = 1: W1 has no column 6 (the forward multiplies it by zero), and dW1 = dz1^T X then carries
            // db1 = dz1^T 1 in its seventh column for free
            const int64_t rx = ROWS ? (int64_t)rx_next : s0 + sj;
            if constexpr (INW == IN) L.X[threadIdx.x] = (s0 + sj < Bn) ? (f < IN ? obs[rx * IN + f] : (f == IN ? 1.f : 0.f)) : 0.f;
            else L.X[threadIdx.x] = (s0 + sj < Bn && f < in) ? obs[rx * in + f] : 0.f;    // no ones column: see above
            if constexpr (ROWS) rx_next = row_of(s0 + (int64_t)gridDim.x * MS + sj);
        }
        int a_s = 0;
        float lpo = 0.f, Ad = 0.f, Rt = 0.f, vo = 0.f;
        const bool loss_lane = (w == 0) && lane < MS && s0 + lane < Bn;
        if (loss_lane) {
            const int64_t rl = ROWS ? (int64_t)rl_next : s0 + lane;
            if constexpr (BC) {
                a_s = act[rl];
                if (ret) Rt = ret[rl];
            } else {
                a_s = act[rl]; lpo = logp_old[rl]; Ad = adv[rl]; Rt = ret[rl]; vo = val_old[rl];
            }
            if constexpr (ROWS) rl_next = row_of(s0 + (int64_t)gridDim.x * MS + lane);
        }
        lds_barrier();
        PROF_MARK(0);
        // ---- forward
        f32x4 xh1[NC][2], xh2[NC];
        float r1[NC], r2[NC];
        {
            float w1a[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) w1a[t][s] = W1L[(32 * w + 16 * t + j) * 8 + 4 * s + kq];
            layer1<NC, H3>(L, w1a, w, j, kq, xh1, r1);
        }
        lds_barrier();
        PROF_MARK(1);
        if constexpr (H3) {
            // ONE address register pair, advanced 4 KB per two-slab chunk, the four fragments of a chunk at immediate offsets:
            // sixteen separate 64-bit addresses (what the compiler makes of w2f + constant) are sixteen spilled pairs
            const unsigned short* pw = w2f;
            asm volatile("" : "+v"(pw));
            layer2_h3<NC>(L, [&](int sl, int pc) {
                if (sl > 0 && (sl & 1) == 0 && pc == 0) { pw += 2048; asm volatile("" : "+v"(pw)); }
                return *reinterpret_cast<const f16x8*>(pw + ((sl & 1) * 2 + pc) * 512);
            }, w, j, kq, xh2, r2);
        } else layer2<NC>(L, [&](int s) { return ld4(wfw + 16 * s); }, w, j, kq, xh2, r2);
        lds_barrier();
        PROF_MARK(2);
        {
            float wh[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) wh[s] = j < 8 ? WHL[j * H2 + 16 * w + 4 * s + kq] : 0.f;
            heads_fwd<NC>(L, wh, bh, w, lane);
        }
        PROF_MARK(3);
        // ---- loss + d(total)/d(heads) for the tile's samples (lanes 0..MS-1 of wave 0)
        if (w == 0) {
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            if (lane < MS) {
                float dz[NA], dV = 0.f;
#pragma unroll
                for (int a = 0; a < NA; ++a) dz[a] = 0.f;
                if (loss_lane) {
                    float z[NA];
#pragma unroll
                    for (int a = 0; a < NA; ++a) z[a] = L.HD[lane * 8 + a];
                    double* ls = LS + lane * LS_STRIDE;
                    LossAcc lacc{ls[0], ls[1], ls[2], ls[3]};
                    if constexpr (BC) {
                        double* bl = BLS + lane * 2;
                        BcAcc bacc{ls[0], ls[1], ls[2], ls[3], bl[0], bl[1]};
                        dV = bc_sample<NA>(z, L.HD[lane * 8 + NA], a_s, ret != nullptr, Rt, inv_n, clip, beta, bacc, dz);
                        lacc = LossAcc{bacc.nll, bacc.vl, bacc.en, bacc.nan};
                        bl[0] = bacc.agree; bl[1] = bacc.cnt;
                    } else if constexpr (DIAG) {
                        DiagAcc* dg = reinterpret_cast<DiagAcc*>(DLS + lane * UAV_PPO_DIAG_N);
                        dV = ppo_sample<NA, true>(z, L.HD[lane * 8 + NA], a_s, lpo, Ad, Rt, vo, inv_n, clip, beta, lacc, dz, dg);
                    } else dV = ppo_sample<NA>(z, L.HD[lane * 8 + NA], a_s, lpo, Ad, Rt, vo, inv_n, clip, beta, lacc, dz);
                    ls[0] = lacc.pl; ls[1] = lacc.vl; ls[2] = lacc.en; ls[3] = lacc.nan;
                    // head-bias gradient sums: f32 running sums as before (kept as f32 VALUES in the f64 slots)
#pragma unroll
                    for (int a = 0; a < NA; ++a) ls[4 + a] = (double)((float)ls[4 + a] + dz[a]);
                    ls[4 + NA] = (double)((float)ls[4 + NA] + dV);
                }
#pragma unroll
                for (int a = 0; a < NA; ++a) DH[lane * 8 + a] = dz[a];
                DH[lane * 8 + NA] = dV;
                DH[lane * 8 + 6] = 0.f;
                DH[lane * 8 + 7] = 0.f;
            }
        }
        lds_barrier();
        PROF_MARK(4);
        // ---- heads backward: dWh += dheads^T a2 (K = the tile's samples), da2 = Wh^T dheads
#pragma unroll
        for (int s = 0; s < MS / 4; ++s) {
            const float a = j < 8 ? DH[(4 * s + kq) * 8 + j] : 0.f;
            dWh = mfma4(a, L.A2[(4 * s + kq) * AS2 + 16 * w + j], dWh);
        }
        // ---- LayerNorm 2 + ReLU backward (mlp.hip: ln_relu_bwd_kernel's arithmetic)
        f32x4 dz2[NC];
        float isc2[NC];                                      // H3: inverse fp16 scale of samples 16 c + j
#pragma unroll
        for (int c = 0; c < NC; ++c) isc2[c] = 1.f;
        {
            const int u = 16 * w + 4 * kq;
            const f32x4 g = ld4(L.prm + 3 * H1 + H2 + u), be = ld4(L.prm + 3 * H1 + 2 * H2 + u);
            f32x4 dxh[NC];
            // per-lane partial sums in f32 (4 terms, fixed order), widened to f64 only for the cross-lane / cross-wave sum:
            // the reference's own LayerNorm backward accumulates in f32; 48 f64 conversions and FMAs per tile and lane
            // here and in LayerNorm 1 were a quarter of these phases' issue time
            float p1[NC], p2[NC];
            f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sb = sg, sz = sg;
            float* a2p = ACC2 + u;
            const float whT[2] = {WHL[kq * H2 + 16 * w + j], WHL[(4 + kq) * H2 + 16 * w + j]};
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                f32x4 da2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 2; ++s) da2 = mfma4(whT[s], DH[(16 * c + j) * 8 + 4 * s + kq], da2);
                float q1 = 0.f, q2 = 0.f, mx = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dy = (xh2[c][r] * g[r] + be[r] > 0.f) ? da2[r] : 0.f;
                    sg[r] += dy * xh2[c][r];
                    sb[r] += dy;
                    dxh[c][r] = dy * g[r];
                    q1 += dxh[c][r];
                    q2 += dxh[c][r] * xh2[c][r];
                    mx = fmaxf(mx, fabsf(dxh[c][r]));
                }
                p1[c] = q1;
                p2[c] = q2;
                if (H3) {        // this wave's max |dxhat| of sample 16 c + j, for the sample's fp16 scale (below)
                    mx = quad_max(mx);
                    if (kq == 0) MX[w * MS + 16 * c + j] = mx;
                }
            }
            sg = row16_sum(sg);                              // dg2, dbe2: summed over the tile's 16 sample lanes, then ONE lane per
            sb = row16_sum(sb);                              // kq group adds them to the per-unit accumulators
            if (j == 0) {
                st4(a2p, ld4(a2p) + sg);
                st4(a2p + H2, ld4(a2p + H2) + sb);
            }
            float S1[NC], S2[NC];
            ln_exchange<NC>(L, w, j, kq, p1, p2, S1, S2);    // barrier inside: every wave's dWh reads of A2 are done
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float m1 = S1[c] * (1.0f / H2), m2 = S2[c] * (1.0f / H2);
#pragma unroll
                for (int r = 0; r < 4; ++r) dz2[c][r] = r2[c] * (dxh[c][r] - m1 - xh2[c][r] * m2);
                if (!H3) st4(L.A2 + (16 * c + j) * AS2 + u, dz2[c]);  // dz2 replaces a2 (the f32 dW2 product reads it)
                sz = sz + dz2[c];
                if (H3) {
                    // The sample's dz2 row as two fp16 planes for da1 = W2^T dz2.  Gradients span dozens of binades, fp16
                    // five bits of exponent: the row is scaled by the power of two that puts a BOUND on its largest
                    // magnitude -- |dz2| <= rstd (max |dxhat| + |m1| + sqrt(127) |m2|), identical in every wave -- into
                    // [2^13, 2^14), and the sample's column of da1 is scaled back exactly.
                    float M = MX[16 * c + j];
#pragma unroll
                    for (int i = 1; i < NWAVE; ++i) M = fmaxf(M, MX[i * MS + 16 * c + j]);
                    const float bound = r2[c] * (M + fabsf(m1) + 11.3f * fabsf(m2));
                    const int e = pow2_to_2e13(bound, 0);
                    const float sc = __uint_as_float((unsigned)(127 + e) << 23);
                    isc2[c] = __uint_as_float((unsigned)(127 - e) << 23);
                    unsigned short b[2][4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        _Float16 p0, p1;
                        split2h(dz2[c][r] * sc, p0, p1);
                        b[0][r] = h_bits(p0); b[1][r] = h_bits(p1);
                    }
#pragma unroll
                    for (int pc = 0; pc < 2; ++pc) {
                        uint2 v;
                        v.x = (unsigned)b[pc][0] | ((unsigned)b[pc][1] << 16);
                        v.y = (unsigned)b[pc][2] | ((unsigned)b[pc][3] << 16);
                        *reinterpret_cast<uint2*>(P2 + (pc * MS + 16 * c + j) * RS2 + u) = v;
                    }
                }
            }
            sz = row16_sum(sz);
            if (j == 0) st4(a2p + 2 * H2, ld4(a2p + 2 * H2) + sz);
            if constexpr (H3) {
                float m = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(dz2[c][r]));
                m = wave_max(m);
                const int e = pow2_to_2e13(m, 100);
                if (e < e_run) {                             // wave-uniform: a larger magnitude than any tile before
                    if (e_run < 100) {
#pragma unroll
                        for (int tj = 0; tj < 16; ++tj)
#pragma unroll
                            for (int r = 0; r < 4; ++r) dW2[tj][r] = __builtin_amdgcn_ldexpf(dW2[tj][r], e - e_run);
                    }
                    e_run = e;
                }
                const float sc = __builtin_amdgcn_ldexpf(1.0f, e_run);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    f32x4 x;
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[r] = dz2[c][r] * sc;
                    st_pieces4<false>(P2w + (16 * c + j) * RS2 + u, MS * RS2, x);
                }
            }
        }
        lds_barrier();                                       // dz2 visible
        PROF_MARK(5);
        // ---- dW2 += dz2^T a1 (row tile w, all 16 column tiles; K = the tile's samples), da1 = W2^T dz2
        if constexpr (H3) {
            // one K = 32 slab (the tile's samples): A = this wave's 16 dz2 rows from P2w, B = a1 from the SAME planes layer 2
            // read row-wise, both through the transposing LDS read.  a b = A0 q0 + 2^-11 A0 q1 + r q0 (+ O(2^-22)) with
            // A0 = fp16(x), r = fp16(x - A0), q0 / q1 = split2h(a1): ONE accumulator, the 2^-11 folded into an operand.
            const f16x8 a0 = tr_frag(P2w + 16 * w, RS2, lane);
            const f16x8 ar = tr_frag(P2w + MS * RS2 + 16 * w, RS2, lane);
            const f16x8 a0s = a0 * (_Float16)(1.0f / 2048.0f);
#pragma unroll
            for (int tj = 0; tj < 16; ++tj) {
                const f16x8 q0 = tr_frag(L.P1 + 16 * tj, RS1, lane);
                const f16x8 q1 = tr_frag(L.P1 + MS * RS1 + 16 * tj, RS1, lane);
                dW2[tj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, q0, dW2[tj], 0, 0, 0);
                dW2[tj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0s, q1, dW2[tj], 0, 0, 0);
                dW2[tj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ar, q0, dW2[tj], 0, 0, 0);
                if ((tj & 3) == 3) asm volatile("" ::: "memory");
            }
        } else {
            float af[MS / 4];
#pragma unroll
            for (int s = 0; s < MS / 4; ++s) af[s] = L.A2[(4 * s + kq) * AS2 + 16 * w + j];
#pragma unroll
            for (int tj = 0; tj < 16; ++tj) {
#pragma unroll
                for (int s = 0; s < MS / 4; ++s) dW2[tj] = mfma4(af[s], L.A1[(4 * s + kq) * AS1 + 16 * tj + j], dW2[tj]);
                if ((tj & 3) == 3) asm volatile("" ::: "memory");      // four column tiles' fragments at a time
            }
        }
        PROF_MARK(6);
        f32x4 da1[NC][2];
#pragma unroll
        for (int c = 0; c < NC; ++c) da1[c][0] = da1[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (H3) {
            // da1^T tile (row tiles 2 w, 2 w + 1 of the 256 units) = W2^T pieces x the scaled dz2 planes, K = 128 in 4 slabs
            const unsigned short* brow = P2 + j * RS2 + 8 * kq;
            f32x4 acl[NC][2];
#pragma unroll
            for (int c = 0; c < NC; ++c) acl[c][0] = acl[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            f16x8 wq[2][2][2];                               // [buffer][row tile][piece]: one slab ahead
            const unsigned short* pb0 = w2b;                 // one address pair per row tile, advanced 2 KB per slab
            const unsigned short* pb1 = w2b + 4 * 1024;
            asm volatile("" : "+v"(pb0), "+v"(pb1));
            wq[0][0][0] = *reinterpret_cast<const f16x8*>(pb0); wq[0][0][1] = *reinterpret_cast<const f16x8*>(pb0 + 512);
            wq[0][1][0] = *reinterpret_cast<const f16x8*>(pb1); wq[0][1][1] = *reinterpret_cast<const f16x8*>(pb1 + 512);
#pragma unroll
            for (int sl = 0; sl < H2 / 32; ++sl) {
                if (sl + 1 < H2 / 32) {
                    pb0 += 1024; pb1 += 1024;
                    asm volatile("" : "+v"(pb0), "+v"(pb1));
                    wq[(sl + 1) & 1][0][0] = *reinterpret_cast<const f16x8*>(pb0); wq[(sl + 1) & 1][0][1] = *reinterpret_cast<const f16x8*>(pb0 + 512);
                    wq[(sl + 1) & 1][1][0] = *reinterpret_cast<const f16x8*>(pb1); wq[(sl + 1) & 1][1][1] = *reinterpret_cast<const f16x8*>(pb1 + 512);
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const f16x8 b0 = *reinterpret_cast<const f16x8*>(brow + (16 * c) * RS2 + 32 * sl);
                    const f16x8 b1 = *reinterpret_cast<const f16x8*>(brow + (MS + 16 * c) * RS2 + 32 * sl);
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        acl[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[sl & 1][t][1], b0, acl[c][t], 0, 0, 0);
                        da1[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[sl & 1][t][0], b0, da1[c][t], 0, 0, 0);
                        acl[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[sl & 1][t][0], b1, acl[c][t], 0, 0, 0);
                    }
                }
                asm volatile("" ::: "memory");
            }
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int t = 0; t < 2; ++t) da1[c][t] = (da1[c][t] + acl[c][t] * H3_LO) * isc2[c];
        } else {
            const float* brow = L.A2 + j * AS2 + 4 * kq;
            f32x4 wq[2][2][2];                               // [buffer][slab in chunk][row tile]: two slabs ahead
#pragma unroll
            for (int i = 0; i < 2; ++i) { wq[0][i][0] = ld4(wbw0 + 16 * i); wq[0][i][1] = ld4(wbw1 + 16 * i); }
#pragma unroll
            for (int ch = 0; ch < H2 / 32; ++ch) {
                if (ch + 1 < H2 / 32) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        wq[(ch + 1) & 1][i][0] = ld4(wbw0 + 16 * (2 * (ch + 1) + i));
                        wq[(ch + 1) & 1][i][1] = ld4(wbw1 + 16 * (2 * (ch + 1) + i));
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    f32x4 b[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) b[c] = ld4(brow + 16 * c * AS2 + 16 * (2 * ch + i));
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            da1[c][0] = mfma4(wq[ch & 1][i][0][k], b[c][k], da1[c][0]);
                            da1[c][1] = mfma4(wq[ch & 1][i][1][k], b[c][k], da1[c][1]);
                        }
                }
                asm volatile("" ::: "memory");
            }
        }
        PROF_MARK(7);
        // ---- LayerNorm 1 + ReLU backward
        {
            f32x4 dxh[NC][2];                                // da1 becomes dxhat in place
            float q1[NC], q2[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) q1[c] = q2[c] = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int u = 32 * w + 16 * t + 4 * kq;
                const f32x4 g = ld4(L.prm + H1 + u), be = ld4(L.prm + 2 * H1 + u);
                f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sb = sg;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float dy = (xh1[c][t][r] * g[r] + be[r] > 0.f) ? da1[c][t][r] : 0.f;
                        sg[r] += dy * xh1[c][t][r];
                        sb[r] += dy;
                        dxh[c][t][r] = dy * g[r];
                        q1[c] += dxh[c][t][r];
                        q2[c] += dxh[c][t][r] * xh1[c][t][r];
                    }
                sg = row16_sum(sg);
                sb = row16_sum(sb);
                if (j == 0) {
                    float* a1p = ACC1 + u;                   // dg1, dbe1
                    st4(a1p, ld4(a1p) + sg);
                    st4(a1p + H1, ld4(a1p + H1) + sb);
                }
            }
            float S1[NC], S2[NC];
            ln_exchange<NC>(L, w, j, kq, q1, q2, S1, S2);    // barrier inside: every wave's dW2 reads of A1 are done
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int u = 32 * w + 16 * t + 4 * kq;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float m1 = S1[c] * (1.0f / H1), m2 = S2[c] * (1.0f / H1);
                    f32x4 dz1;
#pragma unroll
                    for (int r = 0; r < 4; ++r) dz1[r] = r1[c] * (dxh[c][t][r] - m1 - xh1[c][t][r] * m2);
                    st4(L.A1 + (16 * c + j) * AS1 + u, dz1);  // dz1 replaces a1 (db1 = its column sums: the dW1 product below)
                }
            }
        }
        lds_barrier();                                       // dz1 visible
        PROF_MARK(8);
        // ---- dW1 += dz1^T x
#pragma unroll
        for (int s = 0; s < MS / 4; ++s) {
            float b = j < 8 ? L.X[(4 * s + kq) * 8 + j] : 0.f;
            if constexpr (INW != IN) b = (j == IN_MAX && s0 + 4 * s + kq < Bn) ? 1.f : b;       // column 8 = sample valid: db1
#pragma unroll
            for (int t = 0; t < 2; ++t) dW1[t] = mfma4(L.A1[(4 * s + kq) * AS1 + 32 * w + 16 * t + j], b, dW1[t]);
        }
        lds_barrier();                                       // X, A1, A2, DH free for the next tile
        PROF_MARK(9);
    }
    PROF_FLUSH(g_mlp_prof[threadIdx.x >> 6], 16, blockIdx.x == 0 && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < 2);

    // ---- this workgroup's gradient slab (flat parameter layout) and loss partial
    float* slab = slabs + (size_t)blockIdx.x * O.N;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            if (j < in) slab[O.W1 + (32 * w + 16 * t + 4 * kq + r) * in + j] = dW1[t][r];
            else if (j == (INW == IN ? IN : IN_MAX)) slab[O.B1 + 32 * w + 16 * t + 4 * kq + r] = dW1[t][r];   // the ones column: db1
        }
#pragma unroll
    for (int tj = 0; tj < 16; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            slab[O.W2 + (16 * w + 4 * kq + r) * H1 + 16 * tj + j] = H3 ? __builtin_amdgcn_ldexpf(dW2[tj][r], -e_run) : dW2[tj][r];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (4 * kq + r < NH) slab[O.WH + (4 * kq + r) * H2 + 16 * w + j] = dWh[r];
    // LayerNorm / bias gradients from the per-unit accumulators
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * H1; i += 512) slab[(i < H1 ? O.G1 : O.BE1) + (i % H1)] = ACC1[i];
    for (int i = threadIdx.x; i < 3 * H2; i += 512) {
        const int q = i / H2, u = i % H2;
        slab[(q == 0 ? O.G2 : (q == 1 ? O.BE2 : O.B2)) + u] = ACC2[i];
    }
    if (w == 0) {
        // loss sums and the head-bias gradient: the loss lanes park their partial sums, lane 0 adds them in lane order
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            double* pp = loss_partial + (size_t)LOSS_PSTRIDE * blockIdx.x;
            for (int k = 0; k < 4 + NH; ++k) {
                double t = 0.0;
                for (int sj = 0; sj < MS; ++sj) t += LS[sj * LS_STRIDE + k];
                pp[(BC && k >= 4) ? k + 2 : k] = t;              // BC: the head-bias sums behind the six loss sums
                if (k >= 4) slab[O.BH + k - 4] = (float)t;
            }
            if constexpr (BC) {
                for (int k = 0; k < 2; ++k) {
                    double t = 0.0;
                    for (int sj = 0; sj < MS; ++sj) t += BLS[sj * 2 + k];
                    pp[4 + k] = t;
                }
            }
            if constexpr (DIAG) {
                double* dp = diag_partials(loss_partial) + (size_t)UAV_PPO_DIAG_N * blockIdx.x;
                for (int k = 0; k < UAV_PPO_DIAG_N; ++k) {
                    double t = 0.0;
                    for (int sj = 0; sj < MS; ++sj) t += DLS[sj * UAV_PPO_DIAG_N + k];
                    dp[k] = t;
                }
            }
        }
    }
}

// w2t[u1][u2] = W2[u2][u1]  (128 KB; once per gradient call)
__global__ __launch_bounds__(256) void mlp_w2_transpose_kernel(const float* __restrict__ w2, float* __restrict__ w2t) {
    const int i = blockIdx.x * 256 + threadIdx.x;           // i = u1 * H2 + u2
    if (i < H1 * H2) w2t[i] = w2[(i % H2) * H1 + i / H2];
}

// H3: both orientations of W2 as fp16 piece fragments (once per gradient call): forward set [8 row tiles][8 slabs][2][64][8],
// element (i, kq, e) of fragment (w, s) = W2[16 w + i][32 s + 8 kq + e]; backward set [16 row tiles][4 slabs][2][64][8],
// element = W2[32 s + 8 kq + e][16 rt + i].
__global__ __launch_bounds__(256) void mlp_w2_pieces_kernel(const float* __restrict__ w2, unsigned short* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;           // over 2 x H1 * H2 elements
    if (i >= 2 * H1 * H2) return;
    const bool bwd = i >= H1 * H2;
    const int q = bwd ? i - H1 * H2 : i;
    const int e = q & 7, lane = (q >> 3) & 63, row = lane & 15, kq = lane >> 4;
    float v;
    size_t o;
    if (!bwd) {
        const int sl = (q >> 9) & 7, wt = q >> 12;
        v = w2[(16 * wt + row) * H1 + 32 * sl + 8 * kq + e];
        o = ((size_t)(wt * 8 + sl) * 2) * 512 + lane * 8 + e;
    } else {
        const int sl = (q >> 9) & 3, rt = q >> 11;
        v = w2[(32 * sl + 8 * kq + e) * H1 + 16 * rt + row];
        o = (size_t)H1 * H2 * 2 + ((size_t)(rt * 4 + sl) * 2) * 512 + lane * 8 + e;
    }
    _Float16 p0, p1;
    split2h(v, p0, p1);
    out[o] = h_bits(p0);
    out[o + 512] = h_bits(p1);
}

// grad[i] = sum over the workgroups' slabs, 8 independent partial sums in a fixed association (deterministic)
__global__ __launch_bounds__(256) void mlp_slab_reduce_kernel(const float* __restrict__ slabs, int nb, int n, float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    float p8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int b = 0;
    for (; b + 8 <= nb; b += 8)
#pragma unroll
        for (int k = 0; k < 8; ++k) p8[k] += slabs[(size_t)(b + k) * n + c];
    for (; b < nb; ++b) p8[0] += slabs[(size_t)b * n + c];
    out[c] = ((p8[0] + p8[1]) + (p8[2] + p8[3])) + ((p8[4] + p8[5]) + (p8[6] + p8[7]));
}

}  // namespace

// f(b0, b1, ..) with each run-time switch as a std::true_type / std::false_type value: the template arguments of one launch
// from booleans known at the call (the idiom of lstm.hip's with_split)
template <class F>
static int with_bools(F&& f) { return f(); }
template <class F, class... Rest>
static int with_bools(F&& f, bool on, Rest... rest) {
    return on ? with_bools([&](auto... bs) { return f(std::true_type{}, bs...); }, rest...)
              : with_bools([&](auto... bs) { return f(std::false_type{}, bs...); }, rest...);
}

// uav_mlp_ppo_grad (in = 6), uav_mlp_ppo_grad_trend (in = 6 + trend_k) and uav_mlp_ppo_grad_rows (rows != nullptr: the n
// samples are rows[0 .. n) of n_total-row buffers): the arguments are checked by the callers
static int mlp_ppo_grad_impl(const char* who, uav_ctx* ctx, const float* params, const float* obs, const int32_t* act,
                             const float* logp_old, const float* adv, const float* ret, const float* val_old, int64_t n, int in,
                             float inv_n, float clip, float ent_beta, double* loss_sums, float* grad, hipStream_t st,
                             const int32_t* rows = nullptr, int64_t n_total = 0, bool bc = false) {
    const MlpOff O(in);
    const int64_t ntile = (n + UMS - 1) / UMS;
    int nb = ctx->num_cu;
    if (nb > ntile) nb = (int)ntile;
    const bool h3 = ctx->mode.arith == UAV_ARITH_FP16X3;       // the handle's arithmetic (uav_set_lstm_arith); else exact-f32 MFMA
    const size_t head = 65536, w2t_bytes = (size_t)H1 * H2 * sizeof(float) * 2;  // loss partials | W2^T or both piece sets | slabs
    UAV_REQUIRE(ctx->ws_bytes >= head + w2t_bytes + (size_t)nb * O.N * sizeof(float), "%s: workspace too small", who);
    double* partial = (double*)ctx->ws;
    float* w2t = (float*)((char*)ctx->ws + head);
    float* slabs = (float*)((char*)ctx->ws + head + w2t_bytes);
    // uav_set_ppo_diag: attached = the DIAG instantiation + its final pass.  bc (uav_mlp_bc_grad: `ret` = vtarget or NULL, `clip` =
    // value_coef, logp_old / adv / val_old unused, loss_sums = bc_sums[UAV_BC_SUMS_N]) has no such form and leaves the buffer alone
    double* const diag = bc ? nullptr : ctx->ppo_diag;
    UAV_REQUIRE(!diag || (size_t)nb * (LOSS_PSTRIDE + UAV_PPO_DIAG_N) * sizeof(double) <= head, "%s: %d workgroups' loss partials over the workspace head", who, nb);
    if (h3) hipLaunchKernelGGL(mlp_w2_pieces_kernel, dim3(2 * H1 * H2 / 256), dim3(256), 0, st, params + O.W2, reinterpret_cast<unsigned short*>(w2t));
    else hipLaunchKernelGGL(mlp_w2_transpose_kernel, dim3(H1 * H2 / 256), dim3(256), 0, st, params + O.W2, w2t);
    const int rc_grad = with_bools([&](auto h3_, auto six, auto rows_, auto diag_, auto bc_) {
        constexpr bool dg = diag_() && !bc_();
        constexpr auto kern = &mlp_ppo_grad_kernel<h3_(), six() ? IN : 0, rows_(), dg, bc_()>;
        const size_t lds = dg ? UPD_LDS_DIAG : (bc_() ? UPD_LDS_BC : UPD_LDS);
        UAV_CHECK_HIP(uav_dyn_lds(reinterpret_cast<const void*>(kern), (int)lds));
        hipLaunchKernelGGL(kern, dim3(nb), dim3(512), lds, st, params, obs, act, logp_old, adv, ret, val_old, n, inv_n, clip, ent_beta,
                           partial, slabs, w2t, in, rows, n_total);
        return 0;
    }, h3, in == IN, rows != nullptr, diag != nullptr, bc);
    if (rc_grad) return rc_grad;
    hipLaunchKernelGGL(mlp_slab_reduce_kernel, dim3((O.N + 255) / 256), dim3(256), 0, st, slabs, nb, O.N, grad);
    UAV_LAUNCH_CHECK();
    if (bc) return launch_bc_final(partial, nb, NH, loss_sums, nullptr, st);
    const int rc = launch_loss_final(partial, nb, NH, loss_sums, nullptr, st);
    return (rc || !diag) ? rc : launch_diag_final(partial, nb, diag, st);
}

extern "C" int uav_mlp_ppo_grad(uav_ctx* ctx, const float* params, const float* obs, const int32_t* act,
                                const float* logp_old, const float* adv, const float* ret, const float* val_old, int64_t n,
                                int in_dim, int h1, int h2, int n_act, float inv_n, float clip, float ent_beta,
                                double* loss_sums, float* grad, uav_stream stream) {
    UAV_REQUIRE(ctx && params && obs && act && logp_old && adv && ret && val_old && loss_sums && grad && n > 0,
                "uav_mlp_ppo_grad: bad argument");
    UAV_REQUIRE(in_dim == IN && h1 == H1 && h2 == H2 && n_act == NA,
                "uav_mlp_ppo_grad: the fused kernel is the reference's network (6-256-128, 5 actions); got %d-%d-%d, %d",
                in_dim, h1, h2, n_act);
    return mlp_ppo_grad_impl("uav_mlp_ppo_grad", ctx, params, obs, act, logp_old, adv, ret, val_old, n, IN, inv_n, clip, ent_beta,
                             loss_sums, grad, as_stream(stream));
}

extern "C" int uav_mlp_ppo_grad_trend(uav_ctx* ctx, const float* params, const float* obs, const int32_t* act,
                                      const float* logp_old, const float* adv, const float* ret, const float* val_old, int64_t n,
                                      int trend_k, float inv_n, float clip, float ent_beta, double* loss_sums, float* grad,
                                      uav_stream stream) {
    UAV_REQUIRE(ctx && params && obs && act && logp_old && adv && ret && val_old && loss_sums && grad && n > 0,
                "uav_mlp_ppo_grad_trend: bad argument");
    UAV_REQUIRE(trend_k >= 0 && 6 + trend_k <= IN_MAX, "uav_mlp_ppo_grad_trend: trend_k=%d (0 .. 2)", trend_k);
    return mlp_ppo_grad_impl("uav_mlp_ppo_grad_trend", ctx, params, obs, act, logp_old, adv, ret, val_old, n, IN + trend_k, inv_n, clip,
                             ent_beta, loss_sums, grad, as_stream(stream));
}

extern "C" int uav_mlp_ppo_grad_rows(uav_ctx* ctx, const float* params, const float* obs, const int32_t* act,
                                     const float* logp_old, const float* adv, const float* ret, const float* val_old,
                                     int64_t n_total, const int32_t* rows, int64_t n_rows, int trend_k, float inv_n, float clip,
                                     float ent_beta, double* loss_sums, float* grad, uav_stream stream) {
    UAV_REQUIRE(ctx && params && obs && act && logp_old && adv && ret && val_old && rows && loss_sums && grad && n_rows > 0,
                "uav_mlp_ppo_grad_rows: bad argument");
    UAV_REQUIRE(n_total > 0 && n_total <= 0x7fffffffLL, "uav_mlp_ppo_grad_rows: n_total=%lld (1 .. 2^31 - 1: the indices are i32)",
                (long long)n_total);
    UAV_REQUIRE(trend_k >= 0 && 6 + trend_k <= IN_MAX, "uav_mlp_ppo_grad_rows: trend_k=%d (0 .. 2)", trend_k);
    return mlp_ppo_grad_impl("uav_mlp_ppo_grad_rows", ctx, params, obs, act, logp_old, adv, ret, val_old, n_rows, IN + trend_k, inv_n,
                             clip, ent_beta, loss_sums, grad, as_stream(stream), rows, n_total);
}

extern "C" int uav_mlp_bc_grad(uav_ctx* ctx, const float* params, const float* obs, const int32_t* act, const float* vtarget,
                               int64_t n_total, const int32_t* rows, int64_t n_rows, int trend_k, float inv_n, float value_coef,
                               float ent_beta, double* bc_sums, float* grad, uav_stream stream) {
    UAV_REQUIRE(ctx && params && obs && act && bc_sums && grad, "uav_mlp_bc_grad: NULL argument");
    UAV_REQUIRE(n_total > 0 && n_total <= 0x7fffffffLL && (!rows || n_rows > 0),
                "uav_mlp_bc_grad: n_total=%lld n_rows=%lld (n_total 1 .. 2^31 - 1: the indices are i32; n_rows > 0 with rows)",
                (long long)n_total, (long long)n_rows);
    UAV_REQUIRE(trend_k >= 0 && 6 + trend_k <= IN_MAX, "uav_mlp_bc_grad: trend_k=%d (0 .. 2)", trend_k);
    return mlp_ppo_grad_impl("uav_mlp_bc_grad", ctx, params, obs, act, nullptr, nullptr, vtarget, nullptr, rows ? n_rows : n_total,
                             IN + trend_k, inv_n, value_coef, ent_beta, bc_sums, grad, as_stream(stream), rows, n_total, true);
}
