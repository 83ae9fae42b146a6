// disc.hip -- GAIL discriminator: forward + BCE + backward over a whole (expert | policy) row set in one pass, and the
// imitation reward of a rollout buffer.
//
// Reference: PPOV2.0/model.py:58-70 (Discriminator: Linear(obs_dim + n_act, 128), ReLU, Linear(128, 1), Sigmoid),
// PPOV1.1/train_ppo_gail.py:157-175 (two BCELoss means, backward; the optimiser step is uav_clip_adam's).
//
// Shape of the work.  A row is sa = [state | one_hot(action) | 1 | 0...] padded to K = 16, so the bias b1 rides as a column of
// W1 and the whole first layer of 16 rows is 8 unit tiles x 4 v_mfma_f32_16x16x4_f32 (exact f32, the idiom of mlp_tile_core.h's
// small layers).  One wave owns 16 rows at a time:
//   forward   pre[row][unit] = sa W1p^T: A = sa (lane (j, kq) holds sa[row j][col 4 ks + kq]), B = W1p (held in 32 registers
//             for the whole kernel); the result leaves lane (j, kq) with pre[row 4 kq + r][unit 16 ut + j], r < 4, ut < 8.
//   z         w2 . relu(pre): 8 lane-local products per row, then a sum over the 16 lanes of a row group (4 xor steps).
//   loss      t = +z (policy, label 0) or -z (expert, label 1): loss = min(softplus(t), 100), dz = +-sigmoid(t) * weight --
//             both taken from the logit, so neither cancels where D rounds to 0 or 1.
//   backward  dW1p[unit][col] += da^T sa with K = the rows: da[row 4 kq + r][unit 16 ut + j] is ALREADY the A fragment of
//             MFMA step r (a sum over K does not care in which order the K index is walked, as long as B walks it the same
//             way), B = sa[row 4 kq + r][col j].  db1 is column obs_dim + n_act, the one-hot columns need no scatter.
// The 8 x 4 accumulator registers of dW1p, dw2 and db2 stay in registers across all rows of the wave; at the end the four
// waves of a workgroup are added in wave order through LDS and ONE slab of the parameter count goes to the workspace;
// disc_reduce_kernel adds the slabs in slab order.  No atomics: the bits depend on the slab count (workspace size, CU count)
// and on the order of the concatenated rows (expert first), on nothing else.
// Summation.  Expert rows pull every gradient entry one way and policy rows the other, so the sums cancel and a long f32
// chain shows in the RESULT's relative error (first version: 1.4e-6 on db1 over 544 k rows, 4 x torch's pairwise sums).
// Hence no long chain anywhere: the MFMA accumulators take DISC_FLUSH tiles (64 rows) and are then added into the wave's f32
// slab in LDS (a handful of adds per wave; registers are what bounds the kernel's occupancy); dw2 takes one add per tile, db2
// goes to f64 at once; waves, slabs and loss sums are added in f64.
// HBM: obs_dim * 4 + 4 bytes per row, once (the second, B-shaped read of the same 16 rows hits L1); no per-row intermediate
// leaves the CU.  Not memory-bound (15 MB at the headline shape) and not yet MFMA-bound either: 64 MFMAs per 16 rows would be
// ~30 us at 544 k rows, the kernel takes 168 us (profiles/gail_perf.json) -- the per-tile chain of loads, products, the
// 16-lane logit sum and the loss math runs at two waves per SIMD.
#include "common.h"

constexpr int DISC_H = 128, DISC_UT = DISC_H / 16, DISC_LSTRIDE = 8;      // loss partial: 4 doubles used of 8
constexpr int DISC_FLUSH = 4;           // tiles of 16 rows per MFMA accumulation chain

__host__ __device__ static inline size_t disc_params(int obs_dim, int n_act) {
    return (size_t)DISC_H * (obs_dim + n_act) + DISC_H + DISC_H + 1;
}
static inline size_t disc_slab_floats(size_t P) { return (P + 63) / 64 * 64; }

struct DiscRows {           // the concatenated row space: [0, n_e) expert, [n_e, n_e + n_p) policy
    const float* obs_e; const int32_t* act_e; int64_t n_e;
    const float* obs_p; const int32_t* act_p; int64_t n_p;
};

// column `col` of the padded row g (0 for rows past the end; an action outside [0, n_act) sets no column)
__device__ __forceinline__ float disc_sa(const DiscRows& R, int64_t g, int col, int od, int na) {
    if (g >= R.n_e + R.n_p) return 0.f;
    const bool ex = g < R.n_e;
    const int64_t i = ex ? g : g - R.n_e;
    if (col < od) return (ex ? R.obs_e : R.obs_p)[i * od + col];
    if (col < od + na) return (ex ? R.act_e : R.act_p)[i] == col - od ? 1.f : 0.f;
    return col == od + na ? 1.f : 0.f;
}

struct DiscW {              // a lane's share of the parameters: B fragments of W1p, its 8 entries of w2, b2
    float w1[DISC_UT][4], w2[DISC_UT], b2;
    __device__ __forceinline__ void load(const float* __restrict__ params, int od, int na, int j, int kq) {
        const int in = od + na;
        const float* b1 = params + (size_t)DISC_H * in;
#pragma unroll
        for (int ut = 0; ut < DISC_UT; ++ut) {
            const int u = 16 * ut + j;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int col = 4 * ks + kq;
                w1[ut][ks] = col < in ? params[(size_t)u * in + col] : (col == in ? b1[u] : 0.f);
            }
            w2[ut] = b1[DISC_H + u];
        }
        b2 = b1[2 * DISC_H];
    }
};

// pre-activations of the wave's 16 rows starting at row0 and their logits: pre[ut][r] = pre[row0 + 4 kq + r][16 ut + j]
// (ReLU applied; a NaN stays a NaN), z[r] = logit of row0 + 4 kq + r, the same value in all 16 lanes of the row group
__device__ __forceinline__ void disc_forward(const DiscRows& R, const DiscW& W, int64_t row0, int od, int na, int j, int kq,
                                             f32x4 (&pre)[DISC_UT], float (&z)[4]) {
    float a[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a[ks] = disc_sa(R, row0 + j, 4 * ks + kq, od, na);
#pragma unroll
    for (int ut = 0; ut < DISC_UT; ++ut) pre[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int ut = 0; ut < DISC_UT; ++ut) pre[ut] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], W.w1[ut][ks], pre[ut], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float s = 0.f;
#pragma unroll
        for (int ut = 0; ut < DISC_UT; ++ut) {
            const float p = pre[ut][r];
            pre[ut][r] = p < 0.f ? 0.f : p;
            s += W.w2[ut] * pre[ut][r];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
        z[r] = s + W.b2;
    }
}

// softplus(t) = log(1 + e^t) and sigmoid(t), both from e = exp(-|t|) <= 1: no overflow, no cancellation
__device__ __forceinline__ void softplus_sigmoid(float t, float& sp, float& sg) {
    const float e = expf(-fabsf(t)), d = 1.0f + e;
    sp = fmaxf(t, 0.f) + log1pf(e);
    sg = (t >= 0.f ? 1.0f : e) / d;
}

__global__ __launch_bounds__(256, 2) void disc_grad_kernel(DiscRows R, const float* __restrict__ params, int od, int na, float inv_ne,
                                                        float inv_np, float* __restrict__ slabs, size_t slab_floats,
                                                        double* __restrict__ lpart) {
    __shared__ float red[4][DISC_H * 17 + 1];      // per wave: dW1p as [unit][17] (16 columns + dw2), then db2
    __shared__ double lred[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4, in = od + na;
    DiscW W;
    W.load(params, od, na, j, kq);
    f32x4 acc[DISC_UT];                        // the running chain of <= DISC_FLUSH tiles; the chains add up in red[w]
    float dw2[DISC_UT];
    double db2 = 0.0;
#pragma unroll
    for (int ut = 0; ut < DISC_UT; ++ut) {
        acc[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
        dw2[ut] = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w][(16 * ut + 4 * kq + r) * 17 + j] = 0.f;      // each lane owns these slots until the end
    }
    double l_e = 0.0, l_p = 0.0, n_ok = 0.0, n_bad = 0.0;
    const int64_t ntot = R.n_e + R.n_p, ntile = (ntot + 15) / 16;
    int chain = 0;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + w; tile < ntile; tile += (int64_t)gridDim.x * 4) {
        const int64_t row0 = tile * 16;
        f32x4 pre[DISC_UT];
        float z[4], dz[4], b[4];
        disc_forward(R, W, row0, od, na, j, kq, pre, z);
        {   // the 16 lanes of a row group hold the same four logits: lane j works out row j & 3, lanes j < 4 book their row
            const int rr = j & 3;
            const int64_t g = row0 + 4 * kq + rr;
            const bool valid = g < ntot, ex = g < R.n_e;
            const float zr = rr == 0 ? z[0] : (rr == 1 ? z[1] : (rr == 2 ? z[2] : z[3]));
            const float t = ex ? -zr : zr;
            const float e = expf(-fabsf(t)), sg = (t >= 0.f ? 1.0f : e) / (1.0f + e);          // sigmoid(t) without overflow
            const float dzr = valid ? (ex ? -sg * inv_ne : sg * inv_np) : 0.f;
            if (valid && j < 4) {
                const int a = ex ? R.act_e[g] : R.act_p[g - R.n_e];
                const float sp = fmaxf(t, 0.f) + log1pf(e);         // softplus(t) = -log D (expert) / -log(1 - D) (policy)
                (ex ? l_e : l_p) += (double)fminf(sp, 100.f);       // nn.BCELoss clamps its logs at -100
                n_ok += t < 0.f ? 1.0 : 0.0;                         // D > 0.5 on an expert row, D < 0.5 on a policy row
                n_bad += (zr != zr || a < 0 || a >= na) ? 1.0 : 0.0;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dz[r] = __shfl(dzr, r, 16);
                b[r] = disc_sa(R, row0 + 4 * kq + r, j, od, na);
            }
        }
        db2 += (double)((dz[0] + dz[1]) + (dz[2] + dz[3]));
#pragma unroll
        for (int ut = 0; ut < DISC_UT; ++ut) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s += dz[r] * pre[ut][r];
                pre[ut][r] = pre[ut][r] > 0.f ? dz[r] * W.w2[ut] : 0.f;      // da (a NaN pre-activation made z, so dz, NaN)
            }
            dw2[ut] += s;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ut = 0; ut < DISC_UT; ++ut) acc[ut] = __builtin_amdgcn_mfma_f32_16x16x4f32(pre[ut][r], b[r], acc[ut], 0, 0, 0);
        if (++chain == DISC_FLUSH) {
            chain = 0;
#pragma unroll
            for (int ut = 0; ut < DISC_UT; ++ut) {
#pragma unroll
                for (int r = 0; r < 4; ++r) red[w][(16 * ut + 4 * kq + r) * 17 + j] += acc[ut][r];
                acc[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    // ---- wave partials -> LDS: acc[ut][r] = dW1p[unit 16 ut + 4 kq + r][col j]; dw2[ut] = this kq's share of dw2[16 ut + j]
#pragma unroll
    for (int ut = 0; ut < DISC_UT; ++ut) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w][(16 * ut + 4 * kq + r) * 17 + j] += acc[ut][r];
        double s = (double)dw2[ut];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (kq == 0) red[w][(16 * ut + j) * 17 + 16] = (float)s;
    }
    {   // db2: every lane of a row group carries the same four dz -- take lane j = 0 of each group
        double s = db2;
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (lane == 0) red[w][DISC_H * 17] = (float)s;
    }
    l_e = wave_sum(l_e); l_p = wave_sum(l_p); n_ok = wave_sum(n_ok); n_bad = wave_sum(n_bad);
    if (lane == 0) { lred[w][0] = l_e; lred[w][1] = l_p; lred[w][2] = n_ok; lred[w][3] = n_bad; }
    __syncthreads();
    // ---- the four waves in wave order, laid out as `params`
    float* slab = slabs + slab_floats * blockIdx.x;
    const size_t P = disc_params(od, na);
    for (int idx = threadIdx.x; idx < (int)P; idx += 256) {
        int off;
        if (idx < DISC_H * in) off = (idx / in) * 17 + idx % in;                   // net.0.weight
        else if (idx < DISC_H * in + DISC_H) off = (idx - DISC_H * in) * 17 + in;  // net.0.bias: the ones column
        else if (idx < DISC_H * in + 2 * DISC_H) off = (idx - DISC_H * in - DISC_H) * 17 + 16;      // net.2.weight
        else off = DISC_H * 17;                                                    // net.2.bias
        slab[idx] = (float)((((double)red[0][off] + (double)red[1][off]) + (double)red[2][off]) + (double)red[3][off]);
    }
    if (threadIdx.x < 4)
        lpart[(size_t)DISC_LSTRIDE * blockIdx.x + threadIdx.x] =
            ((lred[0][threadIdx.x] + lred[1][threadIdx.x]) + lred[2][threadIdx.x]) + lred[3][threadIdx.x];
}

// grad[i] = sum over the slabs, in slab order, in f64; block 0 also finishes loss_sums (f64, fixed tree)
__global__ __launch_bounds__(256) void disc_reduce_kernel(const float* __restrict__ slabs, size_t slab_floats, int nslab,
                                                          const double* __restrict__ lpart, int P, float* __restrict__ grad,
                                                          double* __restrict__ loss_sums) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int k = 0;
        for (; k + 3 < nslab; k += 4) {
            s0 += slabs[slab_floats * k + i];
            s1 += slabs[slab_floats * (k + 1) + i];
            s2 += slabs[slab_floats * (k + 2) + i];
            s3 += slabs[slab_floats * (k + 3) + i];
        }
        for (; k < nslab; ++k) s0 += slabs[slab_floats * k + i];
        grad[i] = (float)((s0 + s1) + (s2 + s3));
    }
    if (blockIdx.x == 0) {
        __shared__ double sm[4];
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = threadIdx.x; k < nslab; k += 256)
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] += lpart[(size_t)DISC_LSTRIDE * k + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double r = block256_sum(v[c], sm);
            if (threadIdx.x == 0) loss_sums[c] = r;
        }
    }
}

__global__ __launch_bounds__(256) void disc_reward_kernel(DiscRows R, const float* __restrict__ params, int od, int na,
                                                          float env_coef, float gail_coef, const float* rew_env, float* rew_out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
    DiscW W;
    W.load(params, od, na, j, kq);
    const int64_t ntot = R.n_p, ntile = (ntot + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + w; tile < ntile; tile += (int64_t)gridDim.x * 4) {
        f32x4 pre[DISC_UT];
        float z[4];
        disc_forward(R, W, tile * 16, od, na, j, kq, pre, z);
        const float zr = j == 0 ? z[0] : (j == 1 ? z[1] : (j == 2 ? z[2] : z[3]));
        const int64_t i = tile * 16 + 4 * kq + j;
        if (j < 4 && i < ntot) {                    // lane j of a row group writes row 4 kq + j
            float sp, sg;
            softplus_sigmoid(zr, sp, sg);
            const float g = gail_coef * sp;
            rew_out[i] = rew_env ? env_coef * rew_env[i] + g : g;
        }
    }
}

static int disc_check_shape(const char* who, int obs_dim, int n_act, int hidden) {
    UAV_REQUIRE(hidden == DISC_H, "%s: hidden=%d unsupported (the discriminator's hidden width is %d)", who, hidden, DISC_H);
    UAV_REQUIRE(obs_dim >= 1 && n_act >= 1 && obs_dim + n_act + 1 <= 16,
                "%s: obs_dim=%d n_act=%d unsupported ([state | one_hot | 1] must fit one 16-wide tile: obs_dim + n_act + 1 <= 16)",
                who, obs_dim, n_act);
    return 0;
}

extern "C" {

size_t uav_disc_param_count(int obs_dim, int n_act, int hidden) {
    if (disc_check_shape("uav_disc_param_count", obs_dim, n_act, hidden) != 0) return 0;
    return disc_params(obs_dim, n_act);
}

int uav_disc_grad(uav_ctx* ctx, const float* params, const float* obs_e, const int32_t* act_e, int64_t n_e, const float* obs_p,
                  const int32_t* act_p, int64_t n_p, int obs_dim, int n_act, int hidden, float inv_ne, float inv_np,
                  double* loss_sums, float* grad, uav_stream stream) {
    if (int rc = disc_check_shape("uav_disc_grad", obs_dim, n_act, hidden)) return rc;
    UAV_REQUIRE(ctx && params && loss_sums && grad, "uav_disc_grad: NULL argument");
    UAV_REQUIRE(n_e >= 0 && n_p >= 0 && n_e + n_p > 0 && n_e + n_p < (1ll << 40), "uav_disc_grad: n_e=%lld n_p=%lld", (long long)n_e,
                (long long)n_p);
    UAV_REQUIRE((n_e == 0 || (obs_e && act_e)) && (n_p == 0 || (obs_p && act_p)), "uav_disc_grad: NULL row set");
    const size_t P = disc_params(obs_dim, n_act), SF = disc_slab_floats(P);
    const size_t per_slab = SF * sizeof(float) + DISC_LSTRIDE * sizeof(double);
    const int64_t ntile = (n_e + n_p + 15) / 16;
    int64_t nslab = (ntile + 3) / 4;                                  // one 16-row tile per wave at least
    if (nslab > 2 * (int64_t)ctx->num_cu) nslab = 2 * (int64_t)ctx->num_cu;
    if (nslab > (int64_t)(ctx->ws_bytes / per_slab)) nslab = (int64_t)(ctx->ws_bytes / per_slab);      // as wgrad.hip: the workspace bounds the slabs
    UAV_REQUIRE(nslab >= 1, "uav_disc_grad: workspace of %zu bytes holds no partial slab (%zu bytes)", ctx->ws_bytes, per_slab);
    float* slabs = (float*)ctx->ws;
    double* lpart = (double*)((char*)ctx->ws + (size_t)nslab * SF * sizeof(float));
    const DiscRows R{obs_e, act_e, n_e, obs_p, act_p, n_p};
    hipLaunchKernelGGL(disc_grad_kernel, dim3((unsigned)nslab), dim3(256), 0, as_stream(stream), R, params, obs_dim, n_act, inv_ne,
                       inv_np, slabs, SF, lpart);
    hipLaunchKernelGGL(disc_reduce_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, as_stream(stream), slabs, SF, (int)nslab,
                       lpart, (int)P, grad, loss_sums);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_disc_reward(uav_ctx* ctx, const float* params, const float* obs, const int32_t* act, int64_t n, int obs_dim, int n_act,
                    int hidden, float env_coef, float gail_coef, const float* rew_env, float* rew_out, uav_stream stream) {
    if (int rc = disc_check_shape("uav_disc_reward", obs_dim, n_act, hidden)) return rc;
    UAV_REQUIRE(ctx && params && obs && act && rew_out, "uav_disc_reward: NULL argument");
    UAV_REQUIRE(n > 0 && n < (1ll << 40), "uav_disc_reward: n=%lld", (long long)n);
    int64_t nb = ((n + 15) / 16 + 3) / 4;
    if (nb > 4 * (int64_t)ctx->num_cu) nb = 4 * (int64_t)ctx->num_cu;
    const DiscRows R{nullptr, nullptr, 0, obs, act, n};
    hipLaunchKernelGGL(disc_reward_kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), R, params, obs_dim, n_act, env_coef,
                       gail_coef, rew_env, rew_out);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
