// lstm_api.hip -- the C ABI of every LSTM path: argument checks, the choice of kernel family by hidden size and arithmetic mode
// (lstm.hip: persistent h = 64 / 128; lstm_h3.hip: h = 256 on the fp16 split, one launch per step; lstm_generic.hip: exact f32, any
// size; wgrad.hip / wgrad_pc.hip / gemm*.hip: weight gradients), and what a `dgates` / `stash` buffer holds between two calls.  The forms are DECIDED in lstm_forms.h; this file asks
// with the handle's mode as plain values and touches no record.
#include "internal.h"

// out[n][t][4H] = the row of (n, t) in a tile-form gate-gradient buffer (lstm_forms.h: DgTile); one float4 per thread
__global__ __launch_bounds__(256) void dg_tile_to_rows_kernel(const float4* __restrict__ dgates, int N, int T, int H4,
                                                              float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * T * H4) return;
    const int64_t r = i / H4;
    const int c = (int)(i - r * H4), n = (int)(r / T), t = (int)(r - (int64_t)n * T);
    out[i] = dgates[DgTile::row(n, t, T) * H4 + c];
}
static int lstm_dg_tile_to_rows(const float* dgates, int N, int T, int H, float* out, hipStream_t st) {
    const int64_t nv = (int64_t)N * T * H;                   // float4s: 4H / 4 per row
    UAV_REQUIRE(((reinterpret_cast<uintptr_t>(dgates) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 && (nv + 255) / 256 < (1ll << 31),
                "uav_lstm_dgates_f32: tile form needs 16-byte aligned buffers and fewer than 2^39 values");
    hipLaunchKernelGGL(dg_tile_to_rows_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(dgates), N, T, H, reinterpret_cast<float4*>(out));
    UAV_LAUNCH_CHECK();
    return 0;
}

// b[i] = a0[i] + a1[i]
__global__ void add2_kernel(const float* a0, const float* a1, float* b, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) b[i] = a0[i] + a1[i];
}

// One uav_lstm_wgrad call off the fused h = 64 / 128 path: its arguments, and the two other ways to the weight gradients.
struct LstmWgrad {
    uav_ctx* ctx;
    const float *x, *keep, *h0, *y, *stash, *dgates, *w_ih, *dheads;
    int n_heads, N, T, I, H;
    float *dw_ih, *dw_hh, *db, *db_hh, *dw_head, *dx;
    hipStream_t st;
    // what the trailing dx = dG W_ih product takes over from the path that ran: the workspace its slabs may use, where max |dG|
    // lies for the fp16-split product (NULL: exact f32), and the gate gradients as f32 rows
    uav_scratch ws;
    float* red = nullptr;
    unsigned* amax = nullptr;

    int64_t NT() const { return (int64_t)N * T; }

    // The large products go to the 16-bit matrix pipe as three fp16 piece products (gemm_h3.hip) unless exact f32 or
    // the bf16 split was asked for: dG is block-scaled by one power of two from its absolute maximum, which the bias
    // gradient's column-sum pass (it reads all of dG anyway) delivers; h_prev, x and W_ih are inside fp16's range
    // under the same preconditions as the sequence kernels' (include/uavppo.h, uav_set_lstm_arith).
    int product(int64_t M, int64_t Nn, int64_t K, const float* A, int64_t sa_m, int64_t sa_k, const float* B, int64_t sb_k,
                int64_t sb_n, float* C, int64_t ldc) {
        if (amax && gemm_h3_ok(M, Nn, K, A, sa_m, sa_k, B, sb_k, sb_n))
            return gemm_h3(ws, ctx->mode.gemm_tn(), M, Nn, K, A, sa_m, sa_k, B, sb_k, sb_n, C, ldc, nullptr, 0, amax, st);
        return gemm_f32(ws, M, Nn, K, A, sa_m, sa_k, B, sb_k, sb_n, C, ldc, nullptr, 0, st);
    }

    // the other two paths: column sums use the tail of the workspace, the split-K slabs everything in front of it
    int split_workspace() {
        UAV_REQUIRE(stash, "uav_lstm_wgrad: stash is required when I > 6");
        const size_t red_floats = (size_t)1024 * 9 * 4 * H + 64;      // colsum (+ dG^T x) partials + the word for max |dG|
        ws = ctx->scratch().carve(red_floats * sizeof(float), red_floats * sizeof(float), &red);
        UAV_REQUIRE(ws.p, "uav_lstm_wgrad: workspace too small");
        return 0;
    }
    int head_grad() {        // dW_head = dheads^T y [n_heads][H]: a stream over y with the few dheads columns riding along
        if (!dheads) return 0;
        if (H % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0)
            return colsum_xw(ws, y, NT(), H, dheads, n_heads, nullptr, dw_head, red, nullptr, st, 1);
        return gemm_f32(ws, n_heads, H, NT(), dheads, 1, n_heads, y, H, 1, dw_head, H, nullptr, 0, st);
    }

    // h = 256 on the fp16-split step path: `dgates` is the BPTT's piece chunks (lstm_forms.h: DgPack), read as they are by
    // wgrad_pc.hip -- db, dw_hh and dw_ih for a narrow (I <= 8) or hidden-wide (I = 256) input
    int pieces() {
        int rc;
        if ((rc = split_workspace())) return rc;
        if ((rc = lstm_pc_wgrad(ctx, x, y, h0, dgates, N, T, I, dw_ih, dw_hh, db, db_hh, st))) return rc;
        return head_grad();
    }

    // f32 rows (any hidden size in exact f32, h = 256 with UAV_DEBUG_DG_F32) as products over all N T rows.  packed: the buffer
    // holds piece chunks that wgrad_pc.hip does not take at this request (another input width, dx): they are first unpacked to
    // rows in the workspace, with h_prev beside them.
    int rows(bool packed) {
        int rc;
        if ((rc = split_workspace())) return rc;
        const float* hprev = stash + 5 * H;                 // rows of h_prev: the stash's slot, stride 6H
        int64_t ld_hprev = 6 * H;
        if (packed) {
            const size_t f32_bytes = (size_t)NT() * 5 * H * sizeof(float);     // gate gradients 4H + h_prev H (this mode's forward
            float* out;
            ws = ws.carve(f32_bytes, 64u << 20, &out);
            UAV_REQUIRE(ws.p, "uav_lstm_wgrad (h=256, I=%d%s): needs %zu bytes of workspace for "
                        "the gate gradients and h_prev as f32 rows", I, dx ? ", dx" : "", f32_bytes + (64u << 20));   // writes no slot)
            if ((rc = lstm_pc_unpack(dgates, N, T, out, st))) return rc;
            float* hp = out + (size_t)NT() * 4 * H;
            if ((rc = lstm_pc_hprev_rows(y, keep, h0, N, T, hp, st))) return rc;
            dgates = out;
            hprev = hp;
            ld_hprev = H;
        }
        const bool aligned = (reinterpret_cast<uintptr_t>(dgates) & 15) == 0;
        if (!ctx->mode.f32_mfma() && !ctx->mode.bf16x6() && aligned) amax = reinterpret_cast<unsigned*>(red + (size_t)1024 * 9 * 4 * H);
        // a narrow input (layer 1: obs + trend, I <= 8): dW_ih = dG^T x rides on the bias gradient's pass over dG
        const bool narrow = I <= 8 && aligned;
        if (narrow) rc = colsum_xw(ws, dgates, NT(), 4 * H, x, I, db, dw_ih, red, amax, st);
        else rc = colsum_absmax(ws, dgates, NT(), 4 * H, db, red, amax, st);
        if (rc) return rc;
        if (db_hh) UAV_CHECK_HIP(hipMemcpyAsync(db_hh, db, (size_t)4 * H * sizeof(float), hipMemcpyDeviceToDevice, st));
        if ((rc = product(4 * H, H, NT(), dgates, 1, 4 * H, hprev, ld_hprev, 1, dw_hh, H))) return rc;
        if (!narrow && (rc = product(4 * H, I, NT(), dgates, 1, 4 * H, x, I, 1, dw_ih, I))) return rc;
        return head_grad();
    }
};

// uav_lstm_bwd off the persistent kernels, one launch per time step: the fp16-split step path where it runs, else exact f32
static int lstm_bwd_steps(uav_ctx* ctx, const float* keep, const float* stash, const float* w_hh, const float* dy, const float* dheads,
                          const float* w_head, int n_heads, const float* dhn, const float* dcn, int N, int T, int H, float* dgates,
                          float* dh0, float* dc0, const float* w_ih, int I, float* dx, hipStream_t st) {
    const bool h3 = ctx->mode.step_path(H);
    UAV_REQUIRE(dy || h3, "uav_lstm_bwd: this hidden size / arithmetic takes dy (form dheads . w_head with uav_gemm_f32); "
                "see uav_lstm_bwd_caps");
    UAV_REQUIRE(!dx || (w_ih && (ctx->mode.bwd_caps(I, H) & UAV_BWD_FUSES_DX)), "uav_lstm_bwd: dx is formed here only when uav_lstm_bwd_caps(ctx, I, H) "
                "says so (H = 256 = I on the fp16-split arithmetic); otherwise ask uav_lstm_wgrad for it");
    if (h3) return lstm_h3_bwd(ctx, keep, stash, w_hh, dy, dheads, w_head, n_heads, dhn, dcn, N, T, dgates, dh0, dc0, w_ih, dx, st);
    return lstm_generic_bwd(ctx, keep, stash, w_hh, dy, dhn, dcn, N, T, H, dgates, dh0, dc0, st);
}

// the checks of one stepper step, in the name of the entry point `who`
static int stepper_check(const char* who, const uav_lstm_mode& m, const uav_stepper_call& c, int N, int T, int H) {
    UAV_REQUIRE(c.state && c.x && c.y && c.stash && c.hn && c.cn, "%s: NULL argument", who);
    UAV_REQUIRE(uav_lstm_stepper_bytes(N, c.I, H) != 0 && T > 0 && c.t >= 0 && c.t < T, "%s: bad shape (N=%d T=%d t=%d I=%d H=%d)", who, N, T, c.t, c.I, H);
    UAV_REQUIRE(m.step_path(H), "%s: only the fp16-split arithmetic steps (uav_set_lstm_arith)", who);
    UAV_REQUIRE(!c.below || c.I == 256, "%s: `below` needs I = 256 (the layer below's hidden size), got %d", who, c.I);
    return 0;
}

extern "C" {

int uav_lstm_fwd(uav_ctx* ctx, const float* x, const float* keep, const float* h0, const float* c0, const float* w_ih,
                 const float* w_hh, const float* b_ih, const float* b_hh, int N, int T, int I, int H, float* y,
                 float* hn, float* cn, float* stash, const float* w_head, const float* b_head, int n_heads, float* heads,
                 uav_stream stream) {
    UAV_REQUIRE(ctx && x && h0 && c0 && w_ih && w_hh && b_ih && b_hh && y && hn && cn, "uav_lstm_fwd: NULL argument");
    UAV_REQUIRE(N > 0 && T > 0 && I > 0, "uav_lstm_fwd: N=%d T=%d I=%d", N, T, I);
    UAV_REQUIRE(!heads || (w_head && b_head && n_heads > 0 && n_heads <= 8), "uav_lstm_fwd: heads needs w_head, b_head, 1..8 heads");
    hipStream_t st = as_stream(stream);
    const uav_lstm_mode& m = ctx->mode;
    const bool persistent = (H == 64 || H == 128);
    const bool fuse = I <= 8 && persistent;
    const bool step256 = m.step_path(H);      // h = 256: one fused launch per step, input projection inside
    if (step256) UAV_REQUIRE(stash, "uav_lstm_fwd: stash is required when H is not 64/128");
    if (!fuse && !step256) {
        // time-batched input projection into the gates slot of the stash: pre = x W_ih^T + (b_ih + b_hh)
        UAV_REQUIRE(stash, "uav_lstm_fwd: stash is required when I > 8 or H is not 64/128");
        float* bsum = (float*)ctx->ws;   // 4H floats at the head of the workspace... kept clear of GEMM slabs below
        const uav_scratch sub{(char*)ctx->ws + 65536, ctx->ws_bytes - 65536, ctx->num_cu};
        hipLaunchKernelGGL(add2_kernel, dim3((4 * H + 255) / 256), dim3(256), 0, st, b_ih, b_hh, bsum, 4 * H);
        int rc = gemm_f32(sub, (int64_t)N * T, 4 * H, I, x, I, 1, w_ih, 1, I, stash, 6 * H, bsum, 0, st);
        if (rc) return rc;
    }
    bool heads_done = false;
    int rc;
    if (persistent)
        rc = lstm_fwd_seq(m, fuse, x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, N, T, I, H, y, hn, cn, stash, w_head, b_head, n_heads, heads, &heads_done, st);
    else  // any other hidden size: one launch per time step (lstm_h3.hip, lstm_generic.hip)
        rc = step256 ? lstm_h3_fwd(ctx, x, I, w_ih, b_ih, b_hh, keep, h0, c0, w_hh, N, T, y, hn, cn, stash, st)
                     : lstm_generic_fwd(ctx, keep, h0, c0, w_hh, N, T, H, y, hn, cn, stash, st);
    if (rc) return rc;
    // h = 256: whether this stash's h_prev slot was written (the fp16-split step path with packed gate gradients leaves it out)
    if (H == DgPack::H) ctx->forms.stash_written(stash, m.dg_packed(H) ? 0 : 1);
    // kernels without the fused head product: heads = y W_head^T + b_head as one GEMM over the rows of y
    if (heads && !heads_done)
        return gemm_f32(ctx->scratch(), (int64_t)N * T, n_heads, H, y, H, 1, w_head, 1, H, heads, n_heads, b_head, 0, st);
    return 0;
}

int uav_lstm_bwd_caps(uav_ctx* ctx, int I, int H) {
    if (!ctx) return 0;
    if (H == 64 || H == 128) return UAV_BWD_TAKES_DHEADS;            // the persistent sequence kernels
    return ctx->mode.bwd_caps(I, H);                                 // the exact-f32 step path: none
}

size_t uav_lstm_dgates_bytes(uav_ctx* ctx, int N, int T, int H) {
    if (!ctx || N <= 0 || T <= 0 || H <= 0) return 0;
    if (ctx->mode.dg_packed(H)) return DgPack(N, T).bytes();
    return (size_t)N * T * 4 * H * sizeof(float);
}

int uav_lstm_dgates_f32(uav_ctx* ctx, const float* dgates, int N, int T, int H, float* out, uav_stream stream) {
    UAV_REQUIRE(ctx && dgates && out && N > 0 && T > 0 && H > 0, "uav_lstm_dgates_f32: bad argument");
    const int form = ctx->forms.f32_read(dgates, N, T, H, ctx->mode.dg_packed(H));
    if (form < 0) return 2;
    if (form == UAV_DG_TILE) return lstm_dg_tile_to_rows(dgates, N, T, H, out, as_stream(stream));
    if (form == UAV_DG_PIECES) return lstm_pc_unpack(dgates, N, T, out, as_stream(stream));
    UAV_CHECK_HIP(hipMemcpyAsync(out, dgates, (size_t)N * T * 4 * H * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    return 0;
}

size_t uav_lstm_dgates_tile_bytes(uav_ctx* ctx, int N, int T, int I, int H) {
    if (!ctx || N <= 0 || T <= 0 || I <= 0 || H <= 0) return 0;
    if (const char* why = lstm_wgrad_tile_refusal(ctx, N, T, I, H)) {
        uav_set_error("uav_lstm_dgates_tile_bytes(N=%d, T=%d, I=%d, H=%d): %s", N, T, I, H, why);
        return 0;
    }
    return DgTile::bytes(N, T, H);
}

int uav_lstm_dgates_tile(uav_ctx* ctx, float* dgates, int N, int T, int I, int H) {
    UAV_REQUIRE(ctx && dgates && N > 0 && T > 0 && I > 0 && H > 0, "uav_lstm_dgates_tile: bad argument");
    const char* why = lstm_wgrad_tile_refusal(ctx, N, T, I, H);
    UAV_REQUIRE(!why, "uav_lstm_dgates_tile(N=%d, T=%d, I=%d, H=%d): %s", N, T, I, H, why);
    return ctx->forms.arm(dgates, N, T, H) < 0 ? 2 : 0;
}

int uav_lstm_dgates_form(uav_ctx* ctx, const float* dgates) {
    if (!ctx || !dgates) return -1;
    return ctx->forms.form(dgates);
}

int uav_lstm_dgates_forget(uav_ctx* ctx, const float* dgates) {
    UAV_REQUIRE(ctx && dgates, "uav_lstm_dgates_forget: bad argument");
    ctx->forms.forget(dgates);
    return 0;
}

int uav_lstm_bwd_stack(uav_ctx* ctx, int n_layers, const uav_lstm_bwd_layer* layers, const float* dy, const float* dheads,
                       const float* w_head, int n_heads, int N, int T, int H, uav_stream stream) {
    UAV_REQUIRE(ctx && layers, "uav_lstm_bwd_stack: NULL argument");
    UAV_REQUIRE((dy != nullptr) != (dheads != nullptr), "uav_lstm_bwd_stack: give exactly one of dy / dheads");
    UAV_REQUIRE(!dheads || (w_head && n_heads > 0 && n_heads <= 8), "uav_lstm_bwd_stack: dheads needs w_head and 1..8 heads");
    UAV_REQUIRE(N > 0 && T > 0, "uav_lstm_bwd_stack: N=%d T=%d", N, T);
    UAV_REQUIRE(ctx->mode.step_path(H), "uav_lstm_bwd_stack: H = 256 on the fp16-split arithmetic only (uav_lstm_bwd_caps)");
    const int nl = n_layers < 4 ? n_layers : 4;
    for (int l = 0; l < nl; ++l) ctx->forms.forget(layers[l].dgates);       // h = 256 never writes tile form
    const int rc = lstm_h3_bwd_stack(ctx, n_layers, layers, dy, dheads, w_head, n_heads, N, T, as_stream(stream));
    for (int l = 0; l < nl; ++l) ctx->forms.bwd_end(layers[l].dgates, ctx->mode.dg_packed(H) ? UAV_DG_PIECES : UAV_DG_ROWS, rc == 0);
    return rc;
}

int uav_lstm_bwd(uav_ctx* ctx, const float* keep, const float* stash, const float* w_hh, const float* dy,
                 const float* dheads, const float* w_head, int n_heads, const float* dhn, const float* dcn, int N,
                 int T, int H, float* dgates, float* dh0, float* dc0, const float* w_ih, int I, float* dx,
                 uav_stream stream) {
    UAV_REQUIRE(ctx && stash && w_hh && dgates, "uav_lstm_bwd: NULL argument");
    UAV_REQUIRE((dy != nullptr) != (dheads != nullptr), "uav_lstm_bwd: give exactly one of dy / dheads");
    UAV_REQUIRE(!dheads || (w_head && n_heads > 0 && n_heads <= 8), "uav_lstm_bwd: dheads needs w_head and 1..8 heads");
    UAV_REQUIRE(N > 0 && T > 0, "uav_lstm_bwd: N=%d T=%d", N, T);
    // Tile form (lstm_forms.h: DgTile) is written only into a buffer armed for exactly this shape by uav_lstm_dgates_tile, and the
    // record then says so until the next uav_lstm_bwd on the buffer; every other call writes f32 rows (h = 256: or pieces).
    const int form = ctx->forms.bwd_begin(dgates, N, T, H, dx != nullptr);
    if (form < 0) return 2;
    const uav_lstm_mode& m = ctx->mode;
    int rc, wrote;
    if (H != 64 && H != 128) {
        wrote = m.dg_packed(H) ? UAV_DG_PIECES : UAV_DG_ROWS;
        rc = lstm_bwd_steps(ctx, keep, stash, w_hh, dy, dheads, w_head, n_heads, dhn, dcn, N, T, H, dgates, dh0, dc0, w_ih, I, dx,
                            as_stream(stream));
    } else {
        UAV_REQUIRE(!dx, "uav_lstm_bwd: dx is not formed by the H = 64 / 128 sequence kernels (uav_lstm_wgrad does it)");
        wrote = form == UAV_DG_TILE ? UAV_DG_TILE : -1;             // their f32 rows are not recorded
        rc = lstm_bwd_seq(m, keep, stash, w_hh, dy, dheads, w_head, n_heads, dhn, dcn, N, T, H, dgates, form == UAV_DG_TILE, dh0, dc0,
                          as_stream(stream));
    }
    ctx->forms.bwd_end(dgates, wrote, rc == 0);
    return rc;
}

int uav_lstm_wgrad(uav_ctx* ctx, const float* x, const float* keep, const float* h0, const float* y,
                   const float* stash, const float* dgates, const float* w_ih, const float* dheads, int n_heads, int N,
                   int T, int I, int H, float* dw_ih, float* dw_hh, float* db, float* db_hh, float* dw_head, float* dx,
                   uav_stream stream) {
    UAV_REQUIRE(ctx && x && h0 && y && dgates && w_ih && dw_ih && dw_hh && db, "uav_lstm_wgrad: NULL argument");
    UAV_REQUIRE(N > 0 && T > 0 && I > 0 && H > 0, "uav_lstm_wgrad: N=%d T=%d I=%d H=%d", N, T, I, H);
    UAV_REQUIRE(!dheads || (dw_head && n_heads > 0 && n_heads <= 8), "uav_lstm_wgrad: dheads needs dw_head, 1..8 heads");
    // 1. what the buffer holds, and whether this call under the handle's mode may read it
    const uav_lstm_mode& m = ctx->mode;
    const bool packed = m.dg_packed(H);
    const char* no_tile = ctx->forms.form(dgates) == UAV_DG_TILE ? lstm_wgrad_tile_refusal(ctx, N, T, I, H) : nullptr;
    const int form = ctx->forms.wgrad_read(dgates, stash, N, T, H, dx != nullptr, packed, no_tile);
    if (form < 0) return 2;
    // 2. the weight gradients
    LstmWgrad g{ctx, x, keep, h0, y, stash, dgates, w_ih, dheads, n_heads, N, T, I, H, dw_ih, dw_hh, db, db_hh, dw_head, dx,
                as_stream(stream), ctx->scratch()};
    int rc;
    if (I <= 6 && (H == 64 || H == 128))     // one fused pass over rows or tile blocks (wgrad.hip)
        rc = lstm_wgrad_fused(ctx, dgates, y, keep, h0, x, I, dheads, n_heads, N, T, H, dw_ih, dw_hh, db, db_hh, dw_head, form == UAV_DG_TILE, as_stream(stream));
    else if (packed && (I <= 8 || I == H) && !dx) rc = g.pieces();
    else rc = g.rows(packed);
    if (rc) return rc;
    // 3. dx = dG W_ih over the rows the path left
    if (dx) return g.product(g.NT(), I, 4 * H, g.dgates, 4 * H, 1, w_ih, I, 1, dx, I);
    return 0;
}

// ---- uav_lstm_fwd one time step per call (lstm_h3.hip): the checks and the stash record here, layout and launches there
size_t uav_lstm_stepper_bytes(int N, int I, int H) {
    if (H != 256 || N <= 0 || I <= 0 || I > 256) return 0;
    return lstm_h3_stepper_bytes(N, I);
}

int uav_lstm_stepper_begin(uav_ctx* ctx, void* state, const float* w_ih, const float* w_hh, const float* b_ih,
                           const float* b_hh, const float* h0, const float* c0, int N, int I, int H, uav_stream stream) {
    UAV_REQUIRE(ctx && state && w_ih && w_hh && b_ih && b_hh && h0 && c0, "uav_lstm_stepper_begin: NULL argument");
    UAV_REQUIRE(uav_lstm_stepper_bytes(N, I, H) != 0, "uav_lstm_stepper_begin: H = %d, I = %d not supported (H = 256, I <= 256)", H, I);
    UAV_REQUIRE(ctx->mode.step_path(H), "uav_lstm_stepper_begin: only the fp16-split arithmetic steps (uav_set_lstm_arith)");
    return lstm_h3_stepper_begin(state, w_ih, w_hh, b_ih, b_hh, h0, c0, N, I, as_stream(stream));
}

int uav_lstm_stepper_step(uav_ctx* ctx, void* state, const float* x, const void* below, const float* keep_t, int N, int T, int t,
                          int I, int H, float* y, float* stash, float* hn, float* cn, uav_stream stream) {
    UAV_REQUIRE(ctx, "uav_lstm_stepper_step: NULL argument");
    const uav_stepper_call c{state, x, below, keep_t, t, I, y, stash, hn, cn};
    int rc;
    if ((rc = stepper_check("uav_lstm_stepper_step", ctx->mode, c, N, T, H))) return rc;
    const int hslot = ctx->mode.dg_packed(H) ? 0 : 1;
    ctx->forms.stash_step(stash, t, hslot);
    return lstm_h3_stepper_step(c, N, T, hslot, as_stream(stream));
}

int uav_lstm_stepper_step_pair(uav_ctx* ctx, const uav_stepper_call* a, const uav_stepper_call* b, int N, int T, int H,
                               uav_stream stream) {
    UAV_REQUIRE(ctx && a && b, "uav_lstm_stepper_step_pair: NULL argument");
    UAV_REQUIRE(ctx->mode.step_path(H), "uav_lstm_stepper_step_pair: only the fp16-split arithmetic steps (uav_set_lstm_arith)");
    int rc;
    if ((rc = stepper_check("uav_lstm_stepper_step_pair", ctx->mode, *a, N, T, H)) || (rc = stepper_check("uav_lstm_stepper_step_pair", ctx->mode, *b, N, T, H)))
        return rc;
    const int hslot = ctx->mode.dg_packed(H) ? 0 : 1;
    ctx->forms.stash_step(a->stash, a->t, hslot);
    ctx->forms.stash_step(b->stash, b->t, hslot);
    return lstm_h3_stepper_step_pair(*a, *b, N, T, hslot, as_stream(stream));
}

}  // extern "C"
