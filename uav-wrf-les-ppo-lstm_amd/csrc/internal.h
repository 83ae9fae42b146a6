// internal.h -- every function that one .hip file defines and another calls, declared ONCE (the env-typed ones: internal_env.h).
// The defining file includes this header too, so a definition that drifts from its declaration is an overload nobody defines
// and the link (-Wl,--no-undefined) fails -- not the first call.  Default arguments live here only.
#pragma once
#include "common.h"

int env_init_tables(uav_ctx* ctx);                                                                                   // env.hip
// gemm.hip, gemm_h3.hip: C = A B (+ bias) on strided operands, split-K slabs in `ws`; the fp16-split form where gemm_h3_ok says
// so, its dW-shaped products on the TN kernel when `tn` (uav_lstm_mode::gemm_tn)
int gemm_f32(const uav_scratch& ws, int64_t M, int64_t N, int64_t K, const float* A, int64_t sa_m, int64_t sa_k, const float* B,
             int64_t sb_k, int64_t sb_n, float* C, int64_t ldc, const float* bias, int accumulate, hipStream_t st);
bool gemm_h3_ok(int64_t M, int64_t N, int64_t K, const float* A, int64_t sa_m, int64_t sa_k, const float* B, int64_t sb_k, int64_t sb_n);
int gemm_h3(const uav_scratch& ws, bool tn, int64_t M, int64_t N, int64_t K, const float* A, int64_t sa_m, int64_t sa_k, const float* B,
            int64_t sb_k, int64_t sb_n, float* C, int64_t ldc, const float* bias, int accumulate, const unsigned* a_absmax, hipStream_t st);
// mlp.hip: deterministic column reductions
int colsum_absmax(const uav_scratch& ws, const float* X, int64_t B, int C, float* out, float* scratch, unsigned* absmax_bits,
                  hipStream_t st);
int colsum_xw(const uav_scratch& ws, const float* X, int64_t B, int C, const float* x, int I, float* colsum_out, float* xw_out,
              float* scratch, unsigned* absmax_bits, hipStream_t st, int xw_transposed = 0);
// loss.hip: the second stage of the fused kernels' loss / diagnostic sums
int launch_loss_final(double* partial, int nb, int n_heads, double* loss_sums, float* dhead_bias, hipStream_t st);
int launch_bc_final(double* partial, int nb, int n_heads, double* bc_sums, float* dhead_bias, hipStream_t st);
int launch_diag_final(double* partial, int nb, double* diag, hipStream_t st);
// lstm.hip: the persistent h = 64 / 128 sequence kernels, in the arithmetic of the mode `m` handed in
int lstm_fwd_seq(const uav_lstm_mode& m, bool fuse, const float* x, const float* keep, const float* h0, const float* c0, const float* w_ih,
                 const float* w_hh, const float* b_ih, const float* b_hh, int N, int T, int I, int H, float* y, float* hn, float* cn,
                 float* stash, const float* w_head, const float* b_head, int NHD, float* heads, bool* heads_done, hipStream_t st);
int lstm_bwd_seq(const uav_lstm_mode& m, const float* keep, const float* stash, const float* w_hh, const float* dy, const float* dheads,
                 const float* w_head, int NH, const float* dhn, const float* dcn, int N, int T, int H, float* dgates, bool tile, float* dh0,
                 float* dc0, hipStream_t st);
// lstm_generic.hip: one GEMM + one pointwise launch per time step in exact f32, any hidden size
int lstm_generic_fwd(uav_ctx* ctx, const float* keep, const float* h0, const float* c0, const float* w_hh, int N, int T, int H, float* y,
                     float* hn, float* cn, float* stash, hipStream_t st);
int lstm_generic_bwd(uav_ctx* ctx, const float* keep, const float* stash, const float* w_hh, const float* dy, const float* dhn,
                     const float* dcn, int N, int T, int H, float* dgates, float* dh0, float* dc0, hipStream_t st);
void lstm_fill(float* x, const float* src, int64_t n, hipStream_t st);
// lstm_h3.hip: h = 256 on the fp16 split, one fused launch per time step.  Whether the step path runs for a handle, whether its gate
// gradients are kept packed and the UAV_BWD_* bits of its BPTT: uav_lstm_mode (lstm_forms.h), read from ctx->mode
int lstm_h3_fwd(uav_ctx* ctx, const float* x, int I, const float* w_ih, const float* b_ih, const float* b_hh, const float* keep,
                const float* h0, const float* c0, const float* w_hh, int N, int T, float* y, float* hn, float* cn, float* stash, hipStream_t st);
int lstm_h3_bwd(uav_ctx* ctx, const float* keep, const float* stash, const float* w_hh, const float* dy, const float* dheads,
                const float* w_head, int n_heads, const float* dhn, const float* dcn, int N, int T, float* dgates, float* dh0,
                float* dc0, const float* w_ih, float* dx, hipStream_t st);
int lstm_h3_bwd_stack(uav_ctx* ctx, int nl, const uav_lstm_bwd_layer* layers, const float* dy, const float* dheads, const float* w_head,
                      int n_heads, int N, int T, hipStream_t st);
// the stepper behind uav_lstm_stepper_* (H = 256, 0 < I <= 256, arguments and mode checked by the entry points, which hand in
// hslot: 1 = the step writes the stash's h_prev slot, 0 = the mode keeps packed gate gradients and leaves it out)
size_t lstm_h3_stepper_bytes(int N, int I);
int lstm_h3_stepper_begin(void* state, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* h0,
                          const float* c0, int N, int I, hipStream_t st);
int lstm_h3_stepper_step(const uav_stepper_call& c, int N, int T, int hslot, hipStream_t st);
int lstm_h3_stepper_step_pair(const uav_stepper_call& a, const uav_stepper_call& b, int N, int T, int hslot, hipStream_t st);
// wgrad.hip, wgrad_pc.hip: the weight-gradient passes
int lstm_wgrad_fused(uav_ctx* ctx, const float* dgates, const float* y, const float* keep, const float* h0, const float* x, int I,
                     const float* dheads, int NH, int N, int T, int H, float* dw_ih, float* dw_hh, float* db, float* db_hh, float* dw_head,
                     bool tile, hipStream_t st);
const char* lstm_wgrad_tile_refusal(const uav_ctx* ctx, int N, int T, int I, int H);
int lstm_pc_unpack(const void* dgates, int N, int T, float* out, hipStream_t st);
int lstm_pc_hprev_rows(const float* y, const float* keep, const float* h0, int N, int T, float* out, hipStream_t st);
int lstm_pc_wgrad(uav_ctx* ctx, const float* x, const float* y, const float* h0, const void* dgates, int N, int T, int I, float* dw_ih,
                  float* dw_hh, float* db, float* db_hh, hipStream_t st);
