// lstm_forms.h -- the storage forms of the LSTM update's gate-gradient (`dgates`) and `stash` buffers: their layouts, the one
// record a device handle keeps per buffer, and every decision taken from that record; and the handle's arithmetic mode with the
// path decisions taken from it (uav_lstm_mode).  Host-only and free of HIP (plain C++17: tests/host/lstm_forms_check.cpp); the
// kernels see the two layout structs through common.h.  The entry points (lstm_api.hip, the stepper's among them) hand in what
// the handle's mode decides as plain values and never touch an entry themselves.
#pragma once
#include <stddef.h>
#include "../../include/uavppo.h"
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

// ---- "tile form" of the h = 64 / 128 gate gradients: the same f32 values and the same 4H-float rows as [N][T][4H], but the
// 16 rows that one BPTT workgroup (16 envs) writes in a step are adjacent -- one contiguous 16 x 4H block per (tile, step)
// instead of 16 pieces that lie T rows apart:  row(n, t) = ((n / 16) * T + t) * 16 + n % 16,  ceil(N / 16) tiles.
struct DgTile {
    static constexpr int MT = 16;                   // envs per tile = envs per BPTT workgroup
    __host__ __device__ static size_t row(int n, int t, int T) { return ((size_t)(n / MT) * T + t) * MT + n % MT; }
    __host__ __device__ static size_t rows(int N, int T) { return (size_t)((N + MT - 1) / MT) * MT * T; }
    __host__ __device__ static size_t bytes(int N, int T, int H) { return rows(N, T) * 4 * H * sizeof(float); }
};

// ---- gate gradients of the h = 256 fp16-split step path, stored ONCE (round 5): the `dgates` buffer that travels from
// uav_lstm_bwd / _bwd_stack to uav_lstm_wgrad holds what the BPTT's recurrent product consumes -- the two fp16 pieces of
// every row, scaled per (env, step) by the power of two that puts the row's largest magnitude in [2^13, 2^14), in MFMA
// fragment order (lstm_h3.hip: frag_index) -- and the weight-gradient pass reads THAT (wgrad_pc.hip) instead of a second,
// f32 copy (8 of the 17 KB the gate-gradient kernel moved per env-step; -10 % of a C5 iteration by ablation,
// profiles/r05_c5_no_f32_dgates_ablation.log).  Layout, time-major so that a step's block and the GEMM's K walk are linear:
//   halves  pieces[t][rt][s][piece][512]      rt < RT = NP / 16 (16-env row tiles, NP = N rounded up to 64; rows >= N zero),
//                                             s < NS = 4H / 32 (32 gate rows), 512 = (kq * 16 + env) * 8 + i, row 32 s + 8 kq + i
//   floats  isc[t][NP]                        2^-e of (env, step): dG = (p0 + 2^-11 p1) * isc; 0 for rows >= N and for
//                                             rows whose gate gradients are all zero (max isc is the weight-gradient block scale)
//   floats  iscm[t][NP]                       isc * keep[env][step]: the scale under which dW_hh = dG^T h_prev takes h_prev[n][t] = y[n][t-1]
//                                             * keep[n][t] straight from the layer's output y (h0 at t = 0) -- the forward pass then
//                                             need not write an h_prev slot into the stash at all
// The same byte count as f32 [N][T][4H] plus 8 bytes per (env, step): uav_lstm_dgates_bytes.
struct DgPack {
    static constexpr int H = 256, NS = 4 * H / 32;
    int N, T, NP, RT;
    __host__ __device__ DgPack(int n, int t) : N(n), T(t), NP((n + 63) / 64 * 64), RT(NP / 16) {}
    __host__ __device__ size_t step_halves() const { return (size_t)RT * NS * 1024; }
    __host__ __device__ size_t piece_bytes() const { return (size_t)T * step_halves() * 2; }
    __host__ __device__ size_t bytes() const { return piece_bytes() + 2 * (size_t)T * NP * sizeof(float); }
    __host__ __device__ unsigned short* pieces(void* base, int t) const { return (unsigned short*)base + (size_t)t * step_halves(); }
    __host__ __device__ const unsigned short* pieces(const void* base, int t) const { return (const unsigned short*)base + (size_t)t * step_halves(); }
    __host__ __device__ float* isc(void* base, int t) const { return (float*)((char*)base + piece_bytes()) + (size_t)t * NP; }
    __host__ __device__ const float* isc(const void* base, int t) const { return (const float*)((const char*)base + piece_bytes()) + (size_t)t * NP; }
    __host__ __device__ float* iscm(void* base, int t) const { return isc(base, T) + (size_t)t * NP; }
    __host__ __device__ const float* iscm(const void* base, int t) const { return isc(base, T) + (size_t)t * NP; }
};

// ---- the arithmetic mode of a handle (uav_set_lstm_arith, uav_set_debug_flags) as a plain value, and every path decision taken
// from it.  The handle keeps one; whoever launches reads it from its ctx or is handed it (or the value already decided from it).
struct uav_lstm_mode {
    int arith;         // UAV_ARITH_*: how the LSTM sequence kernels evaluate their f32 matrix products
    unsigned debug;    // UAV_DEBUG_*: A/B switches of the h = 256 step path and the dW-shaped split product
    bool f32_mfma() const { return arith == UAV_ARITH_F32_MFMA; }
    bool bf16x6() const { return arith == UAV_ARITH_BF16X6; }
    // The h = 256 step kernels exist in the fp16-split form only (|w| < 65504, |x| < 4096): BOTH other modes -- exact f32 and the
    // bf16 split, which callers select precisely because operands left that range -- take the generic exact-f32 step path
    // (lstm_generic.hip), uav_lstm_bwd_caps reports 0 and the stepper refuses.
    bool step_path(int H) const { return H == 256 && !f32_mfma() && !bf16x6() && !(debug & UAV_DEBUG_STEP_F32); }
    // the gate gradients stay in the packed form only (DgPack) unless the A/B switch asks for the round-4 f32 rows too
    bool dg_packed(int H) const { return step_path(H) && !(debug & UAV_DEBUG_DG_F32); }
    // what the step path's BPTT can do itself: take dheads + w_head; with an input as wide as the state, form dx = dG W_ih in its
    // recurrent product (no separate GEMM) and run a stack as a pipeline
    int bwd_caps(int I, int H) const {
        return step_path(H) ? ((I == H ? UAV_BWD_FUSES_DX | UAV_BWD_STACKS : 0) | UAV_BWD_TAKES_DHEADS) : 0;
    }
    bool x_pieces() const { return !(debug & UAV_DEBUG_X_F32); }            // a wide input of the step path as fp16 piece planes
    bool gemm_tn() const { return !(debug & UAV_DEBUG_GEMM_TN_OFF); }       // dW-shaped split products on gemm_h3_tn8_kernel
};

void uav_set_error(const char* fmt, ...);       // ctx.hip (the check program brings its own)
#define UAV_FORM_REFUSED(...) (uav_set_error(__VA_ARGS__), -1)

// The records of one device handle.  A `dgates` pointer has at most one record: UAV_DG_ROWS / UAV_DG_PIECES as the h = 256 and
// generic BPTTs wrote it, or UAV_DG_TILE_ARMED / UAV_DG_TILE with the shape the buffer was armed for (uav_lstm_dgates_tile; tile
// form is asked for PER BUFFER and per uav_lstm_bwd call, never per handle: the handle is shared by everything that runs on the
// device).  Whatever call last armed or wrote the buffer replaces what was there; the h = 64 / 128 kernels writing f32 rows
// record nothing and only drop a tile record.  A `stash` pointer has at most one record: whether its h_prev slot was written.
// Capacity: 8 tile records that are NEVER evicted (a buffer written in tile form and then forgotten by the table would be read as
// f32 rows), 8 rows / pieces records and 8 stash records of which the oldest makes room.
// Every decision returns the form (UAV_DG_*) the call writes or reads, or -1 with the refusal in uav_set_error.
class uav_lstm_forms {
    struct dg_rec { const void* p; int form, N, T, H; };
    struct stash_rec { const void* p; int hslot; };
    dg_rec tile_[8], ring_[8];
    stash_rec stash_[8];
    int ring_next_, stash_next_;

    dg_rec* dg(const void* p) {
        for (auto& x : tile_)
            if (p && x.p == p) return &x;
        for (auto& x : ring_)
            if (p && x.p == p) return &x;
        return nullptr;
    }
    const dg_rec* dg(const void* p) const { return const_cast<uav_lstm_forms*>(this)->dg(p); }
    static bool is_tile(const dg_rec* e) { return e && (e->form == UAV_DG_TILE_ARMED || e->form == UAV_DG_TILE); }
    void drop(const void* p) {
        if (dg_rec* e = dg(p)) *e = dg_rec{nullptr, 0, 0, 0, 0};
    }

public:
    // ---- uav_lstm_dgates_tile / _forget / _form
    int arm(const void* p, int N, int T, int H) {
        dg_rec* e = dg(p);
        dg_rec* slot = is_tile(e) ? e : nullptr;
        for (auto& x : tile_)
            if (!slot && !x.p) slot = &x;
        if (!slot) return UAV_FORM_REFUSED("uav_lstm_dgates_tile: eight other buffers of this handle are armed for or written in "
                                           "tile form; uav_lstm_dgates_forget one of them first");
        drop(p);
        *slot = dg_rec{p, UAV_DG_TILE_ARMED, N, T, H};
        return UAV_DG_TILE_ARMED;
    }
    void forget(const void* p) {                             // drops a tile record only: rows / pieces records age out
        if (is_tile(dg(p))) drop(p);
    }
    int form(const void* p) const {                          // UAV_DG_ROWS when nothing is recorded
        const dg_rec* e = dg(p);
        return e ? e->form : UAV_DG_ROWS;
    }

    // ---- a BPTT writes `p`.  begin: UAV_DG_TILE when the buffer is armed for exactly this call, a refusal when it is armed for
    // another one, else UAV_DG_ROWS ("not tile"; a record of tile blocks written earlier is dropped).
    int bwd_begin(const void* p, int N, int T, int H, bool dx) {
        const dg_rec* e = dg(p);
        if (!e || e->form != UAV_DG_TILE_ARMED) {
            forget(p);
            return UAV_DG_ROWS;
        }
        if (e->N == N && e->T == T && e->H == H && !dx) return UAV_DG_TILE;
        return UAV_FORM_REFUSED("uav_lstm_bwd: this dgates buffer is armed for tile form at N=%d T=%d H=%d without dx "
                                "(uav_lstm_dgates_tile), not for this call", e->N, e->T, e->H);
    }
    // end: `wrote` = UAV_DG_TILE (the armed record now says written), UAV_DG_PIECES / UAV_DG_ROWS (recorded), or -1 (the h = 64 /
    // 128 kernels' f32 rows: nothing is recorded).  A call that failed leaves no record of the pointer, whatever the form.
    void bwd_end(const void* p, int wrote, bool ok) {
        dg_rec* e = dg(p);
        if (!ok) {
            drop(p);
        } else if (wrote == UAV_DG_TILE) {
            if (e) e->form = UAV_DG_TILE;
        } else if (wrote >= 0) {
            if (is_tile(e)) {
                drop(p);
                e = nullptr;
            }
            if (!e) {
                e = &ring_[ring_next_];
                ring_next_ = (ring_next_ + 1) % 8;
            }
            *e = dg_rec{p, wrote, 0, 0, 0};
        }
    }

    // ---- uav_lstm_wgrad reads `p` (and, for f32 rows at h = 256, the stash's h_prev slot).  packed_now: the handle's mode reads
    // fp16 piece chunks at this H; tile_refusal: why that mode cannot read tile blocks of this shape, or NULL.
    int wgrad_read(const void* p, const void* stash, int N, int T, int H, bool dx, bool packed_now, const char* tile_refusal) const {
        const dg_rec* e = dg(p);
        if (is_tile(e)) {        // read by the split weight-gradient kernels alone, at the shape it was written for
            if (e->form != UAV_DG_TILE)
                return UAV_FORM_REFUSED("uav_lstm_wgrad: this dgates buffer is armed for tile form (uav_lstm_dgates_tile) but no "
                                        "uav_lstm_bwd has written it since: what it holds are not tile blocks");
            if (e->N != N || e->T != T || e->H != H || dx)
                return UAV_FORM_REFUSED("uav_lstm_wgrad: this dgates buffer was written in tile form for N=%d T=%d H=%d, which this "
                                        "call (N=%d T=%d H=%d%s) would read as f32 rows", e->N, e->T, e->H, N, T, H, dx ? ", dx" : "");
            if (tile_refusal)
                return UAV_FORM_REFUSED("uav_lstm_wgrad: this dgates buffer was written in tile form, which this call cannot read: %s "
                                        "(the arithmetic mode must not change between uav_lstm_bwd and uav_lstm_wgrad)", tile_refusal);
            return UAV_DG_TILE;
        }
        if (H != DgPack::H) return UAV_DG_ROWS;
        const int want = packed_now ? UAV_DG_PIECES : UAV_DG_ROWS;
        if (e && e->form != want)
            return UAV_FORM_REFUSED("uav_lstm_wgrad: this dgates buffer was written as %s but the handle's arithmetic mode / debug "
                                    "flags now read %s (they must not change between uav_lstm_bwd and uav_lstm_wgrad)",
                                    e->form == UAV_DG_PIECES ? "fp16 piece chunks" : "f32 rows", packed_now ? "fp16 piece chunks" : "f32 rows");
        // the f32-rows form reads h_prev from the stash's slot: refuse a stash whose forward pass left it out
        if (!packed_now && stash_hslot(stash) == 0)
            return UAV_FORM_REFUSED("uav_lstm_wgrad: this stash was written by uav_lstm_fwd / the stepper on the fp16-split arithmetic, "
                                    "which leaves out its h_prev slot, but the handle's arithmetic mode / debug flags now read that slot "
                                    "(they must not change between the forward pass and uav_lstm_wgrad)");
        return want;
    }
    // ---- uav_lstm_dgates_f32 reads `p`: as recorded by the call that wrote it, else by the mode
    int f32_read(const void* p, int N, int T, int H, bool packed_now) const {
        const dg_rec* e = dg(p);
        if (is_tile(e)) {
            if (e->form != UAV_DG_TILE)
                return UAV_FORM_REFUSED("uav_lstm_dgates_f32: this dgates buffer is armed for tile form (uav_lstm_dgates_tile) but no "
                                        "uav_lstm_bwd has written it since");
            if (e->N != N || e->T != T || e->H != H)
                return UAV_FORM_REFUSED("uav_lstm_dgates_f32: this dgates buffer was written in tile form for N=%d T=%d H=%d, not N=%d "
                                        "T=%d H=%d", e->N, e->T, e->H, N, T, H);
            return UAV_DG_TILE;
        }
        if (H != DgPack::H) return UAV_DG_ROWS;
        return e ? e->form : (packed_now ? UAV_DG_PIECES : UAV_DG_ROWS);
    }

    // ---- the h = 256 stashes: hslot 1 = the h_prev slot was written, 0 = left out by the fp16-split path, -1 = not recorded
    int stash_hslot(const void* stash) const {
        for (auto& x : stash_)
            if (stash && x.p == stash) return x.hslot;
        return -1;
    }
    void stash_written(const void* stash, int hslot) {       // uav_lstm_fwd: the whole stash in one call
        for (auto& x : stash_)
            if (x.p == stash) { x.hslot = hslot; return; }
        stash_[stash_next_] = stash_rec{stash, hslot};
        stash_next_ = (stash_next_ + 1) % 8;
    }
    // the stepper writes a stash one step at a time: its slot counts as written only if every step since step 0 wrote it
    void stash_step(const void* stash, int t, int hslot) { stash_written(stash, t > 0 && stash_hslot(stash) == 0 ? 0 : hslot); }
};
