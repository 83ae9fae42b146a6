// The buffer-form rules and the mode table of csrc/lstm_forms.h and the workspace carve of csrc/scratch.h, exercised on the CPU:
// plain C++17, no HIP header, no device.  Built and run by
// tests/test_lstm_forms_host.py under AddressSanitizer + UBSan; exits 0 when every rule holds, else prints the line and exits 1.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lstm_forms.h"
#include "scratch.h"

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

static char g_err[512];                                       // the library's uav_set_error (ctx.hip), for this program
void uav_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static char g_mem[64];                                        // distinct addresses to stand for device buffers; never dereferenced
static const void* buf(int i) { return g_mem + i; }
static bool says(int form, const char* text) { return form < 0 && strstr(g_err, text) != nullptr; }     // refused, and why

// a whole successful uav_lstm_bwd as the entry point drives it: `wrote` is what the kernels of that H write when not tile
static int bwd(uav_lstm_forms& f, const void* p, int N, int T, int H, bool dx, int wrote, bool ok = true) {
    const int form = f.bwd_begin(p, N, T, H, dx);
    if (form >= 0) f.bwd_end(p, form == UAV_DG_TILE ? UAV_DG_TILE : wrote, ok);
    return form;
}

static void tile_capacity() {
    uav_lstm_forms f{};
    for (int i = 0; i < 8; ++i) CHECK(f.arm(buf(i), 16, 32, 64) >= 0);
    const int ninth = f.arm(buf(8), 16, 32, 64);
    CHECK(says(ninth, "uav_lstm_dgates_tile: eight other buffers of this handle are armed for or written in tile form; "
                      "uav_lstm_dgates_forget one of them first"));
    CHECK(f.form(buf(8)) == UAV_DG_ROWS);
    CHECK(f.arm(buf(3), 16, 32, 64) >= 0);                   // arming again reuses the buffer's own record
    for (int i = 0; i < 20; ++i) bwd(f, buf(20 + i), 64, 8, 256, false, UAV_DG_PIECES);     // 20 pieces records on other pointers
    for (int i = 0; i < 8; ++i) CHECK(f.form(buf(i)) == UAV_DG_TILE_ARMED);
    CHECK(f.arm(buf(8), 16, 32, 64) < 0);
    f.forget(buf(0));
    CHECK(f.form(buf(0)) == UAV_DG_ROWS);
    CHECK(f.arm(buf(8), 16, 32, 64) >= 0 && f.form(buf(8)) == UAV_DG_TILE_ARMED);
    // a written record is kept like an armed one
    CHECK(bwd(f, buf(8), 16, 32, 64, false, -1) == UAV_DG_TILE && f.form(buf(8)) == UAV_DG_TILE);
    for (int i = 0; i < 20; ++i) bwd(f, buf(20 + i), 64, 8, 256, false, UAV_DG_ROWS);
    CHECK(f.form(buf(8)) == UAV_DG_TILE && f.arm(buf(0), 16, 32, 64) < 0);
}

static void tile_write_and_read() {
    uav_lstm_forms f{};
    const void* p = buf(0);
    CHECK(f.arm(p, 16, 32, 64) >= 0);
    // merely armed: nobody reads it
    CHECK(says(f.wgrad_read(p, buf(1), 16, 32, 64, false, false, nullptr), "is armed for tile form (uav_lstm_dgates_tile) but no uav_lstm_bwd has written it since"));
    CHECK(says(f.f32_read(p, 16, 32, 64, false), "uav_lstm_dgates_f32: this dgates buffer is armed for tile form"));
    // armed for another call: refused, and still armed
    CHECK(says(bwd(f, p, 16, 64, 64, false, -1), "is armed for tile form at N=16 T=32 H=64 without dx (uav_lstm_dgates_tile), not for this call"));
    CHECK(says(bwd(f, p, 16, 32, 64, true, -1), "not for this call") && f.form(p) == UAV_DG_TILE_ARMED);
    // armed -> written -> read at the recorded shape
    CHECK(bwd(f, p, 16, 32, 64, false, -1) == UAV_DG_TILE && f.form(p) == UAV_DG_TILE);
    CHECK(f.wgrad_read(p, buf(1), 16, 32, 64, false, false, nullptr) == UAV_DG_TILE);
    CHECK(f.f32_read(p, 16, 32, 64, false) == UAV_DG_TILE);
    CHECK(says(f.wgrad_read(p, buf(1), 17, 32, 64, false, false, nullptr), "written in tile form for N=16 T=32 H=64, which this call (N=17 T=32 H=64) would read as f32 rows"));
    CHECK(says(f.wgrad_read(p, buf(1), 16, 16, 64, false, false, nullptr), "which this call (N=16 T=16 H=64) would read as f32 rows"));
    CHECK(says(f.wgrad_read(p, buf(1), 16, 32, 128, false, false, nullptr), "which this call (N=16 T=32 H=128) would read as f32 rows"));
    CHECK(says(f.wgrad_read(p, buf(1), 16, 32, 64, true, false, nullptr), "which this call (N=16 T=32 H=64, dx) would read as f32 rows"));
    CHECK(says(f.wgrad_read(p, buf(1), 16, 32, 64, false, false, "the exact-f32 kernels read rows"),
               "written in tile form, which this call cannot read: the exact-f32 kernels read rows (the arithmetic mode must not change"));
    CHECK(says(f.f32_read(p, 16, 16, 64, false), "written in tile form for N=16 T=32 H=64, not N=16 T=16 H=64"));
    CHECK(f.form(p) == UAV_DG_TILE);                          // a refused read changes nothing
    // one arming serves one call: a rows-form write on the pointer drops the written record
    CHECK(bwd(f, p, 16, 32, 64, false, -1) == UAV_DG_ROWS && f.form(p) == UAV_DG_ROWS);
    CHECK(f.wgrad_read(p, buf(1), 16, 32, 64, false, false, nullptr) == UAV_DG_ROWS);
    CHECK(f.f32_read(p, 16, 32, 64, false) == UAV_DG_ROWS);
}

static void failed_writes_leave_nothing() {
    uav_lstm_forms f{};
    CHECK(f.arm(buf(0), 16, 32, 64) >= 0);
    CHECK(bwd(f, buf(0), 16, 32, 64, false, -1, false) == UAV_DG_TILE);      // the kernels were to write tile form and failed
    CHECK(f.form(buf(0)) == UAV_DG_ROWS);
    CHECK(f.wgrad_read(buf(0), buf(9), 16, 32, 64, false, false, nullptr) == UAV_DG_ROWS);
    bwd(f, buf(1), 64, 8, 256, false, UAV_DG_PIECES, false);
    CHECK(f.form(buf(1)) == UAV_DG_ROWS);
    CHECK(f.wgrad_read(buf(1), buf(9), 64, 8, 256, false, false, nullptr) >= 0);   // "not recorded": follows the mode, here rows
    // ... also where an earlier call had recorded the pointer
    bwd(f, buf(1), 64, 8, 256, false, UAV_DG_PIECES);
    bwd(f, buf(1), 64, 8, 256, false, UAV_DG_PIECES, false);
    CHECK(f.form(buf(1)) == UAV_DG_ROWS && f.wgrad_read(buf(1), buf(9), 64, 8, 256, false, false, nullptr) >= 0);
}

static void one_record_per_pointer() {
    uav_lstm_forms f{};
    const void* p = buf(0);
    bwd(f, p, 64, 8, 256, false, UAV_DG_PIECES);
    CHECK(f.form(p) == UAV_DG_PIECES);
    CHECK(f.arm(p, 16, 32, 64) >= 0 && f.form(p) == UAV_DG_TILE_ARMED);
    CHECK(bwd(f, p, 16, 32, 64, false, -1) == UAV_DG_TILE && f.form(p) == UAV_DG_TILE);
    f.forget(p);
    CHECK(f.form(p) == UAV_DG_ROWS);                          // not the pieces of three calls ago
    // and the other way round: a pieces write replaces a written tile record, which then takes no tile slot
    CHECK(f.arm(p, 16, 32, 64) >= 0 && bwd(f, p, 16, 32, 64, false, -1) == UAV_DG_TILE);
    CHECK(bwd(f, p, 64, 8, 256, false, UAV_DG_PIECES) == UAV_DG_ROWS && f.form(p) == UAV_DG_PIECES);
    for (int i = 1; i <= 8; ++i) CHECK(f.arm(buf(i), 16, 32, 64) >= 0);
    f.forget(p);                                              // forget drops tile records only
    CHECK(f.form(p) == UAV_DG_PIECES);
}

static void ring_of_eight() {
    uav_lstm_forms f{};
    bwd(f, buf(0), 64, 8, 256, false, UAV_DG_PIECES);
    bwd(f, buf(0), 64, 8, 256, false, UAV_DG_PIECES);         // recording a pointer twice does not consume two slots
    for (int i = 1; i < 8; ++i) bwd(f, buf(i), 64, 8, 256, false, UAV_DG_PIECES);
    for (int i = 0; i < 8; ++i) CHECK(f.form(buf(i)) == UAV_DG_PIECES);
    bwd(f, buf(8), 64, 8, 256, false, UAV_DG_PIECES);         // the ninth pointer evicts the oldest
    CHECK(f.form(buf(0)) == UAV_DG_ROWS);
    CHECK(f.f32_read(buf(0), 64, 8, 256, false) == UAV_DG_ROWS && f.f32_read(buf(0), 64, 8, 256, true) == UAV_DG_PIECES);
    for (int i = 1; i <= 8; ++i) CHECK(f.form(buf(i)) == UAV_DG_PIECES);
}

static void reads_at_h256() {
    uav_lstm_forms f{};
    const void *pc = buf(0), *rows = buf(1), *fresh = buf(2), *stash = buf(3);
    bwd(f, pc, 64, 8, 256, false, UAV_DG_PIECES);
    bwd(f, rows, 64, 8, 256, false, UAV_DG_ROWS);
    CHECK(f.wgrad_read(pc, stash, 64, 8, 256, false, true, nullptr) == UAV_DG_PIECES);
    CHECK(says(f.wgrad_read(pc, stash, 64, 8, 256, false, false, nullptr), "was written as fp16 piece chunks but the handle's arithmetic mode / debug flags now read f32 rows"));
    CHECK(f.wgrad_read(rows, stash, 64, 8, 256, false, false, nullptr) == UAV_DG_ROWS);
    CHECK(says(f.wgrad_read(rows, stash, 64, 8, 256, false, true, nullptr), "was written as f32 rows but the handle's arithmetic mode / debug flags now read fp16 piece chunks"));
    CHECK(f.wgrad_read(fresh, stash, 64, 8, 256, false, true, nullptr) == UAV_DG_PIECES);     // unrecorded: follows the mode
    CHECK(f.wgrad_read(fresh, stash, 64, 8, 256, false, false, nullptr) == UAV_DG_ROWS);
    // uav_lstm_dgates_f32 reads what was recorded whatever the mode says now
    CHECK(f.f32_read(pc, 64, 8, 256, false) == UAV_DG_PIECES && f.f32_read(rows, 64, 8, 256, true) == UAV_DG_ROWS);
    CHECK(f.f32_read(fresh, 64, 8, 256, true) == UAV_DG_PIECES && f.f32_read(fresh, 64, 8, 256, false) == UAV_DG_ROWS);
    // other hidden sizes have rows only, whatever an h = 256 call once left on the pointer
    CHECK(f.wgrad_read(pc, stash, 64, 8, 32, false, false, nullptr) == UAV_DG_ROWS && f.f32_read(pc, 64, 8, 32, false) == UAV_DG_ROWS);
}

static void stash_slots() {
    uav_lstm_forms f{};
    const void *dg = buf(0), *stash = buf(1);
    const char* left_out = "this stash was written by uav_lstm_fwd / the stepper on the fp16-split arithmetic, which leaves out its h_prev slot";
    CHECK(f.stash_hslot(stash) == -1);
    CHECK(f.wgrad_read(dg, stash, 64, 8, 256, false, false, nullptr) >= 0);       // an unrecorded stash is accepted
    f.stash_written(stash, 0);                                                      // uav_lstm_fwd on the packed mode
    CHECK(says(f.wgrad_read(dg, stash, 64, 8, 256, false, false, nullptr), left_out));
    CHECK(f.wgrad_read(dg, stash, 64, 8, 256, false, true, nullptr) >= 0);        // the pieces path does not read the slot
    f.stash_written(stash, 1);
    CHECK(f.wgrad_read(dg, stash, 64, 8, 256, false, false, nullptr) >= 0);
    // the stepper: written only if every step since step 0 wrote it
    f.stash_step(stash, 0, 0);
    f.stash_step(stash, 1, 1);
    CHECK(f.stash_hslot(stash) == 0 && says(f.wgrad_read(dg, stash, 64, 8, 256, false, false, nullptr), left_out));
    f.stash_step(stash, 0, 1);                                                      // step 0 replaces the record
    CHECK(f.stash_hslot(stash) == 1);
    f.stash_step(stash, 1, 1);
    CHECK(f.stash_hslot(stash) == 1);
    f.stash_step(stash, 2, 0);
    f.stash_step(stash, 3, 1);
    CHECK(f.stash_hslot(stash) == 0);
    f.stash_step(buf(2), 5, 1);                                                     // a stash first seen mid-sequence: as the step wrote it
    CHECK(f.stash_hslot(buf(2)) == 1);
    // eight slots, the oldest makes room; a stash recorded twice keeps one
    for (int i = 0; i < 7; ++i) f.stash_written(buf(10 + i), 0);
    f.stash_written(buf(10), 0);
    CHECK(f.stash_hslot(stash) == -1 && f.stash_hslot(buf(2)) == 1);
    f.stash_written(buf(17), 0);
    CHECK(f.stash_hslot(buf(2)) == -1 && f.stash_hslot(buf(10)) == 0);
}

static void layouts() {
    CHECK(DgTile::row(0, 0, 32) == 0 && DgTile::row(15, 0, 32) == 15 && DgTile::row(0, 1, 32) == 16 && DgTile::row(17, 3, 32) == (32 + 3) * 16 + 1);
    CHECK(DgTile::rows(17, 32) == 2 * 16 * 32 && DgTile::bytes(17, 32, 64) == (size_t)32 * 32 * 4 * 64 * 4);
    const DgPack P(65, 8);
    CHECK(P.NP == 128 && P.RT == 8 && P.bytes() == (size_t)128 * 8 * 4 * 256 * 4 + 2 * (size_t)8 * 128 * 4);
}

// ---- uav_lstm_mode: 3 arithmetics x the 16 combinations of the four debug bits x H in {64, 96, 128, 256} x I in {6, 256}.
// The expected values are literals written out from the rules: the step path runs at H = 256 on fp16x3 without STEP_F32; its
// gate gradients are packed without DG_F32; its BPTT takes dheads (2), and with I = H also fuses dx (1) and stacks (4);
// X_F32 and GEMM_TN_OFF decide nothing but x_pieces / gemm_tn.
static void mode_table() {
    static_assert(UAV_DEBUG_STEP_F32 == 1u && UAV_DEBUG_X_F32 == 2u && UAV_DEBUG_DG_F32 == 4u && UAV_DEBUG_GEMM_TN_OFF == 0x10u, "the rows below");
    static_assert(UAV_BWD_FUSES_DX == 1 && UAV_BWD_TAKES_DHEADS == 2 && UAV_BWD_STACKS == 4, "the caps below");
    struct row { unsigned flags; bool step, packed; int caps_i6, caps_i256; bool x_pieces, gemm_tn; };
    static const row fp16x3_h256[16] = {          // what UAV_ARITH_FP16X3 decides at H = 256
        {0x00u, true, true, 2, 7, true, true},     {0x01u, false, false, 0, 0, true, true},
        {0x02u, true, true, 2, 7, false, true},    {0x03u, false, false, 0, 0, false, true},
        {0x04u, true, false, 2, 7, true, true},    {0x05u, false, false, 0, 0, true, true},
        {0x06u, true, false, 2, 7, false, true},   {0x07u, false, false, 0, 0, false, true},
        {0x10u, true, true, 2, 7, true, false},    {0x11u, false, false, 0, 0, true, false},
        {0x12u, true, true, 2, 7, false, false},   {0x13u, false, false, 0, 0, false, false},
        {0x14u, true, false, 2, 7, true, false},   {0x15u, false, false, 0, 0, true, false},
        {0x16u, true, false, 2, 7, false, false},  {0x17u, false, false, 0, 0, false, false},
    };
    const int arith[3] = {UAV_ARITH_FP16X3, UAV_ARITH_BF16X6, UAV_ARITH_F32_MFMA}, Hs[4] = {64, 96, 128, 256}, Is[2] = {6, 256};
    int cases = 0;
    for (int a : arith)
        for (const row& r : fp16x3_h256)
            for (int H : Hs)
                for (int I : Is) {
                    const uav_lstm_mode m{a, r.flags};
                    const bool here = a == UAV_ARITH_FP16X3 && H == 256;      // every other arithmetic, every other H: nothing
                    CHECK(m.f32_mfma() == (a == 2) && m.bf16x6() == (a == 1));
                    CHECK(m.step_path(H) == (here ? r.step : false));
                    CHECK(m.dg_packed(H) == (here ? r.packed : false));
                    CHECK(m.bwd_caps(I, H) == (here ? (I == 6 ? r.caps_i6 : r.caps_i256) : 0));
                    CHECK(m.x_pieces() == r.x_pieces && m.gemm_tn() == r.gemm_tn);
                    ++cases;
                }
    CHECK(cases == 3 * 16 * 4 * 2);
    // the issue's examples, spelled out
    CHECK((uav_lstm_mode{UAV_ARITH_FP16X3, 0u}.bwd_caps(256, 256)) == (UAV_BWD_TAKES_DHEADS | UAV_BWD_FUSES_DX | UAV_BWD_STACKS));
    CHECK((uav_lstm_mode{UAV_ARITH_BF16X6, 0u}.bwd_caps(256, 256)) == 0 && (uav_lstm_mode{UAV_ARITH_F32_MFMA, 0u}.bwd_caps(256, 256)) == 0);
    CHECK((uav_lstm_mode{UAV_ARITH_FP16X3, UAV_DEBUG_STEP_F32}.bwd_caps(256, 256)) == 0 && !(uav_lstm_mode{UAV_ARITH_FP16X3, UAV_DEBUG_STEP_F32}.dg_packed(256)));
    CHECK((uav_lstm_mode{UAV_ARITH_FP16X3, UAV_DEBUG_DG_F32}.step_path(256)) && !(uav_lstm_mode{UAV_ARITH_FP16X3, UAV_DEBUG_DG_F32}.dg_packed(256)));
}

// ---- uav_scratch::carve against the seven tail computations it replaced, each written here as its call site wrote it by hand
// (`ws` + `ws_bytes` arithmetic, its own required front), on a 256 MiB workspace that is never touched.
template <class T>
static void carve_is(const uav_scratch& w, size_t n, size_t front, const T* want_tail, size_t want_front_bytes) {
    T* tail = nullptr;
    const uav_scratch f = w.carve(n, front, &tail);
    CHECK(tail == want_tail && f.p == w.p && f.bytes == want_front_bytes && f.num_cu == w.num_cu);
}
static void carve_sites(char* ws, size_t ws_bytes, int N, int T, int H, int I, size_t h3_total) {
    const uav_scratch w{ws, ws_bytes, 256};
    const size_t slack = 64u << 20;
    {   // mlp.hip, uav_mlp_bwd: the column-reduction scratch behind the split-K slabs
        const size_t red_floats = (size_t)512 * 2 * 512 + 2 * 512 + 1024 * 512;
        carve_is(w, red_floats * sizeof(float), (size_t)(1 << 18) * sizeof(float), (float*)((char*)ws + ws_bytes) - red_floats,
                 ws_bytes - red_floats * sizeof(float));
    }
    {   // lstm_api.hip, LstmWgrad::split_workspace, then ::rows' f32 copy of packed gate gradients + h_prev in front of it
        const size_t red_floats = (size_t)1024 * 9 * 4 * H + 64;
        carve_is(w, red_floats * sizeof(float), red_floats * sizeof(float), (float*)((char*)ws + ws_bytes) - red_floats,
                 ws_bytes - red_floats * sizeof(float));
        float* red;
        const uav_scratch sub = w.carve(red_floats * sizeof(float), red_floats * sizeof(float), &red);
        const size_t f32_bytes = (size_t)N * T * 5 * H * sizeof(float);
        carve_is(sub, f32_bytes, slack, (float*)((char*)sub.p + sub.bytes - f32_bytes), sub.bytes - f32_bytes);
        CHECK((char*)red - (sub.p + sub.bytes - f32_bytes) == (ptrdiff_t)f32_bytes);        // the rows end where `red` begins
    }
    {   // lstm_generic.hip, forward and backward: the recurrent state / its gradient, 2 N H floats
        const int64_t NH = (int64_t)N * H;
        carve_is(w, (size_t)(2 * NH) * sizeof(float), slack, (float*)((char*)ws + ws_bytes) - 2 * NH, ws_bytes - 2 * NH * sizeof(float));
    }
    {   // wgrad_pc.hip, lstm_pc_wgrad: 256 blocks' partial sums (1 + CI columns of 4 * 256 values) + the max-scale word's 64 floats
        const int CI = I == 256 ? 0 : I;
        const size_t part_floats = (size_t)256 * (1 + CI) * 1024 + 64;
        carve_is(w, part_floats * 4, slack, (float*)((char*)ws + ws_bytes) - part_floats, ws_bytes - part_floats * 4);
    }
    {   // lstm_h3.hip, lstm_h3_fwd: the layer state (H3Layout::total, worked out by hand as in test_lstm_h3_layout_host.py); the
        // x piece planes lie in front of it, in what the front leaves over the slack
        carve_is(w, h3_total, slack, (char*)ws + ws_bytes - h3_total, ws_bytes - h3_total);
        char* base;
        CHECK(w.carve(h3_total, slack, &base).bytes - slack == ws_bytes - h3_total - slack);
    }
}
static void scratch_carving() {
    const size_t W = (size_t)256 << 20;
    char* ws = (char*)malloc(W);
    CHECK(ws != nullptr);
    if (!ws) return;
    carve_sites(ws, W, 64, 8, 256, 256, 2363392);            // N = 64, I = 256: 2 * 65536 + 2 * 65536 + 1048576 + 1048576 + 4096
    carve_sites(ws, W, 16, 8, 64, 6, 1347584);               // N = 16, I = 6:   2 * 16384 + 2 * 65536 + 1048576 + 131072 + 4096
    const uav_scratch w{ws, W, 256};
    float* t = (float*)ws;
    // refused: more than the slice; the slice exactly but a byte of front asked for; n and front that only together exceed it
    CHECK(w.carve(W + 1, 0, &t).p == nullptr && t == nullptr);
    t = (float*)ws;
    CHECK(w.carve(W, 1, &t).p == nullptr && t == nullptr);
    t = (float*)ws;
    CHECK(w.carve(W / 2 + 4, W / 2, &t).p == nullptr && t == nullptr && w.carve(W / 2 + 4, W / 2, &t).bytes == 0);
    CHECK(w.carve((size_t)-1, (size_t)-1, &t).p == nullptr);                        // no wrap-around in n + front
    // exactly fitting: granted
    CHECK(w.carve(W / 2, W / 2, &t).p == ws && (char*)t == ws + W / 2);
    CHECK(w.carve(W, 0, &t).p == ws && (char*)t == ws && w.carve(W, 0, &t).bytes == 0);
    // a zero-byte carve returns the slice unchanged
    const uav_scratch z = w.carve(0, 0, &t);
    CHECK(z.p == w.p && z.bytes == w.bytes && z.num_cu == w.num_cu && (char*)t == ws + W);
    // the small workspace the entry points refuse: 1 MiB against the 64 MiB the GEMM slabs are promised
    const uav_scratch small{ws, (size_t)1 << 20, 256};
    CHECK(small.carve(4096, 64u << 20, &t).p == nullptr);
    free(ws);
}

int main() {
    tile_capacity();
    tile_write_and_read();
    failed_writes_leave_nothing();
    one_record_per_pointer();
    ring_of_eight();
    reads_at_h256();
    stash_slots();
    layouts();
    mode_table();
    scratch_carving();
    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("lstm_forms: all checks passed\n");
    return g_failed ? 1 : 0;
}
