// The buffer-form rules of csrc/lstm_forms.h, exercised on the CPU: plain C++17, no HIP header, no device.  Built and run by
// tests/test_lstm_forms_host.py under AddressSanitizer + UBSan; exits 0 when every rule holds, else prints the line and exits 1.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "lstm_forms.h"

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

int main() {
    tile_capacity();
    tile_write_and_read();
    failed_writes_leave_nothing();
    one_record_per_pointer();
    ring_of_eight();
    reads_at_h256();
    stash_slots();
    layouts();
    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("lstm_forms: all checks passed\n");
    return g_failed ? 1 : 0;
}
