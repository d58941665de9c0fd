// Host build of the fold arithmetic the kernels of csrc/mid_fold.hip run (csrc/fold.h is __host__ __device__), so that it can be fuzzed against
// big integers on a machine with no GPU.  Test-only: built by tests/test_precomp_fold_host.py into tests/host/libfoldhost.so.
#include "../../curve25519-dalek_amd/csrc/fold.h"
#include <string.h>
using namespace c25519;

static sc28 load(const uint8_t *b) { u32 w[8]; memcpy(w, b, 32); return sc28_from_words(w); }
static void store(uint8_t *b, const sc28 &a) { u32 w[8]; sc28_to_words(a, w); memcpy(b, w, 32); }

template <int WB>
static sc28 step(const sc28 &acc, const uint8_t *c, const uint8_t *s) {
    u32 cw[WB / 4], sw[8];
    memcpy(cw, c, WB); memcpy(sw, s, 32);
    return fold_step<WB>(acc, fold_weight_from_words<WB>(cw), sw);
}
template <int WB>
static sc28 scale(const uint8_t *c, const uint8_t *s) {
    u32 cw[WB / 4], sw[8];
    memcpy(cw, c, WB); memcpy(sw, s, 32);
    return fold_scale<WB>(fold_weight_from_words<WB>(cw), sw);
}

extern "C" {
// wb: 16 or 32 bytes per weight.  acc: canonical (< l)
void h_fold_step(int wb, const uint8_t *acc, const uint8_t *c, const uint8_t *s, uint8_t *o) { store(o, wb == 16 ? step<16>(load(acc), c, s) : step<32>(load(acc), c, s)); }
void h_fold_scale(int wb, const uint8_t *c, const uint8_t *s, uint8_t *o) { store(o, wb == 16 ? scale<16>(c, s) : scale<32>(c, s)); }
void h_fold_combine(const uint8_t *a, const uint8_t *b, uint8_t *o) { store(o, fold_combine(load(a), load(b))); }
// one column of m rows (weights m x wb, scalars m x 32) cut into `slices` runs of ceil(m / slices) rows, each folded from zero by fold_step,
// the partial sums joined by fold_combine: what k_mid_fold_part and k_mid_fold_finish do with a column
void h_fold_column(int wb, const uint8_t *c, const uint8_t *s, uint64_t m, uint64_t slices, uint8_t *o) {
    const uint64_t rows = (m + slices - 1) / slices;          // slices >= 1; a slice past the last row is empty: zero
    sc28 total = sc28_zero();
    for (uint64_t y = 0; y < slices; y++) {
        sc28 acc = sc28_zero();
        for (uint64_t r = y * rows; r < m && r < (y + 1) * rows; r++) acc = wb == 16 ? step<16>(acc, c + r * 16, s + r * 32) : step<32>(acc, c + r * 32, s + r * 32);
        total = fold_combine(total, acc);
    }
    store(o, total);
}
}
