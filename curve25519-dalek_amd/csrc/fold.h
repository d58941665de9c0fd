// The arithmetic of the random-linear-combination fold (mid_fold.hip): weights c_r, scalars s, everything an integer
// mod l on the 28-bit limbs of sc28.h.
//   fold_step     acc + c * s mod l    one element of a column sum t_j = sum_r c_r * s[r][j]
//   fold_scale    c * d mod l          one dynamic scalar d'_i = c_row(i) * d_i
//   fold_combine  a + b mod l          two partial column sums (row slices, row phases of a block)
// The operands of the products are ANY 32-byte integers (and any 16-byte weight): the product reduces them, so nothing is refused for bit 255
// and every result is canonical (< l).  Sums of canonical values are exact mod l in any order, so the kernels add partial sums in whatever
// order their geometry gives.  WB: bytes of a weight, 16 (a 128-bit z_i, ed25519-dalek/src/batch.rs:207-233: sc28_mul_5x10) or 32 (sc28_mul).
// Host + device (tests/test_precomp_fold_host.py fuzzes it against big integers through tests/host/fold_host.cpp).
#pragma once
#include "sc28.h"

namespace c25519 {

template <int WB> struct fold_weight { u32 v[WB == 16 ? 5 : 10]; };      // 28-bit limbs of a weight: five hold 140 bits, ten 280
// WB / 4 little-endian words -> limbs
template <int WB>
C25519_HD fold_weight<WB> fold_weight_from_words(const u32 *w) {
    static_assert(WB == 16 || WB == 32, "a weight has 16 or 32 bytes");
    fold_weight<WB> c;
    sc28_limbs_from_words<WB / 4, (WB == 16 ? 5 : 10)>(w, c.v);
    return c;
}
// c * s mod l, s eight little-endian words of any value (16-byte weight: the product is < 2^384, inside what sc28_mul_5x10 folds -- hi < 2^132
// there; 32-byte weight: < 2^512, the bound of sc28_mul)
template <int WB>
C25519_HD sc28 fold_scale(const fold_weight<WB> &c, const u32 s[8]) {
    const sc28 b = sc28_from_words(s);
    if constexpr (WB == 16) return sc28_mul_5x10(c.v, b.v);
    else return sc28_mul(c.v, b.v);
}
template <int WB>
C25519_HD sc28 fold_step(const sc28 &acc, const fold_weight<WB> &c, const u32 s[8]) { return sc28_add(acc, fold_scale<WB>(c, s)); }
// canonical operands
C25519_HD sc28 fold_combine(const sc28 &a, const sc28 &b) { return sc28_add(a, b); }

}  // namespace c25519
