// Device-side point self-test kernel ("K2", beside K1 of selftest.h): raw limbs in, canonical bytes out, so that the POINT FORMULAS AS COMPILED FOR THE GPU -- ge26.h,
// the lockstep forms of fe26x.h and mid_long.h: asm pins, v_mad_u64_u32 chains, selects as v_cndmask, operands at the top of their bound class -- are compared
// directly with big-integer arithmetic (tests/pyref_point.py), not only through the one MSM result they add up to.  Included by diag.hip (C25519_CHAIN 1) and
// finish.hip (C25519_CHAIN 0): the same source in both carry forms of fe_mul.  Every op calls the library's function, not a copy.
//   p: 40 u32 per row = X Y Z T (tight limbs); q: 40 u32 per row (null: zeros); aux: one u32 per row (null: zeros); out: 128 bytes per row = canonical X Y Z T
//   op 0: ge_dbl_p3(p)              1: ge_mul_by_pow_2(p, aux), aux in 1 .. 8
//   op 2: ge_p1p1_to_p3(ge_madd(p, aniels_from_words(w))) after aniels_words_cneg(w, aux & 1), w = q[0..24]: three canonical 255-bit values as words
//   op 3: ge_madd_signed_p3(p, q, aux & 1), q = ypx, ymx, xy2d (tight limbs)      4: ge_madd_signed_p3_lockstep, the same operands
//   op 5: ge_madd_lazy_p3(p, q, aux ? ~0 : 0)                                     6: ge_madd_lazy_p3_lockstep, the same operands
//   op 7: ge_from_aniels_signed(q, aux & 1)
//   op 8: ge_p1p1_to_p3(ge_add_cached(p, ge_cached_cneg(ge_p3_to_cached(q), aux & 1))), q a p3 (tight limbs)      9: ge_add(p, q)
//   op 10: ge_add_cached_signed_p3_lockstep(p, q, aux & 1), q = YpX, YmX, Z, T2d (tight limbs)      11: ge_add_cached_lazy_p3_lockstep(p, q, aux ? ~0 : 0)
//   op 12: sixteen ge_madd_lazy_p3_lockstep(acc, q, flip) from acc = p with the sign bookkeeping of accum.hip accumulate_body -- the sign starts at 0, me_k = bit k of
//          aux spread to a mask, flip = me ^ sgn, sgn = me -- and then its sign resolution (ge_lazy_sign_resolve): the output of one lockstep group is the wide and
//          loose operands of the next
//   op 13: ge_neg(p)
//   op 14: predicates, byte 0 of the row (the rest zero): ge_eq(p, q) | ge_is_identity(p) << 1 | ris_eq(p, q) << 2
// The device-only forms (4, 6, 10, 11, 12) exist in the device pass alone, like ops 8 - 13 of K1.
#pragma once
#include "devio.h"
#include "msm_internal.h"
#include "fe26x.h"
#include "mid_long.h"

namespace c25519 {

constexpr int SELFTEST_POINT_OPS = 15;

template <int CHAIN_TAG>
__global__ void __launch_bounds__(256) k_selftest_point(int op, const u32 *__restrict__ p, const u32 *__restrict__ q, const u32 *__restrict__ aux, u64 n, uint8_t *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    feT c[4], d[4];
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 10; j++) { c[k].v[j] = p[40 * i + 10 * k + j]; d[k].v[j] = q ? q[40 * i + 10 * k + j] : 0u; }
    const u32 x = aux ? aux[i] : 0u;
    const bool neg = (x & 1u) != 0;
    const u32 flip = x ? ~0u : 0u;
    ge_p3 P; P.X = c[0]; P.Y = c[1]; P.Z = c[2]; P.T = c[3];
    ge_p3 Q; Q.X = d[0]; Q.Y = d[1]; Q.Z = d[2]; Q.T = d[3];
    ge_aniels A; A.ypx = d[0]; A.ymx = d[1]; A.xy2d = d[2];
    ge_p3 r = P;
    switch (op) {
    case 0: r = ge_dbl_p3(P); break;
    case 1: r = ge_mul_by_pow_2(P, (int)((x - 1u) & 7u) + 1); break;      // (1 .. 8 whatever the word holds: the loop stays short)
    case 2: {
        u32 w[24];
        for (int j = 0; j < 24; j++) w[j] = q ? q[40 * i + j] : 0u;
        aniels_words_cneg(w, neg);
        r = ge_p1p1_to_p3(ge_madd(P, aniels_from_words(w)));
        break;
    }
    case 3: r = ge_madd_signed_p3(P, A, neg); break;
    case 5: r = ge_madd_lazy_p3(P, A, flip); break;
    case 7: r = ge_from_aniels_signed(A, neg); break;
    case 8: r = ge_p1p1_to_p3(ge_add_cached(P, ge_cached_cneg(ge_p3_to_cached(Q), neg))); break;
    case 9: r = ge_add(P, Q); break;
#if defined(__HIP_DEVICE_COMPILE__)
    case 4: r = ge_madd_signed_p3_lockstep(P, A, neg); break;
    case 6: r = ge_madd_lazy_p3_lockstep(P, A, flip); break;
    case 10: r = ge_add_cached_signed_p3_lockstep(P, d[0], d[1], d[2], d[3], neg); break;
    case 11: r = ge_add_cached_lazy_p3_lockstep(P, d[0], d[1], d[2], d[3], flip); break;
    case 12: {
        u32 sgn = 0;
#pragma unroll 1
        for (int k = 0; k < 16; k++) {
            const u32 me = 0u - ((x >> k) & 1u), f = me ^ sgn;
            sgn = me;
            r = ge_madd_lazy_p3_lockstep(r, A, f);
        }
        ge_lazy_sign_resolve(r, sgn);
        break;
    }
#endif
    case 13: r = ge_neg(P); break;
    case 14: {
        const u32 bits = (ge_eq(P, Q) ? 1u : 0u) | (ge_is_identity(P) ? 2u : 0u) | (ris_eq(P, Q) ? 4u : 0u);
        r.X = fe_small(bits); r.Y = fe_zero(); r.Z = fe_zero(); r.T = fe_zero();
        break;
    }
    default: break;
    }
    u32 w[8];
    fe_to_words(r.X, w); store8(out, 4 * i + 0, w);
    fe_to_words(r.Y, w); store8(out, 4 * i + 1, w);
    fe_to_words(r.Z, w); store8(out, 4 * i + 2, w);
    fe_to_words(r.T, w); store8(out, 4 * i + 3, w);
}

}  // namespace c25519
