// Lizard encoding on the fe26 / ge26 layers (host + device), one item per lane, step for step the reference's
// curve25519-dalek/src/lizard/ (the `lizard` feature, D = Sha256):
//
//   lizard_encode                      RistrettoPoint::lizard_encode::<Sha256> (lizard_ristretto.rs:25-42)
//   ris_to_jacobi_quartic              RistrettoPoint::to_jacobi_quartic_ristretto (lizard_ristretto.rs:124-206)
//   jacobi_e_inv_positive              JacobiPoint::e_inv_positive (jacobi_quartic.rs:28-67); dual (:69-74) is a negation of S and T
//   lizard_candidate                   slot c (0..7) of elligator_ristretto_flavor_inverse (lizard_ristretto.rs:81-120)
//   lizard_decode                      RistrettoPoint::lizard_decode::<Sha256> (lizard_ristretto.rs:46-75), hashing 8 candidates
//
// Straight-line: no branch and no address depends on a payload byte or a coordinate.  The candidates are visited by a uniform
// loop (c = 0..7, an SGPR counter) and the Jacobi point of slot c is picked by selects on c, so no register array is indexed at
// run time (such an array would live in scratch).  Everything is computed on the coordinates as given, without normalising
// (X:Y:Z): the SLOT ORDER of map_to_curve_inverse depends on the projective representative, the set of
// preimages and the result of lizard_decode do not.
#pragma once
#include "h2c.h"
#include "sha256.h"

namespace c25519 {

struct jacobi_pt { feT S, T; };
struct jacobi4 { jacobi_pt J0, J1, J2, J3; };

// ---- lizard_encode: SHA-256(data) with the payload spliced into bytes 8..24, b[0] &= 0xFE, b[31] &= 0x3F, then map_to_curve ----
C25519_HD void lizard_tagged_words(const u32 data[4], u32 w[8]) {
    sha256_16(data, w);
    for (int j = 0; j < 4; j++) w[2 + j] = data[j];
    w[0] &= 0xFFFFFFFEu;
    w[7] &= 0x3FFFFFFFu;
}
C25519_HD ge_p3 lizard_encode(const u32 data[4]) {
    u32 w[8];
    lizard_tagged_words(data, w);
    return ris_map_words(w);
}

// ---- the four Jacobi quartic points of the four Edwards representatives of P (lizard_ristretto.rs:124-206) --------------
C25519_HD jacobi4 ris_to_jacobi_quartic(const ge_p3 &P) {
    const u32 c_md[10] = C25519_LIZARD_MDOUBLE_INVSQRT_A_MINUS_D_26, c_mid[10] = C25519_LIZARD_MIDOUBLE_INVSQRT_A_MINUS_D_26,
              c_mis[10] = C25519_LIZARD_MINVSQRT_ONE_PLUS_D_26;
    const feT one = fe_one(), mdouble = fe_const(c_md);
    const feT x2 = fe_sq(P.X), y2 = fe_sq(P.Y), y4 = fe_sq(y2), z2 = fe_sq(P.Z);
    const feL z_min_y = fe_sub(P.Z, P.Y), z_pl_y = fe_add(P.Z, P.Y);
    const feT z2_min_y2 = fe_carry(fe_sub(z2, y2));
    feT gamma;                                                          // 1/sqrt(Y^4 X^2 (Z^2 - Y^2)); 0 when X = 0 or Y = 0
    fe_invsqrt(gamma, fe_mul(fe_mul(y4, x2), z2_min_y2));
    const feT den = fe_mul(gamma, y2);
    const feT s_over_x = fe_mul(den, z_min_y), sp_over_xp = fe_mul(den, z_pl_y);
    jacobi4 r;
    r.J0.S = fe_mul(s_over_x, P.X);
    r.J1.S = fe_mul(fe_neg(sp_over_xp), P.X);
    const feT tmp = fe_mul(mdouble, P.Z);                               // -2/sqrt(-d-1) Z
    r.J0.T = fe_mul(tmp, s_over_x);
    r.J1.T = fe_mul(tmp, sp_over_xp);
    const feT den2 = fe_mul(fe_mul(fe_neg(z2_min_y2), fe_const(c_mis)), gamma);   // -1/sqrt(1+d) (Y^2 - Z^2) gamma
    // the same with (X, Y, Z) = (Y, X, iZ)
    const feT iz = fe_mul(fe_sqrtm1(), P.Z);
    const feT s_over_y = fe_mul(den2, fe_sub(iz, P.X)), sp_over_yp = fe_mul(den2, fe_add(iz, P.X));
    r.J2.S = fe_mul(s_over_y, P.Y);
    r.J3.S = fe_mul(fe_neg(sp_over_yp), P.Y);
    const feT tmp2 = fe_mul(mdouble, iz);
    r.J2.T = fe_mul(tmp2, s_over_y);
    r.J3.T = fe_mul(tmp2, sp_over_yp);
    // X = 0 or Y = 0: (0, 1), (1, -2i/sqrt(-d-1)), (-1, -2i/sqrt(-d-1)); s_i = t_i = 0 there before the selects
    const lanemask xy0 = lane_mask(fe_is_zero(P.X) | fe_is_zero(P.Y));
    const feT mid = fe_const(c_mid);
    r.J0.T = fe_select_m(r.J0.T, one, xy0);
    r.J1.T = fe_select_m(r.J1.T, one, xy0);
    r.J2.T = fe_select_m(r.J2.T, mid, xy0);
    r.J3.T = fe_select_m(r.J3.T, mid, xy0);
    r.J2.S = fe_select_m(r.J2.S, one, xy0);
    r.J3.S = fe_select_m(r.J3.S, fe_minus_one(), xy0);
    return r;
}

// ---- JacobiPoint::e_inv_positive: the non-negative x with e(x) = (S, T), if it exists (jacobi_quartic.rs:28-67) -----------
C25519_HD bool jacobi_e_inv_positive(const feT &S, const feT &T, feT &out) {
    const u32 c_sid[10] = C25519_LIZARD_SQRT_ID_26, c_dp[10] = C25519_LIZARD_DP1_OVER_DM1_26;
    const feT one = fe_one();
    // s = 0: t = 1 -> sqrt(i d), else 0 (t = -1)
    const bool s_is_zero = fe_is_zero(S);
    out = fe_select(fe_zero(), fe_const(c_sid), fe_eq(T, one));
    const feT a = fe_mul(fe_add(T, one), fe_const(c_dp));              // (t + 1) (d + 1)/(d - 1)
    const feT a2 = fe_sq(a);
    const feT s2 = fe_sq(S), s4 = fe_sq(s2);
    feT y;                                                              // 1/sqrt(i (s^4 - a^2))
    const bool sq = fe_invsqrt(y, fe_mul(fe_sub(s4, a2), fe_sqrtm1()));
    const bool is_defined = s_is_zero | sq, done = s_is_zero | !sq;
    const feT pms2 = fe_cneg(s2, fe_is_negative(S) != 0);
    feT x = fe_mul(fe_add(a, pms2), y);                                 // (a + sign(s) s^2) y, then the positive one
    x = fe_cneg(x, fe_is_negative(x) != 0);
    out = fe_select(out, x, !done);
    return is_defined;
}

// slot c (0..7) of elligator_ristretto_flavor_inverse: Jacobi point c/2, its dual when c is odd; slot 8 + c is the negation.
// c is uniform across the wave (a loop counter): the picks are selects on c, not an indexed array.
C25519_HD bool lizard_candidate(const jacobi4 &J, int c, feT &x) {
    const lanemask hi = lane_mask((c & 4) != 0), odd_pair = lane_mask((c & 2) != 0);
    const feT Sa = fe_select_m(J.J0.S, J.J1.S, odd_pair), Ta = fe_select_m(J.J0.T, J.J1.T, odd_pair);
    const feT Sb = fe_select_m(J.J2.S, J.J3.S, odd_pair), Tb = fe_select_m(J.J2.T, J.J3.T, odd_pair);
    feT S = fe_select_m(Sa, Sb, hi), T = fe_select_m(Ta, Tb, hi);
    const lanemask dual = lane_mask((c & 1) != 0);
    S = fe_select_m(S, fe_carry(fe_neg(S)), dual);
    T = fe_select_m(T, fe_carry(fe_neg(T)), dual);
    return jacobi_e_inv_positive(S, T, x);
}

// ---- lizard_decode::<Sha256> on 8 hashes --------------------------------------------------------------------------------
// The reference hashes all 16 candidates.  A defined negative candidate (slot 8 + c) is p - x_c with x_c even, hence odd, and its
// byte 0 fails the check (expected_bytes[0] &= 0xFE) -- unless x_c = 0, when it is x_c itself and matches exactly when slot c does.
// Undefined slots never count (is_some() is false).  So n_found = sum_c match_c (1 + [x_c == 0]), identical to the reference's.
// Returns n_found; payload (4 LE words) holds bytes 8..24 of the last matching candidate (the reference's select order), zero if none.
C25519_HD u32 lizard_decode(const ge_p3 &P, u32 payload[4]) {
    const jacobi4 J = ris_to_jacobi_quartic(P);
    u32 n_found = 0;
    for (int q = 0; q < 4; q++) payload[q] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int c = 0; c < 8; c++) {
        feT x;
        const bool defined = lizard_candidate(J, c, x);
        u32 w[8], d[8];
        fe_to_words(x, w);
        sha256_16(w + 2, d);
        const bool match = defined & (w[0] == (d[0] & 0xFFFFFFFEu)) & (w[1] == d[1]) & (w[6] == d[6]) & (w[7] == (d[7] & 0x3FFFFFFFu));
        const bool zero = (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0;
        n_found += (u32)match << (u32)zero;
        const lanemask m = lane_mask(match);
        for (int q = 0; q < 4; q++) payload[q] = sel_u32(payload[q], w[2 + q], m);
    }
    return n_found;
}

}  // namespace c25519
