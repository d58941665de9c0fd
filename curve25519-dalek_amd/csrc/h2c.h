// Hash-to-group on the fe26 / ge26 layers (host + device), one item per lane:
//
//   ris_elligator         RistrettoPoint::elligator_ristretto_flavor (ristretto/elligator.rs:15-52; RFC 9496 §4.3.4 MAP)
//   mont_elligator2       montgomery::elligator_encode (montgomery.rs:276-363; RFC 9380 Appendix G.2.1)
//   ed_h2c_map            EdwardsPoint::map_to_curve (edwards.rs:651-690; RFC 9380 G.2.2 rational map, exceptional case by selects)
//   xmd_sha512            expand_message_xmd with SHA-512 (field.rs:440-490; RFC 9380 §5.3.1) for 48 or 96 output bytes
//   fe_from_be48          one hash_to_field element (field.rs:397-428): 48 bytes big-endian, mod p
//
// The maps are straight-line: selects only, no branch on data (the inputs of the Ristretto map may be secrets, e.g. an
// OPAQUE password hash).  xmd_sha512 branches on the message and DST lengths only, which are public.
#pragma once
#include "ge26.h"
#include "sc_sha.h"

namespace c25519 {

C25519_HD feT fe_minus_one() { return fe_carry(fe_neg(fe_one())); }

// ---- Ristretto Elligator map, step for step elligator_ristretto_flavor ----------------------------------------------
C25519_HD ge_p3 ris_elligator(const feT &r0) {
    const u32 c_omds[10] = C25519_ONE_MINUS_EDWARDS_D_SQUARED_26, c_dm1s[10] = C25519_EDWARDS_D_MINUS_ONE_SQUARED_26,
              c_sadm1[10] = C25519_SQRT_AD_MINUS_ONE_26;
    const feT one = fe_one(), d = fe_d(), minus_one = fe_minus_one();
    const feT r = fe_mul(fe_sqrtm1(), fe_sq(r0));
    const feT Ns = fe_mul(fe_add(r, one), fe_const(c_omds));
    const feT D = fe_mul(fe_sub(minus_one, fe_mul(d, r)), fe_add(r, d));
    feT s;
    const bool Ns_D_is_sq = fe_sqrt_ratio_i(s, Ns, D);
    feT s_prime = fe_mul(s, r0);
    s_prime = fe_cneg(s_prime, fe_is_negative(s_prime) == 0);       // -|s r0|
    const lanemask not_sq = lane_mask(!Ns_D_is_sq);
    s = fe_select_m(s, s_prime, not_sq);
    const feT c = fe_select_m(minus_one, r, not_sq);
    const feT Nt = fe_carry(fe_sub(fe_mul(fe_mul(c, fe_sub(r, one)), fe_const(c_dm1s)), D));
    const feT s_sq = fe_sq(s);
    // the completed point (curve_models.rs:169) W_0 .. W_3 -> extended (curve_models.rs:365-373)
    ge_p1p1 w;
    w.X = fe_mul(fe_twice(s), D);
    w.Z = fe_mul(Nt, fe_const(c_sadm1));
    w.Y = fe_sub(one, s_sq);
    w.T = fe_add(one, s_sq);
    return ge_p1p1_to_p3(w);
}
// RistrettoPoint::map_to_curve / from_uniform_bytes halves: FieldElement::from_bytes (bit 255 masked, values >= p accepted)
C25519_HD ge_p3 ris_map_words(const u32 w[8]) { return ris_elligator(fe_from_words(w)); }

// ---- RFC 9380 G.2.1 Elligator 2 for curve25519 -> (xn, xd, y), yd = 1 ----------------------------------------------
C25519_HD void mont_elligator2(const feT &u, feT &xn, feT &xd, feT &y) {
    const u32 c_a[10] = C25519_MONTGOMERY_A_26, c_na[10] = C25519_MONTGOMERY_A_NEG_26, c_c2[10] = C25519_H2C_C2_26;
    const feT one = fe_one(), i = fe_sqrtm1(), x1n = fe_const(c_na);
    const feT tv1 = fe_carry(fe_twice(fe_sq(u)));                      // 1-2   tv1 = 2u^2
    xd = fe_carry(fe_add(one, tv1));                                   // 3
    feT tv2 = fe_sq(xd);                                               // 5
    const feT gxd = fe_mul(tv2, xd);                                   // 6
    feT gx1 = fe_mul(fe_const(c_a), tv1);                              // 7
    gx1 = fe_mul(gx1, x1n);                                            // 8
    gx1 = fe_carry(fe_add(gx1, tv2));                                  // 9
    gx1 = fe_mul(gx1, x1n);                                            // 10
    feT tv3 = fe_sq(gxd);                                              // 11
    tv2 = fe_sq(tv3);                                                  // 12
    tv3 = fe_mul(tv3, gxd);                                            // 13
    tv3 = fe_mul(tv3, gx1);                                            // 14
    tv2 = fe_mul(tv2, tv3);                                            // 15
    feT y11 = fe_pow_p58(tv2);                                         // 16
    y11 = fe_mul(y11, tv3);                                            // 17
    const feT y12 = fe_mul(y11, i);                                    // 18
    tv2 = fe_mul(fe_sq(y11), gxd);                                     // 19-20
    const bool e1 = fe_eq(tv2, gx1);                                   // 21
    const feT y1 = fe_select(y12, y11, e1);                            // 22
    const feT x2n = fe_mul(x1n, tv1);                                  // 23
    feT y21 = fe_mul(y11, u);                                          // 24
    y21 = fe_mul(y21, fe_const(c_c2));                                 // 25
    const feT y22 = fe_mul(y21, i);                                    // 26
    const feT gx2 = fe_mul(gx1, tv1);                                  // 27
    tv2 = fe_mul(fe_sq(y21), gxd);                                     // 28-29
    const bool e2 = fe_eq(tv2, gx2);                                   // 30
    const feT y2 = fe_select(y22, y21, e2);                            // 31
    tv2 = fe_mul(fe_sq(y1), gxd);                                      // 32-33
    const bool e3 = fe_eq(tv2, gx1);                                   // 34
    const lanemask m3 = lane_mask(e3);
    xn = fe_select_m(x2n, x1n, m3);                                    // 35
    feT yy = fe_select_m(y2, y1, m3);                                  // 36
    const bool e4 = fe_is_negative(yy) != 0;                           // 37
    y = fe_cneg(yy, e3 != e4);                                         // 38
}

// ---- EdwardsPoint::map_to_curve (RFC 9380 G.2.2): Elligator 2, then the birational map, exceptional case e = (xd yd == 0) ----
C25519_HD ge_p3 ed_h2c_map(const feT &u) {
    const u32 c_c1[10] = C25519_ED25519_SQRTAM2_26;
    feT xMn, xMd, yMn;
    mont_elligator2(u, xMn, xMd, yMn);
    const feT one = fe_one();
    feT xn = fe_mul(xMn, fe_const(c_c1));                              // 2-3 (yMd = 1)
    feT xd = fe_mul(xMd, yMn);                                         // 4
    feT yn = fe_carry(fe_sub(xMn, xMd));                               // 5
    feT yd = fe_carry(fe_add(xMn, xMd));                               // 6
    const lanemask e = lane_mask(fe_is_zero(fe_mul(xd, yd)));          // 7-8
    xn = fe_select_m(xn, fe_zero(), e);                                // 9
    xd = fe_select_m(xd, one, e);                                      // 10
    yn = fe_select_m(yn, one, e);                                      // 11
    yd = fe_select_m(yd, one, e);                                      // 12
    ge_p3 r;
    r.X = fe_mul(xn, yd);
    r.Y = fe_mul(xd, yn);
    r.Z = fe_mul(xd, yd);
    r.T = fe_mul(xn, yn);
    return r;
}

// ---- hash_to_field: a 48-byte big-endian string mod p ---------------------------------------------------------------
// b[0..47] as read: value = lo + 2^256 hi with lo the low 32 bytes (little-endian words lo[0..7]) and hi < 2^128;
// mod p: lo mod 2^255 + 19 (bit 255 of lo) + 38 hi
C25519_HD feT fe_from_be48(const uint8_t b[48]) {
    u32 lo[8], hi[8];
    for (int k = 0; k < 8; k++) {              // word k of lo holds bytes 47-4k .. 44-4k (big-endian string, little-endian integer)
        const int j = 47 - 4 * k;
        lo[k] = (u32)b[j] | ((u32)b[j - 1] << 8) | ((u32)b[j - 2] << 16) | ((u32)b[j - 3] << 24);
    }
    for (int k = 0; k < 4; k++) {
        const int j = 15 - 4 * k;
        hi[k] = (u32)b[j] | ((u32)b[j - 1] << 8) | ((u32)b[j - 2] << 16) | ((u32)b[j - 3] << 24);
        hi[4 + k] = 0;
    }
    const feT l = fe_from_words(lo), h38 = fe_mul_small(fe_from_words(hi), 38u);
    feL s = fe_add(l, h38);
    s.v[0] += 19u * (lo[7] >> 31);
    return fe_carry(s);
}

// ---- expand_message_xmd, SHA-512 (RFC 9380 §5.3.1), len_in_bytes = 48 * count, count 1 or 2 ----------------------------
// msg_prime = Z_pad(128) || msg || I2OSP(len, 2) || 0x00 || DST || I2OSP(len(DST), 1);  b_0 = H(msg_prime),
// b_1 = H(b_0 || 0x01 || DST'), b_2 = H((b_0 ^ b_1) || 0x02 || DST').  out: 48 * count bytes (b_1 || b_2 truncated).
C25519_HD void xmd_dst_tail(sha512_stream &st, const uint8_t *dst, u32 dst_len) {
    st.put_bytes(dst, dst_len);
    st.put_byte(dst_len);
    st.finish();
}
C25519_HD void xmd_sha512(const uint8_t *msg, u64 msg_len, const uint8_t *dst, u32 dst_len, int count, uint8_t *out) {
    const u32 len = 48u * (u32)count;
    sha512_stream st;
    st.init();
    sha512_compress(st.h, st.w);               // Z_pad: one all-zero block (w[] is zero after init)
    for (int j = 0; j < 16; j++) st.w[j] = 0;
    st.total = 128;
    st.put_bytes(msg, msg_len);
    st.put_byte(len >> 8); st.put_byte(len & 0xff); st.put_byte(0);
    xmd_dst_tail(st, dst, dst_len);
    u64 b0[8], bi[8];
    for (int j = 0; j < 8; j++) b0[j] = st.h[j];
    for (int j = 0; j < 8; j++) bi[j] = 0;
    for (int i = 1; i <= count; i++) {
        st.init();
        for (int j = 0; j < 8; j++) st.put_be64(b0[j] ^ bi[j]);
        st.put_byte((u32)i);
        xmd_dst_tail(st, dst, dst_len);
        for (int j = 0; j < 8; j++) bi[j] = st.h[j];
        for (int j = 0; j < 8; j++) {
            const int o = 64 * (i - 1) + 8 * j;
            for (int q = 0; q < 8; q++) if (o + q < (int)len) out[o + q] = (uint8_t)(bi[j] >> (56 - 8 * q));
        }
    }
}
// hash_to_field::<Sha512, count> (field.rs:397-428): count field elements u[0..count)
C25519_HD void hash_to_field(const uint8_t *msg, u64 msg_len, const uint8_t *dst, u32 dst_len, int count, feT u[2]) {
    uint8_t ub[96];
    xmd_sha512(msg, msg_len, dst, dst_len, count, ub);
    u[0] = fe_from_be48(ub);
    if (count == 2) u[1] = fe_from_be48(ub + 48);
}

// EdwardsPoint::hash_to_curve (ro) / encode_to_curve (!ro), edwards.rs:710-750: the map(s), the sum, mul_by_cofactor (x8)
C25519_HD ge_p3 ed_hash_to_curve(const uint8_t *msg, u64 msg_len, const uint8_t *dst, u32 dst_len, bool ro) {
    feT u[2];
    hash_to_field(msg, msg_len, dst, dst_len, ro ? 2 : 1, u);
    ge_p3 Q = ed_h2c_map(u[0]);
    if (ro) Q = ge_add(Q, ed_h2c_map(u[1]));
    return ge_mul_by_pow_2(Q, 3);
}

}  // namespace c25519
