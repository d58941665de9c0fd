// SHA-256 (FIPS 180-4) of exactly 16 bytes, host + device, one message per lane: the only length Lizard hashes
// (lizard/lizard_ristretto.rs: D::digest(data) of the 16-byte payload).  16 bytes + padding + the 64-bit length fit one block,
// so this is one compression with a fixed schedule tail; no streaming state.  Round constants and the initial state are derived
// in tools/gen_constants.py (sha256_constants) and land in constants_gen.h.
#pragma once
#include "fe26.h"
#include "constants_gen.h"

namespace c25519 {

#ifdef __HIP_DEVICE_COMPILE__
__device__ __constant__ static const u32 SHA256_K[64] = C25519_SHA256_K;
#else
static const u32 SHA256_K[64] = C25519_SHA256_K;
#endif
C25519_HD u32 rotr32(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
C25519_HD u32 bswap32(u32 x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

C25519_HD void sha256_round(u32 &a, u32 &b, u32 &c, u32 &d, u32 &e, u32 &f, u32 &g, u32 &h, u32 kw) {
    const u32 S1 = rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25);
    const u32 ch = (e & f) ^ (~e & g);
    const u32 t1 = h + S1 + ch + kw;
    const u32 S0 = rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22);
    const u32 maj = (a & b) ^ (a & c) ^ (b & c);
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + maj;
}

// in: the 16 message bytes as 4 little-endian u32 words (as loaded from memory); out: the 32-byte digest as 8 little-endian words
C25519_HD void sha256_16(const u32 in[4], u32 out[8]) {
    const u32 iv[8] = C25519_SHA256_IV;
    u32 w[16];
    for (int j = 0; j < 4; j++) w[j] = bswap32(in[j]);
    w[4] = 0x80000000u;                                  // the padding bit
    for (int j = 5; j < 15; j++) w[j] = 0;
    w[15] = 128;                                         // message length in bits
    u32 a = iv[0], b = iv[1], c = iv[2], d = iv[3], e = iv[4], f = iv[5], g = iv[6], h = iv[7];
    // rounds 0..15 on the block itself, then three groups of 16 with the message schedule (no branch on the round number:
    // a uniform if inside the loop is lowered to a vcc branch)
#pragma unroll
    for (int j = 0; j < 16; j++) sha256_round(a, b, c, d, e, f, g, h, SHA256_K[j] + w[j]);
#pragma unroll 1
    for (int i = 16; i < 64; i += 16) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const u32 w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
            const u32 s0 = rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3);
            const u32 s1 = rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10);
            w[j] = w[j] + s0 + w[(j + 9) & 15] + s1;
            sha256_round(a, b, c, d, e, f, g, h, SHA256_K[i + j] + w[j]);
        }
    }
    out[0] = bswap32(iv[0] + a); out[1] = bswap32(iv[1] + b); out[2] = bswap32(iv[2] + c); out[3] = bswap32(iv[3] + d);
    out[4] = bswap32(iv[4] + e); out[5] = bswap32(iv[5] + f); out[6] = bswap32(iv[6] + g); out[7] = bswap32(iv[7] + h);
}

}  // namespace c25519
