/* The hash-to-group entry points from plain C (C11, gcc): RistrettoPoint::map_to_curve on the first sage vector of
 * ristretto/elligator.rs, from_uniform_bytes on the first RFC 9496 A.3 one-way-map vector, hash_from_bytes = from_uniform_bytes(SHA-512),
 * RFC 9380 J.5.1 / J.5.2 edwards25519 hash_to_curve / encode_to_curve of "abc" (compressed), the DST and out_fmt statuses, bad offsets, n = 0.
 * Exit code 0 = all good.  Built and run by tests/test_gpu_h2c.py. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/c25519_hip.h"

static int hex2bin(const char *h, uint8_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) { unsigned v; if (sscanf(h + 2 * i, "%2x", &v) != 1) return -1; out[i] = (uint8_t)v; }
    return 0;
}
#define FAIL(code, what) do { fprintf(stderr, "%s: %s\n", what, c25519_last_error(ctx)); return code; } while (0)

int main(void) {
    c25519_ctx *ctx = c25519_ctx_create(0, 0);
    if (!ctx) { fprintf(stderr, "no context\n"); return 2; }
    uint8_t in32[32], in64[64], want[32], out[2][32], raw[160];
    hex2bin("b8f98731fd7b597143a006ef0769d329c0f9b939096646c60f7f071aa0668647", in32, 32);
    hex2bin("b09ded61421d8ca6a85e1a9dd4d8e5a0c3f6e8efa9703fc1402098450bbef656", want, 32);
    if (c25519_ristretto_map_to_curve_batch(ctx, in32, 1, C25519_FMT_RISTRETTO, out[0]) != C25519_OK) FAIL(3, "map_to_curve");
    if (memcmp(out[0], want, 32)) FAIL(4, "map_to_curve mismatch");
    hex2bin("5d1be09e3d0c82fc538112490e35701979d99e06ca3e2b5b54bffe8b4dc772c14d98b696a1bbfb5ca32c436cc61c16563790306c79eaca7705668b47dffe5bb6", in64, 64);
    hex2bin("3066f82a1a747d45120d1740f14358531a8f04bbffe6a819f86dfe50f44a0a46", want, 32);
    if (c25519_ristretto_from_uniform_bytes_batch(ctx, in64, 1, C25519_FMT_RISTRETTO, out[0]) != C25519_OK) FAIL(5, "from_uniform_bytes");
    if (memcmp(out[0], want, 32)) FAIL(6, "from_uniform_bytes mismatch");
    if (c25519_ristretto_from_uniform_bytes_batch(ctx, in64, 1, C25519_FMT_RAW160, raw) != C25519_OK) FAIL(7, "from_uniform_bytes raw");
    if (c25519_compress_batch(ctx, raw, 1, C25519_FMT_RISTRETTO, out[1]) != C25519_OK || memcmp(out[1], want, 32)) FAIL(8, "raw160 -> compress");
    if (c25519_ristretto_map_to_curve_batch(ctx, in32, 1, C25519_FMT_EDWARDS_Y, out[0]) >= 0) FAIL(9, "map_to_curve accepted out_fmt 0");
    /* hash_from_bytes: two messages "abc" and "" */
    const uint8_t msgs[3] = {'a', 'b', 'c'};
    uint64_t off[3] = {0, 3, 3};
    if (c25519_ristretto_hash_from_bytes_batch(ctx, msgs, off, 2, C25519_FMT_RISTRETTO, &out[0][0]) != C25519_OK) FAIL(10, "hash_from_bytes");
    /* Edwards RO / NU of "abc" with the RFC 9380 DSTs */
    const char *dst_ro = "QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_RO_", *dst_nu = "QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_NU_";
    uint64_t off1[2] = {0, 3};
    hex2bin("31558a26887f23fb8218f143e69d5f0af2e7831130bd5b432ef23883b895839a", want, 32);
    if (c25519_edwards_hash_to_curve_batch(ctx, msgs, off1, 1, (const uint8_t *)dst_ro, (uint32_t)strlen(dst_ro), C25519_H2C_RO, C25519_FMT_EDWARDS_Y, out[0]) != C25519_OK) FAIL(11, "hash_to_curve");
    if (memcmp(out[0], want, 32)) FAIL(12, "hash_to_curve mismatch");
    hex2bin("42fa27c8f5a1ae0aa38bb59d5938e5145622ba5dedd11d11736fa2f9502d7367", want, 32);
    if (c25519_edwards_hash_to_curve_batch(ctx, msgs, off1, 1, (const uint8_t *)dst_nu, (uint32_t)strlen(dst_nu), C25519_H2C_NU, C25519_FMT_EDWARDS_Y, out[0]) != C25519_OK) FAIL(13, "encode_to_curve");
    if (memcmp(out[0], want, 32)) FAIL(14, "encode_to_curve mismatch");
    /* statuses */
    if (c25519_edwards_hash_to_curve_batch(ctx, msgs, off1, 1, (const uint8_t *)dst_ro, 0, C25519_H2C_RO, C25519_FMT_EDWARDS_Y, out[0]) != C25519_DOMAIN_SEPARATOR_LENGTH) FAIL(15, "empty DST");
    if (c25519_edwards_hash_to_curve_batch(ctx, msgs, off1, 1, (const uint8_t *)dst_ro, 256, C25519_H2C_RO, C25519_FMT_EDWARDS_Y, out[0]) != C25519_DOMAIN_SEPARATOR_LENGTH) FAIL(16, "long DST");
    if (c25519_edwards_hash_to_curve_batch(ctx, msgs, off1, 1, (const uint8_t *)dst_ro, 52, C25519_H2C_RO, C25519_FMT_RISTRETTO, out[0]) >= 0) FAIL(17, "Edwards accepted out_fmt 1");
    uint64_t bad[3] = {0, 3, 1};
    if (c25519_ristretto_hash_from_bytes_batch(ctx, msgs, bad, 2, C25519_FMT_RISTRETTO, &out[0][0]) >= 0) FAIL(18, "bad offsets accepted");
    if (c25519_ristretto_from_uniform_bytes_batch(ctx, in64, 0, C25519_FMT_RISTRETTO, out[0]) != C25519_OK) FAIL(19, "n = 0");
    if (c25519_edwards_hash_to_curve_batch(ctx, msgs, off1, 0, (const uint8_t *)dst_ro, 52, C25519_H2C_RO, C25519_FMT_RAW160, raw) != C25519_OK) FAIL(20, "n = 0");
    c25519_ctx_destroy(ctx);
    printf("h2c_abi_smoke ok\n");
    return 0;
}
