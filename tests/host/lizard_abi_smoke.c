/* The Lizard entry points from plain C (C11, gcc): lizard_encode::<Sha256> of the reference's first test vector (compressed and
 * RAW160), lizard_decode of it from both formats, map_to_curve_inverse containing the tagged field element in slots 0..7,
 * the BAD_ENCODING and NONE statuses, bad formats and n = 0.  Exit code 0 = all good.  Built and run by tests/test_gpu_lizard.py. */
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
    uint8_t data[16], want[32], enc[32], raw[160], pay[16], st[2], inv[512];
    uint16_t mask = 0;
    uint8_t ok = 0;
    hex2bin("00000000000000000000000000000000", data, 16);
    hex2bin("f0b7e34484f74cf00f15024b738539738646bbbe1e9bc7509a676815227e774f", want, 32);
    if (c25519_ristretto_lizard_encode_sha256_batch(ctx, data, 1, C25519_FMT_RISTRETTO, enc) != C25519_OK) FAIL(3, "encode");
    if (memcmp(enc, want, 32)) FAIL(4, "encode mismatch");
    if (c25519_ristretto_lizard_encode_sha256_batch(ctx, data, 1, C25519_FMT_RAW160, raw) != C25519_OK) FAIL(5, "encode raw");
    memset(pay, 0xAA, 16);
    if (c25519_ristretto_lizard_decode_sha256_batch(ctx, enc, 1, C25519_FMT_RISTRETTO, pay, st) != C25519_OK) FAIL(6, "decode");
    if (st[0] != C25519_LIZARD_OK || memcmp(pay, data, 16)) FAIL(7, "decode mismatch");
    memset(pay, 0xAA, 16);
    if (c25519_ristretto_lizard_decode_sha256_batch(ctx, raw, 1, C25519_FMT_RAW160, pay, st) != C25519_OK) FAIL(8, "decode raw");
    if (st[0] != C25519_LIZARD_OK || memcmp(pay, data, 16)) FAIL(9, "decode raw mismatch");
    /* the tagged element SHA-256(0^16) with the payload spliced in and the bits cleared is among slots 0..7 */
    if (c25519_ristretto_map_to_curve_inverse_batch(ctx, enc, 1, C25519_FMT_RISTRETTO, inv, &mask, &ok) != C25519_OK) FAIL(10, "inverse");
    if (!ok) FAIL(11, "inverse: encoding reported invalid");
    int found = 0;
    for (int j = 0; j < 8; j++) {
        if (!(mask >> j & 1)) continue;
        const uint8_t *x = inv + 32 * j;
        int zero_payload = 1;
        for (int q = 8; q < 24; q++) zero_payload &= x[q] == 0;
        if (zero_payload && !(x[0] & 1) && !(x[31] & 0xC0)) found++;
    }
    if (found != 1) FAIL(12, "inverse: tagged preimage not found once");
    if (c25519_ristretto_map_to_curve_inverse_batch(ctx, raw, 1, C25519_FMT_RAW160, inv, &mask, NULL) != C25519_OK) FAIL(13, "inverse raw, ok = NULL");
    /* statuses: s = p - 1 is not canonical-and-even -> BAD_ENCODING; the basepoint has no Lizard preimage -> NONE */
    uint8_t two[64];
    memset(two, 0xFF, 32); two[0] = 0xEC; two[31] = 0x7F;
    hex2bin("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76", two + 32, 32);
    if (c25519_ristretto_lizard_decode_sha256_batch(ctx, two, 2, C25519_FMT_RISTRETTO, pay, st) != C25519_OK) FAIL(14, "decode statuses");
    if (st[0] != C25519_LIZARD_BAD_ENCODING || st[1] != C25519_LIZARD_NONE) FAIL(15, "decode statuses mismatch");
    for (int q = 0; q < 16; q++) if (pay[q]) FAIL(16, "payload not zeroed");
    if (c25519_ristretto_lizard_encode_sha256_batch(ctx, data, 1, C25519_FMT_EDWARDS_Y, enc) >= 0) FAIL(17, "encode accepted out_fmt 0");
    if (c25519_ristretto_lizard_decode_sha256_batch(ctx, enc, 1, 7, pay, st) >= 0) FAIL(18, "decode accepted in_fmt 7");
    if (c25519_ristretto_map_to_curve_inverse_batch(ctx, enc, 1, C25519_FMT_EDWARDS_Y, inv, &mask, &ok) >= 0) FAIL(19, "inverse accepted in_fmt 0");
    if (c25519_ristretto_lizard_encode_sha256_batch(ctx, data, 0, C25519_FMT_RISTRETTO, enc) != C25519_OK) FAIL(20, "n = 0");
    if (c25519_ristretto_lizard_decode_sha256_batch(ctx, enc, 0, C25519_FMT_RAW160, pay, st) != C25519_OK) FAIL(21, "n = 0");
    if (c25519_ristretto_map_to_curve_inverse_batch(ctx, enc, 0, C25519_FMT_RISTRETTO, inv, &mask, &ok) != C25519_OK) FAIL(22, "n = 0");
    c25519_ctx_destroy(ctx);
    printf("lizard_abi_smoke ok\n");
    return 0;
}
