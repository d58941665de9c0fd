/* The MontgomeryPoint entry points from plain C (C11, gcc): to_edwards of the X25519 basepoint with both signs (the Ed25519
 * basepoint and its negation, montgomery.rs basepoint_montgomery_to_edwards), u = 2 rejected (montgomery_to_edwards_rejects_twist),
 * 1 * u = u through mul, mul_bits_be and mul_base, bad nbits / out_fmt, n = 0.  Exit code 0 = all good.  Built and run by
 * tests/test_gpu_montgomery.py. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/c25519_hip.h"

#define FAIL(code, what) do { fprintf(stderr, "%s: %s\n", what, c25519_last_error(ctx)); return code; } while (0)

int main(void) {
    c25519_ctx *ctx = c25519_ctx_create(0, 0);
    if (!ctx) { fprintf(stderr, "no context\n"); return 2; }
    uint8_t u[2][32] = {{9}, {2}}, signs[2] = {0, 1}, one[32] = {1}, bit1[1] = {0x80}, out[2][32], raw[2][160], st[2], zero[32] = {0};
    uint8_t bp[32], nbp[32];
    memset(bp, 0x66, 32); bp[0] = 0x58;                    /* ED25519_BASEPOINT_COMPRESSED (constants.rs) */
    memcpy(nbp, bp, 32); nbp[31] |= 0x80;                  /* -B: x != 0, so only the sign bit differs */
    uint8_t uu[2][32];
    memcpy(uu[0], u[0], 32); memcpy(uu[1], u[0], 32);
    if (c25519_montgomery_to_edwards_batch(ctx, &uu[0][0], signs, 2, C25519_FMT_EDWARDS_Y, &out[0][0], st) != C25519_OK) FAIL(3, "to_edwards");
    if (st[0] != 1 || st[1] != 1 || memcmp(out[0], bp, 32) || memcmp(out[1], nbp, 32)) FAIL(4, "to_edwards basepoint");
    if (c25519_montgomery_to_edwards_batch(ctx, &u[0][0], signs, 2, C25519_FMT_RAW160, &raw[0][0], st) != C25519_OK) FAIL(5, "to_edwards raw");
    if (st[0] != 1 || st[1] != 0) FAIL(6, "to_edwards u = 2 accepted");
    for (int i = 0; i < 160; i++) if (raw[1][i]) FAIL(7, "None output not zero");
    if (c25519_montgomery_mul_batch(ctx, one, u[0], 1, out[0]) != C25519_OK || memcmp(out[0], u[0], 32)) FAIL(8, "mul by 1");
    if (c25519_montgomery_mul_bits_be_batch(ctx, bit1, 1, u[0], 1, out[0]) != C25519_OK || memcmp(out[0], u[0], 32)) FAIL(9, "mul_bits_be by 1");
    if (c25519_montgomery_mul_bits_be_batch(ctx, NULL, 0, u[0], 1, out[0]) != C25519_OK || memcmp(out[0], zero, 32)) FAIL(10, "mul_bits_be of nothing");
    if (c25519_montgomery_mul_base_batch(ctx, one, 1, out[0]) != C25519_OK || memcmp(out[0], u[0], 32)) FAIL(11, "mul_base(1)");
    if (c25519_montgomery_mul_bits_be_batch(ctx, bit1, 513, u[0], 1, out[0]) >= 0) FAIL(12, "nbits 513 accepted");
    if (c25519_montgomery_to_edwards_batch(ctx, &u[0][0], signs, 1, C25519_FMT_RISTRETTO, &out[0][0], st) >= 0) FAIL(13, "out_fmt 1 accepted");
    if (c25519_montgomery_mul_batch(ctx, one, u[0], 0, out[0]) != C25519_OK) FAIL(14, "n = 0");
    if (c25519_montgomery_to_edwards_batch(ctx, &u[0][0], signs, 0, C25519_FMT_RAW160, &raw[0][0], st) != C25519_OK) FAIL(15, "n = 0");
    c25519_ctx_destroy(ctx);
    printf("montgomery_abi_smoke ok\n");
    return 0;
}
