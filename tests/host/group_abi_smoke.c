/* The group-law entry points from plain C (C11, gcc): B + B, B - B = identity, -B, [8]B, B == B, is_identity, a segmented sum of
 * 16 copies of B with empty segments around it, a Ristretto encoding that must fail to decode, rejected format pairs, n = 0 and m = 0.
 * Expected encodings: ED25519_BASEPOINT_COMPRESSED (constants.rs), BASE2_CMPRSSD / BASE16_CMPRSSD (edwards.rs tests), passed on the
 * command line as hex by tests/test_gpu_group.py.  Exit code 0 = all good. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/c25519_hip.h"

#define FAIL(code, what) do { fprintf(stderr, "%s: %s\n", what, c25519_last_error(ctx)); return code; } while (0)

static void unhex(const char *h, uint8_t out[32]) {
    for (int i = 0; i < 32; i++) { unsigned v; sscanf(h + 2 * i, "%2x", &v); out[i] = (uint8_t)v; }
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    uint8_t b2[32], b16[32], ident[32] = {1};
    uint8_t pts[16][32], out[4][32], ok[16], eq[2];
    unhex(argv[2], b2); unhex(argv[3], b16);
    for (int i = 0; i < 16; i++) unhex(argv[1], pts[i]);
    c25519_ctx *ctx = c25519_ctx_create(0, 0);
    if (!ctx) { fprintf(stderr, "no context\n"); return 2; }
    if (c25519_point_add_batch(ctx, &pts[0][0], &pts[1][0], 2, C25519_POINT_ADD, C25519_FMT_EDWARDS_Y, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK)
        FAIL(3, "add");
    if (memcmp(out[0], b2, 32) || memcmp(out[1], b2, 32) || !ok[0] || !ok[1]) FAIL(4, "B + B");
    if (c25519_point_add_batch(ctx, &pts[0][0], &pts[1][0], 1, C25519_POINT_SUB, C25519_FMT_EDWARDS_Y, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK ||
        memcmp(out[0], ident, 32))
        FAIL(5, "B - B");
    if (c25519_point_map_batch(ctx, &pts[0][0], 1, C25519_POINT_NEG, C25519_FMT_EDWARDS_Y, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK ||
        memcmp(out[0], pts[0], 31) || out[0][31] != (pts[0][31] ^ 0x80))
        FAIL(6, "-B");
    if (c25519_point_eq_batch(ctx, &pts[0][0], &pts[1][0], 2, C25519_FMT_EDWARDS_Y, C25519_FMT_EDWARDS_Y, eq, ok) != C25519_OK || !eq[0] || !eq[1]) FAIL(7, "B == B");
    if (c25519_point_eq_batch(ctx, &pts[0][0], NULL, 1, C25519_FMT_EDWARDS_Y, C25519_FMT_EDWARDS_Y, eq, ok) != C25519_OK || eq[0]) FAIL(8, "B is the identity");
    uint64_t off[5] = {0, 0, 16, 16, 16};      /* empty, 16 x B, empty, empty */
    if (c25519_point_sum_segments(ctx, &pts[0][0], 16, C25519_FMT_EDWARDS_Y, off, 4, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK) FAIL(9, "sum");
    if (memcmp(out[0], ident, 32) || memcmp(out[1], b16, 32) || memcmp(out[2], ident, 32) || memcmp(out[3], ident, 32)) FAIL(10, "sum values");
    uint8_t bad[32];
    memset(bad, 0xff, 32); bad[31] = 0x7f;       /* 2^255 - 1: not a canonical Ristretto encoding */
    if (c25519_point_map_batch(ctx, bad, 1, C25519_POINT_NEG, C25519_FMT_RISTRETTO, C25519_FMT_RISTRETTO, &out[0][0], ok) != C25519_NONE || ok[0]) FAIL(11, "bad Ristretto");
    if (c25519_point_add_batch(ctx, &pts[0][0], &pts[1][0], 1, C25519_POINT_ADD, C25519_FMT_EDWARDS_Y, C25519_FMT_RISTRETTO, &out[0][0], ok) >= 0) FAIL(12, "0 -> 1 accepted");
    if (c25519_point_map_batch(ctx, bad, 1, C25519_POINT_MUL_BY_COFACTOR, C25519_FMT_RISTRETTO, C25519_FMT_RISTRETTO, &out[0][0], ok) >= 0) FAIL(13, "Ristretto cofactor");
    if (c25519_point_add_batch(ctx, &pts[0][0], &pts[1][0], 0, C25519_POINT_ADD, C25519_FMT_EDWARDS_Y, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK) FAIL(14, "n = 0");
    if (c25519_point_sum_segments(ctx, &pts[0][0], 0, C25519_FMT_EDWARDS_Y, off, 0, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK) FAIL(15, "m = 0");
    c25519_ctx_destroy(ctx);
    printf("group_abi_smoke ok\n");
    return 0;
}
