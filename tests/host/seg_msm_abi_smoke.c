/* The segmented vartime MSM from plain C (C11, gcc): the host form on three segments of CompressedEdwardsY terms -- two terms, none (the
 * identity), three -- then an undecodable point in the last segment, a rejected format pair, offsets that do not end at n, and m = 0.
 * Scalars (5 x 32), points (5 x 32) and the three expected sums (3 x 32) come as hex on the command line from tests/test_gpu_seg_msm.py,
 * which takes the sums from the oracle.  Exit code 0 = all good. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/c25519_hip.h"

#define FAIL(code, what) do { fprintf(stderr, "%s: %s\n", what, c25519_last_error(ctx)); return code; } while (0)

static int unhex(const char *h, uint8_t *out, size_t n) {
    if (strlen(h) != 2 * n) return 1;
    for (size_t i = 0; i < n; i++) { unsigned v; if (sscanf(h + 2 * i, "%2x", &v) != 1) return 1; out[i] = (uint8_t)v; }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    uint8_t s[5][32], p[5][32], want[3][32], out[3][32], ok[3], ident[32] = {1};
    if (unhex(argv[1], &s[0][0], 160) || unhex(argv[2], &p[0][0], 160) || unhex(argv[3], &want[0][0], 96)) return 2;
    if (memcmp(want[1], ident, 32)) return 2;
    c25519_ctx *ctx = c25519_ctx_create(0, 0);
    if (!ctx) { fprintf(stderr, "no context\n"); return 2; }
    const uint64_t off[4] = {0, 2, 2, 5};
    memset(out, 0xee, sizeof out); memset(ok, 0xee, sizeof ok);
    if (c25519_msm_vartime_segments(ctx, &s[0][0], &p[0][0], 5, C25519_FMT_EDWARDS_Y, off, 3, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK) FAIL(3, "segments");
    if (memcmp(out, want, sizeof out) || ok[0] != 1 || ok[1] != 1 || ok[2] != 1) FAIL(4, "sums");
    /* each sum is what the single call gives for that segment */
    uint8_t one[32];
    if (c25519_msm_vartime(ctx, &s[2][0], &p[2][0], 3, C25519_FMT_EDWARDS_Y, C25519_FMT_EDWARDS_Y, one) != C25519_OK || memcmp(one, out[2], 32)) FAIL(5, "single");
    /* ok may be NULL */
    memset(out, 0xee, sizeof out);
    if (c25519_msm_vartime_segments(ctx, &s[0][0], &p[0][0], 5, C25519_FMT_EDWARDS_Y, off, 3, C25519_FMT_EDWARDS_Y, &out[0][0], NULL) != C25519_OK ||
        memcmp(out, want, sizeof out))
        FAIL(6, "ok = NULL");
    /* an undecodable point fails its own segment only: four Ristretto identities (all-zero encodings) and 2^255 - 1, which is not canonical */
    uint8_t bad[5][32], rs[32] = {0};
    memset(bad, 0, sizeof bad);
    memset(bad[4], 0xff, 32); bad[4][31] = 0x7f;
    if (c25519_msm_vartime_segments(ctx, &s[0][0], &bad[0][0], 5, C25519_FMT_RISTRETTO, off, 3, C25519_FMT_RISTRETTO, &out[0][0], ok) != C25519_NONE) FAIL(7, "NONE");
    if (ok[0] != 1 || ok[1] != 1 || ok[2] != 0 || memcmp(out[0], rs, 32) || memcmp(out[1], rs, 32)) FAIL(8, "ok bytes");
    if (c25519_msm_vartime_segments(ctx, &s[0][0], &p[0][0], 5, C25519_FMT_EDWARDS_Y, off, 3, C25519_FMT_RISTRETTO, &out[0][0], ok) >= 0) FAIL(9, "0 -> 1 accepted");
    if (c25519_msm_vartime_segments(ctx, &s[0][0], &p[0][0], 4, C25519_FMT_EDWARDS_Y, off, 3, C25519_FMT_EDWARDS_Y, &out[0][0], ok) >= 0) FAIL(10, "seg_off[m] != n accepted");
    if (c25519_msm_vartime_segments(ctx, &s[0][0], &p[0][0], 0, C25519_FMT_EDWARDS_Y, off, 0, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK) FAIL(11, "m = 0");
    /* the context is still good */
    if (c25519_msm_vartime_segments(ctx, &s[0][0], &p[0][0], 5, C25519_FMT_EDWARDS_Y, off, 3, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK || memcmp(out, want, sizeof out))
        FAIL(12, "after the errors");
    c25519_ctx_destroy(ctx);
    printf("seg_msm_abi_smoke ok\n");
    return 0;
}
