/* The bucket route of the segmented vartime MSM from plain C (C11, gcc): c25519_msm_vartime_segments_routes on the offsets, then one call with
 * a short segment on the lane route, a segment of C25519_MSM_SEGMENT_WAVE_MAX + 1 terms (the shortest the bucket route takes) and a wave
 * segment behind it; each sum is compared with c25519_msm_vartime on that segment alone.  The terms are made here: scalars from a 64-bit LCG
 * (below 2^252), points = CompressedEdwardsY of other such scalars times B.  Exit code 0 = all good. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/c25519_hip.h"

#define FAIL(code, what) do { fprintf(stderr, "%s: %s\n", what, c25519_last_error(ctx)); return code; } while (0)
#define SHORT 3
#define WAVE 70

static uint64_t lcg_state = 0x13198a2e03707344ull;
static void fill(uint8_t *s, uint64_t n) {
    for (uint64_t i = 0; i < n * 32; i++) { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; s[i] = (uint8_t)(lcg_state >> 56); }
    for (uint64_t i = 0; i < n; i++) s[32 * i + 31] &= 0x0f;
}

int main(void) {
    const uint64_t b = C25519_MSM_SEGMENT_WAVE_MAX + 1, n = SHORT + b + WAVE;
    const uint64_t off[4] = {0, SHORT, SHORT + b, n};
    uint8_t route[3] = {9, 9, 9};
    if (c25519_msm_vartime_segments_routes(off, 3, route) != C25519_OK) { fprintf(stderr, "routes failed\n"); return 3; }
    if (route[0] != C25519_MSM_SEGMENT_ROUTE_LANE || route[1] != C25519_MSM_SEGMENT_ROUTE_BUCKET || route[2] != C25519_MSM_SEGMENT_ROUTE_WAVE) {
        fprintf(stderr, "routes: unexpected %d %d %d\n", route[0], route[1], route[2]); return 4;
    }
    const uint64_t edge[3] = {0, C25519_MSM_SEGMENT_BUCKET_MAX, 2 * (uint64_t)C25519_MSM_SEGMENT_BUCKET_MAX + 1};
    if (c25519_msm_vartime_segments_routes(edge, 2, route) != C25519_OK || route[0] != C25519_MSM_SEGMENT_ROUTE_BUCKET || route[1] != C25519_MSM_SEGMENT_ROUTE_SINGLE) {
        fprintf(stderr, "routes: the bucket maximum is not the boundary\n"); return 4;
    }
    const uint64_t bad_off[3] = {0, 5, 4};
    if (c25519_msm_vartime_segments_routes(bad_off, 2, route) >= 0) { fprintf(stderr, "routes accepted decreasing offsets\n"); return 5; }

    c25519_ctx *ctx = c25519_ctx_create(0, 0);
    if (!ctx) { fprintf(stderr, "no context\n"); return 2; }
    uint8_t *s = malloc(n * 32), *k = malloc(n * 32), *p = malloc(n * 32);
    if (!s || !k || !p) return 2;
    fill(s, n); fill(k, n);
    if (c25519_mul_base_batch(ctx, k, n, C25519_FMT_EDWARDS_Y, p) != C25519_OK) FAIL(6, "mul_base_batch");
    uint8_t out[3][32], ok[3], one[32];
    memset(out, 0xee, sizeof out); memset(ok, 0xee, sizeof ok);
    if (c25519_msm_vartime_segments(ctx, s, p, n, C25519_FMT_EDWARDS_Y, off, 3, C25519_FMT_EDWARDS_Y, &out[0][0], ok) != C25519_OK) FAIL(7, "segments");
    for (int g = 0; g < 3; g++) {
        if (c25519_msm_vartime(ctx, s + 32 * off[g], p + 32 * off[g], off[g + 1] - off[g], C25519_FMT_EDWARDS_Y, C25519_FMT_EDWARDS_Y, one) != C25519_OK) FAIL(8, "single");
        if (memcmp(one, out[g], 32) || ok[g] != 1) { fprintf(stderr, "segment %d differs from c25519_msm_vartime\n", g); return 9; }
    }
    free(s); free(k); free(p);
    c25519_ctx_destroy(ctx);
    printf("seg_msm_bucket_abi_smoke ok\n");
    return 0;
}
