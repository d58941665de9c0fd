/* The wave route of the segmented vartime MSM from plain C (C11, gcc): c25519_msm_vartime_segments_plan on the offsets, then one call with
 * a segment of C25519_MSM_SEGMENT_DIRECT_MAX + 1 terms (the shortest the wave route takes), a short one on the lane route between, and a
 * segment of C25519_MSM_SEGMENT_WAVE_MAX terms (the longest); each sum is compared with c25519_msm_vartime on that segment alone.  The terms
 * are made here: scalars from a 64-bit LCG (below 2^252), points = CompressedEdwardsY of other such scalars times B.  Exit code 0 = all good. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/c25519_hip.h"

#define FAIL(code, what) do { fprintf(stderr, "%s: %s\n", what, c25519_last_error(ctx)); return code; } while (0)
#define SHORT 3

static uint64_t lcg_state = 0x243f6a8885a308d3ull;
static void fill(uint8_t *s, uint64_t n) {
    for (uint64_t i = 0; i < n * 32; i++) { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; s[i] = (uint8_t)(lcg_state >> 56); }
    for (uint64_t i = 0; i < n; i++) s[32 * i + 31] &= 0x0f;
}

int main(void) {
    const uint64_t a = C25519_MSM_SEGMENT_DIRECT_MAX + 1, b = C25519_MSM_SEGMENT_WAVE_MAX, n = a + SHORT + b;
    const uint64_t off[4] = {0, a, a + SHORT, n};
    uint64_t plan[5] = {9, 9, 9, 9, 9};
    if (c25519_msm_vartime_segments_plan(off, 3, plan) != C25519_OK) { fprintf(stderr, "plan failed\n"); return 3; }
    if (plan[0] != 1 || plan[1] != 2 || plan[2] != 0 || plan[3] != 1 || plan[4] != n) { fprintf(stderr, "plan: unexpected routes\n"); return 4; }
    const uint64_t bad_off[3] = {0, 5, 4};
    if (c25519_msm_vartime_segments_plan(bad_off, 2, plan) >= 0) { fprintf(stderr, "plan accepted decreasing offsets\n"); return 5; }

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
    printf("seg_msm_wave_abi_smoke ok\n");
    return 0;
}
