// The handle of the precomputed-static calls (c25519_precomp_*), shared by extra.hip (create, destroy, len, the bucket call), mid_rows.hip (the
// rows call and its comb table) and mid_mixed.hip (the mixed rows call over the same comb table).  A handle is used from one thread at a time, like its context.
#pragma once
#include <stdint.h>
#include "msm_internal.h"

struct c25519_precomp {
    uint32_t *d_table;                 // the bucket call's table: affine Niels records of 2^(c k) S_i at [k * n + i] (msm_internal.h msm_merged); window 0 is S_i itself
    uint64_t n;
    c25519::msm_merged m;
    // the rows call's comb table, built by its first call (mid_rows.hip rows_build): affine Niels records of e * 16^k * S_j at [(j * 64 + k) * 8 + e - 1],
    // k < 64, e = 1 .. 8 -- 65536 bytes per static point.  rows_bytes is 0 until it is complete.
    uint32_t *d_rows = nullptr;
    uint64_t rows_bytes = 0;
};

// mid_rows.hip: builds the comb table on the context's stream if the handle has none yet (it reserves its scratch in ctx->tmp_f)
int32_t rows_build(c25519_ctx *ctx, c25519_precomp *p);
