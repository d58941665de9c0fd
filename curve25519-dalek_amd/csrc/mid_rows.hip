// Many multiscalar multiplications over ONE precomputed point set in one call:  out[r] = sum_{j < w} scalars[r][j] * S_j  over the first w
// static points of a c25519_precomp handle, r < m -- one VartimePrecomputedMultiscalarMul::vartime_multiscalar_mul (traits.rs:304-419,
// edwards.rs:1037-1076, ristretto.rs:1004) per row.  DESIGN.md section 3.15.
//
//   c25519_precomp_msm_vartime_rows_dev / c25519_precomp_msm_vartime_rows / c25519_precomp_msm_vartime_rows_plan / c25519_precomp_rows_table_bytes
//
// The comb table of the handle (precomp.h d_rows; built by the first rows call, rows_build): the affine Niels record of e * 16^k * S_j for every
// static point j, window k < 64 and e = 1 .. 8, the eight records of one (j, k) next to each other.  A row then needs no doubling and no
// per-call table: one mixed addition per non-zero radix-16 digit, in any order.
//   k_mid_rows_bases       one lane per static point: S_j from the window-0 record of the handle's bucket table, then 16^k S_j for k < 64 as raw
//                          160-byte points (slot e = 1 of every (j, k))
//   k_mid_rows_multiples   one lane per (j, k): e * 16^k S_j for e = 2 .. 8 by repeated addition; prep_points (the MSM's own normaliser) turns
//                          the raw points into the records
//   k_mid_rows_lane        one LANE per row, the 64 lanes of a wave are 64 consecutive rows (straus.h straus_comb_lane): for every j the scalar is
//                          recoded in registers, then for every window the record (j, k, |d|) is added or subtracted.  All lanes of a wave are
//                          on the same (j, k) at the same time: their gathers fall into one 1 KB group of records.
//   k_mid_rows_wave        one WAVE per row, lane l is window l (straus_comb_wave): for every j each lane takes its own digit of the scalar (a
//                          uniform load) and adds record (j, l, |d|); the 64 partial sums are folded across the wave with six shuffle rounds.
// Digits (rows_digits.h) as k_mid_straus_tables makes them (scalar.rs:1019-1051): nibble k of s' = s + 0x0888...8 minus 8, the top nibble left unsigned (0 .. 8); no
// digit array is written.  Complete formulas (ge_madd_signed_p3, ge_add): no special case for identity, equal or opposite operands; a zero
// digit is skipped.  The scalars are public by contract (a *_vartime entry point): branches and table addresses depend on their digits.
// Every loop bound comes from the m and w the host validated; the kernels wait for nothing and use no atomics (the verdict word is set by a
// plain store of 1).  Compressed outputs go through c25519_compress_batch_dev: no inversion here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include "msm_internal.h"
#include "straus.h"                         // (and through it devio.h, kernels.h, ctx.h, knobs.h, precomp.h, rows_digits.h, capi_util.h)
#include "ffi.h"

using namespace c25519;

namespace c25519 {

// (ROWS_WIN, ROWS_ENT, ROWS_REC: rows_digits.h; the loops over the comb table and the verdict words: straus.h, shared with mid_mixed.hip)

// ---- the comb table ---------------------------------------------------------------------------------------------------------------
// Static points [j0, j0 + cnt) of the handle -> raw[((j - j0) * 64 + k) * 8] = 16^k S_j.  S_j = (2x : 2y : 2 : 2xy) from its window-0 record.
__global__ void __launch_bounds__(256) k_mid_rows_bases(const u32 *__restrict__ d_table, u64 j0, u64 cnt, uint8_t *__restrict__ raw) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    ge_p3 P = ge_from_aniels_signed(pts_load(d_table, j0 + i), false);
#pragma unroll 1
    for (int k = 0; k < ROWS_WIN; k++) {
        raw160_store(raw, (i * ROWS_WIN + (u64)k) * ROWS_ENT, P);
        if (k + 1 < ROWS_WIN) P = ge_mul_by_pow_2(P, 4);
    }
}
// (point, window) pair t of the chunk, cnt pairs: raw[t * 8 + e - 1] = e * raw[t * 8] for e = 2 .. 8 (window.rs:97-104)
__global__ void __launch_bounds__(256) k_mid_rows_multiples(uint8_t *raw, u64 cnt) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt) return;
    const ge_p3 P = raw160_load(raw, t * ROWS_ENT);
    const ge_cached c1 = ge_p3_to_cached(P);
    ge_p3 acc = P;
#pragma unroll 1
    for (int e = 1; e < ROWS_ENT; e++) {
        acc = ge_p1p1_to_p3(ge_add_cached(acc, c1));
        raw160_store(raw, t * ROWS_ENT + (u64)e, acc);
    }
}

// ---- the rows ---------------------------------------------------------------------------------------------------------------------
// Lane = row r < m.  tab holds at least w * 512 records (the host checked w against the handle).
__global__ void __launch_bounds__(256) k_mid_rows_lane(const uint8_t *__restrict__ scalars, u64 m, u32 w, const u32 *__restrict__ tab, uint8_t *__restrict__ out_raw,
                                                       u32 *__restrict__ flags) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    ge_p3 acc = ge_identity();
    straus_comb_lane(acc, scalars, r * w, w, tab, flags);
    raw160_store(out_raw, r, acc);
}

// Wave = row r < m (four per block), lane l = window l.  The row index, the scalar's address and every loop bound are wave-uniform; only the
// digit depends on the lane.  No LDS, no barrier.
__global__ void __launch_bounds__(256) k_mid_rows_wave(const uint8_t *__restrict__ scalars, u32 m, u32 w, const u32 *__restrict__ tab, uint8_t *__restrict__ out_raw,
                                                       u32 *__restrict__ flags) {
    const u32 r = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (r >= m) return;
    const u32 lane = threadIdx.x & 63u;
    ge_p3 acc = ge_identity();
    straus_comb_wave(acc, scalars, (u64)r * w, w, tab, lane, flags);
    acc = straus_wave_fold(acc);
    if (lane == 0) raw160_store(out_raw, r, acc);
}

}  // namespace c25519

// ---- host side ----------------------------------------------------------------------------------------------------------------
constexpr uint64_t ROWS_BUILD_CHUNK = 256;                  // static points per build step: 256 x 512 raw points = 20 MB of scratch

// ---- routing: the one place that chooses the kernel of a call ----
static int32_t rows_plan(c25519_ctx *ctx, uint64_t m, uint64_t w, uint64_t plan[2]) {
    if (m >= 0xffffffffull) return bad_arg(ctx, "precomp_msm_vartime_rows: m must be below 2^32 - 1");
    if (w && m > UINT64_MAX / w) return bad_arg(ctx, "precomp_msm_vartime_rows: m * w overflows");
    const bool lane = rows_lane_route(m, w);
    plan[0] = lane ? C25519_PRECOMP_ROWS_LANE : C25519_PRECOMP_ROWS_WAVE;
    plan[1] = lane ? (m + 63) / 64 : m;
    return C25519_OK;
}
EXPORT int32_t c25519_precomp_msm_vartime_rows_plan(uint64_t m, uint64_t w, uint64_t plan[2]) { return rows_plan(nullptr, m, w, plan); }

EXPORT uint64_t c25519_precomp_rows_table_bytes(const c25519_precomp *p) { return p ? p->rows_bytes : 0; }

// everything that is refused before any launch; route_out: the kernel of this call
static int32_t rows_check(c25519_ctx *ctx, const c25519_precomp *p, uint64_t m, uint64_t w, int32_t route, int out_fmt, int32_t &route_out) {
    static const rows_msgs msgs = ROWS_MSGS("precomp_msm_vartime_rows", "scalars");
    uint64_t plan[2];
    int32_t r;
    if ((r = rows_check_handle(ctx, msgs, p, w, route, out_fmt)) || (r = rows_plan(ctx, m, w, plan))) return r;
    route_out = route == C25519_PRECOMP_ROWS_AUTO ? (int32_t)plan[0] : route;
    return C25519_OK;
}

// the comb table of the handle, once: enqueued on the context's stream in front of the first rows kernel (precomp.h: the mixed rows call of
// mid_mixed.hip builds it through this function too)
int32_t rows_build(c25519_ctx *ctx, c25519_precomp *p) {
    if (p->rows_bytes || p->n == 0) return C25519_OK;
    hipStream_t st = ctx->stream;
    const uint64_t n = p->n, chunk = std::min<uint64_t>(n, ROWS_BUILD_CHUNK);
    int32_t r;
    if ((r = ctx_reserve(ctx, ctx->tmp_f, (size_t)(chunk * ROWS_REC) * 160 + 256))) return r;
    if (!p->d_rows) HIPCHK(hipMalloc((void **)&p->d_rows, (size_t)(n * ROWS_REC) * PTS_BYTES));
    uint8_t *raw = (uint8_t *)ctx->tmp_f.p;
    for (uint64_t j0 = 0; j0 < n; j0 += chunk) {            // (one stream: a step's scratch is free again when the next one writes it)
        const uint64_t cnt = std::min(chunk, n - j0);
        hipLaunchKernelGGL(k_mid_rows_bases, dim3(div_up(cnt, 256)), dim3(256), 0, st, (const u32 *)p->d_table, j0, cnt, raw);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_mid_rows_multiples, dim3(div_up(cnt * ROWS_WIN, 256)), dim3(256), 0, st, raw, cnt * ROWS_WIN);
        HIPCHK(hipGetLastError());
        if ((r = prep_points(ctx, raw, cnt * ROWS_REC, C25519_FMT_RAW160, p->d_rows, j0 * ROWS_REC, nullptr))) return r;
    }
    p->rows_bytes = n * ROWS_REC * PTS_BYTES;
    return C25519_OK;
}

// The whole call on device inputs; the arguments have been checked (rows_check) and m > 0.  h_out (host form; may be null): where d_out is
// copied before the one synchronisation.
static int32_t rows_run(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *d_scalars, uint64_t m, uint64_t w, int32_t route, int out_fmt, uint8_t *d_out, uint8_t *h_out) {
    hipStream_t st = ctx->stream;
    uint32_t *flags = (uint32_t *)ctx->d_flag;
    auto enqueue = [&]() -> int32_t {
        int32_t r;
        HIPCHK(hipEventRecord(ctx->ev0, st));
        // tmp_f: the raw sums (compressed output only); a first call's build has its scratch there before them, in stream order (reserved in this
        // order, so the buffer never moves under queued work)
        if (out_fmt != C25519_FMT_RAW160 && (r = ctx_reserve(ctx, ctx->tmp_f, al256(m * 160) + 256))) return r;
        if ((r = rows_build(ctx, p))) return r;
        uint8_t *sums = out_fmt == C25519_FMT_RAW160 ? d_out : (uint8_t *)ctx->tmp_f.p;
        HIPCHK(hipMemsetAsync(flags, 0, 8, st));
        if (route == C25519_PRECOMP_ROWS_LANE) {
            ctx->kname[0] = "c25519::k_mid_rows_lane (one lane per row over the handle's comb table)";
            hipLaunchKernelGGL(k_mid_rows_lane, dim3(div_up(m, 64)), dim3(64), 0, st, d_scalars, m, (u32)w, (const u32 *)p->d_rows, sums, flags);
        } else {                                             // four waves, so four rows, per block
            ctx->kname[0] = "c25519::k_mid_rows_wave (one wave per row, lane l takes window l; the partial sums folded by shuffles)";
            hipLaunchKernelGGL(k_mid_rows_wave, dim3(div_up(m, 4)), dim3(256), 0, st, d_scalars, (u32)m, (u32)w, (const u32 *)p->d_rows, sums, flags);
        }
        HIPCHK(hipGetLastError());
        return straus_finish_enqueue(ctx, sums, m, out_fmt, d_out, nullptr, h_out, nullptr);
    };
    return straus_finish_wait(ctx, enqueue(), false);      // (no kernel of this call raises the NONE word: the handle's points were decoded at its creation)
}

EXPORT int32_t c25519_precomp_msm_vartime_rows_dev(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *d_scalars, uint64_t m, uint64_t w, int32_t route, int out_fmt,
                                                   uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r, kernel = 0;
    if ((r = rows_check(ctx, p, m, w, route, out_fmt, kernel))) return r;
    if (m == 0) return C25519_OK;
    return rows_run(ctx, p, d_scalars, m, w, kernel, out_fmt, d_out, nullptr);
}

EXPORT int32_t c25519_precomp_msm_vartime_rows(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *scalars, uint64_t m, uint64_t w, int32_t route, int out_fmt,
                                               uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r, kernel = 0;
    if ((r = rows_check(ctx, p, m, w, route, out_fmt, kernel))) return r;
    if (m == 0) return C25519_OK;
    const size_t ob = point_bytes(out_fmt), sb = (size_t)(m * w) * 32;       // (w <= 4096 and m < 2^32: no overflow)
    if ((r = ctx_reserve(ctx, ctx->tmp_a, sb + 16)) || (r = ctx_reserve(ctx, ctx->tmp_c, m * ob + 16))) return r;
    ffi_small_begin(ctx);
    uint8_t *d_s = (uint8_t *)ctx->tmp_a.p, *d_out = (uint8_t *)ctx->tmp_c.p;
    if ((r = straus_upload_all(ctx, {{d_s, scalars, sb}}))) return r;
    r = rows_run(ctx, p, d_s, m, w, kernel, out_fmt, d_out, out);
    ffi_small_end(ctx, sb, m * ob);
    return r;
}
