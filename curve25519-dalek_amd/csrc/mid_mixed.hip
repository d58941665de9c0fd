// Many MIXED multiscalar multiplications over ONE precomputed point set in one call:
//   out[r] = sum_{j < w} static_scalars[r][j] * S_j  +  sum_{i in [dyn_off[r], dyn_off[r+1])} dyn_scalars[i] * dyn_points[i],   r < m
// -- one VartimePrecomputedMultiscalarMul::vartime_mixed_multiscalar_mul (traits.rs:304-419, precomputed_straus.rs:29-127) per row: the
// verification equation of a range proof, a Schnorr / DLEQ / Pedersen-opening check, by the thousand.  DESIGN.md section 3.16.
//
//   c25519_precomp_msm_vartime_mixed_rows_dev / c25519_precomp_msm_vartime_mixed_rows / c25519_precomp_msm_vartime_mixed_rows_plan
//
// The dynamic half of a row is Straus with a shared doubling chain over per-term tables (mid_seg.hip; the per-term preparation is
// seg_tables.h, shared with it); the static half needs no doubling -- the records of the handle's comb table (mid_rows.hip rows_build) are
// already scaled by 16^k -- so it is added into the accumulator the window loop leaves behind, AFTER the last doubling: one accumulator per
// lane, one fold, one store per row.
//   k_mid_mixed_tables   one lane per dynamic term of a pass: seg_tables_term (ok byte, {1 .. 8} P, the 64 digit bytes, the bit-255 flag)
//   k_mid_mixed_wave     one WAVE per row: lane l runs the window loop of k_mid_seg_wave over dynamic terms l, l + 64, ... of the row, then the
//                        loop of k_mid_rows_wave -- for every static column j the comb record (j, window l, |digit|) -- into the same accumulator;
//                        one six-round shuffle fold; lane 0 stores the sum and the row's verdict
//   k_mid_mixed_lane     one LANE per row, 64 consecutive rows per wave: the loop of k_mid_seg_straus over the row's dynamic terms (any length),
//                        then the loop of k_mid_rows_lane over its static scalars
// A row without dynamic terms skips the doubling chain altogether.  Complete formulas throughout (no special case for identity, equal or
// opposite operands); a zero digit is skipped.  The scalars are public by contract (a *_vartime entry point): branches and table addresses
// depend on their digits.  Every loop bound comes from the m, w and offsets the host validated; no LDS, no barrier, no atomics, no waiting
// (the two verdict words are set by plain stores of 1).  Compressed outputs go through c25519_compress_batch_dev: no inversion here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include <vector>
#include "../../include/c25519_hip.h"
#include "devio.h"
#include "kernels.h"
#include "ctx.h"
#include "msm_internal.h"
#include "precomp.h"
#include "rows_digits.h"
#include "seg_tables.h"
#include "ffi.h"
#include "knobs.h"
#include "capi_util.h"

using namespace c25519;

namespace c25519 {

template <int IN>
__global__ void __launch_bounds__(256) k_mid_mixed_tables(const uint8_t *__restrict__ scalars, const uint8_t *__restrict__ points, u64 t0, u64 cnt,
                                                          uint4 *__restrict__ tab, uint4 *__restrict__ dig, uint8_t *__restrict__ tok, u32 *__restrict__ flags) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    seg_tables_term<IN>(scalars, points, t0 + i, i, tab, dig, tok, flags);
}

// acc + / - entry |dg| of record i of the pass, for a digit dg != 0 (-8 .. 8)
__device__ __forceinline__ ge_p3 mixed_add_dyn(const ge_p3 &acc, const uint4 *__restrict__ tab, u64 i, int dg) {
    const bool neg = dg < 0;
    const u32 mag = (u32)(neg ? -dg : dg);                  // 1 .. 8
    return ge_p1p1_to_p3(ge_add_cached(acc, ge_cached_cneg(seg_tab_load(tab, i, (mag - 1u) & 7u), neg)));
}
// acc + / - comb record (j, k, |dg|) of the handle, for a digit dg != 0
__device__ __forceinline__ ge_p3 mixed_add_comb(const ge_p3 &acc, const u32 *__restrict__ comb, u32 j, u32 k, int dg) {
    const bool neg = dg < 0;
    const u32 mag = (u32)(neg ? -dg : dg);                  // 1 .. 8
    return ge_madd_signed_p3(acc, pts_load(comb, ((u64)j * ROWS_WIN + k) * ROWS_ENT + ((mag - 1u) & 7u)), neg);
}

// Wave v of the launch (four per block) takes row r0 + v of the call, v < cnt; its dynamic terms are records [dyn_off[r] - t0, dyn_off[r + 1] - t0)
// of the pass (nt records), its static scalars sscal[r * w .. r * w + w).  comb holds at least w * 512 records (the host checked w against the
// handle).  The row index, the offsets and every loop bound are wave-uniform (readfirstlane: SGPRs); only the term predicate, the digits and
// the zero-digit skip depend on the lane.  The comb additions come after the doubling chain has ended: their records are already scaled.
__global__ void __launch_bounds__(256) k_mid_mixed_wave(const u64 *__restrict__ dyn_off, u32 r0, u32 cnt, u64 t0, u64 nt, const uint4 *__restrict__ tab,
                                                        const int8_t *__restrict__ dig, const uint8_t *__restrict__ tok, const uint8_t *__restrict__ sscal, u32 w,
                                                        const u32 *__restrict__ comb, uint8_t *__restrict__ out_raw, uint8_t *__restrict__ ok, u32 *__restrict__ flags) {
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (wv >= cnt) return;
    const u32 lane = threadIdx.x & 63u;
    const u32 r = r0 + wv;
    const u64 a = dyn_off[r], b = dyn_off[(u64)r + 1];
    if (a < t0 || b < a || b - t0 > nt || b - a > 0xffffffc0ull) return;
    const u64 lo = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)((a - t0) >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)(a - t0));
    const u32 len = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(b - a)), rounds = (len + 63u) >> 6;
    u32 good = 1;
    ge_p3 acc = ge_identity();
    if (len) {
        for (u32 q = 0; q < rounds; q++) {
            const u32 j = 64u * q + lane;
            if (j < len) good &= (u32)tok[lo + j];
        }
#pragma unroll 1
        for (int k = SEG_DIG - 1; k >= 0; k--) {
            if (k != SEG_DIG - 1) acc = ge_mul_by_pow_2(acc, 4);
#pragma unroll 1
            for (u32 q = 0; q < rounds; q++) {
                const u32 j = 64u * q + lane;
                if (j < len) {
                    const int dg = (int)dig[(lo + j) * SEG_DIG + (u64)k];
                    if (dg != 0) acc = mixed_add_dyn(acc, tab, lo + j, dg);
                }
            }
            ge_pin(acc);
        }
    }
    // the static half: lane l is window l of every scalar of the row
    const u32 word = lane >> 3, shift = 4u * (lane & 7u);
#pragma unroll 1
    for (u32 j = 0; j < w; j++) {
        u32 s[8];
        load8(sscal, (u64)r * w + j, s);
        if (rows_recode(s)) flags[SEG_FLAG_BIT255] = 1u;
        u32 mine = s[0];
        for (u32 q = 1; q < 8; q++) mine = word == q ? s[q] : mine;
        const int dg = rows_digit((mine >> shift) & 15u, (int)lane);
        if (dg != 0) acc = mixed_add_comb(acc, comb, j, lane, dg);
        ge_pin(acc);
    }
#pragma unroll 1
    for (int off = 32; off > 0; off >>= 1) acc = ge_add(acc, ge_shfl_down(acc, off));
    const bool all_good = __all((int)good) != 0;
    if (lane == 0) {
        raw160_store(out_raw, r, acc);
        ok[r] = all_good ? 1 : 0;
        if (!all_good) flags[SEG_FLAG_NONE] = 1u;
    }
}

// Lane i of the launch takes row r0 + i of the call, i < cnt (64 consecutive rows per wave, four waves per block: one per SIMD of a CU); records and scalars as for
// k_mid_mixed_wave.  Correct for any dynamic length: the window loop runs over all terms of the row.
__global__ void __launch_bounds__(256) k_mid_mixed_lane(const u64 *__restrict__ dyn_off, u64 r0, u64 cnt, u64 t0, u64 nt, const uint4 *__restrict__ tab,
                                                        const int8_t *__restrict__ dig, const uint8_t *__restrict__ tok, const uint8_t *__restrict__ sscal, u32 w,
                                                        const u32 *__restrict__ comb, uint8_t *__restrict__ out_raw, uint8_t *__restrict__ ok, u32 *__restrict__ flags) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const u64 r = r0 + i, a = dyn_off[r], b = dyn_off[r + 1];
    if (a < t0 || b < a || b - t0 > nt || b - a > 0xffffffffull) return;
    const u64 lo = a - t0;
    const u32 len = (u32)(b - a);
    u32 good = 1;
    ge_p3 acc = ge_identity();
    if (len) {
        for (u32 j = 0; j < len; j++) good &= (u32)tok[lo + j];
#pragma unroll 1
        for (int k = SEG_DIG - 1; k >= 0; k--) {
            if (k != SEG_DIG - 1) acc = ge_mul_by_pow_2(acc, 4);
#pragma unroll 1
            for (u32 j = 0; j < len; j++) {
                const int dg = (int)dig[(lo + j) * SEG_DIG + (u64)k];
                if (dg != 0) acc = mixed_add_dyn(acc, tab, lo + j, dg);
            }
            ge_pin(acc);
        }
    }
    // the static half: all lanes of a wave are on the same (j, k) at the same time
#pragma unroll 1
    for (u32 j = 0; j < w; j++) {
        u32 s[8];
        load8(sscal, r * w + j, s);
        if (rows_recode(s)) flags[SEG_FLAG_BIT255] = 1u;
        u32 cur = s[0];
#pragma unroll 1
        for (int k = 0; k < ROWS_WIN; k++) {
            const u32 nib = cur & 15u;
            cur >>= 4;
            if ((k & 7) == 7) {                              // the next word moves down: no register array is indexed by k
                for (int q = 0; q < 7; q++) s[q] = s[q + 1];
                cur = s[0];
            }
            const int dg = rows_digit(nib, k);
            if (dg != 0) acc = mixed_add_comb(acc, comb, j, (u32)k, dg);
            ge_pin(acc);
        }
    }
    raw160_store(out_raw, r, acc);
    ok[r] = (uint8_t)good;
    if (!good) flags[SEG_FLAG_NONE] = 1u;
}

}  // namespace c25519

// ---- host side ----------------------------------------------------------------------------------------------------------------
// (ctx may be null: c25519_precomp_msm_vartime_mixed_rows_plan has none, and then only the code is returned)
static int32_t mixed_bad(c25519_ctx *ctx, const char *what) { return ctx ? bad_arg(ctx, what) : -(int32_t)hipErrorInvalidValue; }

// ---- routing: the one place that validates the shape, chooses the row kernel of AUTO and cuts the passes ----
// AUTO, with t = w + the longest row's dynamic terms (measured: DESIGN.md section 3.16):
//   w >= LANE_WIDTH                         wave
//   no row has a dynamic term               the rule of the rows call: lane iff m >= LANE_MIN_ROWS (the call IS the rows call then)
//   the longest row above MIXED_LANE_DYN_MAX   wave
//   otherwise                               lane iff m >= MIXED_LANE_BASE_ROWS + MIXED_LANE_ROWS_PER_TERM * t
// A pass is a run of consecutive rows of at most seg_pass_terms() dynamic terms in all (one row always fits: a row has at most seg_wave_max() of
// them).
static uint64_t mixed_lane_dyn_max() { static const uint64_t v = (uint64_t)std::max<long long>(0, C25519_KNOB_LL("MIXED_LANE_DYN_MAX", C25519_PRECOMP_MIXED_LANE_DYN_MAX)); return v; }
static uint64_t mixed_lane_base_rows() { static const uint64_t v = (uint64_t)std::max<long long>(0, C25519_KNOB_LL("MIXED_LANE_BASE_ROWS", C25519_PRECOMP_MIXED_LANE_BASE_ROWS)); return v; }
static uint64_t mixed_lane_rows_per_term() {
    static const uint64_t v = (uint64_t)std::max<long long>(0, C25519_KNOB_LL("MIXED_LANE_ROWS_PER_TERM", C25519_PRECOMP_MIXED_LANE_ROWS_PER_TERM));
    return v;
}
struct mixed_pass { uint64_t r0, r1; };                    // rows [r0, r1), dynamic terms [dyn_off[r0], dyn_off[r1])
struct mixed_route {
    int32_t route = C25519_PRECOMP_ROWS_WAVE;               // what AUTO takes
    uint64_t lane_waves = 0, n_pass = 0, maxt = 0;          // waves of the lane route's row launches; passes; most dynamic terms in one pass
    std::vector<mixed_pass> passes;                         // only when asked for (mixed_run)
};
static int32_t mixed_plan(c25519_ctx *ctx, uint64_t m, uint64_t w, const uint64_t *dyn_off, bool lists, mixed_route &R) {
    if (m >= 0xffffffffull) return mixed_bad(ctx, "precomp_msm_vartime_mixed_rows: m must be below 2^32 - 1");      // before dyn_off[m] is read
    if (w && m > UINT64_MAX / w) return mixed_bad(ctx, "precomp_msm_vartime_mixed_rows: m * w overflows");
    if (m == 0) return C25519_OK;
    if (!dyn_off || dyn_off[0] != 0) return mixed_bad(ctx, "precomp_msm_vartime_mixed_rows: dyn_off must run from 0 to n_dyn");
    const uint64_t wmax = seg_wave_max(), ptmax = seg_pass_terms();
    uint64_t r0 = 0, terms = 0, longest = 0;
    auto close = [&](uint64_t r1) {
        if (r1 > r0) {
            R.n_pass++; R.maxt = std::max(R.maxt, terms); R.lane_waves += (r1 - r0 + 63) / 64;
            if (lists) R.passes.push_back({r0, r1});
        }
        terms = 0; r0 = r1;
    };
    for (uint64_t r = 0; r < m; r++) {
        if (dyn_off[r + 1] < dyn_off[r]) return mixed_bad(ctx, "precomp_msm_vartime_mixed_rows: dyn_off must be non-decreasing");
        const uint64_t len = dyn_off[r + 1] - dyn_off[r];
        if (len > wmax)
            return mixed_bad(ctx, "precomp_msm_vartime_mixed_rows: a row has more than C25519_MSM_SEGMENT_WAVE_MAX dynamic terms; run such a row through "
                                  "c25519_precomp_msm_vartime");
        if (terms + len > ptmax) close(r);
        terms += len;
        longest = std::max(longest, len);
    }
    close(m);
    if (dyn_off[m] >= (1ull << 40)) return mixed_bad(ctx, "precomp_msm_vartime_mixed_rows: n_dyn must be < 2^40");
    bool lane = false;                                      // (w < LANE_WIDTH and longest <= wmax: the sum below cannot overflow)
    if (w >= C25519_PRECOMP_ROWS_LANE_WIDTH) lane = false;
    else if (longest == 0) lane = m >= C25519_PRECOMP_ROWS_LANE_MIN_ROWS;
    else lane = longest <= mixed_lane_dyn_max() && m >= mixed_lane_base_rows() + mixed_lane_rows_per_term() * (w + longest);
    R.route = lane ? C25519_PRECOMP_ROWS_LANE : C25519_PRECOMP_ROWS_WAVE;
    return C25519_OK;
}

EXPORT int32_t c25519_precomp_msm_vartime_mixed_rows_plan(uint64_t m, uint64_t w, const uint64_t *dyn_off, uint64_t plan[4]) {
    mixed_route R;
    const int32_t r = mixed_plan(nullptr, m, w, dyn_off, false, R);
    if (r) return r;
    plan[0] = (uint64_t)R.route; plan[1] = R.route == C25519_PRECOMP_ROWS_LANE ? R.lane_waves : m; plan[2] = R.n_pass; plan[3] = R.maxt;
    return C25519_OK;
}

// everything that is refused before any launch; R: the passes and the route AUTO takes
static int32_t mixed_check(c25519_ctx *ctx, const c25519_precomp *p, uint64_t m, uint64_t w, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off, int32_t route,
                           int out_fmt, mixed_route &R) {
    if (!p) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: no handle");
    if (out_fmt < 0 || out_fmt > 2) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: bad out_fmt");
    if (route != C25519_PRECOMP_ROWS_AUTO && route != C25519_PRECOMP_ROWS_LANE && route != C25519_PRECOMP_ROWS_WAVE)
        return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: unknown route");
    if (p->n > C25519_PRECOMP_ROWS_MAX_POINTS)
        return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: the handle has more than 4096 static points; run it through c25519_precomp_msm_vartime, row by row");
    if (w > p->n) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: more static scalars per row than static points (precomputed_straus.rs:86)");
    const bool pair = in_fmt == C25519_FMT_EDWARDS_Y ? ed_fmt_ok(out_fmt)
                    : in_fmt == C25519_FMT_RISTRETTO ? ris_fmt_ok(out_fmt)
                    : in_fmt == C25519_FMT_RAW160 && (ed_fmt_ok(out_fmt) || out_fmt == C25519_FMT_RISTRETTO);
    if (!pair) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: in_fmt and out_fmt must belong to one group");
    if (n_dyn >= (1ull << 40)) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: n_dyn must be < 2^40");
    if (m && m < 0xffffffffull && (!dyn_off || dyn_off[m] != n_dyn)) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: dyn_off must run from 0 to n_dyn");
    return mixed_plan(ctx, m, w, dyn_off, true, R);
}

// The whole call on device inputs; the arguments have been checked (mixed_check) and m > 0.  h_out / h_ok (host form; may be null): where
// d_out / the ok bytes are copied before the one synchronisation.
static int32_t mixed_run(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *d_ss, uint64_t m, uint64_t w, const uint8_t *d_ds, const uint8_t *d_dp, int in_fmt,
                         const uint64_t *dyn_off, const mixed_route &R, int32_t route, int out_fmt, uint8_t *d_out, uint8_t *d_ok, uint8_t *h_out, uint8_t *h_ok) {
    hipStream_t st = ctx->stream;
    const size_t ob = point_bytes(out_fmt);
    // tmp_f: dyn_off | raw sums (compressed output only) | ok (without d_ok) | tables | digits | term ok bytes.  A first call's build has its scratch
    // there before them, in stream order (reserved in this order, so the buffer never moves under queued work)
    const size_t b_off = seg_al256((m + 1) * 8), b_sum = out_fmt == C25519_FMT_RAW160 ? 0 : seg_al256(m * 160), b_ok = d_ok ? 0 : seg_al256(m);
    const size_t b_tab = seg_al256(R.maxt * SEG_ENT * SEG_ENT_Q * 16), b_dig = seg_al256(R.maxt * SEG_DIG), b_tok = seg_al256(R.maxt);
    uint32_t *flags = (uint32_t *)ctx->d_flag;
    uint32_t *verdict = (uint32_t *)ctx->h_msm;           // pinned
    auto enqueue = [&]() -> int32_t {
        int32_t r;
        HIPCHK(hipEventRecord(ctx->ev0, st));
        if ((r = ctx_reserve(ctx, ctx->tmp_f, b_off + b_sum + b_ok + b_tab + b_dig + b_tok + 256))) return r;
        if ((r = rows_build(ctx, p))) return r;
        uint8_t *base = (uint8_t *)ctx->tmp_f.p;
        uint64_t *d_off = (uint64_t *)base;
        uint8_t *sums = out_fmt == C25519_FMT_RAW160 ? d_out : base + b_off;
        uint8_t *okbuf = d_ok ? d_ok : base + b_off + b_sum;
        uint4 *tab = (uint4 *)(base + b_off + b_sum + b_ok);
        uint8_t *dig = base + b_off + b_sum + b_ok + b_tab, *tok = dig + b_dig;
        HIPCHK(hipMemsetAsync(flags, 0, 8, st));
        HIPCHK(hipMemcpyAsync(d_off, dyn_off, (m + 1) * 8, hipMemcpyHostToDevice, st));
        ctx->kname[0] = route == C25519_PRECOMP_ROWS_LANE ? "c25519::k_mid_mixed_lane (one lane per row: its dynamic terms by Straus, then its static scalars over the comb table)"
                                                          : "c25519::k_mid_mixed_wave (one wave per row: dynamic terms by Straus, static scalars over the comb table, one fold)";
        for (const mixed_pass &ps : R.passes) {
            const uint64_t t0 = dyn_off[ps.r0], nt = dyn_off[ps.r1] - t0, nr = ps.r1 - ps.r0;
            if (nt) {
                const dim3 g(div_up(nt, 256)), b(256);
                if (in_fmt == C25519_FMT_EDWARDS_Y) hipLaunchKernelGGL(k_mid_mixed_tables<0>, g, b, 0, st, d_ds, d_dp, t0, nt, tab, (uint4 *)dig, tok, flags);
                else if (in_fmt == C25519_FMT_RISTRETTO) hipLaunchKernelGGL(k_mid_mixed_tables<1>, g, b, 0, st, d_ds, d_dp, t0, nt, tab, (uint4 *)dig, tok, flags);
                else hipLaunchKernelGGL(k_mid_mixed_tables<2>, g, b, 0, st, d_ds, d_dp, t0, nt, tab, (uint4 *)dig, tok, flags);
                HIPCHK(hipGetLastError());
            }
            if (route == C25519_PRECOMP_ROWS_LANE)
                hipLaunchKernelGGL(k_mid_mixed_lane, dim3(div_up(nr, 256)), dim3(256), 0, st, (const u64 *)d_off, ps.r0, nr, t0, nt, (const uint4 *)tab, (const int8_t *)dig,
                                   (const uint8_t *)tok, d_ss, (u32)w, (const u32 *)p->d_rows, sums, okbuf, flags);
            else                                             // four waves, so four rows, per block
                hipLaunchKernelGGL(k_mid_mixed_wave, dim3(div_up(nr, 4)), dim3(256), 0, st, (const u64 *)d_off, (u32)ps.r0, (u32)nr, t0, nt, (const uint4 *)tab,
                                   (const int8_t *)dig, (const uint8_t *)tok, d_ss, (u32)w, (const u32 *)p->d_rows, sums, okbuf, flags);
            HIPCHK(hipGetLastError());
        }
        if (out_fmt != C25519_FMT_RAW160 && (r = c25519_compress_batch_dev(ctx, sums, m, out_fmt, d_out))) return r;
        HIPCHK(hipEventRecord(ctx->ev1, st));
        HIPCHK(hipMemcpyAsync(verdict, flags, 8, hipMemcpyDeviceToHost, st));
        if (h_out) HIPCHK(hipMemcpyAsync(h_out, d_out, m * ob, hipMemcpyDeviceToHost, st));
        if (h_ok) HIPCHK(hipMemcpyAsync(h_ok, okbuf, m, hipMemcpyDeviceToHost, st));
        return C25519_OK;
    };
    const int32_t r = enqueue();
    if (r) { (void)hipStreamSynchronize(st); return r; }   // no queued copy still reads host memory after the return
    HIPCHK(hipStreamSynchronize(st));
    if (verdict[SEG_FLAG_BIT255]) return bad_arg(ctx, "msm: a scalar has bit 255 set (Scalar invariant #1 violated)");
    return verdict[SEG_FLAG_NONE] ? C25519_NONE : C25519_OK;
}

EXPORT int32_t c25519_precomp_msm_vartime_mixed_rows_dev(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *d_static_scalars, uint64_t m, uint64_t w,
                                                         const uint8_t *d_dyn_scalars, const uint8_t *d_dyn_points, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off,
                                                         int32_t route, int out_fmt, uint8_t *d_out, uint8_t *d_ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    mixed_route R;
    if ((r = mixed_check(ctx, p, m, w, n_dyn, in_fmt, dyn_off, route, out_fmt, R))) return r;
    if (m == 0) return C25519_OK;
    return mixed_run(ctx, p, d_static_scalars, m, w, d_dyn_scalars, d_dyn_points, in_fmt, dyn_off, R, route == C25519_PRECOMP_ROWS_AUTO ? R.route : route, out_fmt, d_out,
                     d_ok, nullptr, nullptr);
}

EXPORT int32_t c25519_precomp_msm_vartime_mixed_rows(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *static_scalars, uint64_t m, uint64_t w, const uint8_t *dyn_scalars,
                                                     const uint8_t *dyn_points, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off, int32_t route, int out_fmt,
                                                     uint8_t *out, uint8_t *ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    mixed_route R;
    if ((r = mixed_check(ctx, p, m, w, n_dyn, in_fmt, dyn_off, route, out_fmt, R))) return r;
    if (m == 0) return C25519_OK;
    const size_t pb = point_bytes(in_fmt), ob = point_bytes(out_fmt), sb = (size_t)(m * w) * 32;       // (w <= 4096 and m < 2^32: no overflow)
    if ((r = ctx_reserve(ctx, ctx->tmp_a, sb + 16)) || (r = ctx_reserve(ctx, ctx->tmp_b, n_dyn * 32 + 16)) || (r = ctx_reserve(ctx, ctx->tmp_c, n_dyn * pb + 16)) ||
        (r = ctx_reserve(ctx, ctx->tmp_d, seg_al256(m * ob) + m + 16)))
        return r;
    ffi_small_begin(ctx);
    uint8_t *d_ss = (uint8_t *)ctx->tmp_a.p, *d_ds = (uint8_t *)ctx->tmp_b.p, *d_dp = (uint8_t *)ctx->tmp_c.p, *d_out = (uint8_t *)ctx->tmp_d.p, *d_ok = d_out + seg_al256(m * ob);
    hipError_t e = hipSuccess;
    if (sb) e = hipMemcpyAsync(d_ss, static_scalars, sb, hipMemcpyHostToDevice, ctx->stream);
    if (n_dyn && e == hipSuccess) e = hipMemcpyAsync(d_ds, dyn_scalars, n_dyn * 32, hipMemcpyHostToDevice, ctx->stream);
    if (n_dyn && e == hipSuccess) e = hipMemcpyAsync(d_dp, dyn_points, n_dyn * pb, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return c25519_fail(ctx, e, "hipMemcpyAsync(inputs)"); }
    r = mixed_run(ctx, p, d_ss, m, w, d_ds, d_dp, in_fmt, dyn_off, R, route == C25519_PRECOMP_ROWS_AUTO ? R.route : route, out_fmt, d_out, d_ok, out, ok);
    if (r < 0) (void)hipStreamSynchronize(ctx->stream);    // (an early error: the uploads may still be reading the caller's memory)
    ffi_small_end(ctx, sb + n_dyn * (32 + pb) + (m + 1) * 8, m * ob + (ok ? m : 0));
    return r;
}
