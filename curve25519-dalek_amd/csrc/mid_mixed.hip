// Many MIXED multiscalar multiplications over ONE precomputed point set in one call:
//   out[r] = sum_{j < w} static_scalars[r][j] * S_j  +  sum_{i in [dyn_off[r], dyn_off[r+1])} dyn_scalars[i] * dyn_points[i],   r < m
// -- one VartimePrecomputedMultiscalarMul::vartime_mixed_multiscalar_mul (traits.rs:304-419, precomputed_straus.rs:29-127) per row: the
// verification equation of a range proof, a Schnorr / DLEQ / Pedersen-opening check, by the thousand.  DESIGN.md section 3.16.
//
//   c25519_precomp_msm_vartime_mixed_rows_dev / c25519_precomp_msm_vartime_mixed_rows / c25519_precomp_msm_vartime_mixed_rows_plan
//
// The dynamic half of a row is Straus with a shared doubling chain over per-term tables, as in mid_seg.hip; the static half needs no
// doubling -- the records of the handle's comb table (mid_rows.hip rows_build) are already scaled by 16^k -- so it is added into the
// accumulator the window loop leaves behind, AFTER the last doubling: one accumulator per lane, one fold, one store per row.  Both halves,
// the per-term preparation and the fold are the functions of straus.h that the segments call and the rows call run.
//   k_mid_straus_tables  (emitted by mid_seg.hip) one lane per dynamic term of a pass: seg_tables_term (ok byte, {1 .. 8} P, the 64 digit bytes, the bit-255 flag)
//   k_mid_mixed_wave     one WAVE per row: straus_dyn_wave -- lane l runs the window loop over dynamic terms l, l + 64, ... of the row --, then
//                        straus_comb_wave -- for every static column j the comb record (j, window l, |digit|) -- into the same accumulator;
//                        one six-round shuffle fold; lane 0 stores the sum and the row's verdict
//   k_mid_mixed_lane     one LANE per row, 64 consecutive rows per wave: straus_dyn_lane over the row's dynamic terms (any length), then
//                        straus_comb_lane over its static scalars
// A row without dynamic terms skips the doubling chain altogether.  Complete formulas throughout (no special case for identity, equal or
// opposite operands); a zero digit is skipped.  The scalars are public by contract (a *_vartime entry point): branches and table addresses
// depend on their digits.  Every loop bound comes from the m, w and offsets the host validated; no LDS, no barrier, no atomics, no waiting
// (the two verdict words are set by plain stores of 1).  Compressed outputs go through c25519_compress_batch_dev: no inversion here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include <vector>
#include "msm_internal.h"
#include "straus.h"                         // (and through it devio.h, kernels.h, ctx.h, knobs.h, precomp.h, rows_digits.h, capi_util.h)
#include "ffi.h"

using namespace c25519;

namespace c25519 {

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
    const u32 len = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(b - a));
    u32 good = 1;
    ge_p3 acc = ge_identity();
    if (len) straus_dyn_wave(acc, good, tab, dig, tok, lo, len, lane);      // (a row without dynamic terms skips the doubling chain)
    straus_comb_wave(acc, sscal, (u64)r * w, w, comb, lane, flags);
    straus_wave_store(out_raw, ok, flags, r, straus_wave_fold(acc), good, lane);
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
    if (len) straus_dyn_lane(acc, good, tab, dig, tok, lo, len);            // (a row without dynamic terms skips the doubling chain)
    // The loop of straus_comb_lane, written out: called as that function the shift of the scalar's words compiles to a branch where this form
    // gets eight conditional moves (44 against 48 vector instructions per window, profiles/straus_family_isa.txt), and the call measured 3.6 %
    // slower at 131072 x (2 + 1) (k_mid_rows_lane, alone with that loop, is faster in the function's form).  A change there belongs here too.
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
            if (dg != 0) acc = straus_add_comb(acc, comb, j, (u32)k, dg);
            ge_pin(acc);
        }
    }
    raw160_store(out_raw, r, acc);
    ok[r] = (uint8_t)good;
    if (!good) flags[SEG_FLAG_NONE] = 1u;
}

}  // namespace c25519

// ---- host side ----------------------------------------------------------------------------------------------------------------
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
static const off_msgs MIXED_OFF_MSGS = OFF_MSGS("precomp_msm_vartime_mixed_rows", "dyn_off", "n_dyn",
                                                "precomp_msm_vartime_mixed_rows: a row has more than C25519_MSM_SEGMENT_WAVE_MAX dynamic terms; run such a row through "
                                                "c25519_precomp_msm_vartime");
static int32_t mixed_plan(c25519_ctx *ctx, uint64_t m, uint64_t w, uint64_t n_dyn, const uint64_t *dyn_off, bool lists, mixed_route &R) {
    int32_t q;
    if ((q = check_offsets(ctx, MIXED_OFF_MSGS, n_dyn, dyn_off, m, seg_wave_max()))) return q;
    // (this refusal used to come ahead of the offsets': with a context w <= p->n <= 4096 and m < 2^32 have been checked before, so it cannot be
    // met; without one every refusal is the same status)
    if (w && m > UINT64_MAX / w) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: m * w overflows");
    if (m == 0) return C25519_OK;
    const uint64_t ptmax = seg_pass_terms();
    uint64_t r0 = 0, terms = 0, longest = 0;
    auto close = [&](uint64_t r1) {
        if (r1 > r0) {
            R.n_pass++; R.maxt = std::max(R.maxt, terms); R.lane_waves += (r1 - r0 + 63) / 64;
            if (lists) R.passes.push_back({r0, r1});
        }
        terms = 0; r0 = r1;
    };
    for (uint64_t r = 0; r < m; r++) {
        const uint64_t len = dyn_off[r + 1] - dyn_off[r];
        if (terms + len > ptmax) close(r);
        terms += len;
        longest = std::max(longest, len);
    }
    close(m);
    bool lane;                                              // (w < LANE_WIDTH and longest <= seg_wave_max(): the sum below cannot overflow)
    if (longest == 0) lane = rows_lane_route(m, w);
    else lane = w < C25519_PRECOMP_ROWS_LANE_WIDTH && longest <= mixed_lane_dyn_max() && m >= mixed_lane_base_rows() + mixed_lane_rows_per_term() * (w + longest);
    R.route = lane ? C25519_PRECOMP_ROWS_LANE : C25519_PRECOMP_ROWS_WAVE;
    return C25519_OK;
}

EXPORT int32_t c25519_precomp_msm_vartime_mixed_rows_plan(uint64_t m, uint64_t w, const uint64_t *dyn_off, uint64_t plan[4]) {
    mixed_route R;
    const int32_t r = mixed_plan(nullptr, m, w, offsets_end(dyn_off, m), dyn_off, false, R);
    if (r) return r;
    plan[0] = (uint64_t)R.route; plan[1] = R.route == C25519_PRECOMP_ROWS_LANE ? R.lane_waves : m; plan[2] = R.n_pass; plan[3] = R.maxt;
    return C25519_OK;
}

// everything that is refused before any launch; R: the passes and the route AUTO takes
static int32_t mixed_check(c25519_ctx *ctx, const c25519_precomp *p, uint64_t m, uint64_t w, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off, int32_t route,
                           int out_fmt, mixed_route &R) {
    static const rows_msgs msgs = ROWS_MSGS("precomp_msm_vartime_mixed_rows", "static scalars");
    int32_t r;
    if ((r = rows_check_handle(ctx, msgs, p, w, route, out_fmt))) return r;
    if (!fmt_pair_ok(in_fmt, out_fmt)) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows: in_fmt and out_fmt must belong to one group");
    if (n_dyn >= (1ull << 40)) return bad_arg(ctx, MIXED_OFF_MSGS.n);       // (ahead of m, as this call has always refused)
    return mixed_plan(ctx, m, w, n_dyn, dyn_off, true, R);
}

// The whole call on device inputs; the arguments have been checked (mixed_check) and m > 0.  h_out / h_ok (host form; may be null): where
// d_out / the ok bytes are copied before the one synchronisation.
static int32_t mixed_run(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *d_ss, uint64_t m, uint64_t w, const uint8_t *d_ds, const uint8_t *d_dp, int in_fmt,
                         const uint64_t *dyn_off, const mixed_route &R, int32_t route, int out_fmt, uint8_t *d_out, uint8_t *d_ok, uint8_t *h_out, uint8_t *h_ok) {
    hipStream_t st = ctx->stream;
    // tmp_f (straus_ws): dyn_off | raw sums | ok | tables | digits | term ok bytes.  A first call's build has its scratch there before them, in
    // stream order (reserved in this order, so the buffer never moves under queued work)
    straus_ws ws(m, 0, R.maxt, out_fmt, d_ok != nullptr);
    uint32_t *flags = (uint32_t *)ctx->d_flag;
    auto enqueue = [&]() -> int32_t {
        int32_t r;
        HIPCHK(hipEventRecord(ctx->ev0, st));
        if ((r = ctx_reserve(ctx, ctx->tmp_f, ws.bytes()))) return r;
        if ((r = rows_build(ctx, p))) return r;
        ws.bind(ctx->tmp_f.p, d_out, d_ok);
        HIPCHK(hipMemsetAsync(flags, 0, 8, st));
        HIPCHK(hipMemcpyAsync(ws.d_off, dyn_off, (m + 1) * 8, hipMemcpyHostToDevice, st));
        ctx->kname[0] = route == C25519_PRECOMP_ROWS_LANE ? "c25519::k_mid_mixed_lane (one lane per row: its dynamic terms by Straus, then its static scalars over the comb table)"
                                                          : "c25519::k_mid_mixed_wave (one wave per row: dynamic terms by Straus, static scalars over the comb table, one fold)";
        for (const mixed_pass &ps : R.passes) {
            const uint64_t t0 = dyn_off[ps.r0], nt = dyn_off[ps.r1] - t0, nr = ps.r1 - ps.r0;
            if (nt && (r = straus_launch_tables(ctx, in_fmt, d_ds, d_dp, t0, nt, ws))) return r;
            if (route == C25519_PRECOMP_ROWS_LANE)
                hipLaunchKernelGGL(k_mid_mixed_lane, dim3(div_up(nr, 256)), dim3(256), 0, st, (const u64 *)ws.d_off, ps.r0, nr, t0, nt, (const uint4 *)ws.tab,
                                   (const int8_t *)ws.dig, (const uint8_t *)ws.tok, d_ss, (u32)w, (const u32 *)p->d_rows, ws.sums, ws.okbuf, flags);
            else                                             // four waves, so four rows, per block
                hipLaunchKernelGGL(k_mid_mixed_wave, dim3(div_up(nr, 4)), dim3(256), 0, st, (const u64 *)ws.d_off, (u32)ps.r0, (u32)nr, t0, nt, (const uint4 *)ws.tab,
                                   (const int8_t *)ws.dig, (const uint8_t *)ws.tok, d_ss, (u32)w, (const u32 *)p->d_rows, ws.sums, ws.okbuf, flags);
            HIPCHK(hipGetLastError());
        }
        return straus_finish_enqueue(ctx, ws.sums, m, out_fmt, d_out, ws.okbuf, h_out, h_ok);
    };
    return straus_finish_wait(ctx, enqueue(), false);
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
    ws_layout O; O.part(m * ob);                            // tmp_d: the sums | their ok bytes (the tail: not rounded, and 16 bytes behind it)
    if ((r = ctx_reserve(ctx, ctx->tmp_a, sb + 16)) || (r = ctx_reserve(ctx, ctx->tmp_b, n_dyn * 32 + 16)) || (r = ctx_reserve(ctx, ctx->tmp_c, n_dyn * pb + 16)) ||
        (r = O.reserve(ctx, ctx->tmp_d, m + 16)))
        return r;
    ffi_small_begin(ctx);
    uint8_t *d_ss = (uint8_t *)ctx->tmp_a.p, *d_ds = (uint8_t *)ctx->tmp_b.p, *d_dp = (uint8_t *)ctx->tmp_c.p, *d_out = O.at(0), *d_ok = O.at(O.bytes());
    if ((r = straus_upload_all(ctx, {{d_ss, static_scalars, sb}, {d_ds, dyn_scalars, n_dyn * 32}, {d_dp, dyn_points, n_dyn * pb}}))) return r;
    r = mixed_run(ctx, p, d_ss, m, w, d_ds, d_dp, in_fmt, dyn_off, R, route == C25519_PRECOMP_ROWS_AUTO ? R.route : route, out_fmt, d_out, d_ok, out, ok);
    if (r < 0) (void)hipStreamSynchronize(ctx->stream);    // (an early error: the uploads may still be reading the caller's memory)
    ffi_small_end(ctx, sb + n_dyn * (32 + pb) + (m + 1) * 8, m * ob + (ok ? m : 0));
    return r;
}
