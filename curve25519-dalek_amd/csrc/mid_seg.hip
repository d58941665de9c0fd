// Segmented variable-time multiscalar multiplication: MANY independent sums  out[s] = sum_i scalars[i] * points[i]  over the segments
// [seg_off[s], seg_off[s+1]) of one flat array of terms, in one call (traits.rs:249 VartimeMultiscalarMul, edwards.rs:1002-1031,
// ristretto.rs:984 -- once per segment).  DESIGN.md section 3.13.
//
//   c25519_msm_vartime_segments_dev / c25519_msm_vartime_segments / c25519_msm_vartime_segments_plan
//
// Straus with the doubling chain shared by the terms of a segment (scalar_mul/straus.rs:159-200), one LANE per segment:
//   (the table layout, the tables kernel, the window loops and the three constants live in straus.h, shared with mid_mixed.hip)
//   k_mid_straus_tables   one lane per term: decodes the point, writes its ok byte, the table {1 .. 8} P as eight 160-byte ProjectiveNiels
//                      records (Y+X, Y-X, Z, 2dT) and the 64 signed radix-16 digits of the scalar (scalar.rs:1019-1051), raises the bit-255 flag
//   k_mid_seg_straus   one lane per segment of at most C25519_MSM_SEGMENT_DIRECT_MAX terms (straus_dyn_lane): acc = 16 acc per window, then
//                      + / - entry |d| of every term whose digit d is not zero.  Complete formulas (edwards.rs:797): no special case for equal,
//                      opposite or identity operands.  The sum leaves as a raw 160-byte point.
//   k_mid_seg_wave     one WAVE per segment of at most C25519_MSM_SEGMENT_WAVE_MAX terms (the loop of straus_dyn_wave): lane l takes terms l, l + 64,
//                      l + 128, ... and runs the same window loop over them; the 64 partial sums are folded across the wave with six shuffle
//                      rounds.  (The constant is measured; the kernel itself is correct for any length.)
// Compressed outputs go through c25519_compress_batch_dev (no second inversion here).  Segments longer than the wave maximum and at most
// C25519_MSM_SEGMENT_BUCKET_MAX terms take the bucket route (mid_segb.hip: three launches per pass of such segments); still longer ones run through
// c25519_msm_partial_dev, one call each, and their sums are placed beside the others before that finishing step.
// The scalars are public by contract (a *_vartime entry point): branches and table addresses depend on their digits.  Every loop bound comes
// from the offsets the host validated; the kernels wait for nothing and use no atomics (the two verdict words are set by plain stores of 1).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include <vector>
#include "straus.h"                         // (and through it devio.h, kernels.h, ctx.h, knobs.h, precomp.h, rows_digits.h, capi_util.h)
#include "mid_segb.h"                       // the bucket route: its kernels are in mid_segb.hip
#include "ffi.h"

using namespace c25519;

namespace c25519 {

// the library's one copy of the tables kernel (straus.h declares the three extern)
template __global__ void k_mid_straus_tables<0>(const uint8_t *, const uint8_t *, u64, u64, uint4 *, uint4 *, uint8_t *, u32 *);
template __global__ void k_mid_straus_tables<1>(const uint8_t *, const uint8_t *, u64, u64, uint4 *, uint4 *, uint8_t *, u32 *);
template __global__ void k_mid_straus_tables<2>(const uint8_t *, const uint8_t *, u64, u64, uint4 *, uint4 *, uint8_t *, u32 *);

// Segments [s0, s0 + cnt) of the call, whose terms are records [seg_off[s] - t0, seg_off[s + 1] - t0) of the pass (nt records).  A segment
// that is longer than dmax or does not lie within the records is left alone (the longer ones of a pass belong to k_mid_seg_wave).
__global__ void __launch_bounds__(256) k_mid_seg_straus(const u64 *__restrict__ seg_off, u64 s0, u64 cnt, u64 t0, u64 nt, u32 dmax, const uint4 *__restrict__ tab,
                                                        const int8_t *__restrict__ dig, const uint8_t *__restrict__ tok, uint8_t *__restrict__ out_raw,
                                                        uint8_t *__restrict__ ok, u32 *__restrict__ flags) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const u64 s = s0 + i, a = seg_off[s], b = seg_off[s + 1];
    if (a < t0 || b < a || b - t0 > nt || b - a > (u64)dmax) return;
    const u64 lo = a - t0;
    const u32 len = (u32)(b - a);
    u32 good = 1;
    ge_p3 acc = ge_identity();
    straus_dyn_lane(acc, good, tab, dig, tok, lo, len);
    raw160_store(out_raw, s, acc);
    ok[s] = (uint8_t)good;
    if (!good) flags[SEG_FLAG_NONE] = 1u;
}

// Wave w of the launch takes segment ids[w] (cnt ids: the pass's segments of more than dmax terms), whose terms are records
// [seg_off[s] - t0, seg_off[s + 1] - t0) of the pass, as for k_mid_seg_straus.  Lane l handles terms l, l + 64, ... of the segment
// (the window loop of straus_dyn_wave), then the 64 partial sums are folded and lane 0 stores the sum and the verdict.  Correct for any length >= 1.  The
// segment index, the offsets and every loop bound are wave-uniform (readfirstlane: SGPRs); only the term predicate and the zero-digit skip
// depend on the lane.  No LDS, no barrier.
__global__ void __launch_bounds__(256) k_mid_seg_wave(const u64 *__restrict__ seg_off, const u32 *__restrict__ ids, u32 cnt, u64 t0, u64 nt, const uint4 *__restrict__ tab,
                                                      const int8_t *__restrict__ dig, const uint8_t *__restrict__ tok, uint8_t *__restrict__ out_raw,
                                                      uint8_t *__restrict__ ok, u32 *__restrict__ flags) {
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (wv >= cnt) return;
    const u32 lane = threadIdx.x & 63u;
    const u32 s = ids[wv];
    const u64 a = seg_off[s], b = seg_off[(u64)s + 1];
    if (a < t0 || b < a || b - t0 > nt || b - a > 0xffffffc0ull) return;
    const u64 lo = a - t0;
    const u32 len = (u32)(b - a), rounds = (len + 63u) >> 6;
    // The loop of straus_dyn_wave, written out: called as that function the kernel is allocated 147 VGPRs where this form gets 128, one wave
    // per SIMD fewer (the same instructions; measured on the compiled code, profiles/straus_family_isa.txt).  A change there belongs here too.
    u32 good = 1;
    for (u32 r = 0; r < rounds; r++) {
        const u32 j = 64u * r + lane;
        if (j < len) good &= (u32)tok[lo + j];
    }
    ge_p3 acc = ge_identity();
#pragma unroll 1
    for (int w = SEG_DIG - 1; w >= 0; w--) {
        if (w != SEG_DIG - 1) acc = ge_mul_by_pow_2(acc, 4);
#pragma unroll 1
        for (u32 r = 0; r < rounds; r++) {
            const u32 j = 64u * r + lane;
            if (j < len) {
                const int dg = (int)dig[(lo + j) * SEG_DIG + (u64)w];
                if (dg != 0) acc = straus_add_dyn(acc, tab, lo + j, dg);
            }
        }
        ge_pin(acc);
    }
    straus_wave_store(out_raw, ok, flags, s, straus_wave_fold(acc), good, lane);
}

}  // namespace c25519

// ---- host side ----------------------------------------------------------------------------------------------------------------
static const off_msgs SEG_OFF_MSGS = OFF_MSGS("msm_vartime_segments", "seg_off", "n", nullptr);
static int32_t seg_check(c25519_ctx *ctx, uint64_t n, int in_fmt, const uint64_t *seg_off, uint64_t m, int out_fmt) {
    if (!fmt_pair_ok(in_fmt, out_fmt)) return bad_arg(ctx, "msm_vartime_segments: in_fmt and out_fmt must belong to one group");
    return check_offsets(ctx, SEG_OFF_MSGS, n, seg_off, m);
}

// ---- routing: the one place that decides which kernel a segment gets and where the passes are cut ----
//   len <= dmax   lane   (k_mid_seg_straus; empty segments too: they give the identity)
//   len <= wmax   wave   (k_mid_seg_wave)
//   len <= bmax   bucket (mid_segb.hip)
//   longer        the single-MSM path, one c25519_msm_partial_dev each
// A pass is a run of consecutive lane and wave segments of at most ptmax terms in all (ptmax >= wmax: one segment always fits); only the
// segments above wmax (of either kind: n_long counts both) and the term count cut it.  The wave kernel of a pass runs over wave_ids[w0 .. w1).
// The bucket segments have passes of their own: runs of the list `buckets` of at most bptmax terms in all (bptmax >= bmax).
static int seg_route_of(uint64_t len) {
    return len <= seg_direct_max() ? C25519_MSM_SEGMENT_ROUTE_LANE : len <= seg_wave_max() ? C25519_MSM_SEGMENT_ROUTE_WAVE
         : len <= seg_bucket_max() ? C25519_MSM_SEGMENT_ROUTE_BUCKET : C25519_MSM_SEGMENT_ROUTE_SINGLE;
}
struct seg_pass { uint64_t s0, s1, w0, w1, lanes; };       // segments [s0, s1), terms [seg_off[s0], seg_off[s1]); `lanes` of them on the lane route
struct seg_bpass { uint64_t k0, k1, nt; };                  // buckets[k0 .. k1), nt terms in all
struct seg_route {
    uint64_t n_lane = 0, n_wave = 0, n_long = 0, n_pass = 0, maxt = 0;      // what c25519_msm_vartime_segments_plan reports
    std::vector<seg_pass> passes;                           // the lists: only when asked for (seg_run)
    std::vector<uint32_t> wave_ids;
    std::vector<uint64_t> longs, buckets;
    std::vector<seg_bpass> bpasses;
    uint64_t bmaxt = 0, bmaxseg = 0;                        // most terms / segments of one bucket pass
};
static void seg_plan(const uint64_t *seg_off, uint64_t m, bool lists, seg_route &R) {
    const uint64_t dmax = seg_direct_max(), wmax = seg_wave_max(), ptmax = seg_pass_terms();
    uint64_t s0 = 0, terms = 0, w0 = 0, lanes = 0;
    auto close = [&](uint64_t s1) {
        if (s1 > s0) {
            R.n_pass++; R.maxt = std::max(R.maxt, terms);
            if (lists) R.passes.push_back({s0, s1, w0, R.n_wave, lanes});
        }
        terms = 0; lanes = 0; w0 = R.n_wave;
    };
    for (uint64_t s = 0; s < m; s++) {
        const uint64_t len = seg_off[s + 1] - seg_off[s];
        if (len > wmax) {
            close(s); s0 = s + 1; R.n_long++;
            if (lists) (seg_route_of(len) == C25519_MSM_SEGMENT_ROUTE_BUCKET ? R.buckets : R.longs).push_back(s);
            continue;
        }
        if (terms + len > ptmax) { close(s); s0 = s; }
        terms += len;
        if (len > dmax) { R.n_wave++; if (lists) R.wave_ids.push_back((uint32_t)s); }     // s < m < 2^32 - 1: check_offsets has bounded m
        else { R.n_lane++; lanes++; }
    }
    close(m);
    const uint64_t bptmax = seg_bucket_pass_terms();
    for (uint64_t k = 0; k < R.buckets.size();) {
        seg_bpass p = {k, k, 0};
        for (; p.k1 < R.buckets.size(); p.k1++) {
            const uint64_t len = seg_off[R.buckets[p.k1] + 1] - seg_off[R.buckets[p.k1]];
            if (p.k1 > p.k0 && p.nt + len > bptmax) break;
            p.nt += len;
        }
        R.bmaxt = std::max(R.bmaxt, p.nt); R.bmaxseg = std::max(R.bmaxseg, p.k1 - p.k0);
        R.bpasses.push_back(p);
        k = p.k1;
    }
}

EXPORT int32_t c25519_msm_vartime_segments_routes(const uint64_t *seg_off, uint64_t m, uint8_t *route) {
    int32_t r;
    if ((r = check_offsets(nullptr, SEG_OFF_MSGS, offsets_end(seg_off, m), seg_off, m))) return r;
    for (uint64_t s = 0; s < m; s++) route[s] = (uint8_t)seg_route_of(seg_off[s + 1] - seg_off[s]);
    return C25519_OK;
}

EXPORT int32_t c25519_msm_vartime_segments_plan(const uint64_t *seg_off, uint64_t m, uint64_t plan[5]) {
    int32_t r;
    if ((r = check_offsets(nullptr, SEG_OFF_MSGS, offsets_end(seg_off, m), seg_off, m))) return r;
    seg_route R;
    seg_plan(seg_off, m, false, R);
    plan[0] = R.n_lane; plan[1] = R.n_wave; plan[2] = R.n_long; plan[3] = R.n_pass; plan[4] = R.maxt;
    return C25519_OK;
}

// The whole call on device inputs.  h_out / h_ok (host form; may be null): where d_out / d_ok are copied before the one synchronisation.
// seg_off has been checked (seg_check) and m > 0.
static int32_t seg_run(c25519_ctx *ctx, const uint8_t *d_scalars, const uint8_t *d_points, uint64_t n, int in_fmt, const uint64_t *seg_off, uint64_t m, int out_fmt,
                       uint8_t *d_out, uint8_t *d_ok, uint8_t *h_out, uint8_t *h_ok) {
    hipStream_t st = ctx->stream;
    const size_t pb = point_bytes(in_fmt);
    const uint64_t dmax = seg_direct_max();
    seg_route R;
    seg_plan(seg_off, m, true, R);
    const std::vector<seg_pass> &passes = R.passes;
    const std::vector<uint64_t> &longs = R.longs;
    const uint64_t maxt = R.maxt;
    // long segments first, each through the single-MSM path (it synchronises and uses workspaces of its own: nothing of this call is queued yet)
    std::vector<uint8_t> long_sum(longs.size() * 160), long_ok(longs.size(), 1);
    bool long_none = false;
    for (size_t k = 0; k < longs.size(); k++) {
        const uint64_t a = seg_off[longs[k]], len = seg_off[longs[k] + 1] - a;
        const int32_t r = c25519_msm_partial_dev(ctx, d_scalars + a * 32, d_points + a * pb, len, in_fmt, long_sum.data() + 160 * k);
        if (r == C25519_NONE) {                            // Option::None of this sum alone; its output is unspecified: the identity
            long_ok[k] = 0; long_none = true;
            memset(long_sum.data() + 160 * k, 0, 160);
            long_sum[160 * k + 40] = 1; long_sum[160 * k + 80] = 1;
        } else if (r) return r;
    }
    // tmp_f (straus_ws): seg_off | segment ids of the wave route, pass after pass | raw sums | ok | tables | digits | term ok bytes
    // The bucket passes (segb_ws) use the place of the last three -- the passes of the two kinds run one after the other on the stream -- and
    // their descriptors lie behind it.
    straus_ws ws(m, R.wave_ids.size(), maxt, out_fmt, d_ok != nullptr);
    std::vector<uint64_t> bdesc;                            // the descriptors of all bucket passes, pass after pass (mid_segb.h)
    for (const seg_bpass &p : R.bpasses) {
        uint64_t at = 0;
        for (uint64_t k = p.k0; k < p.k1; k++) { bdesc.push_back(at); at += seg_off[R.buckets[k] + 1] - seg_off[R.buckets[k]]; }
        bdesc.push_back(at);
        for (uint64_t k = p.k0; k < p.k1; k++) bdesc.push_back(seg_off[R.buckets[k]]);
        for (uint64_t k = p.k0; k < p.k1; k++) bdesc.push_back(R.buckets[k]);
    }
    segb_ws bw(R.bmaxt, R.bmaxseg, bdesc.size());
    ws_layout F;
    const size_t o_head = F.part(ws.head_bytes()), o_pass = F.part(std::max(ws.pass_bytes(), bw.pass_bytes())), o_desc = F.part(bw.b_desc);
    int32_t r;
    if ((r = F.reserve(ctx, ctx->tmp_f, 256))) return r;
    ws.bind(F.at(o_head), d_out, d_ok);
    bw.bind(F.at(o_pass), F.at(o_desc));
    uint32_t *flags = (uint32_t *)ctx->d_flag;
    auto enqueue = [&]() -> int32_t {
        HIPCHK(hipMemsetAsync(flags, 0, 8, st));
        HIPCHK(hipEventRecord(ctx->ev0, st));
        HIPCHK(hipMemcpyAsync(ws.d_off, seg_off, (m + 1) * 8, hipMemcpyHostToDevice, st));
        if (!R.wave_ids.empty()) HIPCHK(hipMemcpyAsync(ws.d_ids, R.wave_ids.data(), R.wave_ids.size() * 4, hipMemcpyHostToDevice, st));
        if (!bdesc.empty()) HIPCHK(hipMemcpyAsync(bw.desc, bdesc.data(), bdesc.size() * 8, hipMemcpyHostToDevice, st));
        ctx->kname[0] = !R.wave_ids.empty() ? "c25519::k_mid_seg_wave (one wave per segment, lane l takes terms l, l + 64, ...; the partial sums folded by shuffles)"
                      : !R.buckets.empty()  ? SEGB_KERNEL_NAME
                                            : "c25519::k_mid_seg_straus (one lane per segment, the doubling chain shared by its terms)";
        for (const seg_pass &p : passes) {
            const uint64_t t0 = seg_off[p.s0], nt = seg_off[p.s1] - t0, ns = p.s1 - p.s0;
            int32_t q;
            if (nt && (q = straus_launch_tables(ctx, in_fmt, d_scalars, d_points, t0, nt, ws))) return q;
            if (p.lanes) {                                   // (the wave segments among its lanes are longer than dmax: left alone)
                hipLaunchKernelGGL(k_mid_seg_straus, dim3(div_up(ns, 256)), dim3(256), 0, st, (const u64 *)ws.d_off, p.s0, ns, t0, nt, (u32)dmax, (const uint4 *)ws.tab,
                                   (const int8_t *)ws.dig, (const uint8_t *)ws.tok, ws.sums, ws.okbuf, flags);
                HIPCHK(hipGetLastError());
            }
            if (p.w1 > p.w0) {                               // four waves, so four segments, per block; disjoint outputs: back to back on the stream
                const uint64_t nw = p.w1 - p.w0;
                hipLaunchKernelGGL(k_mid_seg_wave, dim3(div_up(nw, 4)), dim3(256), 0, st, (const u64 *)ws.d_off, (const u32 *)(ws.d_ids + p.w0), (u32)nw, t0, nt,
                                   (const uint4 *)ws.tab, (const int8_t *)ws.dig, (const uint8_t *)ws.tok, ws.sums, ws.okbuf, flags);
                HIPCHK(hipGetLastError());
            }
        }
        {                                                   // the bucket passes, behind the Straus passes: three launches each, disjoint outputs
            size_t at = 0;
            for (const seg_bpass &p : R.bpasses) {
                const uint64_t nb = p.k1 - p.k0;
                int32_t q;
                if ((q = segb_enqueue_pass(ctx, in_fmt, d_scalars, d_points, bw, bw.desc + at, (uint32_t)nb, p.nt, ws.sums, ws.okbuf))) return q;
                at += segb_desc_words(nb);
            }
        }
        for (size_t k = 0; k < longs.size(); k++) {
            HIPCHK(hipMemcpyAsync(ws.sums + longs[k] * 160, long_sum.data() + 160 * k, 160, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(ws.okbuf + longs[k], long_ok.data() + k, 1, hipMemcpyHostToDevice, st));
        }
        return straus_finish_enqueue(ctx, ws.sums, m, out_fmt, d_out, ws.okbuf, h_out, h_ok);
    };
    return straus_finish_wait(ctx, enqueue(), long_none);
}

EXPORT int32_t c25519_msm_vartime_segments_dev(c25519_ctx *ctx, const uint8_t *d_scalars, const uint8_t *d_points, uint64_t n, int in_fmt, const uint64_t *seg_off,
                                               uint64_t m, int out_fmt, uint8_t *d_out, uint8_t *d_ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = seg_check(ctx, n, in_fmt, seg_off, m, out_fmt))) return r;
    if (m == 0) return C25519_OK;
    return seg_run(ctx, d_scalars, d_points, n, in_fmt, seg_off, m, out_fmt, d_out, d_ok, nullptr, nullptr);
}

EXPORT int32_t c25519_msm_vartime_segments(c25519_ctx *ctx, const uint8_t *scalars, const uint8_t *points, uint64_t n, int in_fmt, const uint64_t *seg_off, uint64_t m,
                                           int out_fmt, uint8_t *out, uint8_t *ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = seg_check(ctx, n, in_fmt, seg_off, m, out_fmt))) return r;
    if (m == 0) return C25519_OK;
    const size_t pb = point_bytes(in_fmt), ob = point_bytes(out_fmt);
    ws_layout O; O.part(m * ob);                            // tmp_c: the sums | their ok bytes (the tail: not rounded, and 16 bytes behind it)
    if ((r = ctx_reserve(ctx, ctx->tmp_a, n * 32 + 16)) || (r = ctx_reserve(ctx, ctx->tmp_b, n * pb + 16)) || (r = O.reserve(ctx, ctx->tmp_c, m + 16))) return r;
    ffi_small_begin(ctx);
    uint8_t *d_s = (uint8_t *)ctx->tmp_a.p, *d_p = (uint8_t *)ctx->tmp_b.p, *d_out = O.at(0), *d_ok = O.at(O.bytes());
    if ((r = straus_upload_all(ctx, {{d_s, scalars, n * 32}, {d_p, points, n * pb}}))) return r;
    r = seg_run(ctx, d_s, d_p, n, in_fmt, seg_off, m, out_fmt, d_out, d_ok, out, ok);
    if (r < 0) (void)hipStreamSynchronize(ctx->stream);    // (an early error: the uploads may still be reading the caller's memory)
    ffi_small_end(ctx, n * (32 + pb) + (m + 1) * 8, m * ob + (ok ? m : 0));
    return r;
}
