// The Straus family: what mid_seg.hip (c25519_msm_vartime_segments), mid_rows.hip (c25519_precomp_msm_vartime_rows) and mid_mixed.hip
// (c25519_precomp_msm_vartime_mixed_rows) share.  Device side: the layout of a term's table {1 .. 8} P and of its 64 digit bytes, the kernel
// that writes them (k_mid_straus_tables<IN>), the two verdict words, and the loops of the row / segment kernels, once each --
//   straus_dyn_lane / straus_dyn_wave     the dynamic half: Straus with a shared doubling chain over per-term tables
//   straus_comb_lane / straus_comb_wave   the static half: the comb table of a c25519_precomp handle (rows_digits.h, precomp.h)
//   straus_wave_fold / straus_wave_store  the six-round fold of a wave's partial sums and what lane 0 stores
// Host side: the three constants of the header as the host reads them, and the scaffold of the three calls (refusals, the rows call's
// routing rule, the workspace in ctx->tmp_f, the tables launch, the epilogue, the uploads of the host-pointer forms).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <initializer_list>
#include "../../include/c25519_hip.h"
#include "devio.h"
#include "kernels.h"
#include "ctx.h"
#include "knobs.h"
#include "precomp.h"
#include "rows_digits.h"
#include "capi_util.h"

namespace c25519 {

constexpr int SEG_ENT = 8, SEG_ENT_Q = 10;                  // table entries per term; 16-byte pieces per entry (160 bytes)
constexpr int SEG_DIG = 64;                                 // digit bytes per term (1280 + 64 = 1344 bytes per term, and its ok byte)
enum { SEG_FLAG_NONE = 0, SEG_FLAG_BIT255 = 1 };            // the two verdict words at d_flag, of all three calls

// entry e (0 .. 7 = 1 P .. 8 P) of term i: ten consecutive 16-byte pieces
__device__ __forceinline__ void seg_tab_store(uint4 *tab, u64 i, int e, const ge_cached &c) {
    u32 t[40];
    for (int k = 0; k < 10; k++) { t[k] = c.YpX.v[k]; t[10 + k] = c.YmX.v[k]; t[20 + k] = c.Z.v[k]; t[30 + k] = c.T2d.v[k]; }
    uint4 *q = tab + (i * SEG_ENT + (u64)e) * SEG_ENT_Q;
    for (int k = 0; k < SEG_ENT_Q; k++) q[k] = make_uint4(t[4 * k], t[4 * k + 1], t[4 * k + 2], t[4 * k + 3]);
}
__device__ __forceinline__ ge_cached seg_tab_load(const uint4 *tab, u64 i, u32 e) {
    const uint4 *q = tab + (i * SEG_ENT + (u64)e) * SEG_ENT_Q;
    u32 t[40];
    for (int k = 0; k < SEG_ENT_Q; k++) { const uint4 v = q[k]; t[4 * k] = v.x; t[4 * k + 1] = v.y; t[4 * k + 2] = v.z; t[4 * k + 3] = v.w; }
    ge_cached c;
    for (int k = 0; k < 10; k++) { c.YpX.v[k] = t[k]; c.YmX.v[k] = t[10 + k]; c.Z.v[k] = t[20 + k]; c.T2d.v[k] = t[30 + k]; }
    return c;
}

// Term g of the call -> record i of the pass: tok[i], tab[i], dig[i].  IN: 0 CompressedEdwardsY (ZIP-215 decoder), 1 CompressedRistretto,
// 2 raw 160-byte (trusted).  The caller has checked i against the records of the pass.
template <int IN>
__device__ __forceinline__ void seg_tables_term(const uint8_t *__restrict__ scalars, const uint8_t *__restrict__ points, u64 g, u64 i, uint4 *__restrict__ tab,
                                                uint4 *__restrict__ dig, uint8_t *__restrict__ tok, u32 *__restrict__ flags) {
    ge_p3 P;
    bool good = true;
    if (IN == 2) P = raw160_load(points, g);
    else { u32 w[8]; load8(points, g, w); good = IN == 0 ? ge_decompress(P, w) : ris_decompress(P, w); }
    tok[i] = good ? 1 : 0;
    // {1 .. 8} P by repeated addition of P (window.rs:97-104)
    const ge_cached c1 = ge_p3_to_cached(P);
    seg_tab_store(tab, i, 0, c1);
    ge_p3 acc = P;
#pragma unroll 1
    for (int j = 1; j < SEG_ENT; j++) {
        acc = ge_p1p1_to_p3(ge_add_cached(acc, c1));
        seg_tab_store(tab, i, j, ge_p3_to_cached(acc));
    }
    // digits: nibble_k(s') - 8 with s' = s + 0x0888...8, the top nibble left unsigned (0 .. 8), scalar.rs:1019-1051.  A scalar with bit 255
    // set fails the call; its digits are taken from the low 255 bits so that every digit stays within the table.
    u32 s[8];
    load8(scalars, g, s);
    if (s[7] >> 31) flags[SEG_FLAG_BIT255] = 1u;
    s[7] &= 0x7fffffffu;
    {
        u64 carry = 0;
        for (int k = 0; k < 8; k++) { const u64 v = (u64)s[k] + (k == 7 ? 0x08888888u : 0x88888888u) + carry; s[k] = (u32)v; carry = v >> 32; }
    }
    u32 d[16];                                              // 64 signed bytes, digit k in byte k
    for (int k = 0; k < 16; k++) {
        const u32 h = s[k >> 1] >> ((k & 1) * 16);
        u32 word = 0;
        for (int b = 0; b < 4; b++) {
            const int nib = (int)((h >> (4 * b)) & 15u);
            const int dg = (4 * k + b == 63) ? nib : nib - 8;
            word |= ((u32)dg & 0xffu) << (8 * b);
        }
        d[k] = word;
    }
    uint4 *dq = dig + 4 * i;
    for (int k = 0; k < 4; k++) dq[k] = make_uint4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
}

// Terms [t0, t0 + cnt) of the call -> records 0 .. cnt - 1 of the pass, one lane per term.  The library holds every kernel once
// (tests/test_ct_isa_secret_paths.py): mid_seg.hip instantiates the three explicitly, every other file that includes this header launches
// those (straus_launch_tables below).
template <int IN>
__global__ void __launch_bounds__(256) k_mid_straus_tables(const uint8_t *__restrict__ scalars, const uint8_t *__restrict__ points, u64 t0, u64 cnt,
                                                           uint4 *__restrict__ tab, uint4 *__restrict__ dig, uint8_t *__restrict__ tok, u32 *__restrict__ flags) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    seg_tables_term<IN>(scalars, points, t0 + i, i, tab, dig, tok, flags);
}
extern template __global__ void k_mid_straus_tables<0>(const uint8_t *, const uint8_t *, u64, u64, uint4 *, uint4 *, uint8_t *, u32 *);
extern template __global__ void k_mid_straus_tables<1>(const uint8_t *, const uint8_t *, u64, u64, uint4 *, uint4 *, uint8_t *, u32 *);
extern template __global__ void k_mid_straus_tables<2>(const uint8_t *, const uint8_t *, u64, u64, uint4 *, uint4 *, uint8_t *, u32 *);

// acc + / - entry |dg| of record i of the pass, for a digit dg != 0 (-8 .. 8)
__device__ __forceinline__ ge_p3 straus_add_dyn(const ge_p3 &acc, const uint4 *__restrict__ tab, u64 i, int dg) {
    const bool neg = dg < 0;
    const u32 mag = (u32)(neg ? -dg : dg);                  // 1 .. 8
    return ge_p1p1_to_p3(ge_add_cached(acc, ge_cached_cneg(seg_tab_load(tab, i, (mag - 1u) & 7u), neg)));
}
// acc + / - comb record (j, k, |dg|) of the handle, for a digit dg != 0
__device__ __forceinline__ ge_p3 straus_add_comb(const ge_p3 &acc, const u32 *__restrict__ comb, u32 j, u32 k, int dg) {
    const bool neg = dg < 0;
    const u32 mag = (u32)(neg ? -dg : dg);                  // 1 .. 8
    return ge_madd_signed_p3(acc, pts_load(comb, ((u64)j * ROWS_WIN + k) * ROWS_ENT + ((mag - 1u) & 7u)), neg);
}

// ---- the dynamic half: records [lo, lo + len) of the pass into acc; good &= their ok bytes ----
// acc = 16 acc per window, then + / - entry |d| of every term whose digit d is not zero (scalar_mul/straus.rs:159-200).  Complete formulas
// (edwards.rs:797): no special case for equal, opposite or identity operands.  len = 0 runs the doubling chain all the same (the identity
// stays the identity): a caller that meets it often asks `if (len)` first, as the mixed rows do.
// Lane form: this lane runs over all the records.
__device__ __forceinline__ void straus_dyn_lane(ge_p3 &acc, u32 &good, const uint4 *__restrict__ tab, const int8_t *__restrict__ dig, const uint8_t *__restrict__ tok,
                                                u64 lo, u32 len) {
    for (u32 j = 0; j < len; j++) good &= (u32)tok[lo + j];
#pragma unroll 1
    for (int k = SEG_DIG - 1; k >= 0; k--) {
        if (k != SEG_DIG - 1) acc = ge_mul_by_pow_2(acc, 4);
#pragma unroll 1
        for (u32 j = 0; j < len; j++) {
            const int dg = (int)dig[(lo + j) * SEG_DIG + (u64)k];
            if (dg != 0) acc = straus_add_dyn(acc, tab, lo + j, dg);
        }
        ge_pin(acc);
    }
}
// Wave form (k_mid_seg_wave carries a copy of this loop, for its register count: a change here belongs there too): lane l takes records
// l, l + 64, ... and leaves a partial sum (a lane without a record: what it came with).  lo and len are
// wave-uniform, and so is every loop bound; only the record predicate and the zero-digit skip depend on the lane.
__device__ __forceinline__ void straus_dyn_wave(ge_p3 &acc, u32 &good, const uint4 *__restrict__ tab, const int8_t *__restrict__ dig, const uint8_t *__restrict__ tok,
                                                u64 lo, u32 len, u32 lane) {
    const u32 rounds = (len + 63u) >> 6;
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
                if (dg != 0) acc = straus_add_dyn(acc, tab, lo + j, dg);
            }
        }
        ge_pin(acc);
    }
}

// ---- the static half: scalars [s0, s0 + w) of the call over static points 0 .. w - 1 of the comb table into acc ----
// No doubling: the records are already scaled by 16^k, so this comes AFTER the doubling chain of a dynamic half.  Every scalar is recoded in
// registers (rows_digits.h; no digit array is written); a scalar with bit 255 set raises the verdict word.  comb holds at least w * 512 records.
// Lane form (k_mid_mixed_lane carries a copy of this loop, for the form it compiles to there: a change here belongs there too): all 64
// windows of every scalar; the lanes of a wave are on the same (j, k) at the same time, so their gathers fall into one 1 KB
// group of records.
__device__ __forceinline__ void straus_comb_lane(ge_p3 &acc, const uint8_t *__restrict__ scalars, u64 s0, u32 w, const u32 *__restrict__ comb, u32 *__restrict__ flags) {
#pragma unroll 1
    for (u32 j = 0; j < w; j++) {
        u32 s[8];
        load8(scalars, s0 + j, s);
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
}
// Wave form: lane l is window l of every scalar (a uniform load, s0 is wave-uniform); only the digit depends on the lane.
__device__ __forceinline__ void straus_comb_wave(ge_p3 &acc, const uint8_t *__restrict__ scalars, u64 s0, u32 w, const u32 *__restrict__ comb, u32 lane,
                                                 u32 *__restrict__ flags) {
    const u32 word = lane >> 3, shift = 4u * (lane & 7u);
#pragma unroll 1
    for (u32 j = 0; j < w; j++) {
        u32 s[8];
        load8(scalars, s0 + j, s);
        if (rows_recode(s)) flags[SEG_FLAG_BIT255] = 1u;
        u32 mine = s[0];
        for (u32 q = 1; q < 8; q++) mine = word == q ? s[q] : mine;
        const int dg = rows_digit((mine >> shift) & 15u, (int)lane);
        if (dg != 0) acc = straus_add_comb(acc, comb, j, lane, dg);
        ge_pin(acc);
    }
}

// ---- the end of a wave kernel ----
// the 64 partial sums -> lane 0 (ge_shfl_down, complete additions: a lane without a term holds the identity).  No LDS, no barrier.
__device__ __forceinline__ ge_p3 straus_wave_fold(ge_p3 acc) {
#pragma unroll 1
    for (int off = 32; off > 0; off >>= 1) acc = ge_add(acc, ge_shfl_down(acc, off));
    return acc;
}
// lane 0 stores sum r, its ok byte (every lane's `good`) and, for a sum with an undecodable point, the NONE word
__device__ __forceinline__ void straus_wave_store(uint8_t *__restrict__ out_raw, uint8_t *__restrict__ ok, u32 *__restrict__ flags, u64 r, const ge_p3 &acc, u32 good,
                                                  u32 lane) {
    const bool all_good = __all((int)good) != 0;
    if (lane == 0) {
        raw160_store(out_raw, r, acc);
        ok[r] = all_good ? 1 : 0;
        if (!all_good) flags[SEG_FLAG_NONE] = 1u;
    }
}

}  // namespace c25519

// ---- host side: the three constants of the header; the tuning build reads other values for an A/B run (knobs.h) ----
static inline uint64_t seg_direct_max() { static const uint64_t v = (uint64_t)std::max<long long>(1, C25519_KNOB_LL("SEG_DIRECT_MAX", C25519_MSM_SEGMENT_DIRECT_MAX)); return v; }
static inline uint64_t seg_wave_max() {
    static const uint64_t v = std::max<uint64_t>((uint64_t)std::max<long long>(1, C25519_KNOB_LL("SEG_WAVE_MAX", C25519_MSM_SEGMENT_WAVE_MAX)), seg_direct_max());
    return v;
}
static inline uint64_t seg_pass_terms() {                   // at least the wave maximum: one segment always fits into a pass
    static const uint64_t v = std::max<uint64_t>((uint64_t)std::max<long long>(1, C25519_KNOB_LL("SEG_PASS_TERMS", C25519_MSM_SEGMENT_PASS_TERMS)), seg_wave_max());
    return v;
}

// ---- host side: the scaffold of the three calls ----
// What the rows call and the mixed rows call refuse about the handle, the route and the output format.  `scalars` is what the caller names
// the static scalars of a row.
struct rows_msgs { const char *handle, *out_fmt, *route, *points, *width; };
#define ROWS_MSGS(call, scalars)                                                                                                  \
    { call ": no handle", call ": bad out_fmt", call ": unknown route",                                                           \
      call ": the handle has more than 4096 static points; run it through c25519_precomp_msm_vartime, row by row",                \
      call ": more " scalars " per row than static points (precomputed_straus.rs:86)" }
static inline int32_t rows_check_handle(c25519_ctx *ctx, const rows_msgs &msg, const c25519_precomp *p, uint64_t w, int32_t route, int out_fmt) {
    if (!p) return bad_arg(ctx, msg.handle);
    if (out_fmt < 0 || out_fmt > 2) return bad_arg(ctx, msg.out_fmt);
    if (route != C25519_PRECOMP_ROWS_AUTO && route != C25519_PRECOMP_ROWS_LANE && route != C25519_PRECOMP_ROWS_WAVE) return bad_arg(ctx, msg.route);
    if (p->n > C25519_PRECOMP_ROWS_MAX_POINTS) return bad_arg(ctx, msg.points);
    if (w > p->n) return bad_arg(ctx, msg.width);
    return C25519_OK;
}
// what AUTO takes for m rows of w static scalars and no dynamic term: the lane kernel iff ...
static inline bool rows_lane_route(uint64_t m, uint64_t w) { return w < C25519_PRECOMP_ROWS_LANE_WIDTH && m >= C25519_PRECOMP_ROWS_LANE_MIN_ROWS; }

// The workspace of a call with per-term tables, in ctx->tmp_f:
//   offsets (m + 1) | segment ids of the wave route (n_ids; may be none) | raw sums (compressed output only) | ok (when the caller gave none) |
//   tables | digits | term ok bytes (maxt terms: the most of one pass)
// every part a multiple of 256 bytes, and 256 bytes after the last.  Reserve bytes(), then bind() to the buffer as it stands when
// everything that reserves tmp_f for this call has done so.  The last three are the parts of a pass: head_bytes() lie before them.
struct straus_ws {
    ws_layout L;
    size_t o_off, o_ids, o_sum, o_ok, o_tab, o_dig, o_tok;
    uint64_t *d_off = nullptr;
    uint32_t *d_ids = nullptr;
    uint8_t *sums = nullptr, *okbuf = nullptr;
    uint4 *tab = nullptr;
    uint8_t *dig = nullptr, *tok = nullptr;
    straus_ws(uint64_t m, size_t n_ids, uint64_t maxt, int out_fmt, bool caller_ok)
        : o_off(L.part((m + 1) * 8)), o_ids(L.part(n_ids * 4)), o_sum(L.part(out_fmt == C25519_FMT_RAW160 ? 0 : m * 160)), o_ok(L.part(caller_ok ? 0 : m)),
          o_tab(L.part(maxt * c25519::SEG_ENT * c25519::SEG_ENT_Q * 16)), o_dig(L.part(maxt * c25519::SEG_DIG)), o_tok(L.part(maxt)) {}
    size_t head_bytes() const { return o_tab; }
    size_t pass_bytes() const { return L.bytes() - o_tab; }
    size_t bytes() const { return L.bytes(256); }
    void bind(void *base, uint8_t *d_out, uint8_t *d_ok) {
        L.bind(base);
        d_off = L.at<uint64_t>(o_off); d_ids = L.at<uint32_t>(o_ids); tab = L.at<uint4>(o_tab); dig = L.at(o_dig); tok = L.at(o_tok);
        sums = o_ok != o_sum ? L.at(o_sum) : d_out;          // (no raw sums of its own: the RAW160 output is where they go)
        okbuf = d_ok ? d_ok : L.at(o_ok);
    }
};

// k_mid_straus_tables over terms [t0, t0 + nt) of the call, nt > 0, into the workspace
static inline int32_t straus_launch_tables(c25519_ctx *ctx, int in_fmt, const uint8_t *d_scalars, const uint8_t *d_points, uint64_t t0, uint64_t nt, const straus_ws &ws) {
    using namespace c25519;
    const dim3 g(div_up(nt, 256)), b(256);
    uint32_t *flags = (uint32_t *)ctx->d_flag;
    if (in_fmt == C25519_FMT_EDWARDS_Y) hipLaunchKernelGGL(k_mid_straus_tables<0>, g, b, 0, ctx->stream, d_scalars, d_points, t0, nt, ws.tab, (uint4 *)ws.dig, ws.tok, flags);
    else if (in_fmt == C25519_FMT_RISTRETTO) hipLaunchKernelGGL(k_mid_straus_tables<1>, g, b, 0, ctx->stream, d_scalars, d_points, t0, nt, ws.tab, (uint4 *)ws.dig, ws.tok, flags);
    else hipLaunchKernelGGL(k_mid_straus_tables<2>, g, b, 0, ctx->stream, d_scalars, d_points, t0, nt, ws.tab, (uint4 *)ws.dig, ws.tok, flags);
    HIPCHK(hipGetLastError());
    return C25519_OK;
}

// The end of a call, enqueued behind its kernels: the m raw sums are compressed into d_out (unless the output is RAW160: they are there), ev1,
// the two verdict words to pinned memory, and the copies to the host form's arrays (h_out / h_ok may be null; okbuf only with h_ok).
static inline int32_t straus_finish_enqueue(c25519_ctx *ctx, const uint8_t *sums, uint64_t m, int out_fmt, uint8_t *d_out, const uint8_t *okbuf, uint8_t *h_out, uint8_t *h_ok) {
    hipStream_t st = ctx->stream;
    int32_t r;
    if (out_fmt != C25519_FMT_RAW160 && (r = c25519_compress_batch_dev(ctx, sums, m, out_fmt, d_out))) return r;
    HIPCHK(hipEventRecord(ctx->ev1, st));
    HIPCHK(hipMemcpyAsync(ctx->h_msm, ctx->d_flag, 8, hipMemcpyDeviceToHost, st));
    if (h_out) HIPCHK(hipMemcpyAsync(h_out, d_out, m * point_bytes(out_fmt), hipMemcpyDeviceToHost, st));
    if (h_ok) HIPCHK(hipMemcpyAsync(h_ok, okbuf, m, hipMemcpyDeviceToHost, st));
    return C25519_OK;
}
// ... and the one synchronisation and the verdict.  enq: what enqueueing the call returned; none_elsewhere: a sum that ran outside the
// stream's kernels (the long segments of the segments call) was Option::None.
static inline int32_t straus_finish_wait(c25519_ctx *ctx, int32_t enq, bool none_elsewhere) {
    if (enq) { (void)hipStreamSynchronize(ctx->stream); return enq; }       // no queued copy still reads host memory after the return
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const uint32_t *verdict = (const uint32_t *)ctx->h_msm;                 // pinned
    if (verdict[c25519::SEG_FLAG_BIT255]) return bad_arg(ctx, "msm: a scalar has bit 255 set (Scalar invariant #1 violated)");
    return (verdict[c25519::SEG_FLAG_NONE] || none_elsewhere) ? C25519_NONE : C25519_OK;
}

// The uploads of a host-pointer form, in order; empty ones are skipped.  After a failure nothing queued still reads the caller's memory.
struct straus_upload { void *dst; const void *src; size_t bytes; };
static inline int32_t straus_upload_all(c25519_ctx *ctx, std::initializer_list<straus_upload> ups) {
    for (const straus_upload &u : ups) {
        if (!u.bytes) continue;
        const hipError_t e = hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return c25519_fail(ctx, e, "hipMemcpyAsync(inputs)"); }
    }
    return C25519_OK;
}
