// Batched group law (curve25519-dalek/src/edwards.rs, ristretto.rs), on points already produced on the device:
//
//   c25519_point_add_batch        impl Add / Sub for EdwardsPoint (edwards.rs:808-835) and RistrettoPoint (ristretto.rs:852-880)
//   c25519_point_map_batch        impl Neg (edwards.rs:853-875, ristretto.rs:897-907), EdwardsPoint::mul_by_cofactor (edwards.rs:1365)
//   c25519_point_eq_batch         ConstantTimeEq (edwards.rs:501-512, ristretto.rs:815-830), is_identity (traits.rs:45, ristretto.rs:1197)
//   c25519_point_sum_segments     impl Sum (edwards.rs:837-851, ristretto.rs:882-895) over many independent segments of one flat array
//
// The elementwise calls run one item per lane and end, for compressed output, in the existing batched compressors.  The segmented sum
// is DESIGN.md §3.11: chunks of SUM_C points per wave, a per-lane serial fold of SUM_K points, a segmented shuffle scan across the wave,
// and the pieces of segments that cross a chunk edge folded again by the same kernel until one chunk is left.  No branch and no address
// depends on point data (tests/test_ct_isa_group.py asserts it on the compiled code); the sum branches on segment keys, which come from
// the public offsets only.
#include <hip/hip_runtime.h>
#include <string.h>
#include "../../include/c25519_hip.h"
#include "devio.h"
#include "kernels.h"
#include "ctx.h"
#include "ffi.h"
#include "capi_util.h"

using namespace c25519;

namespace c25519 {

enum { GR_ADD = 0, GR_SUB = 1, GR_NEG = 2, GR_COF = 3 };    // elementwise operations
enum { GR_RAW = 0, GR_P32 = 1 };                            // a raw 160-byte point, or a P32 record for launch_compress_p32
constexpr int SUM_K = 8, SUM_C = 64 * SUM_K;                // points per lane / per wave (chunk) of the segmented sum
constexpr u32 KEY_NONE = 0xffffffffu;                       // a piece that belongs to no segment (an absent head or tail piece)

// input point idx: IN 0 CompressedEdwardsY (ZIP-215 decoder), 1 CompressedRistretto, 2 raw 160-byte (trusted), 3 a P40 record
template <int IN>
__device__ __forceinline__ ge_p3 grp_load(const uint8_t *in, u64 idx, bool &ok) {
    if (IN == 2) { ok = true; return raw160_load(in, idx); }
    if (IN == 3) { ok = true; return p40_load(reinterpret_cast<const u32 *>(in), idx); }
    u32 w[8];
    load8(in, idx, w);
    ge_p3 P;
    ok = IN == 0 ? ge_decompress(P, w) : ris_decompress(P, w);
    return P;
}
template <int OUT>
__device__ __forceinline__ void grp_emit(const ge_p3 &P, u64 idx, uint8_t *out_raw, u32 *scratch) {
    if (OUT == GR_RAW) raw160_store(out_raw, idx, P);
    else p32_store(scratch, idx, P.X, P.Y, P.Z);
}
__device__ __forceinline__ ge_p3 ge_select(const ge_p3 &a, const ge_p3 &b, bool choose_b) {
    const lanemask m = lane_mask(choose_b);
    ge_p3 r;
    r.X = fe_select_m(a.X, b.X, m); r.Y = fe_select_m(a.Y, b.Y, m); r.Z = fe_select_m(a.Z, b.Z, m); r.T = fe_select_m(a.T, b.T, m);
    return r;
}

// out[i] = p[i] + q[i], p[i] - q[i], -p[i] or [8] p[i]; ok[i] = every input of item i decodes
template <int IN, int OUT, int OP>
__global__ void __launch_bounds__(256) k_group_elem(const uint8_t *__restrict__ p, const uint8_t *__restrict__ q, u64 n, uint8_t *__restrict__ out_raw,
                                                    u32 *__restrict__ scratch, uint8_t *__restrict__ ok) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    bool okp, okq = true;
    const ge_p3 P = grp_load<IN>(p, idx, okp);
    ge_p3 R;
    if (OP == GR_ADD || OP == GR_SUB) {
        const ge_p3 Q = grp_load<IN>(q, idx, okq);
        R = ge_add(P, OP == GR_SUB ? ge_neg(Q) : Q);
    } else if (OP == GR_NEG) {
        R = ge_neg(P);
    } else {                                                // ge_mul_by_pow_2(P, 3) written out: its loop would be a branch on vcc
        ge_p2 s = ge_p1p1_to_p2(ge_dbl(P.X, P.Y, P.Z));
        s = ge_p1p1_to_p2(ge_dbl(s.X, s.Y, s.Z));
        R = ge_p1p1_to_p3(ge_dbl(s.X, s.Y, s.Z));
    }
    grp_emit<OUT>(R, idx, out_raw, scratch);
    ok[idx] = (okp & okq) ? 1 : 0;
}

// eq[i] = p[i] == q[i] in the group (GROUP 0 Edwards, 1 Ristretto), or p[i] == identity without q; 0 where an input does not decode
template <int IN, int GROUP, bool HASQ>
__global__ void __launch_bounds__(256) k_group_eq(const uint8_t *__restrict__ p, const uint8_t *__restrict__ q, u64 n, uint8_t *__restrict__ eq,
                                                  uint8_t *__restrict__ ok) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    bool okp, okq = true;
    const ge_p3 P = grp_load<IN>(p, idx, okp);
    const ge_p3 Q = HASQ ? grp_load<IN>(q, idx, okq) : ge_identity();
    const bool e = GROUP == 1 ? ris_eq(P, Q) : (HASQ ? ge_eq(P, Q) : ge_is_identity(P));
    const bool good = okp & okq;
    eq[idx] = (e & good) ? 1 : 0;
    ok[idx] = good ? 1 : 0;
}

// flag |= 1 if some ok byte is 0 (the C25519_NONE status of a call with compressed inputs)
__global__ void __launch_bounds__(256) k_group_any_bad(const uint8_t *__restrict__ ok, u64 n, u32 *__restrict__ flag) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    if (!ok[idx]) atomicOr(flag, 1u);
}

// ---- segmented sum -------------------------------------------------------------------------------------------------------------
// key[g] = the segment of point g: the largest s < m with seg_off[s] <= g (empty segments own no point)
__global__ void __launch_bounds__(256) k_seg_keys(const u64 *__restrict__ seg_off, u64 m, u64 n, u32 *__restrict__ key) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    u64 lo = 0, hi = m;                 // seg_off[lo] <= g < seg_off[hi] = n
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (seg_off[mid] <= g) lo = mid; else hi = mid;
    }
    key[g] = (u32)lo;
}

// One level of the segmented sum over nL items (points of format IN with keys `key`; at level 0 the caller's points, later the pieces
// of the level before).  Wave w folds chunk w = items [w C, w C + C): lane l its K items [w C + l K, + K) serially, then a segmented
// inclusive scan of the lanes' open pieces.  A segment whose first and last item lie in the chunk is complete: its sum goes to
// S40[key] with Sbad[key] (some point did not decode).  A segment open at the chunk's start leaves its head piece at P[2w], one open at
// its end the tail piece at P[2w + 1] (a chunk inside one segment: the whole sum at P[2w + 1], the identity at P[2w], both keyed);
// absent pieces are the identity keyed KEY_NONE.  So the pieces of a segment that spans chunks w0..w1 sit at P[2 w0 + 1 .. 2 w1],
// contiguous, and the next level folds them with the same rule.  Every branch and store address follows from the keys.
template <int IN>
__global__ void __launch_bounds__(256) k_seg_sum(const uint8_t *__restrict__ pts, const u32 *__restrict__ key, const uint8_t *__restrict__ bad_in, u64 nL, u64 nch,
                                                 u32 *__restrict__ P40, u32 *__restrict__ Pkey, uint8_t *__restrict__ Pbad, u32 *__restrict__ S40,
                                                 uint8_t *__restrict__ Sbad) {
    const u64 c = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nch) return;                                   // wave-uniform
    const u32 lane = threadIdx.x & 63u;
    const u64 lo = c * SUM_C, base = lo + (u64)lane * SUM_K, last = nL - 1;
    auto key_at = [&](u64 g) -> u32 { const u32 k = key[g < nL ? g : last]; return g < nL ? k : KEY_NONE; };
    const u32 kfirst = key_at(base);
    u32 kprev = base ? key_at(base - 1) : KEY_NONE;
    const bool first_head = kfirst == KEY_NONE || kfirst != kprev;
    ge_p3 acc = ge_identity(), F = ge_identity();
    u32 accb = 0, Fb = 0;
    bool seen = false, tail = false;
#pragma unroll 1
    for (int j = 0; j < SUM_K; j++) {
        const u64 g = base + (u64)j;
        const u32 kc = key_at(g), kn = key_at(g + 1);
        const bool head = kc == KEY_NONE || kc != kprev;
        tail = kc == KEY_NONE || kc != kn;
        bool okx;
        const ge_p3 x = grp_load<IN>(pts, g < nL ? g : last, okx);
        const u32 bx = (IN == 3 ? (u32)bad_in[g < nL ? g : last] : 0u) | (okx ? 0u : 1u);
        const ge_p3 s = ge_add(acc, x);
        const bool fh = head & !seen;                       // the first head of the lane: what came before it is the lane's first piece
        F = ge_select(F, acc, fh);
        Fb = fh ? accb : Fb;
        acc = ge_select(s, x, head);
        accb = head ? bx : (accb | bx);
        seen |= head;
        ge_pin(acc); ge_pin(F);
        if (tail & seen & (kc != KEY_NONE)) {               // head and tail in this lane: complete
            p40_store(S40, kc, acc);
            Sbad[kc] = (uint8_t)accb;
        }
        kprev = kc;
    }
    F = ge_select(F, acc, !seen);                            // no head: the whole lane is its first piece
    Fb = seen ? Fb : accb;
    // segmented inclusive scan of (seen, acc) across the wave: inc = seen ? acc : inc(lane - 1) + acc
    ge_p3 inc = acc;
    u32 incb = accb, f = seen ? 1u : 0u;
#pragma unroll 1
    for (u32 off = 1; off < 64; off <<= 1) {
        ge_p3 o;
        for (int i = 0; i < 10; i++) {
            o.X.v[i] = __shfl_up(inc.X.v[i], off, 64); o.Y.v[i] = __shfl_up(inc.Y.v[i], off, 64);
            o.Z.v[i] = __shfl_up(inc.Z.v[i], off, 64); o.T.v[i] = __shfl_up(inc.T.v[i], off, 64);
        }
        const u32 ob = __shfl_up(incb, off, 64), of = __shfl_up(f, off, 64);
        const bool in_range = lane >= off;
        const bool take = in_range & (f == 0u);
        inc = ge_select(inc, ge_add(o, inc), take);
        incb = take ? (ob | incb) : incb;
        f = in_range ? (f | of) : f;
        ge_pin(inc);
    }
    ge_p3 cin;                                               // what the lanes before this one hold of the segment open at its start
    for (int i = 0; i < 10; i++) {
        cin.X.v[i] = __shfl_up(inc.X.v[i], 1, 64); cin.Y.v[i] = __shfl_up(inc.Y.v[i], 1, 64);
        cin.Z.v[i] = __shfl_up(inc.Z.v[i], 1, 64); cin.T.v[i] = __shfl_up(inc.T.v[i], 1, 64);
    }
    u32 cinb = __shfl_up(incb, 1, 64);
    cin = ge_select(cin, ge_identity(), lane == 0);
    cinb = lane == 0 ? 0u : cinb;
    const ge_p3 tot = ge_add(cin, F);
    const u32 totb = cinb | Fb;
    // the chunk's edges
    const u64 e = (lo + SUM_C < nL ? lo + SUM_C : nL) - 1;
    const u32 sa = key_at(lo), sb = key_at(e);
    const bool in_open = lo > 0 && sa != KEY_NONE && sa == key_at(lo - 1);
    const bool out_open = sb != KEY_NONE && sb == key_at(e + 1);
    const bool whole = in_open & out_open & (sa == sb);
    // a lane whose first piece continues a segment and is closed in the lane: a complete sum, or the chunk's head piece
    if (!first_head & (seen | tail) & (kfirst != KEY_NONE)) {
        if (in_open & (kfirst == sa)) { p40_store(P40, 2 * c, tot); Pkey[2 * c] = sa; Pbad[2 * c] = (uint8_t)totb; }
        else { p40_store(S40, kfirst, tot); Sbad[kfirst] = (uint8_t)totb; }
    }
    if (lane == 63) {
        p40_store(P40, 2 * c + 1, ge_select(ge_identity(), inc, out_open));
        Pkey[2 * c + 1] = out_open ? sb : KEY_NONE;
        Pbad[2 * c + 1] = out_open ? (uint8_t)incb : (uint8_t)0;
        if (!in_open | whole) { p40_store(P40, 2 * c, ge_identity()); Pkey[2 * c] = whole ? sa : KEY_NONE; Pbad[2 * c] = 0; }
    }
}

// sums[s]: the identity for an empty segment, else S40[s]; ok[s] = no point of segment s failed to decode
template <int OUT>
__global__ void __launch_bounds__(256) k_seg_finish(const u64 *__restrict__ seg_off, u64 m, const u32 *__restrict__ S40, const uint8_t *__restrict__ Sbad,
                                                    uint8_t *__restrict__ out_raw, u32 *__restrict__ scratch, uint8_t *__restrict__ ok) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m) return;
    const bool empty = seg_off[s] == seg_off[s + 1];
    const ge_p3 P = ge_select(p40_load(S40, s), ge_identity(), empty);
    grp_emit<OUT>(P, s, out_raw, scratch);
    ok[s] = (empty || !Sbad[s]) ? 1 : 0;
}

}  // namespace c25519

// ---- host side ----------------------------------------------------------------------------------------------------------------
// (the format rule of every call here: capi_util.h fmt_pair_ok)
static inline bool grp_compressed(int in_fmt) { return in_fmt != C25519_FMT_RAW160; }

template <int OP, int IN>
static void elem_launch2(int outm, const uint8_t *p, const uint8_t *q, uint64_t n, uint8_t *raw, uint32_t *scratch, uint8_t *ok, hipStream_t st) {
    if (outm == GR_RAW) hipLaunchKernelGGL((k_group_elem<IN, GR_RAW, OP>), dim3(div_up(n, 256)), dim3(256), 0, st, p, q, n, raw, scratch, ok);
    else hipLaunchKernelGGL((k_group_elem<IN, GR_P32, OP>), dim3(div_up(n, 256)), dim3(256), 0, st, p, q, n, raw, scratch, ok);
}
template <int OP>
static void elem_launch1(int in_fmt, int outm, const uint8_t *p, const uint8_t *q, uint64_t n, uint8_t *raw, uint32_t *scratch, uint8_t *ok, hipStream_t st) {
    if (in_fmt == C25519_FMT_EDWARDS_Y) elem_launch2<OP, 0>(outm, p, q, n, raw, scratch, ok, st);
    else if (in_fmt == C25519_FMT_RAW160) elem_launch2<OP, 2>(outm, p, q, n, raw, scratch, ok, st);
    else if constexpr (OP != GR_COF) elem_launch2<OP, 1>(outm, p, q, n, raw, scratch, ok, st);
}

// the output of n points written by `launch(outm, raw, scratch)`: straight to d_out (RAW160), through the batched Edwards compressor, or
// through the Ristretto compressor from a raw staging buffer (tmp_e)
template <class L>
static int32_t grp_out(c25519_ctx *ctx, uint64_t n, int out_fmt, uint8_t *d_out, L &&launch) {
    int32_t r;
    if (out_fmt == C25519_FMT_RAW160) {
        launch(GR_RAW, d_out, (uint32_t *)nullptr);
        HIPCHK(hipGetLastError());
    } else if (out_fmt == C25519_FMT_RISTRETTO) {
        if ((r = ctx_reserve(ctx, ctx->tmp_e, n * 160 + 16))) return r;
        launch(GR_RAW, (uint8_t *)ctx->tmp_e.p, (uint32_t *)nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(launch_compress_ristretto((const uint8_t *)ctx->tmp_e.p, n, d_out, ctx->stream));
    } else {
        if ((r = ctx_reserve(ctx, ctx->scratch, n * 128)) || (r = ctx_reserve(ctx, ctx->prefix, n * 48))) return r;
        launch(GR_P32, (uint8_t *)nullptr, (uint32_t *)ctx->scratch.p);
        HIPCHK(hipGetLastError());
        HIPCHK(launch_compress_p32((const uint32_t *)ctx->scratch.p, (uint32_t *)ctx->prefix.p, n, d_out, ctx->stream));
    }
    return C25519_OK;
}
// the ok bytes: the caller's, or tmp_f
static int32_t grp_ok_buf(c25519_ctx *ctx, uint64_t n, uint8_t *d_ok, uint8_t **okbuf) {
    if (d_ok) { *okbuf = d_ok; return C25519_OK; }
    int32_t r = ctx_reserve(ctx, ctx->tmp_f, n + 16);
    *okbuf = (uint8_t *)ctx->tmp_f.p;
    return r;
}
// compressed inputs: OR "some ok byte is 0" into d_flag (zeroed by the entry point)
static int32_t grp_flag_bad(c25519_ctx *ctx, int in_fmt, const uint8_t *okbuf, uint64_t n) {
    if (!grp_compressed(in_fmt) || n == 0) return C25519_OK;
    hipLaunchKernelGGL(k_group_any_bad, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, okbuf, n, (uint32_t *)ctx->d_flag);
    HIPCHK(hipGetLastError());
    return C25519_OK;
}
// C25519_NONE iff d_flag was raised (synchronises the context's stream)
static int32_t grp_status(c25519_ctx *ctx) {
    uint32_t *bad = (uint32_t *)ctx->h_msm;              // pinned
    HIPCHK(hipMemcpyAsync(bad, ctx->d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return *bad ? C25519_NONE : C25519_OK;
}

static int32_t elem_enqueue(c25519_ctx *ctx, const uint8_t *d_p, const uint8_t *d_q, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *d_out, uint8_t *d_ok) {
    uint8_t *okbuf;
    int32_t r;
    if ((r = grp_ok_buf(ctx, n, d_ok, &okbuf))) return r;
    r = grp_out(ctx, n, out_fmt, d_out, [&](int outm, uint8_t *raw, uint32_t *scratch) {
        if (op == GR_ADD) elem_launch1<GR_ADD>(in_fmt, outm, d_p, d_q, n, raw, scratch, okbuf, ctx->stream);
        else if (op == GR_SUB) elem_launch1<GR_SUB>(in_fmt, outm, d_p, d_q, n, raw, scratch, okbuf, ctx->stream);
        else if (op == GR_NEG) elem_launch1<GR_NEG>(in_fmt, outm, d_p, d_q, n, raw, scratch, okbuf, ctx->stream);
        else elem_launch1<GR_COF>(in_fmt, outm, d_p, d_q, n, raw, scratch, okbuf, ctx->stream);
    });
    return r ? r : grp_flag_bad(ctx, in_fmt, okbuf, n);
}
static int32_t elem_dev(c25519_ctx *ctx, const uint8_t *d_p, const uint8_t *d_q, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *d_out, uint8_t *d_ok) {
    if (n == 0) return C25519_OK;
    if (grp_compressed(in_fmt)) HIPCHK(hipMemsetAsync(ctx->d_flag, 0, 4, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    int32_t r = elem_enqueue(ctx, d_p, d_q, n, op, in_fmt, out_fmt, d_out, d_ok);
    if (r) return r;
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return grp_compressed(in_fmt) ? grp_status(ctx) : C25519_OK;
}
static int32_t elem_host(c25519_ctx *ctx, const uint8_t *p, const uint8_t *q, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *out, uint8_t *ok) {
    if (n == 0) return C25519_OK;
    if (grp_compressed(in_fmt)) HIPCHK(hipMemsetAsync(ctx->d_flag, 0, 4, ctx->stream));
    const size_t pb = point_bytes(in_fmt);
    const bool binary = op == GR_ADD || op == GR_SUB;
    const int32_t r = ffi_twin(ctx, n, 1u << 16, {{p, pb, FFI_TMP_A, 16}, {binary ? q : nullptr, binary ? pb : 0, FFI_TMP_A, 16}},
                               {{out, point_bytes(out_fmt), FFI_TMP_B, 16}, {ok, 1, FFI_TMP_C, 16}},
                               [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) {
                                   return elem_enqueue(ctx, d_in[0], binary ? d_in[1] : nullptr, m, op, in_fmt, out_fmt, d_out[0], d_out[1]);
                               });
    if (r) return r;
    return grp_compressed(in_fmt) ? grp_status(ctx) : C25519_OK;
}

static int32_t add_check(c25519_ctx *ctx, int op, int in_fmt, int out_fmt) {
    if (op != C25519_POINT_ADD && op != C25519_POINT_SUB) return bad_arg(ctx, "point_add: op must be C25519_POINT_ADD or C25519_POINT_SUB");
    if (!fmt_pair_ok(in_fmt, out_fmt)) return bad_arg(ctx, "point_add: in_fmt and out_fmt must belong to one group");
    return C25519_OK;
}
static int32_t map_check(c25519_ctx *ctx, int op, int in_fmt, int out_fmt) {
    if (op != C25519_POINT_NEG && op != C25519_POINT_MUL_BY_COFACTOR) return bad_arg(ctx, "point_map: op must be C25519_POINT_NEG or C25519_POINT_MUL_BY_COFACTOR");
    if (!fmt_pair_ok(in_fmt, out_fmt)) return bad_arg(ctx, "point_map: in_fmt and out_fmt must belong to one group");
    if (op == C25519_POINT_MUL_BY_COFACTOR && (in_fmt == C25519_FMT_RISTRETTO || out_fmt == C25519_FMT_RISTRETTO))
        return bad_arg(ctx, "point_map: mul_by_cofactor is an Edwards operation");
    return C25519_OK;
}

EXPORT int32_t c25519_point_add_batch_dev(c25519_ctx *ctx, const uint8_t *d_p, const uint8_t *d_q, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *d_out,
                                          uint8_t *d_ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = add_check(ctx, op, in_fmt, out_fmt))) return r;
    return elem_dev(ctx, d_p, d_q, n, op == C25519_POINT_ADD ? GR_ADD : GR_SUB, in_fmt, out_fmt, d_out, d_ok);
}
EXPORT int32_t c25519_point_add_batch(c25519_ctx *ctx, const uint8_t *p, const uint8_t *q, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *out, uint8_t *ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = add_check(ctx, op, in_fmt, out_fmt))) return r;
    return elem_host(ctx, p, q, n, op == C25519_POINT_ADD ? GR_ADD : GR_SUB, in_fmt, out_fmt, out, ok);
}
EXPORT int32_t c25519_point_map_batch_dev(c25519_ctx *ctx, const uint8_t *d_p, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *d_out, uint8_t *d_ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = map_check(ctx, op, in_fmt, out_fmt))) return r;
    return elem_dev(ctx, d_p, nullptr, n, op == C25519_POINT_NEG ? GR_NEG : GR_COF, in_fmt, out_fmt, d_out, d_ok);
}
EXPORT int32_t c25519_point_map_batch(c25519_ctx *ctx, const uint8_t *p, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *out, uint8_t *ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = map_check(ctx, op, in_fmt, out_fmt))) return r;
    return elem_host(ctx, p, nullptr, n, op == C25519_POINT_NEG ? GR_NEG : GR_COF, in_fmt, out_fmt, out, ok);
}

// ---- equality -------------------------------------------------------------------------------------------------------------------
static bool eq_fmt_ok(int in_fmt, int group) {
    if (group != C25519_FMT_EDWARDS_Y && group != C25519_FMT_RISTRETTO) return false;
    return in_fmt == group || in_fmt == C25519_FMT_RAW160;
}
template <int IN>
static void eq_launch1(int group, bool hasq, const uint8_t *p, const uint8_t *q, uint64_t n, uint8_t *eq, uint8_t *ok, hipStream_t st) {
    const dim3 g(div_up(n, 256)), b(256);
    if (group == C25519_FMT_RISTRETTO) {
        if constexpr (IN != 0) {
            if (hasq) hipLaunchKernelGGL((k_group_eq<IN, 1, true>), g, b, 0, st, p, q, n, eq, ok);
            else hipLaunchKernelGGL((k_group_eq<IN, 1, false>), g, b, 0, st, p, q, n, eq, ok);
        }
    } else if constexpr (IN != 1) {
        if (hasq) hipLaunchKernelGGL((k_group_eq<IN, 0, true>), g, b, 0, st, p, q, n, eq, ok);
        else hipLaunchKernelGGL((k_group_eq<IN, 0, false>), g, b, 0, st, p, q, n, eq, ok);
    }
}
static int32_t eq_enqueue(c25519_ctx *ctx, const uint8_t *d_p, const uint8_t *d_q, uint64_t n, int in_fmt, int group, uint8_t *d_eq, uint8_t *d_ok) {
    uint8_t *okbuf;
    int32_t r;
    if ((r = grp_ok_buf(ctx, n, d_ok, &okbuf))) return r;
    if (in_fmt == C25519_FMT_EDWARDS_Y) eq_launch1<0>(group, d_q != nullptr, d_p, d_q, n, d_eq, okbuf, ctx->stream);
    else if (in_fmt == C25519_FMT_RISTRETTO) eq_launch1<1>(group, d_q != nullptr, d_p, d_q, n, d_eq, okbuf, ctx->stream);
    else eq_launch1<2>(group, d_q != nullptr, d_p, d_q, n, d_eq, okbuf, ctx->stream);
    HIPCHK(hipGetLastError());
    return grp_flag_bad(ctx, in_fmt, okbuf, n);
}
EXPORT int32_t c25519_point_eq_batch_dev(c25519_ctx *ctx, const uint8_t *d_p, const uint8_t *d_q, uint64_t n, int in_fmt, int group, uint8_t *d_eq, uint8_t *d_ok) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!eq_fmt_ok(in_fmt, group)) return bad_arg(ctx, "point_eq: group must be 0 or 1, and a compressed in_fmt must equal it");
    if (n == 0) return C25519_OK;
    if (grp_compressed(in_fmt)) HIPCHK(hipMemsetAsync(ctx->d_flag, 0, 4, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    int32_t r = eq_enqueue(ctx, d_p, d_q, n, in_fmt, group, d_eq, d_ok);
    if (r) return r;
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return grp_compressed(in_fmt) ? grp_status(ctx) : C25519_OK;
}
EXPORT int32_t c25519_point_eq_batch(c25519_ctx *ctx, const uint8_t *p, const uint8_t *q, uint64_t n, int in_fmt, int group, uint8_t *eq, uint8_t *ok) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!eq_fmt_ok(in_fmt, group)) return bad_arg(ctx, "point_eq: group must be 0 or 1, and a compressed in_fmt must equal it");
    if (n == 0) return C25519_OK;
    if (grp_compressed(in_fmt)) HIPCHK(hipMemsetAsync(ctx->d_flag, 0, 4, ctx->stream));
    const size_t pb = point_bytes(in_fmt);
    const int32_t r = ffi_twin(ctx, n, 1u << 16, {{p, pb, FFI_TMP_A, 16}, {q, q ? pb : 0, FFI_TMP_A, 16}}, {{eq, 1, FFI_TMP_B, 16}, {ok, 1, FFI_TMP_C, 16}},
                               [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) {
                                   return eq_enqueue(ctx, d_in[0], q ? d_in[1] : nullptr, m, in_fmt, group, d_out[0], d_out[1]);
                               });
    if (r) return r;
    return grp_compressed(in_fmt) ? grp_status(ctx) : C25519_OK;
}

// ---- segmented sum --------------------------------------------------------------------------------------------------------------
static int32_t sum_enqueue(c25519_ctx *ctx, const uint8_t *d_points, uint64_t n, int in_fmt, const uint64_t *d_seg_off, uint64_t m, int out_fmt, uint8_t *d_sums,
                           uint8_t *d_ok) {
    hipStream_t st = ctx->stream;
    // tmp_f: ok (m) | S40 (m x 160) | Sbad (m) | keys of level 0 (n x 4) | two piece buffers of n1 = 2 ceil(n / C) records (P40, key, bad)
    const uint64_t nch0 = (n + SUM_C - 1) / SUM_C, n1 = 2 * nch0;
    ws_layout F;
    const size_t o_ok = F.part(m), o_S = F.part(m * 160), o_Sb = F.part(m), o_k = F.part(n * 4);
    size_t o_P40[2], o_Pkey[2], o_Pbad[2];
    for (int i = 0; i < 2; i++) { o_P40[i] = F.part(n1 * 160); o_Pkey[i] = F.part(n1 * 4); o_Pbad[i] = F.part(n1); }
    int32_t r;
    if ((r = F.reserve(ctx, ctx->tmp_f, 256))) return r;
    uint8_t *okbuf = d_ok ? d_ok : F.at(o_ok), *Sbad = F.at(o_Sb);
    u32 *S40 = F.at<u32>(o_S), *keys0 = F.at<u32>(o_k);
    auto P40_of = [&](int i) { return F.at<u32>(o_P40[i]); };
    auto Pkey_of = [&](int i) { return F.at<u32>(o_Pkey[i]); };
    auto Pbad_of = [&](int i) { return F.at(o_Pbad[i]); };
    if (n) {
        hipLaunchKernelGGL(k_seg_keys, dim3(div_up(n, 256)), dim3(256), 0, st, d_seg_off, m, n, keys0);
        const unsigned g0 = div_up(nch0, 4);
        const uint8_t *none = nullptr;
        if (in_fmt == C25519_FMT_EDWARDS_Y)
            hipLaunchKernelGGL(k_seg_sum<0>, dim3(g0), dim3(256), 0, st, d_points, keys0, none, n, nch0, P40_of(0), Pkey_of(0), Pbad_of(0), S40, Sbad);
        else if (in_fmt == C25519_FMT_RISTRETTO)
            hipLaunchKernelGGL(k_seg_sum<1>, dim3(g0), dim3(256), 0, st, d_points, keys0, none, n, nch0, P40_of(0), Pkey_of(0), Pbad_of(0), S40, Sbad);
        else
            hipLaunchKernelGGL(k_seg_sum<2>, dim3(g0), dim3(256), 0, st, d_points, keys0, none, n, nch0, P40_of(0), Pkey_of(0), Pbad_of(0), S40, Sbad);
        HIPCHK(hipGetLastError());
        // fold the pieces until one chunk is left: each level shrinks the array by SUM_C / 2
        uint64_t nch = nch0;
        int cur = 0;
        while (nch > 1) {
            const uint64_t nL = 2 * nch, nn = (nL + SUM_C - 1) / SUM_C;
            hipLaunchKernelGGL(k_seg_sum<3>, dim3(div_up(nn, 4)), dim3(256), 0, st, (const uint8_t *)P40_of(cur), Pkey_of(cur), Pbad_of(cur), nL, nn,
                               P40_of(cur ^ 1), Pkey_of(cur ^ 1), Pbad_of(cur ^ 1), S40, Sbad);
            HIPCHK(hipGetLastError());
            nch = nn;
            cur ^= 1;
        }
    }
    r = grp_out(ctx, m, out_fmt, d_sums, [&](int outm, uint8_t *raw, uint32_t *scratch) {
        if (outm == GR_RAW) hipLaunchKernelGGL(k_seg_finish<GR_RAW>, dim3(div_up(m, 256)), dim3(256), 0, st, d_seg_off, m, S40, Sbad, raw, scratch, okbuf);
        else hipLaunchKernelGGL(k_seg_finish<GR_P32>, dim3(div_up(m, 256)), dim3(256), 0, st, d_seg_off, m, S40, Sbad, raw, scratch, okbuf);
    });
    return r ? r : grp_flag_bad(ctx, in_fmt, okbuf, m);
}
static int32_t sum_check(c25519_ctx *ctx, int in_fmt, uint64_t m, int out_fmt) {
    if (!fmt_pair_ok(in_fmt, out_fmt)) return bad_arg(ctx, "point_sum_segments: in_fmt and out_fmt must belong to one group");
    if (m >= KEY_NONE) return bad_arg(ctx, "point_sum_segments: m must be below 2^32 - 1");
    return C25519_OK;
}
EXPORT int32_t c25519_point_sum_segments_dev(c25519_ctx *ctx, const uint8_t *d_points, uint64_t n, int in_fmt, const uint64_t *d_seg_off, uint64_t m, int out_fmt,
                                             uint8_t *d_sums, uint8_t *d_ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = sum_check(ctx, in_fmt, m, out_fmt))) return r;
    if (m == 0) return C25519_OK;
    if (grp_compressed(in_fmt)) HIPCHK(hipMemsetAsync(ctx->d_flag, 0, 4, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    if ((r = sum_enqueue(ctx, d_points, n, in_fmt, d_seg_off, m, out_fmt, d_sums, d_ok))) return r;
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return grp_compressed(in_fmt) ? grp_status(ctx) : C25519_OK;
}
EXPORT int32_t c25519_point_sum_segments(c25519_ctx *ctx, const uint8_t *points, uint64_t n, int in_fmt, const uint64_t *seg_off, uint64_t m, int out_fmt,
                                         uint8_t *sums, uint8_t *ok) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = sum_check(ctx, in_fmt, m, out_fmt))) return r;
    if (m == 0) return C25519_OK;
    if (seg_off[0] != 0 || seg_off[m] != n) return bad_arg(ctx, "point_sum_segments: seg_off must run from 0 to n");
    for (uint64_t s = 0; s < m; s++)
        if (seg_off[s + 1] < seg_off[s]) return bad_arg(ctx, "point_sum_segments: seg_off must be non-decreasing");
    const size_t pb = point_bytes(in_fmt), ob = point_bytes(out_fmt);
    ws_layout O; O.part(m * ob);                            // tmp_c: the sums | their ok bytes (the tail: not rounded, and 16 bytes behind it)
    if ((r = ctx_reserve(ctx, ctx->tmp_a, n * pb + 16)) || (r = ctx_reserve(ctx, ctx->tmp_b, (m + 1) * 8 + 16)) || (r = O.reserve(ctx, ctx->tmp_c, m + 16))) return r;
    ffi_small_begin(ctx);
    hipStream_t st = ctx->stream;
    uint8_t *d_sums = O.at(0), *d_ok = O.at(O.bytes());
    if (grp_compressed(in_fmt)) HIPCHK(hipMemsetAsync(ctx->d_flag, 0, 4, st));
    if (n) HIPCHK(hipMemcpyAsync(ctx->tmp_a.p, points, n * pb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->tmp_b.p, seg_off, (m + 1) * 8, hipMemcpyHostToDevice, st));
    if ((r = sum_enqueue(ctx, (const uint8_t *)ctx->tmp_a.p, n, in_fmt, (const uint64_t *)ctx->tmp_b.p, m, out_fmt, d_sums, d_ok))) {
        (void)hipStreamSynchronize(st);                    // no queued copy still reads the caller's memory after the return
        return r;
    }
    HIPCHK(hipMemcpyAsync(sums, d_sums, m * ob, hipMemcpyDeviceToHost, st));
    if (ok) HIPCHK(hipMemcpyAsync(ok, d_ok, m, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ffi_small_end(ctx, n * pb + (m + 1) * 8, m * ob + (ok ? m : 0));
    return grp_compressed(in_fmt) ? grp_status(ctx) : C25519_OK;
}
