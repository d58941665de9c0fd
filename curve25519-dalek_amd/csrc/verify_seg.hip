// Segmented verify_batch: MANY independent Ed25519 batches in one call -- status[s] is what ed25519_verify_batch_keys returns for the
// signatures [seg_off[s], seg_off[s+1]) alone (batch.rs:146-251, once per segment).  DESIGN.md section 3.14.
//
//   ed25519_verify_batch_segments_dev / ed25519_verify_batch_segments / ed25519_verify_batch_segments_plan
//   ed25519_batch_transcript_zs_segments_dev / ed25519_batch_transcript_zs_segments / ed25519_batch_transcript_zs_segments_plan
//
// A segment of k <= ED25519_VERIFY_SEGMENT_MAX signatures becomes one segment of 2k + 1 terms [B | R_0 .. R_{k-1} | A_0 .. A_{k-1}] of the
// segmented MSM (mid_seg.hip); a longer one runs through ed25519_verify_batch_keys_dev on its slice before anything else is queued.
//   launch_hram (verify.hip)   H(R || A || M) of every signature of the call: messages do not care about segments
//   k_mid_vseg_ztree     device z-mode, one WAVE per segment, four per block: the BLAKE2b tree of verify.hip (k_ztree_first / k_ztree_block / k_zderive)
//                        over the segment alone -- <= 256 leaf nodes and <= 4 upper levels through LDS -- tagged with the segment's own length;
//                        the per-level states come from a table the host builds once per distinct length (ztree_make_ivs)
//   k_mid_vseg_transcript   transcript z-mode, one LANE per segment of at most ED25519_TRANSCRIPT_SEGMENT_DEVICE_MAX signatures: the segment's Merlin
//                        transcript (transcript_dev.h: the sponge in registers, the block under assembly in LDS); longer segments keep the host sponge
//                        (ed25519_batch_transcript_zs, one synchronisation in the middle of the call -- only when there is such a segment).  Also the
//                        whole of ed25519_batch_transcript_zs_segments[_dev], there at any length
//   k_mid_vseg_terms     two lanes per signature: the R lane decodes R_i (negated where z_i is negative), writes |z_i| and z_i s_i mod l and
//                        records "s >= l" / "R does not decode"; the A lane decodes A_i (or loads the cached point) and writes z_i h_i mod l.
//                        A point that does not decode is replaced by the identity: the MSM only ever sees points
//   k_mid_vseg_segs      one wave per segment: -sum z_i s_i mod l (strided sums, then six shuffle rounds of sc28_add: no LDS, no barrier), the
//                        basepoint, and the OR of the segment's flags
//   c25519_msm_vartime_segments_dev   the sums, RAW160 -> RAW160, one pass of it per pass of this call
//   k_mid_vseg_verdict   one lane per segment: key decoding over ScalarFormat over Verify (batch.rs:208-211, :244-250), then is_identity of the sum
//                        (no cofactor multiplication: batch.rs:246)
// Everything here is public data: nothing is constant-time and nothing is wiped.  Every loop bound comes from the offsets the host validated.
// (The kernels are named k_mid_vseg_*: members of the k_mid_* family of the vartime MSM and verify_batch, which tests/test_ct_isa_secret_paths.py
// classifies as PUBLIC as a whole -- signatures, keys, messages and the coefficients derived from them.)
// Measured (profiles/verify_seg_numbers.txt; 2^16 signatures, device z-mode): the call beats one ed25519_verify_batch_keys_dev per segment from 8 - 64
// segments on (from 16 at lengths 1, 4 and 256; 8 at 64; 64 at 16; 32 at 1023) and by x2.6 (64 segments of 1023) to x4600 (65536 of 1) at 2^16
// signatures.  It LOSES to ed25519_verify_each_dev over the same signatures at every measured length (x1.3 .. x5.3; the MSM's Straus chains cost more
// per signature than the double-base ladder): callers who do not need the batch equation's own verdict per segment call verify_each.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include <vector>
#include "../../include/c25519_hip.h"
#include "devio.h"
#include "blake2b.h"
#include "sc28.h"
#include "kernels.h"
#include "ctx.h"
#include "ffi.h"
#include "knobs.h"
#include "ztree.h"
#include "transcript_dev.h"
#include "capi_util.h"

using namespace c25519;

static_assert(2 * ED25519_VERIFY_SEGMENT_MAX + 1 <= C25519_MSM_SEGMENT_WAVE_MAX, "the longest segment stays on the segmented MSM's wave route");

namespace c25519 {

constexpr int VSEG_LEVELS = 5;                              // leaf level and four upper ones: 1023 signatures -> 256 -> 64 -> 16 -> 4 -> 1 nodes
constexpr int VSEG_LEAVES = 256, VSEG_IV_U64 = VSEG_LEVELS * 8;
enum { VSEG_BAD_A = 1, VSEG_BAD_S = 2, VSEG_BAD_R = 4 };    // per signature and, ORed, per segment

// Wave w of the launch takes segment s0 + w (cnt of them).  iv_slot[len]: which row of `ivs` (VSEG_IV_U64 words: iv[0 .. 4][8]) belongs to a tree
// over len signatures.  hram: 64 bytes per signature of the call, sigs: 64 bytes each; z16: 16 bytes per signature, written for the signatures
// of the segment only.  Every wave of a block runs the same number of barriers (a wave without a segment works on length 0).
__global__ void __launch_bounds__(256) k_mid_vseg_ztree(const u64 *__restrict__ seg_off, u64 s0, u64 cnt, const uint8_t *__restrict__ hram, const uint8_t *__restrict__ sigs,
                                                    const uint16_t *__restrict__ iv_slot, const u64 *__restrict__ ivs, uint8_t *__restrict__ z16) {
    __shared__ u64 buf0[4][VSEG_LEAVES * 4], buf1[4][(VSEG_LEAVES / 4) * 4];
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u64 idx = (u64)blockIdx.x * 4 + wave;
    u64 a = 0;
    u32 len = 0;
    if (idx < cnt) {
        a = seg_off[s0 + idx];
        const u64 b = seg_off[s0 + idx + 1];
        if (b >= a && b - a <= (u64)ED25519_VERIFY_SEGMENT_MAX) len = (u32)(b - a);
    }
    const u64 *iv = ivs + (u64)iv_slot[len] * VSEG_IV_U64;
    const u32 nleaf = (len + 3) / 4;
    // level 0 (k_ztree_first): (h_c mod l) || s_c of four signatures, two blocks
#pragma unroll 1
    for (u32 r = 0; r < VSEG_LEAVES / 64; r++) {
        const u32 j = 64u * r + lane;
        if (j < nleaf) {
            u64 hs[8], rec[32];
            for (int q = 0; q < 8; q++) hs[q] = iv[q];
#pragma unroll 1
            for (int k = 0; k < 4; k++) {
                const u32 c = 4 * j + (u32)k;
                u32 hred[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                u64 sw[4] = {0, 0, 0, 0};
                if (c < len) {
                    const u32 *hw = reinterpret_cast<const u32 *>(hram) + 16 * (a + c);
                    u32 h16[16];
                    for (int q = 0; q < 16; q++) h16[q] = hw[q];
                    sc28_to_words(sc28_from_wide(h16), hred);
                    const u64 *sg = reinterpret_cast<const u64 *>(sigs) + 8 * (a + c) + 4;
                    for (int q = 0; q < 4; q++) sw[q] = sg[q];
                }
                for (int q = 0; q < 4; q++) { rec[8 * k + q] = (u64)hred[2 * q] | ((u64)hred[2 * q + 1] << 32); rec[8 * k + 4 + q] = sw[q]; }
            }
            blake2b_compress(hs, rec, 256, false);
            blake2b_compress(hs, rec + 16, 384, true);
            for (int q = 0; q < 4; q++) buf0[wave][4 * j + q] = hs[q];
        }
    }
    __syncthreads();
    // upper levels (k_ztree_block): four children, one compression; at most 64 nodes per level, one lane each
    u64 *cur = buf0[wave], *nxt = buf1[wave];
    u32 m = nleaf;
#pragma unroll 1
    for (int lv = 1; lv < VSEG_LEVELS; lv++) {
        const u32 mo = (m + 3) / 4;
        const bool live = m > 1;                            // (wave-uniform)
        if (live && lane < mo) {
            u64 hs[8], w[16];
            for (int q = 0; q < 8; q++) hs[q] = iv[8 * lv + q];
            for (int ch = 0; ch < 4; ch++) {
                const u32 c = 4 * lane + (u32)ch;
                for (int q = 0; q < 4; q++) w[4 * ch + q] = c < m ? cur[4 * c + q] : 0ull;
            }
            blake2b_compress(hs, w, 256, true);
            for (int q = 0; q < 4; q++) nxt[4 * lane + q] = hs[q];
        }
        __syncthreads();
        if (live) { u64 *t = cur; cur = nxt; nxt = t; m = mo; }
    }
    // k_zderive: (z_4i .. z_4i+3) = the four quarters of BLAKE2b-512(root || LE64(i)); only the signatures the segment has are written
#pragma unroll 1
    for (u32 r = 0; r < VSEG_LEAVES / 64; r++) {
        const u32 i = 64u * r + lane;
        if (i < nleaf) {
            u64 hs[8], w[16];
            blake2b_init(hs, 64);
            for (int q = 0; q < 4; q++) w[q] = cur[q];
            w[4] = i;
            for (int q = 5; q < 16; q++) w[q] = 0;
            blake2b_compress(hs, w, 40, true);
            for (u32 q = 0; q < 4; q++) {
                if (4 * i + q < len) {
                    u64 *o = reinterpret_cast<u64 *>(z16) + 2 * (a + 4 * i + q);
                    o[0] = hs[2 * q]; o[1] = hs[2 * q + 1];
                }
            }
        }
    }
}

// Transcript z-mode: LANE j of the launch takes segment s0 + j (cnt of them) and runs its Merlin transcript (transcript_dev.h) over its hram rows and
// s halves: len x 16 bytes of z16, the reference's z_i of that segment alone (batch.rs:168-222).  An empty segment and one longer than max_len (the
// host's share) write nothing.  One wave per block: a wave alone on its SIMD runs a permutation in 11.7 us whatever the number of its lanes, and the
// 64 lanes of a wave beat the same segments spread over more waves at every size measured (one-wave blocks that share a CU land on one SIMD).
// stage: the lane's block under assembly, 248 bytes of LDS; the sponge itself stays in registers.  `pre`: the sponge after the domain separator, the
// same for every transcript.  No barrier: a lane without work leaves.
__global__ void __launch_bounds__(64) k_mid_vseg_transcript(const u64 *__restrict__ seg_off, u64 s0, u64 cnt, u64 max_len, const u64 *__restrict__ hram,
                                                        const u64 *__restrict__ sigs, u64 *__restrict__ z16, const c25519_trd::prefix pre) {
    __shared__ u64 stage[64][c25519_trd::STAGE_WORDS];
    const u32 lane = threadIdx.x & 63u;
    const u64 idx = (u64)blockIdx.x * 64 + lane;
    if (idx >= cnt) return;
    const u64 a = seg_off[s0 + idx], b = seg_off[s0 + idx + 1];
    if (b <= a || b - a > max_len) return;
    for (int w = 0; w < c25519_trd::STAGE_WORDS; w++) stage[lane][w] = 0;
    c25519_trd::transcript_zs(pre, hram + 8 * a, sigs + 8 * a, b - a, z16 + 2 * a, stage[lane]);
}

// Lanes [0, np): the R lane of signature a0 + t; lanes [np, 2 np): its A lane.  The pass holds segments [s0, s1) = signatures [a0, a0 + np); segment s
// owns terms tb = 2 (seg_off[s] - a0) + (s - s0) onwards: [B | R.. | A..].  zs: ten 28-bit limbs of z_i s_i mod l per signature of the pass;
// fl_r / fl_a: one flag byte each.  signed_z: z16 is sign-magnitude (device z-mode, k_zderive).  Scalars as k_batch_scalars makes them.
__global__ void __launch_bounds__(256) k_mid_vseg_terms(const u64 *__restrict__ seg_off, u64 s0, u64 s1, u64 a0, u64 np, const uint8_t *__restrict__ hram,
                                                    const uint8_t *__restrict__ sigs, const uint8_t *__restrict__ pks, const uint8_t *__restrict__ pk_points,
                                                    const uint8_t *__restrict__ z16, int signed_z, uint8_t *__restrict__ scal, uint8_t *__restrict__ pts,
                                                    u32 *__restrict__ zs, uint8_t *__restrict__ fl_r, uint8_t *__restrict__ fl_a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * np || s1 <= s0) return;
    const bool role_a = t >= np;
    const u64 p = role_a ? t - np : t, i = a0 + p;
    // the segment of signature i: the first s with seg_off[s + 1] > i (empty segments own nothing)
    u64 lo = s0, hi = s1 - 1;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (seg_off[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    const u64 sa = seg_off[lo], len = seg_off[lo + 1] - sa;
    if (i < sa || i - sa >= len) return;                    // (offsets the host validated never get here)
    const u64 k = i - sa, tb = 2 * (sa - a0) + (lo - s0);
    const u32 *zw = reinterpret_cast<const u32 *>(z16) + 4 * i;
    const bool neg = signed_z && (zw[3] >> 31);
    u32 zwords[8] = {zw[0], zw[1], zw[2], signed_z ? (zw[3] & 0x7fffffffu) : zw[3], 0, 0, 0, 0};
    u32 zl[5];
    sc28_limbs_from_words<4, 5>(zwords, zl);
    if (!role_a) {
        u32 r[8], s[8];
        load8(sigs, 2 * i, r);
        load8(sigs, 2 * i + 1, s);
        u32 fl = sc28_words_canonical(s) ? 0u : (u32)VSEG_BAD_S;            // signature.rs:89-94 check_scalar
        ge_p3 R;
        if (!ge_decompress(R, r)) { R = ge_identity(); fl |= (u32)VSEG_BAD_R; }
        if (neg) R = ge_neg(R);                             // the scalar stays |z_i| < 2^127: the MSM skips the zero digits of its upper half
        raw160_store(pts, tb + 1 + k, R);
        store8(scal, tb + 1 + k, zwords);
        sc28 v = sc28_mul_5x10(zl, sc28_from_words(s).v);   // |z| s   (a non-canonical s is reduced here and fails the segment through its flag)
        if (neg) v = sc28_neg(v);
        for (int j = 0; j < 10; j++) zs[p * 10 + j] = v.v[j];
        fl_r[p] = (uint8_t)fl;
    } else {
        ge_p3 A;
        bool good = true;
        if (pk_points) A = raw160_load(pk_points, i);       // the key's cached point: trusted (the contract of ed25519_verify_batch_keys)
        else { u32 w[8]; load8(pks, i, w); good = ge_decompress(A, w); }
        if (!good) A = ge_identity();
        raw160_store(pts, tb + 1 + len + k, A);
        const u32 *hw = reinterpret_cast<const u32 *>(hram) + 16 * i;
        u32 h16[16];
        for (int j = 0; j < 16; j++) h16[j] = hw[j];
        sc28 hz = sc28_mul_5x10(zl, sc28_from_wide(h16).v); // |z| h
        if (neg) hz = sc28_neg(hz);
        u32 out[8];
        sc28_to_words(hz, out);
        store8(scal, tb + 1 + len + k, out);
        fl_a[p] = good ? 0 : (uint8_t)VSEG_BAD_A;
    }
}

// Wave w of the launch takes segment s0 + w (cnt of them, signatures from a0 on): term tb gets the basepoint and -sum z_i s_i mod l (batch.rs:240),
// seg_fl[w] the OR of the segment's flags.  Wave-uniform bounds; no LDS, no barrier.
__global__ void __launch_bounds__(256) k_mid_vseg_segs(const u64 *__restrict__ seg_off, u64 s0, u64 cnt, u64 a0, const u32 *__restrict__ zs, const uint8_t *__restrict__ fl_r,
                                                   const uint8_t *__restrict__ fl_a, uint8_t *__restrict__ scal, uint8_t *__restrict__ pts, uint8_t *__restrict__ seg_fl) {
    const u64 w = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= cnt) return;
    const u32 lane = threadIdx.x & 63u;
    const u64 sa = seg_off[s0 + w], sb = seg_off[s0 + w + 1];
    const u64 len = sb >= sa ? sb - sa : 0, p0 = sa - a0, tb = 2 * p0 + w;
    sc28 acc = sc28_zero();
    u32 fl = 0;
#pragma unroll 1
    for (u64 k = lane; k < len; k += 64) {
        sc28 v;
        for (int j = 0; j < 10; j++) v.v[j] = zs[(p0 + k) * 10 + j];
        acc = sc28_add(acc, v);
        fl |= (u32)fl_r[p0 + k] | (u32)fl_a[p0 + k];
    }
#pragma unroll 1
    for (int off = 32; off > 0; off >>= 1) {
        sc28 o;
        for (int j = 0; j < 10; j++) o.v[j] = (u32)__shfl_down((int)acc.v[j], off);
        acc = sc28_add(acc, o);
        fl |= (u32)__shfl_down((int)fl, off);
    }
    if (lane == 0) {
        u32 out[8];
        sc28_to_words(sc28_neg(acc), out);
        store8(scal, tb, out);
        raw160_store(pts, tb, ge_basepoint());
        seg_fl[w] = (uint8_t)fl;
    }
}

// status of segments s0 .. s0 + cnt - 1 from their flags and sums (cnt raw points)
__global__ void __launch_bounds__(256) k_mid_vseg_verdict(const uint8_t *__restrict__ seg_fl, const uint8_t *__restrict__ sums, u64 s0, u64 cnt, uint8_t *__restrict__ status) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    const u32 fl = seg_fl[j];
    uint8_t v;
    if (fl & VSEG_BAD_A) v = C25519_NONE;                   // a key that VerifyingKey::from_bytes rejects
    else if (fl & VSEG_BAD_S) v = C25519_SCALAR_FORMAT;     // batch.rs:208-211
    else if (fl & VSEG_BAD_R) v = C25519_VERIFY;            // batch.rs:244
    else v = ge_is_identity(raw160_load(sums, j)) ? C25519_OK : C25519_VERIFY;      // batch.rs:246-250
    status[s0 + j] = v;
}

}  // namespace c25519

// ---- host side ----------------------------------------------------------------------------------------------------------------
static uint64_t vseg_pass_terms() {                         // (tuning build: other pass sizes for an A/B run; at least one longest segment)
    static const uint64_t v = std::max<uint64_t>((uint64_t)std::max<long long>(1, C25519_KNOB_LL("VSEG_PASS_TERMS", C25519_MSM_SEGMENT_PASS_TERMS)),
                                                 2 * (uint64_t)ED25519_VERIFY_SEGMENT_MAX + 1);
    return v;
}
// the checks of c25519_msm_vartime_segments on its offsets (ctx may be null: the *_plan exports have none)
static const off_msgs VSEG_OFF_MSGS = OFF_MSGS("verify_batch_segments", "seg_off", "n", nullptr);
static int32_t vseg_check_off(c25519_ctx *ctx, uint64_t n, const uint64_t *seg_off, uint64_t m) { return check_offsets(ctx, VSEG_OFF_MSGS, n, seg_off, m); }

// ---- the transcripts of the segments ----
// The longest segment whose transcript ed25519_verify_batch_segments runs on the device (longer ones of the segmented route: the host sponge).
// (tuning build: other boundaries for an A/B run; 0 = every transcript on the host)
static uint64_t vseg_tr_dev_max() {
    static const uint64_t v = (uint64_t)std::min<long long>(ED25519_VERIFY_SEGMENT_MAX, std::max<long long>(0, C25519_KNOB("VSEG_TRANSCRIPT_DEV_MAX", ED25519_TRANSCRIPT_SEGMENT_DEVICE_MAX)));
    return v;
}
static const c25519_trd::prefix &vseg_tr_prefix() {
    static const c25519_trd::prefix p = [] { c25519_trd::prefix q; c25519_trd::make_prefix(q); return q; }();
    return p;
}
// k_mid_vseg_transcript over segments [0, m) of d_off, those of at most max_len signatures
static hipError_t vseg_launch_transcript(c25519_ctx *ctx, const uint64_t *d_off, uint64_t m, uint64_t max_len, const uint8_t *d_hram, const uint8_t *d_sigs, uint8_t *d_z16) {
    hipLaunchKernelGGL(k_mid_vseg_transcript, dim3(div_up(m, 64)), dim3(64), 0, ctx->stream, d_off, (u64)0, m, max_len, (const u64 *)d_hram, (const u64 *)d_sigs,
                       (u64 *)d_z16, vseg_tr_prefix());
    return hipGetLastError();
}

EXPORT int32_t ed25519_batch_transcript_zs_segments_plan(const uint64_t *seg_off, uint64_t m, uint64_t plan[2]) {
    int32_t r;
    if ((r = vseg_check_off(nullptr, offsets_end(seg_off, m), seg_off, m))) return r;
    plan[0] = plan[1] = 0;
    for (uint64_t s = 0; s < m; s++) {
        const uint64_t len = seg_off[s + 1] - seg_off[s];
        if (len <= vseg_tr_dev_max()) plan[0]++;
        else if (len <= (uint64_t)ED25519_VERIFY_SEGMENT_MAX) plan[1]++;
    }
    return C25519_OK;
}

// every segment on the device, whatever its length; enqueue only
EXPORT int32_t ed25519_batch_transcript_zs_segments_dev(c25519_ctx *ctx, const uint8_t *d_hram, const uint8_t *d_sigs, uint64_t n, const uint64_t *seg_off, uint64_t m,
                                                        uint8_t *d_z16) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = vseg_check_off(ctx, n, seg_off, m))) return r;
    if (m == 0 || n == 0) return C25519_OK;
    if (((uintptr_t)d_hram | (uintptr_t)d_sigs | (uintptr_t)d_z16) & 7) return bad_arg(ctx, "batch_transcript_zs_segments: device buffers must be 8-byte aligned");
    if ((r = ctx_reserve(ctx, ctx->tmp_c2, (m + 1) * 8))) return r;
    uint64_t *d_off = (uint64_t *)ctx->tmp_c2.p;
    HIPCHK(hipMemcpyAsync(d_off, seg_off, (m + 1) * 8, hipMemcpyHostToDevice, ctx->stream));   // (pageable memory: the caller's array is free on return)
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    HIPCHK(vseg_launch_transcript(ctx, d_off, m, ~0ull, d_hram, d_sigs, d_z16));
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}

EXPORT int32_t ed25519_batch_transcript_zs_segments(c25519_ctx *ctx, const uint8_t *hram, const uint8_t *sigs, uint64_t n, const uint64_t *seg_off, uint64_t m, uint8_t *z16) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = vseg_check_off(ctx, n, seg_off, m))) return r;
    if (m == 0 || n == 0) return C25519_OK;
    if ((r = ctx_reserve(ctx, ctx->tmp_a, n * 64)) || (r = ctx_reserve(ctx, ctx->tmp_c, n * 64)) || (r = ctx_reserve(ctx, ctx->tmp_b, n * 16))) return r;
    ffi_small_begin(ctx);
    uint8_t *d_h = (uint8_t *)ctx->tmp_a.p, *d_s = (uint8_t *)ctx->tmp_c.p, *d_z = (uint8_t *)ctx->tmp_b.p;
    hipError_t e = hipMemcpyAsync(d_h, hram, n * 64, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_s, sigs, n * 64, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return c25519_fail(ctx, e, "hipMemcpyAsync(inputs)"); }
    r = ed25519_batch_transcript_zs_segments_dev(ctx, d_h, d_s, n, seg_off, m, d_z);
    if (r == C25519_OK && (e = hipMemcpyAsync(z16, d_z, n * 16, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) r = c25519_fail(ctx, e, "hipMemcpyAsync(z16)");
    e = hipStreamSynchronize(ctx->stream);                  // (also after an error: no queued copy still touches the caller's memory)
    if (r == C25519_OK && e != hipSuccess) r = c25519_fail(ctx, e, "hipStreamSynchronize");
    ffi_small_end(ctx, n * 128 + (m + 1) * 8, n * 16);
    return r;
}

// ---- routing: the one place that decides which route a segment takes and where the passes are cut ----
//   len <= ED25519_VERIFY_SEGMENT_MAX   one segment of 2 len + 1 terms of the segmented MSM (empty segments too: 0 * B is the identity)
//   longer                              a single batch, ed25519_verify_batch_keys_dev on its slice
// A pass is a run of consecutive segments of the first kind with at most C25519_MSM_SEGMENT_PASS_TERMS terms in all -- one pass of the MSM; the
// single batches and the term count cut it.
struct vseg_pass { uint64_t s0, s1; };
struct vseg_route {
    uint64_t n_seg = 0, n_long = 0, n_pass = 0, maxt = 0;   // what ed25519_verify_batch_segments_plan reports
    uint64_t max_sigs = 0, max_segs = 0;                    // of a pass: what sizes the workspaces
    std::vector<vseg_pass> passes;                          // the lists: only when asked for
    std::vector<uint64_t> longs;
};
static void vseg_plan(const uint64_t *seg_off, uint64_t m, bool lists, vseg_route &R) {
    const uint64_t ptmax = vseg_pass_terms();
    uint64_t s0 = 0, terms = 0;
    auto close = [&](uint64_t s1) {
        if (s1 > s0) {
            R.n_pass++; R.maxt = std::max(R.maxt, terms);
            R.max_sigs = std::max(R.max_sigs, seg_off[s1] - seg_off[s0]); R.max_segs = std::max(R.max_segs, s1 - s0);
            if (lists) R.passes.push_back({s0, s1});
        }
        terms = 0;
    };
    for (uint64_t s = 0; s < m; s++) {
        const uint64_t len = seg_off[s + 1] - seg_off[s];
        if (len > (uint64_t)ED25519_VERIFY_SEGMENT_MAX) { close(s); s0 = s + 1; R.n_long++; if (lists) R.longs.push_back(s); continue; }
        if (terms + 2 * len + 1 > ptmax) { close(s); s0 = s; }
        terms += 2 * len + 1;
        R.n_seg++;
    }
    close(m);
}

EXPORT int32_t ed25519_verify_batch_segments_plan(const uint64_t *seg_off, uint64_t m, uint64_t plan[4]) {
    int32_t r;
    if ((r = vseg_check_off(nullptr, offsets_end(seg_off, m), seg_off, m))) return r;
    vseg_route R;
    vseg_plan(seg_off, m, false, R);
    plan[0] = R.n_seg; plan[1] = R.n_long; plan[2] = R.n_pass; plan[3] = R.maxt;
    return C25519_OK;
}

// The whole call on device inputs; seg_off has been checked and m > 0.  d_status (device, m bytes) or, for the host form, h_status (host, m bytes:
// the statuses are then kept in a workspace and copied out before the last synchronisation).
static int32_t vseg_run(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len, const uint8_t *d_sigs, const uint8_t *d_pks,
                        const uint8_t *d_pk_points, uint64_t n, const uint64_t *seg_off, uint64_t m, uint32_t z_mode, uint8_t *d_status, uint8_t *h_status) {
    hipStream_t st = ctx->stream;
    vseg_route R;
    vseg_plan(seg_off, m, true, R);
    int32_t r;
    // long segments first, each a single batch (it synchronises and uses workspaces of its own: nothing of this call is queued yet)
    std::vector<uint8_t> long_status(R.longs.size());
    for (size_t k = 0; k < R.longs.size(); k++) {
        const uint64_t a = seg_off[R.longs[k]], len = seg_off[R.longs[k] + 1] - a;
        r = ed25519_verify_batch_keys_dev(ctx, d_msgs, d_msg_off + a, msgs_len, d_sigs + a * 64, d_pks + a * 32, d_pk_points ? d_pk_points + a * 160 : nullptr, len, z_mode);
        if (r < 0) return r;
        long_status[k] = (uint8_t)r;
    }
    // the tree states: one row per distinct length among the segments of the segmented route
    std::vector<uint16_t> iv_slot(ED25519_VERIFY_SEGMENT_MAX + 1, 0);
    std::vector<uint64_t> ivs;
    const bool dev_z = z_mode == C25519_Z_DEVICE;
    if (dev_z) {
        std::vector<uint8_t> seen(ED25519_VERIFY_SEGMENT_MAX + 1, 0);
        uint32_t rows = 0;
        for (const vseg_pass &p : R.passes)
            for (uint64_t s = p.s0; s < p.s1; s++) {
                const uint64_t len = seg_off[s + 1] - seg_off[s];
                if (seen[len]) continue;
                seen[len] = 1;
                ztree_ivs t;
                ztree_make_ivs(len, t);
                iv_slot[len] = (uint16_t)rows++;
                for (int l = 0; l < VSEG_LEVELS; l++) for (int q = 0; q < 8; q++) ivs.push_back(t.iv[l][q]);
            }
        if (ivs.empty()) ivs.assign(VSEG_IV_U64, 0);
    }
    // transcript z-mode: how many segments of the segmented route run their transcript on the device, how many on the host -- by length alone
    const uint64_t tr_max = vseg_tr_dev_max();
    // (n_tr_runs: the runs of consecutive rows the host's segments form)
    constexpr uint64_t VSEG_TR_RUNS = 32;
    uint64_t n_tr_dev = 0, n_tr_host = 0, n_tr_runs = 0, tr_end = ~0ull;
    if (!dev_z)
        for (const vseg_pass &p : R.passes)
            for (uint64_t s = p.s0; s < p.s1; s++) {
                const uint64_t len = seg_off[s + 1] - seg_off[s];
                if (len > tr_max) { n_tr_host++; if (seg_off[s] != tr_end) n_tr_runs++; tr_end = seg_off[s + 1]; }
                else if (len) n_tr_dev++;
            }
    // tmp_c2 (the call): hram | its two counters | z16 | seg_off | tree states | statuses (host form)
    // tmp_d (sized by the largest pass): term scalars | term points | sums | z s | flags of R, of A, of the segments
    ws_layout C, P;
    const size_t c_h = C.part(n * 64), c_fl = C.part(256), c_z = C.part((n + 4) * 16), c_off = C.part((m + 1) * 8), c_slot = C.part(iv_slot.size() * 2),
                 c_iv = C.part(ivs.size() * 8), c_st = C.part(d_status ? 0 : m);
    const size_t p_sc = P.part(R.maxt * 32), p_pt = P.part(R.maxt * 160), p_sum = P.part(R.max_segs * 160), p_zs = P.part(R.max_sigs * 40),
                 p_fr = P.part(R.max_sigs), p_fa = P.part(R.max_sigs), p_sf = P.part(R.max_segs);
    if ((r = C.reserve(ctx, ctx->tmp_c2, 256)) || (r = P.reserve(ctx, ctx->tmp_d, 256))) return r;
    uint8_t *hram = C.at(c_h), *z16 = C.at(c_z), *status = d_status ? d_status : C.at(c_st);
    uint32_t *hfl = C.at<uint32_t>(c_fl);
    uint64_t *d_off = C.at<uint64_t>(c_off), *d_ivs = C.at<uint64_t>(c_iv);
    uint16_t *d_slot = C.at<uint16_t>(c_slot);
    uint8_t *scal = P.at(p_sc), *pts = P.at(p_pt), *sums = P.at(p_sum), *fl_r = P.at(p_fr), *fl_a = P.at(p_fa), *seg_fl = P.at(p_sf);
    uint32_t *zs = P.at<uint32_t>(p_zs);
    uint32_t h_fl[2] = {0, 0};
    std::vector<uint64_t> toff;
    auto enqueue = [&]() -> int32_t {
        HIPCHK(hipEventRecord(ctx->ev0, st));
        HIPCHK(hipMemsetAsync(hfl, 0, 64, st));
        HIPCHK(hipMemcpyAsync(d_off, seg_off, (m + 1) * 8, hipMemcpyHostToDevice, st));
        HIPCHK(launch_hram(d_msgs, d_msg_off, msgs_len, d_sigs, d_pks, n, hram, hfl, st));
        if (dev_z) {
            HIPCHK(hipMemcpyAsync(d_slot, iv_slot.data(), iv_slot.size() * 2, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_ivs, ivs.data(), ivs.size() * 8, hipMemcpyHostToDevice, st));
        } else if (!n_tr_host) {
            // the reference's transcript (batch.rs:168-222), one per segment: on the device, one lane each, up to vseg_tr_dev_max() signatures.  (The kernel reads
            // d_sigs as 64-bit words, as k_mid_vseg_ztree does: the header's general contract has device buffers of 64-byte items 16-byte aligned.)
            if (n_tr_dev) HIPCHK(vseg_launch_transcript(ctx, d_off, m, tr_max, hram, d_sigs, z16));
        } else {
            // ... and with longer segments of the segmented route: those on the host -- the one mid-call synchronisation of this z-mode, only when there is
            // such a segment.  The hashes and the signatures come to the host first; then the kernel is queued and the host sponge runs BESIDE it, and the
            // host's rows go back in runs of consecutive rows (the kernel writes the others; empty segments own none).  Where short and long segments
            // alternate so often that there would be more than VSEG_TR_RUNS such copies, the host goes first instead, its rows go up in ONE copy from the
            // first to the last of them, and the kernel, queued behind that copy, overwrites the rows in between that are its own.
            int32_t q;
            if ((q = ctx_host_stage(ctx, n * 144 + 64))) return q;
            uint8_t *hh = (uint8_t *)ctx->h_stage, *hs = hh + n * 64, *hz = hs + n * 64;
            HIPCHK(hipMemcpyAsync(hh, hram, n * 64, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(hs, d_sigs, n * 64, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_fl, hfl, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (h_fl[1]) return bad_arg(ctx, "verify_batch_segments: msg_off is not monotone or runs past msgs_len");
            const bool beside = n_tr_runs <= VSEG_TR_RUNS;
            if (n_tr_dev && beside) HIPCHK(vseg_launch_transcript(ctx, d_off, m, tr_max, hram, d_sigs, z16));
            uint64_t run_a = 0, run_b = 0, first = n, last = 0;
            for (const vseg_pass &p : R.passes)
                for (uint64_t s = p.s0; s < p.s1; s++) {
                    const uint64_t a = seg_off[s], len = seg_off[s + 1] - a;
                    if (len <= tr_max) continue;
                    ed25519_batch_transcript_zs(hh + a * 64, hs + a * 64, len, hz + a * 16);
                    first = std::min(first, a); last = a + len;
                    if (a != run_b) {
                        if (beside && run_b > run_a) HIPCHK(hipMemcpyAsync(z16 + run_a * 16, hz + run_a * 16, (run_b - run_a) * 16, hipMemcpyHostToDevice, st));
                        run_a = a;
                    }
                    run_b = a + len;
                }
            if (beside) {
                if (run_b > run_a) HIPCHK(hipMemcpyAsync(z16 + run_a * 16, hz + run_a * 16, (run_b - run_a) * 16, hipMemcpyHostToDevice, st));
            } else {
                HIPCHK(hipMemcpyAsync(z16 + first * 16, hz + first * 16, (last - first) * 16, hipMemcpyHostToDevice, st));
                if (n_tr_dev) HIPCHK(vseg_launch_transcript(ctx, d_off, m, tr_max, hram, d_sigs, z16));
            }
        }
        for (const vseg_pass &p : R.passes) {
            const uint64_t a0 = seg_off[p.s0], np = seg_off[p.s1] - a0, ns = p.s1 - p.s0;
            if (dev_z && np) hipLaunchKernelGGL(k_mid_vseg_ztree, dim3(div_up(ns, 4)), dim3(256), 0, st, (const u64 *)d_off, p.s0, ns, (const uint8_t *)hram, d_sigs,
                                                (const uint16_t *)d_slot, (const u64 *)d_ivs, z16);
            if (np) hipLaunchKernelGGL(k_mid_vseg_terms, dim3(div_up(2 * np, 256)), dim3(256), 0, st, (const u64 *)d_off, p.s0, p.s1, a0, np, (const uint8_t *)hram, d_sigs, d_pks,
                                       d_pk_points, (const uint8_t *)z16, dev_z ? 1 : 0, scal, pts, zs, fl_r, fl_a);
            hipLaunchKernelGGL(k_mid_vseg_segs, dim3(div_up(ns, 4)), dim3(256), 0, st, (const u64 *)d_off, p.s0, ns, a0, (const u32 *)zs, (const uint8_t *)fl_r,
                               (const uint8_t *)fl_a, scal, pts, seg_fl);
            HIPCHK(hipGetLastError());
            toff.resize(ns + 1);
            for (uint64_t j = 0; j <= ns; j++) toff[j] = 2 * (seg_off[p.s0 + j] - a0) + j;
            // (RAW160 in: every term is a point, so the call cannot return C25519_NONE; it synchronises the stream)
            const int32_t q = c25519_msm_vartime_segments_dev(ctx, scal, pts, 2 * np + ns, C25519_FMT_RAW160, toff.data(), ns, C25519_FMT_RAW160, sums, nullptr);
            if (q < 0) return q;
            if (q != C25519_OK) return bad_arg(ctx, "verify_batch_segments: internal error (the segmented MSM rejected a term)");
            hipLaunchKernelGGL(k_mid_vseg_verdict, dim3(div_up(ns, 256)), dim3(256), 0, st, (const uint8_t *)seg_fl, (const uint8_t *)sums, p.s0, ns, status);
            HIPCHK(hipGetLastError());
        }
        for (size_t k = 0; k < R.longs.size(); k++) HIPCHK(hipMemcpyAsync(status + R.longs[k], long_status.data() + k, 1, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(ctx->ev1, st));
        HIPCHK(hipMemcpyAsync(h_fl, hfl, 8, hipMemcpyDeviceToHost, st));
        if (h_status) HIPCHK(hipMemcpyAsync(h_status, status, m, hipMemcpyDeviceToHost, st));
        return C25519_OK;
    };
    r = enqueue();
    if (r) { (void)hipStreamSynchronize(st); return r; }   // no queued copy still reads host memory after the return
    HIPCHK(hipStreamSynchronize(st));
    if (h_fl[1]) return bad_arg(ctx, "verify_batch_segments: msg_off is not monotone or runs past msgs_len");
    return C25519_OK;
}

EXPORT int32_t ed25519_verify_batch_segments_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len, const uint8_t *d_sigs,
                                                 const uint8_t *d_pks, const uint8_t *d_pk_points, uint64_t n, const uint64_t *seg_off, uint64_t m, uint32_t z_mode,
                                                 uint8_t *d_status) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = vseg_check_off(ctx, n, seg_off, m))) return r;
    if (z_mode > 1) return bad_arg(ctx, "verify_batch_segments: bad z_mode");
    if (m == 0) return C25519_OK;
    return vseg_run(ctx, d_msgs, d_msg_off, msgs_len, d_sigs, d_pks, d_pk_points, n, seg_off, m, z_mode, d_status, nullptr);
}

EXPORT int32_t ed25519_verify_batch_segments(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs, const uint8_t *pks,
                                             const uint8_t *pk_points, uint64_t n, const uint64_t *seg_off, uint64_t m, uint32_t z_mode, uint8_t *status) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = vseg_check_off(ctx, n, seg_off, m))) return r;
    if (z_mode > 1) return bad_arg(ctx, "verify_batch_segments: bad z_mode");
    if (m == 0) return C25519_OK;
    for (uint64_t i = 0; i < n; i++)
        if (msg_off[i] > msg_off[i + 1]) return bad_arg(ctx, "verify_batch_segments: msg_off is not monotone");
    const uint64_t mlen = n ? msg_off[n] : 0;
    if ((r = ctx_reserve(ctx, ctx->tmp_a, mlen + 64)) || (r = ctx_reserve(ctx, ctx->tmp_b, (n + 1) * 8)) || (r = ctx_reserve(ctx, ctx->tmp_c, n * 64 + 16)) ||
        (r = ctx_reserve(ctx, ctx->scratch, n * 32 + (pk_points ? n * 160 : 0) + 16)))
        return r;
    ffi_small_begin(ctx);
    uint8_t *d_msg = (uint8_t *)ctx->tmp_a.p, *d_sig = (uint8_t *)ctx->tmp_c.p, *d_pk = (uint8_t *)ctx->scratch.p, *d_pp = pk_points ? d_pk + n * 32 : nullptr;
    uint64_t *d_off = (uint64_t *)ctx->tmp_b.p;
    if (n) {
        hipError_t e = mlen ? hipMemcpyAsync(d_msg, msgs, mlen, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
        if (e == hipSuccess) e = hipMemcpyAsync(d_off, msg_off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_sig, sigs, n * 64, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_pk, pks, n * 32, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && pk_points) e = hipMemcpyAsync(d_pp, pk_points, n * 160, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return c25519_fail(ctx, e, "hipMemcpyAsync(inputs)"); }
    }
    r = vseg_run(ctx, d_msg, d_off, mlen, d_sig, d_pk, d_pp, n, seg_off, m, z_mode, nullptr, status);
    if (r < 0) (void)hipStreamSynchronize(ctx->stream);    // (an early error: the uploads may still be reading the caller's memory)
    ffi_small_end(ctx, mlen + (n + 1) * 8 + n * 96 + (pk_points ? n * 160 : 0) + (m + 1) * 8, m);
    return r;
}
