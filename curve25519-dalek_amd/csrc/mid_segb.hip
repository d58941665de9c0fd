// The bucket route of the segmented variable-time multiscalar multiplication (mid_seg.hip, c25519_msm_vartime_segments): segments of more than
// C25519_MSM_SEGMENT_WAVE_MAX and at most C25519_MSM_SEGMENT_BUCKET_MAX terms, each by the bucket method (scalar_mul/pippenger.rs:67-160: signed
// digits, buckets, running-sum reduction, Horner fold) at one window width, 8 bits, ALL such segments of a pass side by side: three launches per
// pass, whatever the number of segments.  DESIGN.md section 3.13.
//
//   k_mid_segb_front<IN>   one lane per term of the pass's bucket segments: decodes the point (as seg_tables_term does), writes its ok byte, ONE
//                          160-byte ProjectiveNiels record (Y+X, Y-X, Z, 2dT; no table, no inversion) and the 32 signed radix-256 digits of the
//                          scalar (segb_digits.h), window-major; raises the bit-255 flag.
//   k_mid_segb_window      one workgroup of two waves per (segment, window): an LDS histogram of the window's digits over the 256 lists (bucket, sign),
//                          a scan, the term indices placed list after list into the (segment, window) slice of a global u16 array (the index is
//                          relative to the segment; the sign is the list's).  Then the placed entries -- NOT the lists -- are cut into 128 equal
//                          chunks, one per lane: a lane adds the records of its chunk (complete additions, 8 M) and stores the sum of every bucket
//                          that STARTS in its chunk into the LDS bucket array (128 x 160 bytes); what it added to a bucket that started earlier
//                          (the head of its chunk) is folded with its neighbours' by a segmented shuffle scan and added to the bucket wave after
//                          wave.  So the work of a lane is ceil(nonzero digits / 128) additions at ANY digit distribution -- all scalars equal
//                          (one list as long as the segment) costs what uniform digits cost, plus the head pass: at most twice.
//                          sum_k k B_k is the sum of the suffix sums S_j = sum_{k >= j} B_k: a shuffle suffix scan and a shuffle fold per wave,
//                          14 complete additions deep.  The window sum leaves as 40 tight limbs; the AND of a 1/32 of the segment's ok bytes beside it.
//   k_mid_segb_finish      one lane per bucket segment: Horner over its 32 window sums (8 doublings and one addition per window), the AND of
//                          its 32 ok bytes; the sum as RAW160 and the verdict where the other routes put theirs.
// The scalars are public by contract (a *_vartime entry point): branches and addresses depend on their digits.  Every loop bound comes from the
// offsets the host validated; no global atomics (the two verdict words are set by plain stores of 1; the histogram's atomics are on LDS); barriers
// are within a workgroup, nothing waits on another workgroup.
#include <hip/hip_runtime.h>
#include "mid_segb.h"

using namespace c25519;

namespace c25519 {

constexpr int SEGB_T = 128;                                 // lanes of a window workgroup = buckets of a window

__device__ __forceinline__ void segb_rec_store(uint4 *rec, u64 i, const ge_cached &c) {
    u32 t[40];
    for (int k = 0; k < 10; k++) { t[k] = c.YpX.v[k]; t[10 + k] = c.YmX.v[k]; t[20 + k] = c.Z.v[k]; t[30 + k] = c.T2d.v[k]; }
    uint4 *q = rec + i * 10;
    for (int k = 0; k < 10; k++) q[k] = make_uint4(t[4 * k], t[4 * k + 1], t[4 * k + 2], t[4 * k + 3]);
}
__device__ __forceinline__ ge_cached segb_rec_load(const uint4 *rec, u64 i) {
    const uint4 *q = rec + i * 10;
    u32 t[40];
    for (int k = 0; k < 10; k++) { const uint4 v = q[k]; t[4 * k] = v.x; t[4 * k + 1] = v.y; t[4 * k + 2] = v.z; t[4 * k + 3] = v.w; }
    ge_cached c;
    for (int k = 0; k < 10; k++) { c.YpX.v[k] = t[k]; c.YmX.v[k] = t[10 + k]; c.Z.v[k] = t[20 + k]; c.T2d.v[k] = t[30 + k]; }
    return c;
}
// bucket b of the LDS array: limb-major (word i of bucket b at i * 128 + b), so a lane per bucket meets no bank twice
__device__ __forceinline__ void segb_lds_store(u32 *bk, u32 b, const ge_p3 &p) {
    for (int i = 0; i < 10; i++) {
        bk[i * SEGB_T + b] = p.X.v[i]; bk[(10 + i) * SEGB_T + b] = p.Y.v[i]; bk[(20 + i) * SEGB_T + b] = p.Z.v[i]; bk[(30 + i) * SEGB_T + b] = p.T.v[i];
    }
}
__device__ __forceinline__ ge_p3 segb_lds_load(const u32 *bk, u32 b) {
    ge_p3 p;
    for (int i = 0; i < 10; i++) {
        p.X.v[i] = bk[i * SEGB_T + b]; p.Y.v[i] = bk[(10 + i) * SEGB_T + b]; p.Z.v[i] = bk[(20 + i) * SEGB_T + b]; p.T.v[i] = bk[(30 + i) * SEGB_T + b];
    }
    return p;
}

// Record i of the pass (i < nt) is term term0[k] + (i - rec_off[k]) of the call, k the segment of the pass with rec_off[k] <= i < rec_off[k + 1].
template <int IN>
__global__ void __launch_bounds__(256) k_mid_segb_front(const uint8_t *__restrict__ scalars, const uint8_t *__restrict__ points, const u64 *__restrict__ desc, u32 nb, u64 nt,
                                                        uint4 *__restrict__ rec, uint8_t *__restrict__ dig, uint8_t *__restrict__ tok, u32 *__restrict__ flags) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt || nb == 0) return;
    const u64 *rec_off = desc, *term0 = desc + nb + 1;
    u32 lo = 0, hi = nb;                                    // rec_off[0] = 0 <= i
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (rec_off[mid] <= i) lo = mid; else hi = mid;
    }
    if (i >= rec_off[lo + 1]) return;                       // (not a record of the descriptor)
    const u64 g = term0[lo] + (i - rec_off[lo]);
    ge_p3 P;
    bool good = true;
    if (IN == 2) P = raw160_load(points, g);
    else { u32 w[8]; load8(points, g, w); good = IN == 0 ? ge_decompress(P, w) : ris_decompress(P, w); }
    tok[i] = good ? 1 : 0;
    segb_rec_store(rec, i, ge_p3_to_cached(P));
    // digits: byte k of s' = (s mod 2^255) + 0x0080...80, biased by 128 below the top one (segb_digits.h).  A scalar with bit 255 set fails the call; its
    // digits are taken from the low 255 bits so that every digit stays within the buckets.
    u32 s[8];
    load8(scalars, g, s);
    if (segb_recode(s)) flags[SEG_FLAG_BIT255] = 1u;
    for (int k = 0; k < SEGB_WIN; k++) dig[(u64)k * nt + i] = (uint8_t)(s[k >> 2] >> (8 * (k & 3)));
}

// Block k * 32 + w: window w of segment k of the pass.
__global__ void __launch_bounds__(SEGB_T) k_mid_segb_window(const u64 *__restrict__ desc, u32 nb, u64 nt, const uint4 *__restrict__ rec, const uint8_t *__restrict__ dig,
                                                            const uint8_t *__restrict__ tok, uint16_t *__restrict__ idx, u32 *__restrict__ wsum, uint8_t *__restrict__ wok) {
    __shared__ u32 bk[40 * SEGB_T];                         // the bucket sums
    __shared__ u32 cnt[SEGB_SLOTS];                         // histogram, then the write cursors of the lists
    __shared__ u32 start[SEGB_SLOTS + 1];                   // where each list starts among the placed entries; start[256] = their number
    __shared__ u32 xch[40];
    __shared__ u32 wtot, sgood;
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 k = blockIdx.x / SEGB_WIN, w = blockIdx.x % SEGB_WIN;
    if (k >= nb) return;
    const u64 r0 = desc[k], r1 = desc[k + 1];
    if (r1 < r0 || r1 > nt || r1 - r0 > 65536ull) return;   // (block-uniform)
    const u32 len = (u32)(r1 - r0);
    const uint8_t *wdig = dig + (u64)w * nt + r0;
    uint16_t *widx = idx + (u64)w * nt + r0;
    const uint4 *srec = rec + r0 * 10;

    cnt[2 * tid] = 0; cnt[2 * tid + 1] = 0;
    if (tid == 0) sgood = 1u;
    segb_lds_store(bk, tid, ge_identity());
    __syncthreads();
    // histogram over the 256 lists; lanes w, w + 32, ... also AND the ok bytes of their terms (the 32 windows of a segment share that work)
    {
        u32 good = 1;
        const bool mine = (tid & 31u) == w;
        for (u32 j = tid; j < len; j += SEGB_T) {
            const int d = segb_digit(wdig[j], (int)w);
            if (d != 0) atomicAdd(&cnt[segb_slot(d)], 1u);
            if (mine) good &= (u32)tok[r0 + j];
        }
        if (!good) sgood = 0u;
    }
    __syncthreads();
    // exclusive scan of the 256 counts: two per lane, a shuffle scan per wave, wave 1 on top of wave 0
    {
        const u32 a = cnt[2 * tid], b = cnt[2 * tid + 1];
        u32 incl = a + b;
        for (int off = 1; off < 64; off <<= 1) { const u32 u = __shfl_up(incl, off, 64); if (lane >= (u32)off) incl += u; }
        if (tid == 63) wtot = incl;
        __syncthreads();
        const u32 excl = (wave ? wtot : 0u) + incl - (a + b);
        start[2 * tid] = excl; start[2 * tid + 1] = excl + a;
        cnt[2 * tid] = excl; cnt[2 * tid + 1] = excl + a;
        if (tid == SEGB_T - 1) start[SEGB_SLOTS] = excl + a + b;
    }
    __syncthreads();
    for (u32 j = tid; j < len; j += SEGB_T) {
        const int d = segb_digit(wdig[j], (int)w);
        if (d != 0) widx[atomicAdd(&cnt[segb_slot(d)], 1u)] = (uint16_t)j;
    }
    __syncthreads();                                        // (the indices are read back by other lanes of this workgroup only)

    // entries [cs, ce) are this lane's
    const u32 nz = start[SEGB_SLOTS], q = (nz + SEGB_T - 1) / SEGB_T;
    const u32 cs = min(tid * q, nz), ce = min(cs + q, nz);
    u32 k0 = 0;                                             // the list that holds entry cs: the last one with start <= cs
    {
        u32 hi = SEGB_SLOTS;
        while (hi - k0 > 1) {
            const u32 mid = (k0 + hi) >> 1;
            if (start[mid] <= cs) k0 = mid; else hi = mid;
        }
    }
    const u32 bf = k0 >> 1;
    const bool head = cs < ce && start[2 * bf] < cs;        // bucket bf started in an earlier lane's chunk
    const u32 hend = head ? min(start[2 * bf + 2], ce) : cs;
    ge_p3 acc = ge_identity();
    {                                                       // behind the head: every bucket met here starts in this chunk, and this lane alone stores it
        u32 ks = k0, cur = 0xffffffffu;
#pragma unroll 1
        for (u32 p = hend; p < ce; p++) {
            while (start[ks + 1] <= p) ks++;                // (p < nz = start[256]: ends at 255 at the latest)
            const u32 b = ks >> 1;
            if (b != cur) {
                if (cur != 0xffffffffu) segb_lds_store(bk, cur, acc);
                acc = ge_identity();
                cur = b;
            }
            acc = ge_p1p1_to_p3(ge_add_cached(acc, ge_cached_cneg(segb_rec_load(srec, (u64)widx[p]), (ks & 1u) != 0)));
            ge_pin(acc);
        }
        if (cur != 0xffffffffu) segb_lds_store(bk, cur, acc);
    }
    acc = ge_identity();
    {                                                       // the head: left in acc
        u32 ks = k0;
#pragma unroll 1
        for (u32 p = cs; p < hend; p++) {
            while (start[ks + 1] <= p) ks++;
            acc = ge_p1p1_to_p3(ge_add_cached(acc, ge_cached_cneg(segb_rec_load(srec, (u64)widx[p]), (ks & 1u) != 0)));
            ge_pin(acc);
        }
    }
    __syncthreads();
    // The heads of one bucket sit in consecutive lanes: a segmented suffix fold leaves their sum (within the wave) in the first of them, which adds
    // it to the bucket -- wave 0, then wave 1, as a bucket's heads may lie in both.
    {
        const u32 key = head ? bf : 0x1000u + tid;
        const u32 prev = __shfl_up(key, 1, 64);
        const bool leader = head && (lane == 0 || prev != key);
#pragma unroll 1
        for (int off = 1; off < 64; off <<= 1) {
            const ge_p3 o = ge_shfl_down(acc, off);
            const u32 okey = __shfl_down(key, off, 64);
            if (lane + (u32)off < 64u && okey == key) acc = ge_add(acc, o);
            ge_pin(acc);
        }
#pragma unroll 1
        for (u32 wv = 0; wv < SEGB_T / 64; wv++) {
            if (wave == wv && leader) segb_lds_store(bk, bf, ge_add(segb_lds_load(bk, bf), acc));
            __syncthreads();
        }
    }
    // lane t holds bucket t + 1 (|digit| = t + 1).  S = the suffix sums, then their sum.
    acc = segb_lds_load(bk, tid);
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        const ge_p3 o = ge_shfl_down(acc, off);
        if (lane + (u32)off < 64u) acc = ge_add(acc, o);
        ge_pin(acc);
    }
    if (tid == 64) { for (int i = 0; i < 10; i++) { xch[i] = acc.X.v[i]; xch[10 + i] = acc.Y.v[i]; xch[20 + i] = acc.Z.v[i]; xch[30 + i] = acc.T.v[i]; } }
    __syncthreads();
    if (wave == 0) {                                        // the buckets of wave 1 lie above every bucket of wave 0
        ge_p3 o;
        for (int i = 0; i < 10; i++) { o.X.v[i] = xch[i]; o.Y.v[i] = xch[10 + i]; o.Z.v[i] = xch[20 + i]; o.T.v[i] = xch[30 + i]; }
        acc = ge_add(acc, o);
    }
    acc = straus_wave_fold(acc);
    __syncthreads();
    if (tid == 64) { for (int i = 0; i < 10; i++) { xch[i] = acc.X.v[i]; xch[10 + i] = acc.Y.v[i]; xch[20 + i] = acc.Z.v[i]; xch[30 + i] = acc.T.v[i]; } }
    __syncthreads();
    if (tid == 0) {
        ge_p3 o;
        for (int i = 0; i < 10; i++) { o.X.v[i] = xch[i]; o.Y.v[i] = xch[10 + i]; o.Z.v[i] = xch[20 + i]; o.T.v[i] = xch[30 + i]; }
        p40_store(wsum, (u64)k * SEGB_WIN + w, ge_add(acc, o));
        wok[(u64)k * SEGB_WIN + w] = (uint8_t)sgood;
    }
}

// Segment k of the pass: sum = sum_w 256^w (window sum w), ok = the AND of its window ok bytes; stored as sum sid[k] of the call.
__global__ void __launch_bounds__(64) k_mid_segb_finish(const u64 *__restrict__ desc, u32 nb, const u32 *__restrict__ wsum, const uint8_t *__restrict__ wok,
                                                        uint8_t *__restrict__ out_raw, uint8_t *__restrict__ ok, u32 *__restrict__ flags) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    const u64 s = desc[2 * (u64)nb + 1 + k];
    ge_p3 acc = p40_load(wsum, (u64)k * SEGB_WIN + SEGB_WIN - 1);
#pragma unroll 1
    for (int w = SEGB_WIN - 2; w >= 0; w--) {
        acc = ge_mul_by_pow_2(acc, SEGB_C);
        acc = ge_add(acc, p40_load(wsum, (u64)k * SEGB_WIN + (u64)w));
        ge_pin(acc);
    }
    u32 good = 1;
    for (int w = 0; w < SEGB_WIN; w++) good &= (u32)wok[(u64)k * SEGB_WIN + (u64)w];
    raw160_store(out_raw, s, acc);
    ok[s] = (uint8_t)good;
    if (!good) flags[SEG_FLAG_NONE] = 1u;
}

}  // namespace c25519

const char *const SEGB_KERNEL_NAME = "c25519::k_mid_segb_window (one workgroup per segment and window: bucket lists in LDS order, 128 equal chunks of entries, suffix-scan reduction)";

int32_t segb_enqueue_pass(c25519_ctx *ctx, int in_fmt, const uint8_t *d_scalars, const uint8_t *d_points, const segb_ws &ws, const uint64_t *d_desc, uint32_t nb, uint64_t nt,
                          uint8_t *sums, uint8_t *okbuf) {
    if (!nb || !nt) return C25519_OK;
    hipStream_t st = ctx->stream;
    uint32_t *flags = (uint32_t *)ctx->d_flag;
    const dim3 g(div_up(nt, 256)), b(256);
    if (in_fmt == C25519_FMT_EDWARDS_Y) hipLaunchKernelGGL(k_mid_segb_front<0>, g, b, 0, st, d_scalars, d_points, d_desc, nb, nt, ws.rec, ws.dig, ws.tok, flags);
    else if (in_fmt == C25519_FMT_RISTRETTO) hipLaunchKernelGGL(k_mid_segb_front<1>, g, b, 0, st, d_scalars, d_points, d_desc, nb, nt, ws.rec, ws.dig, ws.tok, flags);
    else hipLaunchKernelGGL(k_mid_segb_front<2>, g, b, 0, st, d_scalars, d_points, d_desc, nb, nt, ws.rec, ws.dig, ws.tok, flags);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_mid_segb_window, dim3(nb * SEGB_WIN), dim3(SEGB_T), 0, st, d_desc, nb, nt, (const uint4 *)ws.rec, (const uint8_t *)ws.dig, (const uint8_t *)ws.tok, ws.idx,
                       ws.wsum, ws.wok);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_mid_segb_finish, dim3(div_up(nb, 64)), dim3(64), 0, st, d_desc, nb, (const u32 *)ws.wsum, (const uint8_t *)ws.wok, sums, okbuf, flags);
    HIPCHK(hipGetLastError());
    return C25519_OK;
}
