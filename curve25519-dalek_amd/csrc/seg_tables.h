// The per-term preparation of the Straus kernels, shared by mid_seg.hip (c25519_msm_vartime_segments) and mid_mixed.hip
// (c25519_precomp_msm_vartime_mixed_rows): the layout of a term's table {1 .. 8} P and of its 64 digit bytes, the body of the kernel that writes
// them, the two verdict words, and the three constants of the header as the host reads them.  Each file instantiates a kernel of its own
// around seg_tables_term (k_mid_seg_tables<IN>, k_mid_mixed_tables<IN>).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/c25519_hip.h"
#include "devio.h"
#include "kernels.h"
#include "knobs.h"

namespace c25519 {

constexpr int SEG_ENT = 8, SEG_ENT_Q = 10;                  // table entries per term; 16-byte pieces per entry (160 bytes)
constexpr int SEG_DIG = 64;                                 // digit bytes per term (1280 + 64 = 1344 bytes per term, and its ok byte)
enum { SEG_FLAG_NONE = 0, SEG_FLAG_BIT255 = 1 };            // the two verdict words at d_flag

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

}  // namespace c25519

// ---- host side: the three constants of the header; the tuning build reads other values for an A/B run (knobs.h) ----
static inline size_t seg_al256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline uint64_t seg_direct_max() { static const uint64_t v = (uint64_t)std::max<long long>(1, C25519_KNOB_LL("SEG_DIRECT_MAX", C25519_MSM_SEGMENT_DIRECT_MAX)); return v; }
static inline uint64_t seg_wave_max() {
    static const uint64_t v = std::max<uint64_t>((uint64_t)std::max<long long>(1, C25519_KNOB_LL("SEG_WAVE_MAX", C25519_MSM_SEGMENT_WAVE_MAX)), seg_direct_max());
    return v;
}
static inline uint64_t seg_pass_terms() {                   // at least the wave maximum: one segment always fits into a pass
    static const uint64_t v = std::max<uint64_t>((uint64_t)std::max<long long>(1, C25519_KNOB_LL("SEG_PASS_TERMS", C25519_MSM_SEGMENT_PASS_TERMS)), seg_wave_max());
    return v;
}
