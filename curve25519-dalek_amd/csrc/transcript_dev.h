// The reference's batch-verification transcript (ed25519-dalek/src/batch.rs:168-222 over batch/transcript.rs:39-207) as __host__ __device__ code:
// Merlin framing on STROBE-128/1600 and Keccak-f[1600], restated from transcript_host.h (which stays the host path) for ONE TRANSCRIPT PER LANE.
// The sponge is sequential, so one batch gains nothing from a GPU; many independent batches (verify_seg.hip, k_mid_vseg_transcript) are as many
// independent sponges.
//
// What shapes the code:
//   - the 25 words of the state stay in registers: every state index is a compile-time constant (each round is written out over constant indices;
//     the 24 rounds are a loop), so nothing spills and the kernel has no private segment;
//   - WHERE the next byte is absorbed depends on the number of signatures, which differs from lane to lane, so it cannot index registers.  The bytes
//     of the current block are assembled in a per-lane staging buffer (LDS on the device, the caller's array on the host) with byte stores at
//     lane-dependent addresses, and XORed into the state as 21 whole words when the block is full or an operation forces the permutation;
//   - the stream is a run of framed pieces of at most 76 bytes (put_msg).  A piece is written past the end of the block without a test per byte --
//     the staging buffer has room for the overflow -- and at most one permutation follows it; what overflowed is then moved down to the start of
//     the next block.  The positions, and with them the control flow, depend only on the number of signatures and the step, never on data: lanes
//     with segments of equal length run in uniform control flow; a lane with another length diverges at the permutations only;
//   - the state after Merlin's initialisation and the domain separator (one permutation and 54 absorbed bytes) is the same for every transcript:
//     the host computes it once (make_prefix) and every lane starts from it;
//   - after the key operation of the ZeroRng (transcript.rs:157-173) the positions are constants: every z is one permutation with three constant
//     words XORed in (words 4, 5, 20 for the first, 2, 3, 20 for the others: the observation of transcript_host.h), two words out and zeroed.
// tests/test_transcript_dev_host.py builds this header for the host and compares it with the host path and the independent STROBE of tests/pyref.py
// for every segment length 0 .. 200: every alignment of every piece against the 166-byte block.
#pragma once
#include <stdint.h>
#include "constants_gen.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define C25519_TR_HD __host__ __device__ __forceinline__
#else
#define C25519_TR_HD inline
#endif

namespace c25519_trd {

typedef uint64_t u64;
typedef uint32_t u32;

enum { R = 166, FI = 1, FA = 2, FC = 4, FT = 8, FM = 16, FK = 32 };   // STROBE-128/1600: the rate and the operation flags
// staging buffer of one transcript, in words: the 166 bytes of a block and the at most 75 bytes a piece may overflow it by.  All zero before the
// first piece; every byte from the write position on is zero between pieces.
constexpr int STAGE_WORDS = 31;

// rotation by a compile-time constant.  Device: two V_ALIGNBIT_B32 on the halves (the compiler turns the shift form into two 64-bit shifts and two ORs)
C25519_TR_HD u64 rotl(u64 x, unsigned n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    if (n == 0) return x;
    if (n == 32) return (u64)lo << 32 | hi;
    const u32 a = n < 32 ? hi : lo, b = n < 32 ? lo : hi, s = 32 - (n & 31);       // rotl by n > 32: by n - 32 with the halves swapped
    return (u64)__builtin_amdgcn_alignbit(a, b, s) << 32 | __builtin_amdgcn_alignbit(b, a, s);
#else
    return n ? (x << n) | (x >> (64 - n)) : x;
#endif
}

// one round of Keccak-f[1600] (FIPS 202 section 3.2): theta, rho and pi as one renaming, chi, iota
C25519_TR_HD void keccak_round(u64 (&a)[25], u64 rc) {
    constexpr unsigned ROT[25] = C25519_KECCAK_ROT;
    u64 c[5], d[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1);
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y] ^ d[x], ROT[x + 5 * y]);
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    a[0] ^= rc;
}
C25519_TR_HD void keccak_f(u64 (&a)[25]) {
    constexpr u64 RC[24] = C25519_KECCAK_RC;
#pragma unroll 1
    for (int rnd = 0; rnd < 24; rnd++) keccak_round(a, RC[rnd]);
}

// the sponge every transcript starts from: Transcript::new(b"ed25519 batch verification") (batch.rs:168, transcript.rs:54-74)
struct prefix { u64 st[25]; u32 pos, pos_begin; };
inline void make_prefix(prefix &p) {
    uint8_t b[200] = {1, R + 2, 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
    u64 a[25];
    for (int w = 0; w < 25; w++) { a[w] = 0; for (int j = 0; j < 8; j++) a[w] |= (u64)b[8 * w + j] << (8 * j); }
    keccak_f(a);
    // meta_ad("Merlin v1.0") at 0; then append_message("dom-sep", ...) at 13: its two operation headers name where the operation before began
    const uint8_t s[54] = {0, FM | FA, 'M', 'e', 'r', 'l', 'i', 'n', ' ', 'v', '1', '.', '0',
                           1, FM | FA, 'd', 'o', 'm', '-', 's', 'e', 'p', 26, 0, 0, 0, 14, FA,
                           'e', 'd', '2', '5', '5', '1', '9', ' ', 'b', 'a', 't', 'c', 'h', ' ', 'v', 'e', 'r', 'i', 'f', 'i', 'c', 'a', 't', 'i', 'o', 'n'};
    for (int k = 0; k < 54; k++) a[k >> 3] ^= (u64)s[k] << (8 * (k & 7));
    for (int w = 0; w < 25; w++) p.st[w] = a[w];
    p.pos = 54; p.pos_begin = 27;
}

constexpr u64 le64(u64 b0, u64 b1, u64 b2, u64 b3, u64 b4, u64 b5, u64 b6, u64 b7) {
    return b0 | b1 << 8 | b2 << 16 | b3 << 24 | b4 << 32 | b5 << 40 | b6 << 48 | b7 << 56;
}

// One framed piece of the stream: two operation headers and what they frame (append_message, transcript.rs:69-74: meta_ad(label) and
// meta_ad(length, more) behind the first header, ad(data) behind the second).  Bytes 0 .. H2 + 1 are c0 | c1 << 64 -- the flags of the first header,
// the label, the length, the flags of the second header at H2 + 1 -- with bytes 0 and H2 left zero for the two headers' "where the operation before
// began"; NW words of data follow.  At most one block boundary falls into a piece (it is shorter than a block): the piece is written as a whole,
// then the block is absorbed (STROBE's run_f: pos_begin at R, the padding 0x04 and 0x80 at R + 1) and what overflowed becomes the start of the next.
template <int H2, int NW>
C25519_TR_HD void put_msg(u64 (&a)[25], u32 &pos, u32 &pos_begin, u64 *stage, u64 c0, u64 c1, const u64 *d) {
    constexpr int L = H2 + 2 + 8 * NW;
    static_assert(H2 >= 2 && H2 + 2 <= 16 && L < R && (R - 1 + L + 7) / 8 <= STAGE_WORDS, "a piece overflows the block by less than the staging buffer holds");
    const u32 p0 = pos, room = R - p0;                      // bytes [0, room) of the piece belong to this block
    const bool h2_here = (u32)H2 < room;                    // the second header starts in this block
    uint8_t *bb = reinterpret_cast<uint8_t *>(stage) + p0;
    c0 |= (u64)pos_begin;                                   // begin_op: {pos_begin, flags}, then pos_begin = pos + 1; a permutation in between clears it
    const u64 hb = h2_here ? (u64)(p0 + 1) : 0;
    if (H2 < 8) c0 |= hb << (8 * (H2 & 7)); else c1 |= hb << (8 * (H2 & 7));
#pragma unroll
    for (int k = 0; k < H2 + 2; k++) bb[k] = (uint8_t)((k < 8 ? c0 : c1) >> (8 * (k & 7)));
#pragma unroll
    for (int w = 0; w < NW; w++)
#pragma unroll
        for (int j = 0; j < 8; j++) bb[H2 + 2 + 8 * w + j] = (uint8_t)(d[w] >> (8 * j));
    if (p0 + (u32)L < (u32)R) { pos = p0 + L; pos_begin = p0 + H2 + 1; return; }
    // the block is full
    const u64 pad = (u64)(h2_here ? p0 + H2 + 1 : p0 + 1) << 48 | 0x84ull << 56;
#pragma unroll
    for (int w = 0; w < 20; w++) a[w] ^= stage[w];
    a[20] ^= (stage[20] & 0x0000ffffffffffffull) | pad;
    constexpr int OW = (L - 1 + 7) / 8, HI = (R - 1 + L - 1) / 8;      // words the overflow can reach; the last word a piece can have written
    u64 nx[OW];
#pragma unroll
    for (int w = 0; w < OW; w++) nx[w] = stage[20 + w] >> 48 | stage[21 + w] << 16;
#pragma unroll
    for (int w = 0; w <= HI; w++) stage[w] = w < OW ? nx[w] : 0;
    keccak_f(a);
    pos = p0 + L - R;
    pos_begin = h2_here ? 0 : H2 - room + 1;
}

// The z_i of one batch of n >= 1 signatures (batch.rs:195-222): hram n x 8 words, sigs n x 8 words (s = words 4 .. 7), z n x 2 words out.
// stage: STAGE_WORDS words, all zero, this transcript's own.
C25519_TR_HD void transcript_zs(const prefix &pre, const u64 *hram, const u64 *sigs, u64 n, u64 *z, u64 *stage) {
    u64 a[25];
#pragma unroll
    for (int w = 0; w < 25; w++) a[w] = pre.st[w];
    u32 pos = pre.pos, pos_begin = pre.pos_begin;
    u64 d[8], nx[8];
    // append_message("hram", h_i, 64), batch.rs:195-197
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = hram[w];
#pragma unroll 1
    for (u64 i = 0; i < n; i++) {
        const u64 *q = hram + 8 * (i + 1 < n ? i + 1 : i);  // (the next row is on its way while this one is absorbed)
#pragma unroll
        for (int w = 0; w < 8; w++) nx[w] = q[w];
        put_msg<10, 8>(a, pos, pos_begin, stage, le64(0, FM | FA, 'h', 'r', 'a', 'm', 64, 0), le64(0, 0, 0, FA, 0, 0, 0, 0), d);
#pragma unroll
        for (int w = 0; w < 8; w++) d[w] = nx[w];
    }
    // append_message("sig.s", s_i, 32), :199-201
#pragma unroll
    for (int w = 0; w < 4; w++) d[w] = sigs[4 + w];
#pragma unroll 1
    for (u64 i = 0; i < n; i++) {
        const u64 *q = sigs + 8 * (i + 1 < n ? i + 1 : i) + 4;
#pragma unroll
        for (int w = 0; w < 4; w++) nx[w] = q[w];
        put_msg<11, 4>(a, pos, pos_begin, stage, le64(0, FM | FA, 's', 'i', 'g', '.', 's', 32), le64(0, 0, 0, 0, FA, 0, 0, 0), d);
#pragma unroll
        for (int w = 0; w < 4; w++) d[w] = nx[w];
    }
    // the ZeroRng, transcript.rs:157-173: meta_ad("rng"), then key(32 zero bytes) -- its header, the permutation its C flag forces unless the header ended a
    // block, and the overwrite of bytes 0 .. 31
    put_msg<5, 0>(a, pos, pos_begin, stage, le64(0, FM | FA, 'r', 'n', 'g', 0, FA | FC, 0), 0, d);
    if (pos != 0) {
        uint8_t *bb = reinterpret_cast<uint8_t *>(stage) + pos;
        bb[0] = (uint8_t)pos_begin; bb[1] = 0x04;
#pragma unroll
        for (int w = 0; w < 21; w++) a[w] ^= stage[w];
        a[20] ^= 0x80ull << 56;
        keccak_f(a);
    }
    a[0] = 0; a[1] = 0; a[2] = 0; a[3] = 0;
    // transcript.rs:200-206: meta_ad(LE32(16)) and prf(16) per z.  The first finds the sponge at pos = 32, pos_begin = 0: headers {0, M|A} at 32 and
    // {33, I|A|C} at 38 around the length, then run_f at 40 (pos_begin = 39, 0x04 at 41, 0x80 at R + 1).  It leaves pos = 16, pos_begin = 0, and so does
    // every later one: the same bytes 16 lower.
    constexpr u64 k4 = le64(0, FM | FA, 16, 0, 0, 0, 33, FI | FA | FC), k5 = le64(39, 0x04, 0, 0, 0, 0, 0, 0);
    constexpr u64 k2 = le64(0, FM | FA, 16, 0, 0, 0, 17, FI | FA | FC), k3 = le64(23, 0x04, 0, 0, 0, 0, 0, 0), k20 = 0x80ull << 56;
#pragma unroll 1
    for (u64 i = 0; i < n; i++) {
        if (i == 0) { a[4] ^= k4; a[5] ^= k5; } else { a[2] ^= k2; a[3] ^= k3; }
        a[20] ^= k20;
        keccak_f(a);
        z[2 * i] = a[0]; z[2 * i + 1] = a[1];
        a[0] = 0; a[1] = 0;
    }
}

}  // namespace c25519_trd
