// The digit recoding of the segmented MSM's bucket route (mid_segb.hip), host and device: tests/host/segb_digits_host.cpp runs it stand-alone
// against Python integers (tests/test_seg_msm_bucket_host.py).
#pragma once
#include "fe26.h"

namespace c25519 {

constexpr int SEGB_C = 8;                                   // window width of the whole route
constexpr int SEGB_WIN = 32;                                // radix-256 windows per scalar
constexpr int SEGB_BUCKETS = 128;                           // |digit| = 1 .. 128
constexpr int SEGB_SLOTS = 2 * SEGB_BUCKETS;                // (|digit|, sign): the positive list of a bucket, then its negative list

// s (eight little-endian words) -> s' = (s mod 2^255) + 0x0080 80...80; returns bit 255 of s.  Byte k of s' minus 128 is digit k for k < 31 (-128 .. 127),
// the top byte (0 .. 128: s mod 2^255 < 2^255 and the carry into it is at most 1) is digit 31 as it stands: sum_k d_k 256^k = s mod 2^255.  The same
// recoding as rows_digits.h at twice the width.
C25519_HD bool segb_recode(u32 s[8]) {
    const bool top = (s[7] >> 31) != 0;
    s[7] &= 0x7fffffffu;
    u64 carry = 0;
    for (int k = 0; k < 8; k++) { const u64 v = (u64)s[k] + (k == 7 ? 0x00808080u : 0x80808080u) + carry; s[k] = (u32)v; carry = v >> 32; }
    return top;
}
C25519_HD int segb_digit(u32 byte, int k) { return k == SEGB_WIN - 1 ? (int)byte : (int)byte - 128; }
// a digit d != 0 -> its list among the SEGB_SLOTS of a window: bucket |d| - 1, the negative digits of a bucket behind its positive ones
C25519_HD u32 segb_slot(int d) { return d < 0 ? 2u * (u32)(-d - 1) + 1u : 2u * (u32)(d - 1); }

}  // namespace c25519
