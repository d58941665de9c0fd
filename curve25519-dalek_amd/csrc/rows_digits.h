// The digit recoding of the precomputed rows calls (mid_rows.hip, mid_mixed.hip), host and device: tests/host/rows_digits_host.cpp runs it stand-alone against
// Python integers (tests/test_precomp_rows_host.py).
#pragma once
#include "fe26.h"

namespace c25519 {

constexpr int ROWS_WIN = 64;                                // radix-16 windows per scalar
constexpr int ROWS_ENT = 8;                                 // comb records per window (1 .. 8 times the window's base)
constexpr u64 ROWS_REC = (u64)ROWS_WIN * ROWS_ENT;          // comb records per static point: 512 x 128 bytes

// s (eight little-endian words) -> s' = (s mod 2^255) + 0x0888...8; returns bit 255 of s.  Nibble k of s' minus 8 is digit k for k < 63, the top
// nibble (0 .. 8: s mod 2^255 < 2^255 and the carry into it is at most 1) is digit 63 as it stands: sum_k d_k 16^k = s mod 2^255.
C25519_HD bool rows_recode(u32 s[8]) {
    const bool top = (s[7] >> 31) != 0;
    s[7] &= 0x7fffffffu;
    u64 carry = 0;
    for (int k = 0; k < 8; k++) { const u64 v = (u64)s[k] + (k == 7 ? 0x08888888u : 0x88888888u) + carry; s[k] = (u32)v; carry = v >> 32; }
    return top;
}
C25519_HD int rows_digit(u32 nib, int k) { return k == ROWS_WIN - 1 ? (int)nib : (int)nib - 8; }

}  // namespace c25519
