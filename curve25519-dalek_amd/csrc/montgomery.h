// The Montgomery ladder of montgomery.rs:183-211 (mul_bits_be), shared by k_x25519 (kernels.hip, the clamped caller) and the
// unclamped kernels of montgomery.hip.  Device only: the swaps are lane-mask selects (fe26.h fe_cswap).
#pragma once
#include "ge26.h"

namespace c25519 {

// one step: conditional_swap on prev ^ cur, then differential_add_and_double (montgomery.rs:196-204)
__device__ __forceinline__ void mont_ladder_step(mont_pp &x0, mont_pp &x1, const feT &au, u32 prev, u32 cur) {
    const u32 sw = prev ^ cur;
    fe_cswap(x0.U, x1.U, sw); fe_cswap(x0.W, x1.W, sw);
    mont_diff_add_and_double(x0, x1, au);
}

// u([n] P) in projective form (U : W) for the little-endian 256-bit integer n = s[0..7] and u(P) = au, over bits 254 .. 0 of n:
// bit 255 is skipped, as Mul<&Scalar> skips it (montgomery.rs:488-491, bits_le().rev().skip(1)).  No clamping, no reduction.
// On entry x0 = (1 : 0) and x1 = (au : 1); on return x0 holds the result.  s is consumed: it is kept as a 256-bit shift register so
// no register is indexed dynamically.
__device__ __forceinline__ void mont_ladder_255(u32 s[8], const feT &au, mont_pp &x0, mont_pp &x1) {
    // bit 254 -> position 255
#pragma unroll
    for (int i = 7; i > 0; i--) s[i] = (s[i] << 1) | (s[i - 1] >> 31);
    s[0] <<= 1;
    u32 prev = 0;
#pragma unroll 1
    for (int i = 0; i < 255; i++) {
        u32 cur = s[7] >> 31;
#pragma unroll
        for (int k = 7; k > 0; k--) s[k] = (s[k] << 1) | (s[k - 1] >> 31);
        s[0] <<= 1;
        mont_ladder_step(x0, x1, au, prev, cur);
        prev = cur;
    }
    fe_cswap(x0.U, x1.U, prev); fe_cswap(x0.W, x1.W, prev);    // the final swap on bit 0 (montgomery.rs:206)
}

}  // namespace c25519
