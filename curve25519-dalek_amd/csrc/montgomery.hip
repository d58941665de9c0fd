// Batched MontgomeryPoint arithmetic (curve25519-dalek/src/montgomery.rs), one item per lane:
//
//   c25519_montgomery_mul_batch            impl Mul<&Scalar> for &MontgomeryPoint (montgomery.rs:484-492): the ladder over bits 254..0, unclamped
//   c25519_montgomery_mul_bits_be_batch    MontgomeryPoint::mul_bits_be (montgomery.rs:183-211): the ladder over nbits caller-given bits
//   c25519_montgomery_mul_base_batch       MontgomeryPoint::mul_base (montgomery.rs:144-146) = EdwardsPoint::mul_base(s).to_montgomery()
//   c25519_montgomery_to_edwards_batch     MontgomeryPoint::to_edwards (montgomery.rs:239-268)
//
// The ladders are those of k_x25519 (montgomery.h) and end in the batched division of k_ratio_p32, so W = 0 gives u = 0 as
// as_affine does (montgomery.rs:409).  Everything is constant-time in the scalar, the bits and the point: selects only, loops whose
// trip counts are public (tests/test_ct_isa_montgomery.py asserts it on the compiled code).  Item i reads and writes its own slots only.
#include <hip/hip_runtime.h>
#include <string.h>
#define C25519_CHAIN 1   // chained-carry fe_mul / fe_sq (fe26.h), as kernels.hip compiles k_x25519: the ladders here are the same code
#include "../../include/c25519_hip.h"
#include "devio.h"
#include "montgomery.h"
#include "kernels.h"
#include "knobs.h"
#include "ctx.h"
#include "ffi.h"
#include "capi_util.h"

using namespace c25519;

namespace c25519 {

// u(n P) as (U : W) in P32 scratch for 32-byte n taken as given (bit 255 skipped by the ladder) and u from FieldElement::from_bytes
__global__ void __launch_bounds__(256) k_mont_mul(const uint8_t *__restrict__ ks, const uint8_t *__restrict__ us, u64 n, u32 *__restrict__ scratch) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    u32 s[8], uw[8];
    load8(ks, idx, s);
    load8(us, idx, uw);
    const feT au = fe_from_words(uw);
    mont_pp x0, x1;
    x0.U = fe_one(); x0.W = fe_zero(); x1.U = au; x1.W = fe_one();
    mont_ladder_255(s, au, x0, x1);
    p32_store(scratch, idx, x0.U, x0.U, x0.W);     // (U : W); the division is batched in k_ratio_p32
}

// bytes j .. j+3 of an nb-byte item as a big-endian word, zero past the item's end; j and nb are public, and the address is clamped
// into the item so no lane reads past it (the select on a uniform condition is not a branch)
__device__ __forceinline__ u32 be32_at(const uint8_t *b, u32 j, u32 nb) {
    u32 w = 0;
#pragma unroll
    for (u32 q = 0; q < 4; q++) {
        const u32 k = j + q;
        const u32 v = b[k < nb ? k : nb - 1];
        w = (w << 8) | (k < nb ? v : 0u);
    }
    return w;
}

// mul_bits_be: item idx holds nbits big-endian bits, MSB first, in nb = ceil(nbits / 8) bytes at bits + idx * nb.  The step count
// nbits is a kernel argument (uniform); the bits arrive one 32-bit word per 32 steps at an offset given by the loop counter.
__global__ void __launch_bounds__(256) k_mont_mul_bits(const uint8_t *__restrict__ bits, u32 nbits, u32 nb, const uint8_t *__restrict__ us, u64 n,
                                                       u32 *__restrict__ scratch) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    u32 uw[8];
    load8(us, idx, uw);
    const feT au = fe_from_words(uw);
    const uint8_t *b = bits + idx * nb;
    mont_pp x0, x1;
    x0.U = fe_one(); x0.W = fe_zero(); x1.U = au; x1.W = fe_one();
    u32 prev = 0, word = 0;
#pragma unroll 1
    for (u32 i = 0; i < nbits; i++) {
        if ((i & 31u) == 0u) word = be32_at(b, i >> 3, nb);
        const u32 cur = word >> 31;
        word <<= 1;
        mont_ladder_step(x0, x1, au, prev, cur);
        prev = cur;
    }
    fe_cswap(x0.U, x1.U, prev); fe_cswap(x0.W, x1.W, prev);
    p32_store(scratch, idx, x0.U, x0.U, x0.W);
}

enum { TE_Y = 0, TE_RAW = 1 };   // output of to_edwards: CompressedEdwardsY (32 B) or raw EdwardsPoint (160 B)

// to_edwards, first kernel of the batched division: (u - 1 : u + 1) as a P32 record for k_ratio_p32 (mode 0: N = X, D = Z)
__global__ void __launch_bounds__(256) k_mont_to_edwards_prep(const uint8_t *__restrict__ us, u64 n, u32 *__restrict__ scratch) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    u32 uw[8];
    load8(us, idx, uw);
    const feT u = fe_from_words(uw);
    const feT num = fe_carry(fe_sub(u, fe_one()));
    p32_store(scratch, idx, num, num, fe_carry(fe_add(u, fe_one())));
}

// to_edwards(sign): y = (u - 1) / (u + 1), its canonical bytes with the top byte XORed by the u8 sign << 7, then decompress (edwards.rs:211-258).
// u = -1 is rejected, as is a y that fails sqrt_ratio_i (u on the twist).  BATCHED (the default): y comes canonical from k_ratio_p32 in
// ybuf; otherwise one fe_invert per lane (the A/B arm).  status[i] = 1 (Some) or 0 (None); a None item's output is all zero.
template <int OUT, bool BATCHED>
__global__ void __launch_bounds__(256) k_mont_to_edwards(const uint8_t *__restrict__ us, const uint8_t *__restrict__ signs, const uint8_t *__restrict__ ybuf,
                                                         u64 n, uint8_t *__restrict__ out, uint8_t *__restrict__ status) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    u32 uw[8], yw[8];
    load8(us, idx, uw);
    const feT u = fe_from_words(uw);
    const feT den = fe_carry(fe_add(u, fe_one()));
    const bool minus_one = fe_is_zero(den);                   // montgomery.rs:245 (then y = 0 would decode)
    if (BATCHED) load8(ybuf, idx, yw);
    else fe_to_words(fe_mul(fe_carry(fe_sub(u, fe_one())), fe_invert(den)), yw);
    yw[7] ^= (u32)(uint8_t)(signs[idx] << 7) << 24;           // y_bytes[31] ^= sign << 7 in u8: only bit 0 of sign survives
    ge_p3 P;
    const bool ok = ge_decompress(P, yw) & !minus_one;
    const lanemask m = lane_mask(ok);
    if (OUT == TE_Y) {
        u32 w[8];
        ge_affine_compress(P.X, P.Y, w);                      // x = 0 with the sign bit set stays 0: the encoding of y alone
        for (int q = 0; q < 8; q++) w[q] = sel_u32(0u, w[q], m);
        store8(out, idx, w);
    } else {
        const feT z = fe_zero();
        P.X = fe_select_m(z, P.X, m); P.Y = fe_select_m(z, P.Y, m); P.Z = fe_select_m(z, P.Z, m); P.T = fe_select_m(z, P.T, m);
        raw160_store(out, idx, P);
    }
    status[idx] = ok ? 1 : 0;
}

}  // namespace c25519

// ---- _dev forms --------------------------------------------------------------------------------------------------------------
// the ladder kernel, then U / W batched; scratch / prefix hold secret-derived values and are wiped on every exit path
template <class L>
static int32_t ladder_dev(c25519_ctx *ctx, uint64_t n, uint8_t *d_out, const char *kname, L &&launch) {
    int32_t r;
    if ((r = ctx_reserve(ctx, ctx->scratch, n * 128)) || (r = ctx_reserve(ctx, ctx->prefix, n * 48))) return r;
    stream_wipe wipe(ctx->stream);
    wipe.add(ctx->scratch.p, n * 128); wipe.add(ctx->prefix.p, n * 48);
    hipEvent_t *ring = ctx_ring_item(ctx);
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    ctx->kname[0] = kname;
    HIPCHK(hipEventRecord(ring[0], ctx->stream));
    launch((uint32_t *)ctx->scratch.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ring[1], ctx->stream));
    HIPCHK(launch_ratio_p32(0, (const uint32_t *)ctx->scratch.p, (uint32_t *)ctx->prefix.p, n, d_out, ctx->stream));   // U / W, 0 -> 0
    HIPCHK(hipEventRecord(ring[2], ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}
EXPORT int32_t c25519_montgomery_mul_batch_dev(c25519_ctx *ctx, const uint8_t *d_k, const uint8_t *d_u, uint64_t n, uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (n == 0) return C25519_OK;
    return ladder_dev(ctx, n, d_out, "c25519::k_mont_mul", [&](uint32_t *scratch) {
        hipLaunchKernelGGL(k_mont_mul, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_k, d_u, n, scratch);
    });
}
EXPORT int32_t c25519_montgomery_mul_bits_be_batch_dev(c25519_ctx *ctx, const uint8_t *d_bits, uint32_t nbits, const uint8_t *d_u, uint64_t n, uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (nbits > C25519_MONTGOMERY_MAX_BITS) return bad_arg(ctx, "montgomery_mul_bits_be: nbits must be at most 512");
    if (n == 0) return C25519_OK;
    const uint32_t nb = (nbits + 7) / 8;
    return ladder_dev(ctx, n, d_out, "c25519::k_mont_mul_bits", [&](uint32_t *scratch) {
        hipLaunchKernelGGL(k_mont_mul_bits, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_bits, nbits, nb, d_u, n, scratch);
    });
}
// fixed base, unclamped: c25519_x25519_base_batch_dev without the clamp (constant-time tables unless C25519_FLAG_VARTIME_TABLES)
EXPORT int32_t c25519_montgomery_mul_base_batch_dev(c25519_ctx *ctx, const uint8_t *d_scalars, uint64_t n, uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (n == 0) return C25519_OK;
    int32_t r;
    if ((r = ctx_reserve(ctx, ctx->scratch, n * 128)) || (r = ctx_reserve(ctx, ctx->prefix, n * 48))) return r;
    stream_wipe wipe(ctx->stream);                        // secret-derived intermediates, on every exit path
    wipe.add(ctx->scratch.p, n * 128); wipe.add(ctx->prefix.p, n * 48);
    hipEvent_t *ring = ctx_ring_item(ctx);
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    HIPCHK(hipEventRecord(ring[0], ctx->stream));
    if (ctx_secret_default(ctx)) HIPCHK(launch_mul_base_ct(d_scalars, n, ctx->d_table_ct, (uint32_t *)ctx->scratch.p, nullptr, ctx->num_cus, ctx->stream));
    else HIPCHK(launch_mul_base(ctx->w, d_scalars, n, ctx->d_table, (uint32_t *)ctx->scratch.p, nullptr, ctx->num_cus, ctx->stream));
    HIPCHK(hipEventRecord(ring[1], ctx->stream));
    HIPCHK(launch_ratio_p32(1, (const uint32_t *)ctx->scratch.p, (uint32_t *)ctx->prefix.p, n, d_out, ctx->stream));   // (Z+Y)/(Z-Y)
    HIPCHK(hipEventRecord(ring[2], ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}
EXPORT int32_t c25519_montgomery_to_edwards_batch_dev(c25519_ctx *ctx, const uint8_t *d_u, const uint8_t *d_signs, uint64_t n, int out_fmt, uint8_t *d_out,
                                                      uint8_t *d_status) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ed_fmt_ok(out_fmt)) return bad_arg(ctx, "montgomery_to_edwards: out_fmt must be 0 or 2");
    if (n == 0) return C25519_OK;
    // y through the batched division of k_ratio_p32 (one inversion per 16 items): 0.98 ms at 2^20 against 1.52 ms with one fe_invert per lane,
    // which stays as the A/B arm (knob 0, tuning build only; DESIGN.md §3.10, profiles/montgomery_numbers.txt)
    static const bool batched = C25519_KNOB("MONT_TO_EDWARDS_BATCHED", 1) != 0;
    const uint8_t *ybuf = nullptr;
    if (batched) {
        int32_t r;
        if ((r = ctx_reserve(ctx, ctx->scratch, n * 128)) || (r = ctx_reserve(ctx, ctx->prefix, n * 48)) || (r = ctx_reserve(ctx, ctx->tmp_e, n * 32))) return r;
    }
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    if (batched) {
        hipLaunchKernelGGL(k_mont_to_edwards_prep, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_u, n, (uint32_t *)ctx->scratch.p);
        HIPCHK(hipGetLastError());
        HIPCHK(launch_ratio_p32(0, (const uint32_t *)ctx->scratch.p, (uint32_t *)ctx->prefix.p, n, (uint8_t *)ctx->tmp_e.p, ctx->stream));
        ybuf = (const uint8_t *)ctx->tmp_e.p;
    }
#define C25519_TE(OUT, B) hipLaunchKernelGGL((k_mont_to_edwards<OUT, B>), dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_u, d_signs, ybuf, n, d_out, d_status)
    if (out_fmt == C25519_FMT_EDWARDS_Y) { if (batched) C25519_TE(TE_Y, true); else C25519_TE(TE_Y, false); }
    else { if (batched) C25519_TE(TE_RAW, true); else C25519_TE(TE_RAW, false); }
#undef C25519_TE
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}

// ---- host twins: chunked through the copy streams (ffi.h) ----------------------------------------------------------------------
EXPORT int32_t c25519_montgomery_mul_batch(c25519_ctx *ctx, const uint8_t *k, const uint8_t *u, uint64_t n, uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (n == 0) return C25519_OK;
    return ffi_twin(ctx, n, 1u << 17, {{k, 32, FFI_TMP_A, 0, true}, {u, 32, FFI_TMP_B}}, {{out, 32, FFI_TMP_C, 0, true}},      /* the products are shared secrets: wiped like the scalars */
                    [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) { return c25519_montgomery_mul_batch_dev(ctx, d_in[0], d_in[1], m, d_out[0]); });
}
EXPORT int32_t c25519_montgomery_mul_bits_be_batch(c25519_ctx *ctx, const uint8_t *bits, uint32_t nbits, const uint8_t *u, uint64_t n, uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (nbits > C25519_MONTGOMERY_MAX_BITS) return bad_arg(ctx, "montgomery_mul_bits_be: nbits must be at most 512");
    if (n == 0) return C25519_OK;
    const size_t nb = (nbits + 7) / 8;
    // the staged bits are wiped; with nbits = 0 there is nothing to copy
    return ffi_twin(ctx, n, 1u << 17, {{u, 32, FFI_TMP_B}, {nb ? bits : nullptr, nb, FFI_TMP_A, 16, true}}, {{out, 32, FFI_TMP_C, 0, true}},
                    [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) { return c25519_montgomery_mul_bits_be_batch_dev(ctx, d_in[1], nbits, d_in[0], m, d_out[0]); });
}
EXPORT int32_t c25519_montgomery_mul_base_batch(c25519_ctx *ctx, const uint8_t *scalars, uint64_t n, uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (n == 0) return C25519_OK;
    return ffi_twin(ctx, n, 1u << 18, {{scalars, 32, FFI_TMP_A, 0, true}}, {{out, 32, FFI_TMP_B}},
                    [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) { return c25519_montgomery_mul_base_batch_dev(ctx, d_in[0], m, d_out[0]); });
}
EXPORT int32_t c25519_montgomery_to_edwards_batch(c25519_ctx *ctx, const uint8_t *u, const uint8_t *signs, uint64_t n, int out_fmt, uint8_t *out, uint8_t *status) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ed_fmt_ok(out_fmt)) return bad_arg(ctx, "montgomery_to_edwards: out_fmt must be 0 or 2");
    if (n == 0) return C25519_OK;
    // tmp_c: the n sign bytes, then the n status bytes
    return ffi_twin(ctx, n, 1u << 17, {{u, 32, FFI_TMP_A}, {signs, 1, FFI_TMP_C}}, {{out, point_bytes(out_fmt), FFI_TMP_B}, {status, 1, FFI_TMP_C}},
                    [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) { return c25519_montgomery_to_edwards_batch_dev(ctx, d_in[0], d_in[1], m, out_fmt, d_out[0], d_out[1]); });
}
