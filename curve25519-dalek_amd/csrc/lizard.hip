// Batched Lizard encoding (csrc/lizard.h has the arithmetic), one item per lane:
//
//   c25519_ristretto_lizard_encode_sha256_batch    RistrettoPoint::lizard_encode::<Sha256> (lizard/lizard_ristretto.rs:25-42)
//   c25519_ristretto_lizard_decode_sha256_batch    RistrettoPoint::lizard_decode::<Sha256> (lizard/lizard_ristretto.rs:46-75)
//   c25519_ristretto_map_to_curve_inverse_batch    RistrettoPoint::map_to_curve_inverse (lizard/lizard_ristretto.rs:232-238)
//
// All three are constant-time in their inputs: selects only, the candidates visited by a uniform loop
// (tests/test_ct_isa_lizard.py asserts it on the compiled code).  Item i reads and writes its own slots only.
#include <hip/hip_runtime.h>
#include <string.h>
#include "../../include/c25519_hip.h"
#include "devio.h"
#include "lizard.h"
#include "ctx.h"
#include "ffi.h"
#include "capi_util.h"

using namespace c25519;

namespace c25519 {

enum { LZ_RIS = 0, LZ_RAW = 1 };   // point format of an input or output: CompressedRistretto (32 B) or raw EdwardsPoint (160 B)

template <int OUT>
__device__ __forceinline__ void lz_write(uint8_t *out, u64 i, const ge_p3 &P) {
    if (OUT == LZ_RIS) { u32 w[8]; ris_compress(P, w); store8(out, i, w); }
    else raw160_store(out, i, P);
}
// -> the point as given (RAW160) or as decompressed (Z = 1, the reference's decompress); ok = the encoding was canonical and valid
template <int IN>
__device__ __forceinline__ ge_p3 lz_read(const uint8_t *in, u64 i, bool &ok) {
    ge_p3 P;
    if (IN == LZ_RIS) { u32 w[8]; load8(in, i, w); ok = ris_decompress(P, w); }
    else { P = raw160_load(in, i); ok = true; }
    return P;
}

// 16 bytes -> lizard_encode::<Sha256>
template <int OUT>
__global__ void __launch_bounds__(256) k_lizard_encode(const uint8_t *__restrict__ in16, u64 n, uint8_t *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 q = reinterpret_cast<const uint4 *>(in16)[i];
    const u32 data[4] = {q.x, q.y, q.z, q.w};
    lz_write<OUT>(out, i, lizard_encode(data));
}
// point -> 16 bytes + status (C25519_LIZARD_*); the 16 bytes are zero unless the status is OK
template <int IN>
__global__ void __launch_bounds__(256) k_lizard_decode(const uint8_t *__restrict__ in, u64 n, uint8_t *__restrict__ out16, uint8_t *__restrict__ status) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok;
    const ge_p3 P = lz_read<IN>(in, i, ok);
    u32 pay[4];
    const u32 n_found = lizard_decode(P, pay);
    const bool good = ok & (n_found == 1u);
    const lanemask m = lane_mask(good);
    for (int q = 0; q < 4; q++) pay[q] = sel_u32(0u, pay[q], m);
    reinterpret_cast<uint4 *>(out16)[i] = make_uint4(pay[0], pay[1], pay[2], pay[3]);
    status[i] = (uint8_t)sel_u32(sel_u32((u32)C25519_LIZARD_NONE, (u32)C25519_LIZARD_OK, m), (u32)C25519_LIZARD_BAD_ENCODING, lane_mask(!ok));
}
// point -> 16 x 32 bytes (slot c at out512 + 512 i + 32 c; an undefined slot is zero), mask bit c = slot c defined,
// ok[i] = the encoding was valid (compressed input only)
template <int IN>
__global__ void __launch_bounds__(256) k_map_to_curve_inverse(const uint8_t *__restrict__ in, u64 n, uint8_t *__restrict__ out512, uint16_t *__restrict__ mask,
                                                              uint8_t *__restrict__ okb) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok;
    const ge_p3 P = lz_read<IN>(in, i, ok);
    const jacobi4 J = ris_to_jacobi_quartic(P);
    u32 bits = 0;
#pragma unroll 1
    for (int c = 0; c < 8; c++) {
        feT x;
        const bool defined = lizard_candidate(J, c, x);
        const lanemask m = lane_mask(defined);
        u32 w[8], wn[8];
        fe_to_words(x, w);
        fe_to_words(fe_neg(x), wn);
        for (int q = 0; q < 8; q++) { w[q] = sel_u32(0u, w[q], m); wn[q] = sel_u32(0u, wn[q], m); }
        store8(out512, 16 * i + c, w);
        store8(out512, 16 * i + 8 + c, wn);
        bits |= sel_u32(0u, 0x101u << c, m);
    }
    mask[i] = (uint16_t)bits;
    if (IN == LZ_RIS) okb[i] = ok ? 1 : 0;
}

}  // namespace c25519

// ---- _dev forms --------------------------------------------------------------------------------------------------------------
EXPORT int32_t c25519_ristretto_lizard_encode_sha256_batch_dev(c25519_ctx *ctx, const uint8_t *d_data16, uint64_t n, int out_fmt, uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(out_fmt)) return bad_arg(ctx, "ristretto_lizard_encode: out_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    if (out_fmt == C25519_FMT_RISTRETTO) hipLaunchKernelGGL(k_lizard_encode<LZ_RIS>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_data16, n, d_out);
    else hipLaunchKernelGGL(k_lizard_encode<LZ_RAW>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_data16, n, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}
EXPORT int32_t c25519_ristretto_lizard_decode_sha256_batch_dev(c25519_ctx *ctx, const uint8_t *d_in, uint64_t n, int in_fmt, uint8_t *d_out16, uint8_t *d_status) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(in_fmt)) return bad_arg(ctx, "ristretto_lizard_decode: in_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    if (in_fmt == C25519_FMT_RISTRETTO) hipLaunchKernelGGL(k_lizard_decode<LZ_RIS>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_in, n, d_out16, d_status);
    else hipLaunchKernelGGL(k_lizard_decode<LZ_RAW>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_in, n, d_out16, d_status);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}
EXPORT int32_t c25519_ristretto_map_to_curve_inverse_batch_dev(c25519_ctx *ctx, const uint8_t *d_in, uint64_t n, int in_fmt, uint8_t *d_out512, uint16_t *d_mask,
                                                               uint8_t *d_ok) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(in_fmt)) return bad_arg(ctx, "ristretto_map_to_curve_inverse: in_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    if (in_fmt == C25519_FMT_RISTRETTO && !d_ok) return bad_arg(ctx, "ristretto_map_to_curve_inverse: d_ok may be NULL for RAW160 input only");
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    if (in_fmt == C25519_FMT_RISTRETTO)
        hipLaunchKernelGGL(k_map_to_curve_inverse<LZ_RIS>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_in, n, d_out512, d_mask, d_ok);
    else hipLaunchKernelGGL(k_map_to_curve_inverse<LZ_RAW>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_in, n, d_out512, d_mask, d_ok);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}

// ---- host twins: chunked through the copy streams (ffi.h) ----------------------------------------------------------------------
EXPORT int32_t c25519_ristretto_lizard_encode_sha256_batch(c25519_ctx *ctx, const uint8_t *data16, uint64_t n, int out_fmt, uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(out_fmt)) return bad_arg(ctx, "ristretto_lizard_encode: out_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    return ffi_twin(ctx, n, 1u << 16, {{data16, 16, FFI_TMP_A, 0, true}}, {{out, point_bytes(out_fmt), FFI_TMP_B, 0, true}},      /* the payload and the point that carries it: wiped */
                    [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) { return c25519_ristretto_lizard_encode_sha256_batch_dev(ctx, d_in[0], m, out_fmt, d_out[0]); });
}
EXPORT int32_t c25519_ristretto_lizard_decode_sha256_batch(c25519_ctx *ctx, const uint8_t *in, uint64_t n, int in_fmt, uint8_t *out16, uint8_t *status) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(in_fmt)) return bad_arg(ctx, "ristretto_lizard_decode: in_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    return ffi_twin(ctx, n, 1u << 16, {{in, point_bytes(in_fmt), FFI_TMP_A, 0, true}}, {{out16, 16, FFI_TMP_B, 0, true}, {status, 1, FFI_TMP_C}},
                    [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) { return c25519_ristretto_lizard_decode_sha256_batch_dev(ctx, d_in[0], m, in_fmt, d_out[0], d_out[1]); });
}
EXPORT int32_t c25519_ristretto_map_to_curve_inverse_batch(c25519_ctx *ctx, const uint8_t *in, uint64_t n, int in_fmt, uint8_t *out512, uint16_t *mask,
                                                           uint8_t *ok) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(in_fmt)) return bad_arg(ctx, "ristretto_map_to_curve_inverse: in_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    if (in_fmt == C25519_FMT_RISTRETTO && !ok) return bad_arg(ctx, "ristretto_map_to_curve_inverse: ok may be NULL for RAW160 input only");
    const bool want_ok = ok != nullptr && in_fmt == C25519_FMT_RISTRETTO;
    // tmp_c: the n uint16 masks, then the n validity bytes (staged, not copied back, when unused)
    return ffi_twin(ctx, n, 1u << 14, {{in, point_bytes(in_fmt), FFI_TMP_A}}, {{out512, 512, FFI_TMP_B}, {mask, 2, FFI_TMP_C}, {want_ok ? ok : nullptr, 1, FFI_TMP_C}},
                    [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) {
                        return c25519_ristretto_map_to_curve_inverse_batch_dev(ctx, d_in[0], m, in_fmt, d_out[0], (uint16_t *)d_out[1], want_ok ? d_out[2] : nullptr);
                    });
}
