// Batched hash-to-group (csrc/h2c.h has the arithmetic), one item per lane:
//
//   c25519_ristretto_from_uniform_bytes_batch   RistrettoPoint::from_uniform_bytes (ristretto.rs:774)
//   c25519_ristretto_map_to_curve_batch         RistrettoPoint::map_to_curve (ristretto/elligator.rs:62-68)
//   c25519_ristretto_hash_from_bytes_batch      RistrettoPoint::hash_from_bytes::<Sha512> (ristretto.rs:736-761)
//   c25519_edwards_hash_to_curve_batch          EdwardsPoint::hash_to_curve / encode_to_curve::<Sha512> (edwards.rs:710-750)
//
// The map kernels read no message: they are constant-time in their inputs (selects only; tests/test_ct_isa_h2c.py asserts
// it on the compiled code).  The hashing kernels branch on message lengths, which are public.
#include <hip/hip_runtime.h>
#include <string.h>
#include "../../include/c25519_hip.h"
#include "devio.h"
#include "h2c.h"
#include "kernels.h"
#include "ctx.h"
#include "ffi.h"
#include "capi_util.h"

using namespace c25519;

namespace c25519 {

// output writers: 0 CompressedRistretto (32 B), 1 raw EdwardsPoint (160 B), 2 P32 record for the batched Edwards compression (k_compress_p32)
enum { H2C_OUT_RIS = 0, H2C_OUT_RAW = 1, H2C_OUT_P32 = 2 };
template <int OUT>
__device__ __forceinline__ void h2c_write(uint8_t *out, u64 i, const ge_p3 &P) {
    if (OUT == H2C_OUT_RIS) { u32 w[8]; ris_compress(P, w); store8(out, i, w); }
    else if (OUT == H2C_OUT_RAW) raw160_store(out, i, P);
    else p32_store(reinterpret_cast<u32 *>(out), i, P.X, P.Y, P.Z);
}

// 64 uniform bytes -> two maps, the sum
template <int OUT>
__global__ void __launch_bounds__(256) k_ristretto_from_uniform(const uint8_t *__restrict__ in64, u64 n, uint8_t *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 a[8], b[8];
    load8(in64, 2 * i, a);
    load8(in64, 2 * i + 1, b);
    h2c_write<OUT>(out, i, ge_add(ris_map_words(a), ris_map_words(b)));
}
// 32 bytes -> one map
template <int OUT>
__global__ void __launch_bounds__(256) k_ristretto_map(const uint8_t *__restrict__ in32, u64 n, uint8_t *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 a[8];
    load8(in32, i, a);
    h2c_write<OUT>(out, i, ris_map_words(a));
}
// SHA-512(message i) -> from_uniform_bytes.  flags[1] |= 1 if the offsets are not monotone or run past msgs_len (as k_hram: that
// message is hashed as empty, nothing outside [msgs, msgs + msgs_len) is read)
template <int OUT>
__global__ void __launch_bounds__(256) k_ristretto_hash(const uint8_t *__restrict__ msgs, const u64 *__restrict__ msg_off, u64 msgs_len, u64 n,
                                                        u32 *__restrict__ flags, uint8_t *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 o0 = msg_off[i], o1 = msg_off[i + 1];
    const bool okoff = o0 <= o1 && o1 <= msgs_len;
    if (!okoff) atomicOr(&flags[1], 1u);
    sha512_stream st;
    st.init();
    st.put_bytes(msgs + (okoff ? o0 : 0), okoff ? o1 - o0 : 0);
    st.finish();
    u32 w[16];
    sha512_digest_words(st.h, w);
    h2c_write<OUT>(out, i, ge_add(ris_map_words(w), ris_map_words(w + 8)));
}
// RFC 9380 edwards25519_XMD:SHA-512_ELL2_RO_ (RO) / _NU_: expand_message_xmd with one DST for the batch (device memory, like k_hram_dom's dom2),
// one or two maps, the sum for RO, x8
template <bool RO, int OUT>
__global__ void __launch_bounds__(256) k_edwards_h2c(const uint8_t *__restrict__ msgs, const u64 *__restrict__ msg_off, u64 msgs_len, const uint8_t *__restrict__ dst,
                                                     u32 dst_len, u64 n, u32 *__restrict__ flags, uint8_t *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 o0 = msg_off[i], o1 = msg_off[i + 1];
    const bool okoff = o0 <= o1 && o1 <= msgs_len;
    if (!okoff) atomicOr(&flags[1], 1u);
    h2c_write<OUT>(out, i, ed_hash_to_curve(msgs + (okoff ? o0 : 0), okoff ? o1 - o0 : 0, dst, dst_len, RO));
}

}  // namespace c25519

// bad offsets flagged by a hashing kernel -> error, like verify_batch / sign_batch.  Synchronises the context's stream.
static int32_t h2c_offsets_verdict(c25519_ctx *ctx, const char *what) {
    uint32_t fl[4] = {0, 0, 0, 0};
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(fl, ctx->d_flag, 16, hipMemcpyDeviceToHost));
    if (fl[1]) return bad_arg(ctx, what);
    return C25519_OK;
}

// ---- Ristretto from_uniform_bytes / map_to_curve ---------------------------------------------------------------------------
EXPORT int32_t c25519_ristretto_from_uniform_bytes_batch_dev(c25519_ctx *ctx, const uint8_t *d_in64, uint64_t n, int out_fmt, uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(out_fmt)) return bad_arg(ctx, "ristretto_from_uniform_bytes: out_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    if (out_fmt == C25519_FMT_RISTRETTO) hipLaunchKernelGGL(k_ristretto_from_uniform<H2C_OUT_RIS>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_in64, n, d_out);
    else hipLaunchKernelGGL(k_ristretto_from_uniform<H2C_OUT_RAW>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_in64, n, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}
EXPORT int32_t c25519_ristretto_map_to_curve_batch_dev(c25519_ctx *ctx, const uint8_t *d_in32, uint64_t n, int out_fmt, uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(out_fmt)) return bad_arg(ctx, "ristretto_map_to_curve: out_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    if (out_fmt == C25519_FMT_RISTRETTO) hipLaunchKernelGGL(k_ristretto_map<H2C_OUT_RIS>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_in32, n, d_out);
    else hipLaunchKernelGGL(k_ristretto_map<H2C_OUT_RAW>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_in32, n, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return C25519_OK;
}
// host twins: chunked through the copy streams (ffi.h)
static int32_t ris_fixed_host(c25519_ctx *ctx, const uint8_t *in, size_t in_bytes, uint64_t n, int out_fmt, uint8_t *out,
                              int32_t (*dev)(c25519_ctx *, const uint8_t *, uint64_t, int, uint8_t *), const char *what) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(out_fmt)) return bad_arg(ctx, what);
    if (n == 0) return C25519_OK;
    return ffi_twin(ctx, n, 1u << 16, {{in, in_bytes, FFI_TMP_A, 0, true}}, {{out, point_bytes(out_fmt), FFI_TMP_B, 0, true}},      /* the uniform bytes may be a secret (a blinded value): staged copies wiped */
                    [&](uint64_t m, uint8_t *const *d_in, uint8_t *const *d_out) { return dev(ctx, d_in[0], m, out_fmt, d_out[0]); });
}
EXPORT int32_t c25519_ristretto_from_uniform_bytes_batch(c25519_ctx *ctx, const uint8_t *in64, uint64_t n, int out_fmt, uint8_t *out) {
    return ris_fixed_host(ctx, in64, 64, n, out_fmt, out, c25519_ristretto_from_uniform_bytes_batch_dev, "ristretto_from_uniform_bytes: out_fmt must be 1 or 2");
}
EXPORT int32_t c25519_ristretto_map_to_curve_batch(c25519_ctx *ctx, const uint8_t *in32, uint64_t n, int out_fmt, uint8_t *out) {
    return ris_fixed_host(ctx, in32, 32, n, out_fmt, out, c25519_ristretto_map_to_curve_batch_dev, "ristretto_map_to_curve: out_fmt must be 1 or 2");
}

// ---- hashing entry points ------------------------------------------------------------------------------------------------------
EXPORT int32_t c25519_ristretto_hash_from_bytes_batch_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len, uint64_t n,
                                                          int out_fmt, uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(out_fmt)) return bad_arg(ctx, "ristretto_hash_from_bytes: out_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    HIPCHK(hipMemsetAsync(ctx->d_flag, 0, 16, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    uint32_t *fl = (uint32_t *)ctx->d_flag;
    if (out_fmt == C25519_FMT_RISTRETTO)
        hipLaunchKernelGGL(k_ristretto_hash<H2C_OUT_RIS>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_msgs, d_msg_off, msgs_len, n, fl, d_out);
    else hipLaunchKernelGGL(k_ristretto_hash<H2C_OUT_RAW>, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_msgs, d_msg_off, msgs_len, n, fl, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return h2c_offsets_verdict(ctx, "ristretto_hash_from_bytes: msg_off is not monotone or runs past msgs_len");
}

// DST (a HOST pointer, 1 .. 255 bytes) into the context's small device buffer; the host copy stays in the context until the next call
static int32_t dst_upload(c25519_ctx *ctx, const uint8_t *dst, uint32_t dst_len) {
    if (dst_len == 0 || dst_len > 255) { ctx->err = "hash_to_curve: the domain separator must have 1 .. 255 bytes"; return C25519_DOMAIN_SEPARATOR_LENGTH; }
    if (!dst) return bad_arg(ctx, "hash_to_curve: null domain separator");
    int32_t r;
    if ((r = ctx_reserve(ctx, ctx->dom, 512))) return r;
    ctx->h_dom.assign(dst, dst + dst_len);
    HIPCHK(hipMemcpyAsync(ctx->dom.p, ctx->h_dom.data(), dst_len, hipMemcpyHostToDevice, ctx->stream));
    return C25519_OK;
}
EXPORT int32_t c25519_edwards_hash_to_curve_batch_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len, uint64_t n,
                                                      const uint8_t *dst, uint32_t dst_len, int mode, int out_fmt, uint8_t *d_out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (dst_len == 0 || dst_len > 255) { ctx->err = "hash_to_curve: the domain separator must have 1 .. 255 bytes"; return C25519_DOMAIN_SEPARATOR_LENGTH; }
    if (mode != C25519_H2C_RO && mode != C25519_H2C_NU) return bad_arg(ctx, "hash_to_curve: mode must be C25519_H2C_RO or C25519_H2C_NU");
    if (!ed_fmt_ok(out_fmt)) return bad_arg(ctx, "hash_to_curve: out_fmt must be 0 or 2");
    if (n == 0) return C25519_OK;
    int32_t r;
    if ((r = dst_upload(ctx, dst, dst_len))) return r;
    const bool ro = mode == C25519_H2C_RO, raw = out_fmt == C25519_FMT_RAW160;
    uint8_t *dest = d_out;
    if (!raw) {
        if ((r = ctx_reserve(ctx, ctx->scratch, n * 128)) || (r = ctx_reserve(ctx, ctx->prefix, n * 48))) return r;
        dest = (uint8_t *)ctx->scratch.p;
    }
    HIPCHK(hipMemsetAsync(ctx->d_flag, 0, 16, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
    const uint8_t *d_dst = (const uint8_t *)ctx->dom.p;
    uint32_t *fl = (uint32_t *)ctx->d_flag;
#define H2C_LAUNCH(RO_, OUT_) hipLaunchKernelGGL((k_edwards_h2c<RO_, OUT_>), dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, d_msgs, d_msg_off, msgs_len, d_dst, dst_len, n, fl, dest)
    if (ro) { if (raw) H2C_LAUNCH(true, H2C_OUT_RAW); else H2C_LAUNCH(true, H2C_OUT_P32); }
    else { if (raw) H2C_LAUNCH(false, H2C_OUT_RAW); else H2C_LAUNCH(false, H2C_OUT_P32); }
#undef H2C_LAUNCH
    HIPCHK(hipGetLastError());
    // compressed output: one shared inversion per 16-point lane chunk (the finish of the fixed-base kernels) instead of one per item
    if (!raw) HIPCHK(launch_compress_p32((const uint32_t *)ctx->scratch.p, (uint32_t *)ctx->prefix.p, n, d_out, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
    return h2c_offsets_verdict(ctx, "hash_to_curve: msg_off is not monotone or runs past msgs_len");
}

// host twins: messages and offsets up as whole arrays, one chunk (the _dev form reads its offsets flag back)
template <class F>
static int32_t h2c_msgs_host(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, int out_fmt, uint8_t *out, const char *what, F &&dev) {
    const size_t ob = point_bytes(out_fmt);
    ffi_msgs mm;
    const int32_t r = ffi_upload_msgs(ctx, msgs, msg_off, n, what, n * ob, mm);
    if (r) return r;
    uint8_t *dout = (uint8_t *)ctx->tmp_c.p;
    const ffi_out o = {out, dout, ob};
    return ffi_pipeline(ctx, n, n, nullptr, 0, &o, 1, [&](uint64_t lo, uint64_t m) -> int32_t { return dev(mm.d_msgs, mm.d_off + lo, mm.mlen, m, dout + lo * ob); },
                        true, mm.up_bytes);
}
EXPORT int32_t c25519_ristretto_hash_from_bytes_batch(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, int out_fmt, uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ris_fmt_ok(out_fmt)) return bad_arg(ctx, "ristretto_hash_from_bytes: out_fmt must be 1 or 2");
    if (n == 0) return C25519_OK;
    return h2c_msgs_host(ctx, msgs, msg_off, n, out_fmt, out, "ristretto_hash_from_bytes: msg_off is not monotone",
                         [&](const uint8_t *dm, const uint64_t *doff, uint64_t mlen, uint64_t m, uint8_t *dout) {
                             return c25519_ristretto_hash_from_bytes_batch_dev(ctx, dm, doff, mlen, m, out_fmt, dout);
                         });
}
EXPORT int32_t c25519_edwards_hash_to_curve_batch(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, const uint8_t *dst, uint32_t dst_len,
                                                  int mode, int out_fmt, uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    if (dst_len == 0 || dst_len > 255) { ctx->err = "hash_to_curve: the domain separator must have 1 .. 255 bytes"; return C25519_DOMAIN_SEPARATOR_LENGTH; }
    if (mode != C25519_H2C_RO && mode != C25519_H2C_NU) return bad_arg(ctx, "hash_to_curve: mode must be C25519_H2C_RO or C25519_H2C_NU");
    if (!ed_fmt_ok(out_fmt)) return bad_arg(ctx, "hash_to_curve: out_fmt must be 0 or 2");
    if (n == 0) return C25519_OK;
    return h2c_msgs_host(ctx, msgs, msg_off, n, out_fmt, out, "hash_to_curve: msg_off is not monotone",
                         [&](const uint8_t *dm, const uint64_t *doff, uint64_t mlen, uint64_t m, uint8_t *dout) {
                             return c25519_edwards_hash_to_curve_batch_dev(ctx, dm, doff, mlen, m, dst, dst_len, mode, out_fmt, dout);
                         });
}
