/* c25519_hip.h -- C ABI of libc25519hip.so, the MI355X (gfx950) batched Curve25519 engine.
 *
 * Drop-in boundary for the hot path of dalek-cryptography/curve25519-dalek.  The
 * reference has no FFI; the seam these entry points serve is its internal backend switch
 * (curve25519-dalek/src/backend.rs:45-277) plus the three callers that bypass it
 * (edwards.rs:1192 mul_base, montgomery.rs:183 mul_bits_be, ed25519-dalek/src/batch.rs:146
 * verify_batch).  INTEGRATION.md shows the Rust `extern "C"` block and the BackendKind::Hip arm a
 * maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes; all buffers caller-owned, contiguous, little-endian; nothing is
 *     retained after return.
 *   - `_dev` entry points take DEVICE pointers (HBM) and enqueue on the context's HIP stream;
 *     those that return a verdict/point to the host synchronise that stream.  The un-suffixed
 *     twins take HOST pointers and move the data themselves: the batch is cut into chunks (passes), and chunk c+1 travels up
 *     on a copy stream while chunk c computes and chunk c-1 travels down, so a call costs about max(link, kernels), not
 *     their sum.  Any host memory works; pageable memory whose pages have been touched moves at the link rate on this
 *     platform, but an OUTPUT buffer that has never been written (a fresh allocation) pays first-touch page faults at
 *     ~5 GB/s: reuse output buffers, or take them from c25519_host_alloc.
 *   - return value: int32 status.  0 OK; 1 NONE (a point failed to decompress: the Rust side maps
 *     it to Option::None); 2 SCALAR_FORMAT; 3 VERIFY; 4 ARRAY_LENGTH (mirrors
 *     ed25519-dalek/src/errors.rs:21-42 InternalError); negative = -(hipError_t) runtime failure.
 *   - point formats (`fmt`): 0 = 32-byte CompressedEdwardsY (edwards.rs:175),
 *     1 = 32-byte CompressedRistretto (ristretto.rs:223),
 *     2 = 160-byte raw EdwardsPoint {X,Y,Z,T} x 5 x u64 radix-2^51 limbs (u64/field.rs:43-52).  The reference keeps
 *         limbs below 2^52 (its debug_assert!s, field.rs:162-166); INPUT limbs here may be ANY u64 values -- the
 *         element read is sum_i l_i 2^(51 i) mod p exactly (no truncation, no status: there is no limb pattern without a
 *         meaning), so unreduced sums are accepted as what they denote; OUTPUT limbs are canonical (< 2^51, value < p).
 *         (edwards.rs:390-395 is not repr(C); the Rust shim copies limb-by-limb into this layout).
 *   - scalars: 32 bytes little-endian, < 2^255 (Scalar invariant #1, scalar.rs:197-205); they need
 *     NOT be reduced mod l for point multiplication (clamped integers are legal).
 *   - device buffers of 32-, 64- and 160-byte items must be 16-byte aligned (hipMalloc / torch
 *     allocations are); message blobs may have any alignment.
 *   - a context is bound to one GPU and one stream; calls on one context must not overlap.
 *     Results never depend on which GPU ran them.
 */
#ifndef C25519_HIP_H
#define C25519_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C25519_OK 0
#define C25519_NONE 1
#define C25519_SCALAR_FORMAT 2
#define C25519_VERIFY 3
#define C25519_ARRAY_LENGTH 4
#define C25519_PREHASHED_CONTEXT_LENGTH 5   /* Ed25519ph: context longer than 255 octets (errors.rs InternalError::PrehashedContextLength) */
#define C25519_DOMAIN_SEPARATOR_LENGTH 6    /* hash-to-curve: a DST of 0 or more than 255 bytes (the reference panics, field.rs:457-462) */

#define C25519_FMT_EDWARDS_Y 0
#define C25519_FMT_RISTRETTO 1
#define C25519_FMT_RAW160 2

/* ed25519_verify_batch z_mode: how the 128-bit batch coefficients z_i are derived.
 * C25519_Z_TRANSCRIPT (0, the default of every host-language wrapper): byte for byte the reference's derivation --
 *   ONE Merlin/STROBE-128 transcript over the whole batch (batch.rs:168-222, batch/transcript.rs), whatever n is and
 *   however many passes, contexts (ed25519_verify_batch_multi) or ranks (multi.verify_batch_sharded) share the batch, and
 *   ONE equation over the whole batch (batch.rs:235-250: the partial sums of passes / contexts / ranks are added).  It is
 *   a sequential sponge (about 1.7 Keccak-f per signature), so it runs on one host core and bounds the call near
 *   2-3 x 10^6 signatures/s; the curve arithmetic still runs on the GPU.
 * C25519_Z_DEVICE (1, explicit opt-in, NOT the reference's derivation and not a reviewed standard construction):
 *   z_i = a 16-byte quarter of BLAKE2b-512(root || LE64(i / 4)), read as sign-magnitude (uniform on the 2^128 - 1 integers
 *   -(2^127 - 1) .. 2^127 - 1), where root is the root of a hash tree over what the reference's transcript
 *   absorbs: H(R_i || A_i || M_i) -- SHA-512 as in Ed25519, taken mod l, 32 bytes: the batch equation only sees that residue
 *   (batch.rs:213-217) -- and the 32-byte s_i of every signature.  Every node is a plain unkeyed BLAKE2b-256 digest (RFC 7693):
 *   node = BLAKE2b-256(TAG || data), TAG = one 128-byte block: the string "c25519-hip/verify_batch/z-tree/v5", zero bytes, then
 *   level, number of inputs of the level and batch size as little-endian u64 (bytes 104 .. 127); level 0: data = (h_i mod l) || s_i of
 *   4 signatures (256 bytes, absent signatures = zero bytes); upper levels: data = 4 child nodes (128 bytes, absent = zero bytes).
 *   (Rounds 2-5 built the same tree from SHA-512's compression function, tag .../v4; the values differ.  BLAKE2b because the tree's
 *   levels are a chain of dependent compressions that one wavefront per SIMD executes, and BLAKE2b's is 12 rounds against 80:
 *   csrc/blake2b.h.)  tests/pyref.py device_zs restates the derivation with hashlib.blake2b.  Every z_i depends on every bit of the batch;
 *   honest batches give the same verdict in both modes; a batch containing an invalid signature passes with
 *   probability <= 2^-127.99 (reference: 2^-128) under the usual assumption that BLAKE2b (and SHA-512 in h_i) is
 *   collision resistant and its output unpredictable.  BINDING MARGIN of the tree leaves (since v4): the z_i bind (R_i, A_i, M_i) only
 *   through h_i mod l, a 252-bit value, where the reference's transcript absorbs the full 64-byte hash (batch.rs:191-199).  Two
 *   different (R, A, M) triples with equal h mod l would produce identical z_i for two different batch equations; finding such a pair
 *   is a birthday search on 252 bits, about 2^126 hash evaluations -- near, not at, the 128-bit level of the rest of the construction
 *   (the same order as the cross-pass birthday bound this library refuses elsewhere by checking sub-batches independently).  Callers
 *   that need the reference's full margin use C25519_Z_TRANSCRIPT.  Batches beyond ~1.5 x 2^20 signatures are checked as
 *   independent sub-batches (own tree, own z_i, own identity check).  The z_i VALUES differ from the reference's. */
#define C25519_Z_TRANSCRIPT 0
#define C25519_Z_DEVICE 1

/* c25519_ctx_create flags, bit 8: VARTIME_TABLES.  By default every entry point that replaces a CONSTANT-TIME function
 * of the reference -- mul_base (edwards.rs:918, :1192-1209), `&EdwardsPoint * &Scalar` (variable_base.rs), sign / keygen,
 * X25519 public keys -- gives what the reference's LookupTable::select gives (window.rs:54-76): no memory ADDRESS and no
 * BRANCH depends on the scalar.
 *   variable base: the 8-entry table of variable_base.rs, every entry read and the wanted one kept by selects.
 *   fixed base (round 5): radix-2^5 tables in LDS, 52 additions, and the digit never reaches an address at all -- lane j of each
 *   32-lane half of a wave reads the table entry of the signed digit value j - 16 (an address made of its LANE INDEX), and every
 *   lane then pulls the entry of ITS digit out of the registers of lane (half base + digit + 16) with ds_bpermute_b32, a
 *   register-to-register transfer through the LDS crossbar that reads no memory.  The digit is the permute's lane selector and
 *   nothing else; the sign is part of the selector (no conditional negation).  MEASURED before it was adopted
 *   (profiles/r05_instruction_rates.txt, c25519_microbench 50-67): throughput and latency of the permute are the same for
 *   identity, all-equal, random-within-the-half, pairs 32 lanes apart and two-source selector patterns (24.2 - 24.4 cycles per
 *   wave-instruction, 71 - 73 cycles of latency); a selector pattern that crosses the two halves at random is 16 % slower --
 *   which is why a lane's sources stay inside its own 32-lane half BY CONSTRUCTION (radix 2^6 over the whole wave was not
 *   built).  Round 6 added the many-to-one patterns -- groups of 2, 4, 8, 16, 32 lanes of a half pulling ONE source lane, what equal
 *   digits in neighbouring lanes make of the selector (c25519_microbench 80-89, profiles/r06_instruction_rates.txt).  This timing
 *   independence is a MEASURED property of gfx950 (the kernels are built for nothing else), not an architectural guarantee: a port to
 *   another GPU must repeat the probe, or use the full-window scan.  Asserted on the compiled code: tests/test_ct_isa.py (exactly 6 + 3 LDS reads and 30 permutes per window, no other
 *   memory access, no exec / vcc branch in the window loop).  The full-window scan of rounds 2-4 remains as k_mul_base<5, CT>
 *   behind the CT_FETCH knob of the tuning build (2.77 against 1.84 ms per 2^20 scalars).
 * With this flag those entry points use the fast tables instead -- fixed base: the radix-2^16 tables in HBM, 16
 * additions, 4x faster -- whose ADDRESSES depend on the scalar: set it only when every scalar handed to this context
 * is public (or call the *_vartime entry points).  The X25519 ladder is constant-time in either mode; MSM /
 * verify_batch / double_base are variable-time by definition, as in the reference. */
#define C25519_FLAG_VARTIME_TABLES 0x100u

typedef struct c25519_ctx c25519_ctx;

/* Create a context on HIP device `device` (>= 0).  Builds the fixed-base table and uploads it:
 * flags & 0x1f selects the fixed-base algorithm (results are identical):
 * 4, 5 or 6: one radix-2^w window table per digit position, the structure of the reference's
 * EdwardsBasepointTable (edwards.rs:1131-1141, :1246-1282) sized for the 160 KiB LDS;
 * 9: signed 9-tooth x 6-table comb in LDS (31 additions + 4 doublings per scalar, 147 KB);
 * 10 .. 20: the EdwardsBasepointTable structure with radix 2^w and the table in HBM, served by L2 / MALL:
 * ceil(256/w) additions with one 128-byte gather each, no doublings (table 1.7 MB at w = 10, 71 MB at w = 16);
 * 0 (default) = 16.  The table is computed on the device when the context is created.
 * flags & C25519_FLAG_VARTIME_TABLES: see above.  Returns NULL if there is no usable GPU: there is NO CPU fallback. */
c25519_ctx *c25519_ctx_create(int device, uint32_t flags);
void c25519_ctx_destroy(c25519_ctx *ctx);
/* Use an existing hipStream_t (e.g. PyTorch's current stream) instead of the context's own. */
int32_t c25519_ctx_set_stream(c25519_ctx *ctx, void *hip_stream);
/* Block until everything enqueued on the context's stream has finished. */
int32_t c25519_ctx_synchronize(c25519_ctx *ctx);
const char *c25519_last_error(const c25519_ctx *ctx);
/* Page-locked host memory (hipHostMalloc) for input / output buffers of the host-pointer entry points: DMA-able as is, never
 * pays a first-touch fault.  c25519_last_ffi_ms: wall-clock milliseconds of the most recent host-pointer call of this
 * context and the bytes it moved each way (either pointer may be NULL); -1 before the first such call. */
void *c25519_host_alloc(size_t bytes);
void c25519_host_free(void *p);
double c25519_last_ffi_ms(const c25519_ctx *ctx, uint64_t *h2d_bytes, uint64_t *d2h_bytes);
/* Release the workspaces earlier calls left allocated (a 2^24-term MSM keeps ~2.6 GB: gather records prepared ahead, the
 * normaliser's prefix products, staging copies of host-pointer calls).  Synchronises the context; the next call
 * re-allocates what it needs.  For long-lived contexts that see an occasional very large call. */
int32_t c25519_ctx_trim(c25519_ctx *ctx);
/* name of the kernel that c25519_phase_ms phase 0 (which = 0) / phase 3 (which = 1) of the latest entry point timed */
const char *c25519_last_kernel_name(const c25519_ctx *ctx, int which);
/* milliseconds the device spent in the most recent entry point's kernels (hipEvent pair on the
 * context's stream); valid after the call returned / the stream was synchronised. */
float c25519_last_kernel_ms(c25519_ctx *ctx);
/* Host clock of the phases of the latest synchronous MSM / verify_batch call on this context, microseconds since the call was entered:
 * out4[0] inputs staged and their upload enqueued (0 for the device-pointer forms), [1] every kernel enqueued, [2] results on the host (the last
 * kernel writes them into page-locked host memory and the host polls a sequence word: no copy engine, no interrupt), [3] folded and encoded. */
int32_t c25519_last_call_host_us(const c25519_ctx *ctx, double *out4);
/* Event counters of a context since its creation (diagnostics; tools/soak_small.py logs them).  Small and mid-size MSM / verify_batch calls (single passes up to 2^18 terms:
 * vartime_multiscalar_mul at the sizes of benches/dalek_benchmarks.rs:16, verify_batch of ed25519-dalek/benches/ed25519_benchmarks.rs:53) end with their last
 * kernel writing the record into page-locked host memory and the host polling a sequence word.  which = 0: calls whose record had not arrived after 2 ms of polling --
 * the host then blocked on the stream (a busy stream, a shared GPU); 1: calls whose record never arrived although the stream drained without error -- each was re-run
 * through the slot + copy path and returned its normal status (none observed: profiles/r06_soak_small.txt); 2: directly published calls.  Like
 * ed25519-dalek/src/batch.rs:146-251, a call returns or errs; it never waits on wall-clock alone. */
uint64_t c25519_ctx_counter(const c25519_ctx *ctx, int32_t which);

/* Per-call phase timing from a ring of hipEvents recorded on the launch streams (the last 64 calls of this context):
 * phase 0 = the dominant kernel of the call made `back` calls ago (0 = most recent) -- k_mul_base_*, k_x25519,
 * k_var_base, or k_accumulate for an MSM / verify_batch pass; phase 1 = the kernels after it (batched compression;
 * bucket reduction); for MSM / verify_batch passes also phase 2 = the whole pass and phase 3 = the decompression of
 * R_i (verify_batch).  Synchronises that call's last event.  Returns -1 if unavailable. */
float c25519_phase_ms(c25519_ctx *ctx, uint32_t back, int phase);
/* The same, summed over every pass of the most recent c25519_msm_* / ed25519_verify_batch* call (large inputs run as
 * several passes that alternate between two stream sets); *passes (may be NULL) receives the number of passes. */
float c25519_last_call_phase_ms(c25519_ctx *ctx, int phase, uint32_t *passes);

/* ---- fixed base: out[i] = scalars[i] * B ------------------------------------------------------
 * replaces EdwardsBasepointTable::mul_base / EdwardsPoint::mul_base (edwards.rs:918, :1192-1209),
 * followed by compress (edwards.rs:615 / :634 batch) when out_fmt is 0 or 1.
 * scalars: n x 32;  out: n x 32 (fmt 0/1) or n x 160 (fmt 2). */
int32_t c25519_mul_base_batch_dev(c25519_ctx *ctx, const uint8_t *d_scalars, uint64_t n, int out_fmt, uint8_t *d_out);
int32_t c25519_mul_base_batch(c25519_ctx *ctx, const uint8_t *scalars, uint64_t n, int out_fmt, uint8_t *out);
/* the same for scalars the caller declares PUBLIC: always the context's fast tables (variable-time table access). */
int32_t c25519_mul_base_batch_vartime_dev(c25519_ctx *ctx, const uint8_t *d_scalars, uint64_t n, int out_fmt, uint8_t *d_out);

/* EdwardsPoint::mul_base_clamped (edwards.rs:948-956): out[i] = clamp_integer(bytes[i]) * B -- the clamped integer is NOT
 * reduced mod l (scalar.rs:1407; legal for point multiplication, scalar.rs:197-222).  Secrets: constant-time tables unless the
 * context was created with C25519_FLAG_VARTIME_TABLES; the clamped copies are wiped. */
int32_t c25519_mul_base_clamped_batch_dev(c25519_ctx *ctx, const uint8_t *d_bytes, uint64_t n, int out_fmt, uint8_t *d_out);
int32_t c25519_mul_base_clamped_batch(c25519_ctx *ctx, const uint8_t *bytes, uint64_t n, int out_fmt, uint8_t *out);

/* ---- constant-time fixed-base tables for a CALLER'S point -----------------------------------------------------------------
 * replaces EdwardsBasepointTable::create(&P) (edwards.rs:1131-1141, generic over the basepoint; radices :1246-1292) and
 * RistrettoBasepointTable::create (ristretto.rs:1080-1110), then `&scalar * &table` = mul_base on that table
 * (edwards.rs:1192-1209).  create: point = 32 bytes (fmt 0 / 1) or 160 bytes (fmt 2), HOST pointer; the table (radix 2^5:
 * 52 windows x 17 affine Niels entries, the layout of the context's own constant-time table) is built once and stays in device
 * memory.  mul_table: out[i] = scalars[i] * P, ALWAYS with the constant-time lookup of the default fixed-base kernel (no address and
 * no branch depends on the scalar: see C25519_FLAG_VARTIME_TABLES above), whatever the context's flags -- these tables exist for secret scalars: Pedersen commitments
 * a*G + b*H, ElGamal / DH keys on a fixed generator.  out_fmt 0 / 1 / 2; fmt 1 gives RistrettoBasepointTable's result. */
typedef struct c25519_basetable c25519_basetable;
c25519_basetable *c25519_basetable_create(c25519_ctx *ctx, const uint8_t *point, int in_fmt);
void c25519_basetable_destroy(c25519_ctx *ctx, c25519_basetable *t);
int32_t c25519_mul_table_batch_dev(c25519_ctx *ctx, const c25519_basetable *t, const uint8_t *d_scalars, uint64_t n, int out_fmt, uint8_t *d_out);
int32_t c25519_mul_table_batch(c25519_ctx *ctx, const c25519_basetable *t, const uint8_t *scalars, uint64_t n, int out_fmt, uint8_t *out);

/* ---- X25519: out[i] = x25519(k[i], u[i]) -------------------------------------------------------
 * replaces x25519-dalek/src/x25519.rs:390 = MontgomeryPoint(u).mul_clamped(k) (montgomery.rs:150,
 * :183-211): k is clamped inside, bit 255 of u ignored, u >= p reduced, low-order u -> all-zero. */
int32_t c25519_x25519_batch_dev(c25519_ctx *ctx, const uint8_t *d_k, const uint8_t *d_u, uint64_t n, uint8_t *d_out);
int32_t c25519_x25519_batch(c25519_ctx *ctx, const uint8_t *k, const uint8_t *u, uint64_t n, uint8_t *out);
/* The same with SharedSecret::was_contributory (x25519-dalek/src/x25519.rs:335) as a batched flag: contributory[i] = 1 iff
 * out[i] is not all-zero (a low-order u[i] gives the all-zero shared secret, montgomery.rs:403-412).  MontgomeryPoint::
 * mul_clamped (montgomery.rs:150-162) is exactly this function: k is clamped inside. */
int32_t c25519_x25519_contributory_batch_dev(c25519_ctx *ctx, const uint8_t *d_k, const uint8_t *d_u, uint64_t n, uint8_t *d_out, uint8_t *d_contributory);
int32_t c25519_x25519_contributory_batch(c25519_ctx *ctx, const uint8_t *k, const uint8_t *u, uint64_t n, uint8_t *out, uint8_t *contributory);
/* X25519 public keys: out[i] = x25519(k[i], 9), computed the way x25519-dalek does it -- PublicKey::from(&secret) =
 * EdwardsPoint::mul_base_clamped(secret).to_montgomery() (x25519.rs:105-109, :255-259; edwards.rs:948, :574-590) --
 * i.e. through the fixed-base tables and the birational map (Z+Y)/(Z-Y), 12x cheaper than the ladder. */
int32_t c25519_x25519_base_batch_dev(c25519_ctx *ctx, const uint8_t *d_k, uint64_t n, uint8_t *d_out);
int32_t c25519_x25519_base_batch(c25519_ctx *ctx, const uint8_t *k, uint64_t n, uint8_t *out);

/* ---- (de)compression ------------------------------------------------------------------------------
 * decompress: CompressedEdwardsY::decompress (edwards.rs:211-258, ZIP-215 rules) for in_fmt 0,
 * CompressedRistretto::decompress (ristretto.rs:266-345) for in_fmt 1.
 * in: n x 32; out: n x 160 raw points (unspecified where ok[i] == 0); ok: n bytes (1 = Some).
 * Returns C25519_NONE if any ok[i] == 0, else C25519_OK (ok[] tells which). */
int32_t c25519_decompress_batch_dev(c25519_ctx *ctx, const uint8_t *d_in, uint64_t n, int in_fmt, uint8_t *d_out, uint8_t *d_ok);
int32_t c25519_decompress_batch(c25519_ctx *ctx, const uint8_t *in, uint64_t n, int in_fmt, uint8_t *out, uint8_t *ok);
/* compress: EdwardsPoint::compress_batch (edwards.rs:621-647) for out_fmt 0,
 * RistrettoPoint::compress (ristretto.rs:500-533) for out_fmt 1.  in: n x 160 raw; out: n x 32. */
int32_t c25519_compress_batch_dev(c25519_ctx *ctx, const uint8_t *d_in, uint64_t n, int out_fmt, uint8_t *d_out);
int32_t c25519_compress_batch(c25519_ctx *ctx, const uint8_t *in, uint64_t n, int out_fmt, uint8_t *out);

/* Edwards -> Montgomery u-coordinate, batched: EdwardsPoint::to_montgomery_batch (edwards.rs:595-612),
 * u = (Z+Y)/(Z-Y) with one shared inversion per lane-chunk; the identity maps to u = 0 (edwards.rs:574-590).
 * in: n x 160 raw points; out: n x 32 MontgomeryPoint bytes. */
int32_t c25519_to_montgomery_batch_dev(c25519_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out);
int32_t c25519_to_montgomery_batch(c25519_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out);

/* ---- variable-time multiscalar multiplication: out = sum scalars[i] * points[i] -----------------
 * replaces backend::pippenger_optional_multiscalar_mul / straus_optional_multiscalar_mul
 * (backend.rs:79, :224; edwards.rs:1002-1031; ristretto.rs:984).  points: n x 32 (fmt 0/1) or
 * n x 160 (fmt 2).  `out` is a HOST pointer (32 or 160 bytes) in both variants; the call
 * synchronises.  Returns C25519_NONE iff some point fails to decompress (Option::None of the
 * reference); n == 0 gives the identity. */
int32_t c25519_msm_vartime_dev(c25519_ctx *ctx, const uint8_t *d_scalars, const uint8_t *d_points, uint64_t n, int in_fmt, int out_fmt, uint8_t *out);
int32_t c25519_msm_vartime(c25519_ctx *ctx, const uint8_t *scalars, const uint8_t *points, uint64_t n, int in_fmt, int out_fmt, uint8_t *out);
/* Multi-GPU building block: this rank's partial sum as a raw 160-byte point (no final compress),
 * and the fold of `count` partial points gathered from all ranks.  Both are
 * deterministic functions of their inputs.  c25519_fold_partials is host arithmetic over `count`
 * points (count = number of GPUs) and accepts ctx == NULL. */
int32_t c25519_msm_partial_dev(c25519_ctx *ctx, const uint8_t *d_scalars, const uint8_t *d_points, uint64_t n, int in_fmt, uint8_t *out160);
int32_t c25519_fold_partials(c25519_ctx *ctx, const uint8_t *partials160, uint64_t count, int out_fmt, uint8_t *out);

/* MANY independent sums in one call: out[s] = sum of scalars[i] * points[i] for i in [seg_off[s], seg_off[s+1]), s < m -- one
 * VartimeMultiscalarMul::optional_multiscalar_mul (traits.rs:249; edwards.rs:1002-1031, ristretto.rs:984) per segment: Schnorr / DLEQ /
 * Pedersen-opening checks of a few terms each, thousands at a time, whose verdicts must stay separate.  Variable time: the scalars are
 * public by contract, as for c25519_msm_vartime.  (Secret scalars: c25519_mul_batch_dev on a constant-time context, then
 * c25519_point_sum_segments_dev.)
 *   - scalars n x 32, points n x 32 | 160, out m x 32 | 160, ok m bytes (may be NULL): HOST pointers in the un-suffixed form, DEVICE
 *     pointers in the _dev form.  seg_off is a HOST array in BOTH forms -- the lengths are public and the host routes by them: m + 1
 *     non-decreasing values with seg_off[0] = 0 and seg_off[m] = n, anything else returns -(hipErrorInvalidValue) before any launch.
 *     m must be below 2^32 - 1; m == 0 returns C25519_OK.  An empty segment gives the identity.
 *   - formats as for the group law below: in C25519_FMT_EDWARDS_Y -> out 0 or 2, in C25519_FMT_RISTRETTO -> out 1 or 2, in
 *     C25519_FMT_RAW160 -> out 0, 1 or 2; any other pair returns -(hipErrorInvalidValue).  A RAW160 input is trusted to be a point;
 *     compressed inputs decode as in c25519_decompress_batch.
 *   - ok[s] = 0 iff some point of segment s does not decode (the reference's Option::None, per sum; out[s] is then unspecified).  The call
 *     returns C25519_NONE if any segment failed and C25519_OK otherwise; the other segments are unaffected.
 *   - a scalar with bit 255 set, anywhere, returns -(hipErrorInvalidValue) with the message of c25519_msm_vartime; scalars need not be
 *     reduced mod l.
 *   - both forms synchronise the context's stream once, at the end, to read the two verdict words.
 *   - every out[s] is byte for byte what c25519_msm_vartime returns for that segment alone (canonical encodings); a RAW160 output is the
 *     same point (equal under ct_eq), not the same limbs.
 * Cost: four routes, chosen by the length of each segment alone (c25519_msm_vartime_segments_routes reports the choice per segment,
 * c25519_msm_vartime_segments_plan its counts).
 *   - at most C25519_MSM_SEGMENT_DIRECT_MAX terms: one GPU LANE per segment -- Straus with the doubling chain shared by the terms of the
 *     segment (scalar_mul/straus.rs:159-200), radix 16 -- so a wave of 64 consecutive segments costs what its LONGEST one costs: group
 *     segments of similar length next to each other.
 *   - at most C25519_MSM_SEGMENT_WAVE_MAX terms (Bulletproofs-size verification equations): one WAVE per segment -- lane l runs the same
 *     loop over terms l, l + 64, ... and the 64 partial sums are folded at the end -- so a segment costs 252 doublings plus ceil(len / 64)
 *     additions per window in every lane, and thousands of such segments run side by side inside the one call.  (A wave would carry
 *     64 x 64 terms at the serial depth of the lane route's maximum; from 64 segments per call on it is not slower than the single-MSM
 *     route up to 2048 terms, which is where the constant stands.  One lone segment is faster through c25519_msm_vartime.)
 *   - at most C25519_MSM_SEGMENT_BUCKET_MAX terms (aggregated range proofs, large-ring checks): the BUCKET method per segment
 *     (scalar_mul/pippenger.rs:67-160) at one window width, 8 bits, for all such segments of the call side by side -- one record and 32
 *     signed digits per term, one workgroup per (segment, window) that sorts the window's digits into 128 bucket lists, adds them up in
 *     128 equal shares of the entries (so equal scalars cost what uniform ones cost) and reduces the buckets by a suffix scan, then one
 *     lane per segment for the Horner fold: 32 len bucket additions and 248 doublings per segment, three launches however many segments
 *     there are, nothing synchronised before the end of the call.  (64 segments of 2049 / 4096 / 32768 terms: 1.25 / 1.61 / 8.0 ms against
 *     7.5 / 9.5 / 14.3 ms on the single-MSM route; at 65536 terms it loses, which is where the constant stands.  One lone segment is
 *     faster through c25519_msm_vartime.)
 *   - longer: each segment runs as a c25519_msm_partial_dev of its own before the rest is queued (tens of microseconds of latency apiece,
 *     one after the other).
 * The tables of at most C25519_MSM_SEGMENT_PASS_TERMS terms (1344 bytes per term) are resident at a time; more terms of the first two
 * routes run as several passes, cut at segment boundaries.  The bucket segments have passes of their own, of at most
 * C25519_MSM_SEGMENT_BUCKET_PASS_TERMS terms, in the same workspace.  tools/seg_msm_numbers.py times the call against one
 * c25519_msm_vartime_dev per segment and against c25519_mul_batch_dev + c25519_point_sum_segments_dev. */
#define C25519_MSM_SEGMENT_DIRECT_MAX 64       /* longest segment that runs in one lane */
#define C25519_MSM_SEGMENT_WAVE_MAX 2048       /* longest segment that runs in one wave (measured: DESIGN.md section 3.13) */
#define C25519_MSM_SEGMENT_PASS_TERMS 262144   /* most terms whose tables are resident at once (2^18: a 352 MB workspace) */
#define C25519_MSM_SEGMENT_BUCKET_MAX 32768    /* longest segment on the bucket route (measured: DESIGN.md section 3.13; at most 65536, a term index within its segment is 16 bits) */
/* Most terms of one bucket pass.  Per term: a 160-byte record, 32 digit bytes, 32 two-byte indices and an ok byte = 257 bytes; per segment
 * (more than 2048 terms each, so at most 511 of them): 32 window sums of 160 bytes and 32 ok bytes = 5152 bytes.  2^20 x 257 + 511 x 5152 =
 * 272.1 MB, below the 352 MB of a Straus pass, whose place it takes; 2^21 terms would need 539 MB. */
#define C25519_MSM_SEGMENT_BUCKET_PASS_TERMS 1048576
int32_t c25519_msm_vartime_segments_dev(c25519_ctx *ctx, const uint8_t *d_scalars, const uint8_t *d_points, uint64_t n, int in_fmt,
                                        const uint64_t *seg_off /* HOST, m + 1 */, uint64_t m, int out_fmt, uint8_t *d_out /* device, m x (32 | 160) */,
                                        uint8_t *d_ok /* device, m bytes, may be NULL */);
int32_t c25519_msm_vartime_segments(c25519_ctx *ctx, const uint8_t *scalars, const uint8_t *points, uint64_t n, int in_fmt, const uint64_t *seg_off, uint64_t m,
                                    int out_fmt, uint8_t *out, uint8_t *ok);
/* how c25519_msm_vartime_segments routes these offsets: plan[0] lane segments, [1] wave segments,
 * [2] segments longer than the wave maximum (bucket and single-MSM segments together), [3] passes of the lane and wave segments, [4] most
 * terms resident in one of those passes.  Same validation and error as the call (n is seg_off[m]).  Host arithmetic: no context, no GPU. */
int32_t c25519_msm_vartime_segments_plan(const uint64_t *seg_off, uint64_t m, uint64_t plan[5]);
/* ... and segment by segment: route[s] is one of the four codes.  Same validation and error; host arithmetic. */
#define C25519_MSM_SEGMENT_ROUTE_LANE   0
#define C25519_MSM_SEGMENT_ROUTE_WAVE   1
#define C25519_MSM_SEGMENT_ROUTE_BUCKET 2
#define C25519_MSM_SEGMENT_ROUTE_SINGLE 3
int32_t c25519_msm_vartime_segments_routes(const uint64_t *seg_off, uint64_t m, uint8_t *route /* m bytes */);

/* The same decomposition WITHOUT the partial sum ever visiting the host (what curve25519-dalek_amd/multi.py runs, one
 * process per GPU): c25519_msm_partial_record_dev only ENQUEUES on the context's stream and leaves a fixed-size RECORD in
 * device memory -- the window column sums of this rank's terms (the reference's `columns`, pippenger.rs:146-151, before
 * the Horner fold :159), its counters (a point that does not decode, a scalar with bit 255 set) and the number of terms
 * and the window width the window layout was derived from.  The exchange step is ONE all_gather of C25519_PARTIAL_RECORD_BYTES per rank
 * (RCCL, device to device), one copy to the host, and c25519_fold_partial_records: records with the same layout are
 * added column by column and folded once; the others are folded one by one (host arithmetic over count x <= 56 points;
 * ctx may be NULL).  Returns C25519_NONE iff any rank saw a point that does not decode.  The result is bit-identical to
 * c25519_msm_vartime over all terms on one context.  d_record: device pointer, 16-byte aligned. */
#define C25519_PARTIAL_RECORD_BYTES 9024
int32_t c25519_msm_partial_record_dev(c25519_ctx *ctx, const uint8_t *d_scalars, const uint8_t *d_points, uint64_t n, int in_fmt, uint8_t *d_record);
int32_t c25519_fold_partial_records(c25519_ctx *ctx, const uint8_t *records, uint64_t count, int out_fmt, uint8_t *out);
/* A record that holds a given 160-byte point: lets a participant whose partial sum was computed elsewhere (the host-pointer
 * entry points, another library) join the same fold.  status: C25519_OK or C25519_NONE; counters8 (may be NULL): eight
 * u32 counters in the order of the record's flags.  Host arithmetic, no context. */
int32_t c25519_partial_record_pack(const uint8_t *point160, int32_t status, const uint32_t *counters8, uint8_t *record);

/* One process driving several GPUs (SURVEY.md 8e for a host without torch / RCCL, e.g. the Rust shim): the terms are cut
 * into nctx contiguous shards, shard r runs the whole single-GPU path on ctxs[r] (contexts on different devices, or
 * several on one) from its own host thread, and the nctx partial sums are folded on the host -- the one exchange step of
 * the path, 160 bytes per context.  HOST pointers; the result is identical to c25519_msm_vartime on one context.
 * (With one process PER GPU the same decomposition is c25519_msm_partial_dev + an all_gather of the partials over
 * RCCL + c25519_fold_partials: curve25519-dalek_amd/multi.py.) */
int32_t c25519_msm_vartime_multi(c25519_ctx **ctxs, int32_t nctx, const uint8_t *scalars, const uint8_t *points, uint64_t n, int in_fmt, int out_fmt, uint8_t *out);

/* ---- ed25519_dalek::verify_batch (ed25519-dalek/src/batch.rs:146-251) ---------------------------
 * msgs: concatenated messages; msg_off: n+1 offsets into msgs (u64); sigs: n x 64; pks: n x 32.
 * Error precedence as in the reference: a public key that does not decompress -> C25519_NONE (the
 * reference fails earlier, at VerifyingKey::from_bytes, verifying.rs:167); any non-canonical s ->
 * SCALAR_FORMAT; any R that does not decompress, or a non-identity result -> VERIFY.
 * (ARRAY_LENGTH is raised by the host-language wrapper, which owns the three lengths.)
 * msg_off must be non-decreasing with msg_off[n] <= msgs_len (the bytes readable at msgs); otherwise the call returns
 * -(hipErrorInvalidValue) and no byte outside [msgs, msgs + msgs_len) is read. */
int32_t ed25519_verify_batch_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len,
                                 const uint8_t *d_sigs, const uint8_t *d_pks, uint64_t n, uint32_t z_mode);
int32_t ed25519_verify_batch(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off,
                             const uint8_t *sigs, const uint8_t *pks, uint64_t n, uint32_t z_mode);
/* verify_batch over several contexts / GPUs from one process, contiguous shards of the signatures.  C25519_Z_TRANSCRIPT: the
 * reference's ONE transcript over the whole batch and its single equation -- every context hashes its shard, the host runs
 * the transcript once over all H(R||A||M) and s, every context evaluates its share of the equation with its z_i, and the
 * partial sums are folded into one identity check: z_i, equation and verdict are those of the reference whatever nctx is.
 * C25519_Z_DEVICE: each shard is its own random linear combination; the verdict is the worst shard verdict in the
 * reference's precedence. */
int32_t ed25519_verify_batch_multi(c25519_ctx **ctxs, int32_t nctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs, const uint8_t *pks,
                                   uint64_t n, uint32_t z_mode);
/* The same check for callers that hold VerifyingKey values: the reference's VerifyingKey keeps the decompressed
 * point beside the 32 key bytes (verifying.rs:64-71, built once by from_bytes :167-175), so its verify_batch
 * never decompresses A_i (batch.rs:236 uses pk.point directly).  pk_points: n x 160 raw
 * EdwardsPoints matching pks (e.g. from c25519_decompress_batch), or NULL = decompress the key bytes here.
 * CONTRACT (the reference's VerifyingKey type invariant, verifying.rs:64-71): pk_points[i] MUST be the decompression of
 * pks[i].  The hash uses the bytes and the group equation the point; a mismatched pair verifies against a key that
 * was not hashed.  The library does not re-check it (that would be the decompression this entry point exists to skip);
 * host-language wrappers must only build the pair through from_bytes (dalek.VerifyingKey does). */
int32_t ed25519_verify_batch_keys_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len,
                                      const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_points, uint64_t n, uint32_t z_mode);
int32_t ed25519_verify_batch_keys(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off,
                                  const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_points, uint64_t n, uint32_t z_mode);

/* MANY independent batches in one call: status[s] is, byte for byte, what ed25519_verify_batch_keys[_dev] returns for the signatures
 * [seg_off[s], seg_off[s+1]) alone in the same z_mode (batch.rs:146-251, once per segment) -- a block's transactions, a gossip round's
 * votes, a certificate chain: batches of 4 .. 256 signatures whose verdicts must stay separate; or the halves, quarters, ... of a large
 * batch that failed, to locate the defect in one call.
 *   - status[s]: 0 OK; 1 a key of the segment does not decode; 2 a non-canonical s in the segment; 3 an R that does not decode, or a
 *     non-identity sum.  Precedence 1 over 2 over 3; an empty segment is 0.  A defect in one segment changes no other segment's status.
 *   - the return value is C25519_OK whenever the statuses were written, whatever they are (as ed25519_verify_each); negative values are
 *     argument or HIP errors.  m == 0 returns C25519_OK.
 *   - seg_off is a HOST array in BOTH forms (the lengths are public and the host routes by them), validated as by
 *     c25519_msm_vartime_segments: m + 1 non-decreasing values from 0 to n, m below 2^32 - 1; anything else returns -(hipErrorInvalidValue)
 *     before any launch.  msg_off as for ed25519_verify_batch_dev (the _dev form checks it on the device; no byte outside msgs is read).
 *   - pk_points (n x 160, or NULL): the contract of ed25519_verify_batch_keys.
 *   - the z_i of a segment are those the single call derives for that segment alone: C25519_Z_TRANSCRIPT -- one Merlin transcript per
 *     segment over its hram and s: on the device, one lane per segment, up to ED25519_TRANSCRIPT_SEGMENT_DEVICE_MAX signatures; on the host
 *     for longer segments (one synchronisation in the middle of the call, only when there is such a segment:
 *     ed25519_batch_transcript_zs_segments_plan reports it); C25519_Z_DEVICE -- the hash tree over the segment, tagged with the segment's
 *     own length.  (Verdicts on points with a torsion component depend on the z_i.)
 * Route, by the length of each segment alone (ed25519_verify_batch_segments_plan reports it): at most ED25519_VERIFY_SEGMENT_MAX signatures
 * -- the segment is one segment of 2k + 1 terms [B | R_0 .. R_{k-1} | A_0 .. A_{k-1}] of c25519_msm_vartime_segments_dev (its lane route up to
 * 31 signatures, its wave route beyond); longer -- the segment runs through ed25519_verify_batch_keys_dev on its slice before anything else is
 * queued.  Segmented-route work is cut into passes of at most C25519_MSM_SEGMENT_PASS_TERMS terms at segment boundaries.  As on the MSM's lane
 * route, a wave of 64 consecutive short segments costs what its longest one costs: keep segments of similar length together.
 * Measured (tools/verify_seg_numbers.py, profiles/verify_seg_numbers.txt; 2^16 device-resident signatures, device
 * z-mode): 1.6 - 6.3 ms per call for segments of 1 .. 1023 signatures, against 15 ms .. 12.9 s for one ed25519_verify_batch_keys_dev per
 * segment.  Break-even against the per-segment calls: from 16 segments for lengths 1, 4 and 256, from 8 at 64, from 64 at 16, from 32 at
 * 1023; a handful of batches is faster one call each.  ed25519_verify_each_dev over the same signatures (1.2 ms) is FASTER at every
 * measured length, x1.3 (64 per segment) to x5.3 (16 and 1023 per segment), and at 2^20 signatures still x1.4 - x1.9: a caller who only
 * needs to know which signatures are good calls verify_each.  This call is for callers who need verify_batch's own verdict per batch
 * (the two differ on keys and R with a torsion component).  The transcript z-mode costs 1.9 / 2.5 / 6.4 / 2.8 / 7.5 / 25.0 ms per 2^16
 * signatures in segments of 1 / 4 / 16 / 64 / 256 / 1023 (device transcripts up to 256 signatures, the host sponge at 1023; 21 - 47 ms
 * before the transcripts moved to the device).  A call with FEW segments of 64 .. 256 signatures is slower in this z-mode than with the
 * host sponge it had before -- one segment of 64: 1.2 -> 2.75 ms, one of 256: 2.2 -> 8.1 ms; level from about 64 segments, faster from
 * 256 -- because a lane's chain costs 20 us per signature however few lanes run: see ed25519_batch_transcript_zs_segments below. */
#define ED25519_VERIFY_SEGMENT_MAX 1023   /* 2k+1 <= C25519_MSM_SEGMENT_WAVE_MAX: longest segment on the segmented route */
int32_t ed25519_verify_batch_segments_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len,
                                          const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_points /* n x 160 or NULL */, uint64_t n,
                                          const uint64_t *seg_off /* HOST, m + 1 */, uint64_t m, uint32_t z_mode, uint8_t *d_status /* device, m bytes */);
int32_t ed25519_verify_batch_segments(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs, const uint8_t *pks,
                                      const uint8_t *pk_points, uint64_t n, const uint64_t *seg_off, uint64_t m, uint32_t z_mode, uint8_t *status);
/* how the call routes these offsets: plan[0] segments on the segmented route, [1] segments run as single batches, [2] passes, [3] most terms
 * in one pass.  Same validation and error as the call (n is seg_off[m]).  Host arithmetic: no context, no GPU. */
int32_t ed25519_verify_batch_segments_plan(const uint64_t *seg_off, uint64_t m, uint64_t plan[4]);

/* The Merlin transcripts of MANY independent batches (batch.rs:168-222 over batch/transcript.rs, once per segment) on the GPU: z16 rows
 * [seg_off[s], seg_off[s+1]) are, byte for byte, what ed25519_batch_transcript_zs returns for the hram and sigs rows of that segment alone.
 * One transcript per LANE: STROBE-128/1600 and Keccak-f[1600] with the sponge in registers (csrc/transcript_dev.h).  A transcript is
 * sequential -- 1.73 permutations per signature, one chain -- so the call's time is that of its LONGEST segment, 20 - 23 us per
 * signature (11.7 us per permutation: a wave alone on its SIMD), however many segments there are up to 65536, one wave each per 64; the
 * host function needs 0.29 us per signature, one segment after the other.  THE COST OF A LONG SEGMENT: 1023 signatures hold the call
 * for 21 - 24 ms, 4096 for 96 ms, while the host function is done with them in 0.3 / 1.3 ms: the device pays off through the NUMBER of
 * segments, never through the length of one.
 *   - the _dev form only enqueues on the context's stream and does not synchronise: ed25519_batch_hram_dev -> this ->
 *     ed25519_verify_batch_record_dev never visits the host.  It runs EVERY segment on the device whatever its length.  d_hram, d_sigs and
 *     d_z16 are 8-byte aligned; the host form uploads, runs, downloads and synchronises.
 *   - seg_off is a HOST array in both forms, validated exactly as by ed25519_verify_batch_segments: the same -(hipErrorInvalidValue), before
 *     any launch; it is free on return.  m == 0 returns C25519_OK; an empty segment writes nothing.
 *   - ed25519_batch_transcript_zs_segments_plan (host arithmetic, no context): how ed25519_verify_batch_segments routes the transcripts of
 *     these offsets in C25519_Z_TRANSCRIPT -- plan[0] segments of at most ED25519_TRANSCRIPT_SEGMENT_DEVICE_MAX signatures: on the device;
 *     plan[1] longer ones up to ED25519_VERIFY_SEGMENT_MAX: the host sponge.  Still longer segments are single batches and counted in neither.
 * Measured (tools/verify_seg_numbers.py --transcript-arms, the last section of profiles/verify_seg_numbers.txt, DESIGN.md section 3.14;
 * 2^16 device-resident signatures in segments of 1 / 4 / 16 / 64 / 256 / 1023): the kernel alone 0.046 / 0.10 / 0.34 / 1.30 / 5.13 / 20.7 ms
 * against 276 / 82 / 35 / 23 / 19.8 / 19.0 ms of the host function over the same segments.  Inside ed25519_verify_batch_segments_dev
 * (transcript z-mode, cached key points; the arms alternate in one process, spread 0.1 - 0.4 ms): 1.85 / 2.46 / 6.44 / 2.83 / 7.54 / 26.6 ms
 * with every transcript on the device against 47.3 / 27.6 / 27.0 / 21.0 / 21.6 / 24.9 ms with every one on the host (the parent's code: the same
 * within the spread) -- the device wins by x25.6 .. x2.9 up to 256 signatures and loses by x1.07 at 1023, hence the constant.  Break-even
 * against the host path, m segments of one length: from m = 64 at 4 signatures, from 256 at 64 (a tie at 64) and from 256 at 256 (x1.04
 * slower at 64); below that the host path is faster by up to x2.2 (64) / x3.8 (256), 1.4 / 6 ms per call.  Routing stays by length alone. */
#define ED25519_TRANSCRIPT_SEGMENT_DEVICE_MAX 256   /* the largest measured length at which the device transcript beats the host's by more than the spread */
int32_t ed25519_batch_transcript_zs_segments_dev(c25519_ctx *ctx, const uint8_t *d_hram /* n x 64 */, const uint8_t *d_sigs /* n x 64 */, uint64_t n,
                                                 const uint64_t *seg_off /* HOST, m + 1 */, uint64_t m, uint8_t *d_z16 /* n x 16 */);
int32_t ed25519_batch_transcript_zs_segments(c25519_ctx *ctx, const uint8_t *hram, const uint8_t *sigs, uint64_t n, const uint64_t *seg_off, uint64_t m, uint8_t *z16);
int32_t ed25519_batch_transcript_zs_segments_plan(const uint64_t *seg_off, uint64_t m, uint64_t plan[2]);

/* ---- verify_batch across ranks with the reference's ONE transcript (C25519_Z_TRANSCRIPT; SURVEY.md 8e: "the sequential
 * transcript runs once on the host and the z_i are scattered") -- the building blocks multi.verify_batch_sharded and
 * ed25519_verify_batch_multi are made of:
 *   1. ed25519_batch_hram_dev      this rank's H(R_i || A_i || M_i) (batch.rs:179-191) to device memory: n x 64 bytes followed
 *                                  by a 64-byte trailer of counters (u32 [0] signatures with a non-canonical s, [1] bad
 *                                  message offsets); enqueue only.  d_hram needs room for n x 64 + 64 bytes.
 *   2. (exchange)                  every hram and every s reaches whoever runs the transcript -- one all_gather
 *   3. ed25519_batch_transcript_zs the reference's Merlin/STROBE transcript over the WHOLE batch (batch.rs:168-222), HOST
 *                                  pointers, no context: hram n x 64, sigs n x 64 (s = bytes 32..63) -> z16 n x 16
 *   4. ed25519_verify_batch_record_dev   this rank's share of the batch equation (batch.rs:213-244) with ITS z_i (d_z16) and
 *                                  its hram buffer from step 1 (trailer included), as a partial-result record in device
 *                                  memory (layout and size as c25519_msm_partial_record_dev); enqueue only
 *   5. (exchange) + ed25519_fold_verify_records   the records of all ranks -> the reference's single identity check
 *                                  (batch.rs:246-250) and error precedence; HOST pointer, ctx may be NULL.
 * The z_i, the equation and the verdict are those of the reference on the whole batch, whatever the number of ranks. */
int32_t ed25519_batch_hram_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len, const uint8_t *d_sigs, const uint8_t *d_pks, uint64_t n,
                               uint8_t *d_hram);
int32_t ed25519_batch_transcript_zs(const uint8_t *hram, const uint8_t *sigs, uint64_t n, uint8_t *z16);
int32_t ed25519_verify_batch_record_dev(c25519_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_points, const uint8_t *d_hram, const uint8_t *d_z16,
                                        uint64_t n, uint8_t *d_record);
int32_t ed25519_fold_verify_records(c25519_ctx *ctx, const uint8_t *records, uint64_t count);

/* diagnostics for the tests that pin the z derivation: the z_i a batch of n <= 1.5 x 2^20 signatures gets, 16 bytes each
 * to the HOST buffer out_z16 (HOST pointers throughout).  z_mode 0: little-endian u128, the reference's values;
 * z_mode 1: bit 127 = sign, bits 0..126 = magnitude; z_mode 2 (this entry point only): the values of z_mode 1 computed by the host
 * restatement of the derivation that batches of at most 128 signatures use (no kernel runs) -- equal to z_mode 1 byte for byte. */
int32_t c25519_debug_batch_zs(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs, const uint8_t *pks, uint64_t n,
                              uint32_t z_mode, uint8_t *out_z16);

/* diagnostics for kernel traces: the SORT of one MSM pass alone (n scalars on the device, 4096 <= n <= 2^22; the window layout of
 * `layout_terms` terms, 0 = of n), `reps` times back to back on the context's stream, then a synchronisation.  No result:
 * tools/sort_only.py runs it under rocprofv3 to time the sort kernels without an accumulation beside them. */
int32_t c25519_debug_sort(c25519_ctx *ctx, const uint8_t *d_scalars, uint64_t n, uint64_t layout_terms, int32_t reps);

/* ---- variable base: out[i] = scalars[i] * points[i] ------------------------------------------------
 * replaces backend::variable_base_mul (backend.rs:253 -> scalar_mul/variable_base.rs:11-47;
 * `&EdwardsPoint * &Scalar`, edwards.rs:890-911), radix-16 fixed windows, one pair per lane.
 * points: n x 32 (fmt 0) or n x 160 (fmt 2); out: n x 32 (fmt 0) or n x 160 (fmt 2);
 * ok (may be NULL): n bytes, 0 where a compressed point did not decode (that output is unspecified).
 * RistrettoPoint * Scalar (ristretto.rs:910-935): in_fmt C25519_FMT_RISTRETTO with out_fmt 1 or 2, or in_fmt 2 with out_fmt 1 (the
 * same ladder; Ristretto decoding and compression).  c25519_mul_clamped_batch stays Edwards only. */
int32_t c25519_mul_batch_dev(c25519_ctx *ctx, const uint8_t *d_scalars, const uint8_t *d_points, uint64_t n, int in_fmt, int out_fmt, uint8_t *d_out, uint8_t *d_ok);
int32_t c25519_mul_batch(c25519_ctx *ctx, const uint8_t *scalars, const uint8_t *points, uint64_t n, int in_fmt, int out_fmt, uint8_t *out, uint8_t *ok);

/* EdwardsPoint::mul_clamped (edwards.rs:932-946): out[i] = clamp_integer(bytes[i]) * points[i] (not reduced mod l). */
int32_t c25519_mul_clamped_batch_dev(c25519_ctx *ctx, const uint8_t *d_bytes, const uint8_t *d_points, uint64_t n, int in_fmt, int out_fmt, uint8_t *d_out, uint8_t *d_ok);
int32_t c25519_mul_clamped_batch(c25519_ctx *ctx, const uint8_t *bytes, const uint8_t *points, uint64_t n, int in_fmt, int out_fmt, uint8_t *out, uint8_t *ok);

/* ---- order checks: flags[i] of point i ----------------------------------------------------------------------
 * replaces EdwardsPoint::is_small_order (edwards.rs:1405-1407: mul_by_cofactor().is_identity()), EdwardsPoint::is_torsion_free
 * (edwards.rs:1435-1437: (self * BASEPOINT_ORDER).is_identity()) and, through them, VerifyingKey::is_weak
 * (ed25519-dalek/src/verifying.rs:192-194), batched.  in_fmt: C25519_FMT_EDWARDS_Y or C25519_FMT_RAW160.
 * flags[i]: C25519_POINT_DECODES (always set for raw points) | C25519_POINT_SMALL_ORDER | C25519_POINT_TORSION_FREE;
 * a point that does not decode has flags[i] = 0.  `which` selects the checks to run (C25519_POINT_SMALL_ORDER, C25519_POINT_TORSION_FREE
 * or both; the torsion check is a full variable-base multiplication by l).  Variable time: the points are public keys / signature parts. */
#define C25519_POINT_DECODES 1
#define C25519_POINT_SMALL_ORDER 2
#define C25519_POINT_TORSION_FREE 4
int32_t c25519_point_order_checks_batch_dev(c25519_ctx *ctx, const uint8_t *d_points, uint64_t n, int in_fmt, int which, uint8_t *d_flags);
int32_t c25519_point_order_checks_batch(c25519_ctx *ctx, const uint8_t *points, uint64_t n, int in_fmt, int which, uint8_t *flags);

/* ---- double base: out[i] = a[i] * A[i] + b[i] * B ---------------------------------------------------------
 * replaces backend::vartime_double_base_mul (backend.rs:267 -> scalar_mul/vartime_double_base.rs:23-72;
 * EdwardsPoint::vartime_double_scalar_mul_basepoint, edwards.rs:1099-1106), the single-signature kernel,
 * batched: a radix-16 ladder on A_i plus the fixed-base table on B.  Formats and `ok` as c25519_mul_batch, the Ristretto pairs included:
 * RistrettoPoint::vartime_double_scalar_mul_basepoint (ristretto.rs:1054). */
int32_t c25519_double_base_batch_dev(c25519_ctx *ctx, const uint8_t *d_a, const uint8_t *d_A, const uint8_t *d_b, uint64_t n, int in_fmt, int out_fmt, uint8_t *d_out, uint8_t *d_ok);
int32_t c25519_double_base_batch(c25519_ctx *ctx, const uint8_t *a, const uint8_t *A, const uint8_t *b, uint64_t n, int in_fmt, int out_fmt, uint8_t *out, uint8_t *ok);

/* ---- per-signature verification: status[i] for every signature ----------------------------------------
 * replaces VerifyingKey::verify (verifying.rs:565 -> raw_verify :203 -> RCompute::finish :549-556 over
 * vartime_double_base::mul, scalar_mul/vartime_double_base.rs:23-72) and, with strict != 0,
 * VerifyingKey::verify_strict (verifying.rs:359-382: R must decode, R and A must not be of small
 * order).  status[i]: 0 OK, 1 key does not decode (VerifyingKey::from_bytes), 2 SCALAR_FORMAT, 3 VERIFY.
 * This is what locates the bad signature after a failed batch. */
int32_t ed25519_verify_each_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len,
                                const uint8_t *d_sigs, const uint8_t *d_pks, uint64_t n, int strict, uint8_t *d_status);
int32_t ed25519_verify_each(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs, const uint8_t *pks,
                            uint64_t n, int strict, uint8_t *status);

/* Ed25519ph / Ed25519ctx, per signature (RFC 8032 5.1; replaces VerifyingKey::verify_prehashed ed25519-dalek/src/verifying.rs:284 ->
 * raw_verify_prehashed :230-257, verify_prehashed_strict :424-461, challenge by RCompute::new :520-534 with prehash_ctx = Some(ctx)):
 * hram_i = SHA-512("SigEd25519 no Ed25519 collisions" || 0x01 || len(ctx) || ctx || R_i || A_i || PH(M_i)).
 * prehashes: n x 64 bytes, PH(M_i) = SHA-512(M_i) (the reference takes the digest state and finalises it); context: HOST pointer in both
 * forms, 0 .. 255 bytes (NULL allowed when context_len = 0 -- the reference's `None`), ONE context for the batch; a longer context returns
 * C25519_PREHASHED_CONTEXT_LENGTH.  status per signature as ed25519_verify_each. */
int32_t ed25519_verify_each_prehashed_dev(c25519_ctx *ctx, const uint8_t *d_prehashes, const uint8_t *context, uint32_t context_len,
                                          const uint8_t *d_sigs, const uint8_t *d_pks, uint64_t n, int strict, uint8_t *d_status);
int32_t ed25519_verify_each_prehashed(c25519_ctx *ctx, const uint8_t *prehashes, const uint8_t *context, uint32_t context_len, const uint8_t *sigs, const uint8_t *pks,
                                      uint64_t n, int strict, uint8_t *status);

/* ---- batched key generation and signing (consumers of the fixed-base kernel) ---------------------------
 * keygen: pk_i = compress(clamp(SHA-512(seed_i)[0..32]) * B)   (verifying.rs:97-101, RFC 8032 5.1.5)
 * sign:   RFC 8032 5.1.6 as in signing.rs:878-905; also returns the public keys.  seeds: n x 32. */
int32_t ed25519_keygen_batch_dev(c25519_ctx *ctx, const uint8_t *d_seeds, uint64_t n, uint8_t *d_pks);
int32_t ed25519_sign_batch_dev(c25519_ctx *ctx, const uint8_t *d_seeds, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len,
                               uint64_t n, uint8_t *d_pks, uint8_t *d_sigs);
int32_t ed25519_sign_batch(c25519_ctx *ctx, const uint8_t *seeds, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, uint8_t *pks, uint8_t *sigs);
/* Ed25519ph signing (SigningKey::sign_prehashed signing.rs:312 -> raw_sign_prehashed :917-976): r = H(dom2 || prefix || PH(M)), k = H(dom2 || R || A ||
 * PH(M)); prehashes n x 64 bytes, context a HOST pointer of 0 .. 255 bytes (as ed25519_verify_each_prehashed). */
int32_t ed25519_sign_batch_prehashed_dev(c25519_ctx *ctx, const uint8_t *d_seeds, const uint8_t *d_prehashes, const uint8_t *context, uint32_t context_len,
                                         uint64_t n, uint8_t *d_pks, uint8_t *d_sigs);
int32_t ed25519_sign_batch_prehashed(c25519_ctx *ctx, const uint8_t *seeds, const uint8_t *prehashes, const uint8_t *context, uint32_t context_len, uint64_t n,
                                     uint8_t *pks, uint8_t *sigs);

/* ---- precomputed static points: VartimePrecomputedMultiscalarMul (traits.rs:304-419) ---------------------
 * replaces backend::VartimePrecomputedStraus::{new, len, optional_mixed_multiscalar_mul}
 * (backend.rs:100-192 -> scalar_mul/precomputed_straus.rs:29-127; edwards.rs:1037-1076).
 * create: for static points S_i (HOST pointer; fmt 0/1/2) the multiples 2^(c k) S_i of every window k are computed
 * once and stay resident in HBM as affine Niels records (17 x 128 bytes per point at c = 16): the bucket-method
 * counterpart of the reference's per-point NAF tables.  A call then needs no point preparation, no per-window passes and
 * no doubling chain -- one bucket accumulation and one bucket reduction over all digits of all scalars.  Returns NULL
 * if a point does not decode.  msm: sum static_scalars[i]*S_i (the first n_static_scalars static points;
 * more scalars than points is an error, precomputed_straus.rs:86) + sum dyn_scalars[j]*dyn_points[j] (the dynamic terms
 * run through the ordinary MSM and are added).
 * All pointers of the msm call are HOST pointers; returns C25519_NONE iff a dynamic point does not decode. */
typedef struct c25519_precomp c25519_precomp;
c25519_precomp *c25519_precomp_create(c25519_ctx *ctx, const uint8_t *static_points, uint64_t n, int in_fmt);
void c25519_precomp_destroy(c25519_ctx *ctx, c25519_precomp *p);
uint64_t c25519_precomp_len(const c25519_precomp *p);
int32_t c25519_precomp_msm_vartime(c25519_ctx *ctx, const c25519_precomp *p, const uint8_t *static_scalars, uint64_t n_static_scalars,
                                   const uint8_t *dyn_scalars, const uint8_t *dyn_points, uint64_t n_dyn, int in_fmt, int out_fmt, uint8_t *out);

/* MANY multiscalar muls over ONE precomputation in one call: out[r] = sum_{j < w} scalars[r][j] * S_j over the first w static points of the
 * handle, r < m -- one VartimePrecomputedMultiscalarMul::vartime_multiscalar_mul (traits.rs:304-419; edwards.rs:1037-1076, ristretto.rs:1004)
 * per row: Pedersen / vector commitments to thousands of vectors, the generator side of thousands of Bulletproofs-size equations, polynomial
 * commitments row by row.  Variable time: the scalars are public by contract, as for c25519_msm_vartime.
 *   - scalars m x w x 32, row-major; out m x 32 | 160: HOST pointers in the un-suffixed form, DEVICE pointers in the _dev form.
 *   - each of these returns -(hipErrorInvalidValue) before any launch: w above c25519_precomp_len (precomputed_straus.rs:86), out_fmt outside
 *     0 .. 2, an unknown route, m not below 2^32 - 1, m * w overflowing, a handle of more than C25519_PRECOMP_ROWS_MAX_POINTS points (run such a
 *     handle through c25519_precomp_msm_vartime, row by row).  m == 0 returns C25519_OK and touches nothing; w == 0 writes m identities.
 *   - a scalar with bit 255 set, anywhere, returns -(hipErrorInvalidValue) with the message of c25519_msm_vartime; scalars need not be
 *     reduced mod l.  There is no ok array: the static points were decoded at create, so the call returns C25519_OK or an error.
 *   - both forms synchronise the context's stream once, at the end, to read the bit-255 verdict word.
 *   - every out[r] in format 0 or 1 is byte for byte what c25519_precomp_msm_vartime returns for that row alone; a RAW160 output is the same
 *     point (equal under ct_eq), not the same limbs.  Any out_fmt goes with any handle, as there.
 * The comb table: the FIRST rows call on a handle computes e * 16^k * S_j for every static point j, window k < 64 and e = 1 .. 8 and keeps them
 * resident as affine Niels records, the eight of one (j, k) next to each other: 65536 bytes per static point (256 MB at
 * C25519_PRECOMP_ROWS_MAX_POINTS), owned by the handle and freed by c25519_precomp_destroy.  c25519_precomp_create, its footprint and the
 * results of c25519_precomp_msm_vartime are unchanged; c25519_precomp_rows_table_bytes is 0 until that first call and the table's size after
 * it.  The build runs on the context's stream, 256 static points at a time (20 MB of scratch); with the allocation it adds 0.7 / 2.7 / 10.5 ms to
 * that first call for 128 / 1024 / 4096 points.
 * A handle is used from one thread at a time, like its context.
 * Cost: a row needs no doubling and no per-call table -- at most 64 mixed additions per term (radix-16 signed digits, scalar.rs:1019-1051; a
 * zero digit is skipped), which no doubling chain orders.  Two routes, chosen by (m, w) alone (c25519_precomp_msm_vartime_rows_plan reports it;
 * route = C25519_PRECOMP_ROWS_LANE / _WAVE forces one, and both are correct for every shape):
 *   - LANE: one GPU lane per row, 64 consecutive rows per wave, all on the same (j, k) at the same time so that their gathers fall into one
 *     1 KB group of records; 64 w serial additions per lane, so it needs tens of thousands of rows to fill the GPU.
 *   - WAVE: one wave per row, lane l takes window l of every scalar; the 64 partial sums are folded with six shuffle rounds: w + about 8
 *     addition slots per row.
 *   C25519_PRECOMP_ROWS_AUTO takes the lane route iff w < C25519_PRECOMP_ROWS_LANE_WIDTH and m >= C25519_PRECOMP_ROWS_LANE_MIN_ROWS, both set
 *   at the crossover measured by tools/precomp_rows_numbers.py (profiles/precomp_rows_numbers.txt).
 * Measured against one c25519_precomp_msm_vartime per row (0.16 - 0.19 ms each) and against c25519_msm_vartime_segments_dev with the
 * generators replicated into every row: 4096 rows of 128 scalars 1.46 ms against 670 and 3.86 ms; 131072 rows of 2: 0.78 ms against 22 s and
 * 2.08 ms; 64 rows of 2048: 6.99 ms against 11.9 and 7.04 ms -- LEVEL with the segments call there (x1.01): 64 waves do not fill the GPU, and a
 * row is one wave's chain of w additions however few rows there are. */
#define C25519_PRECOMP_ROWS_MAX_POINTS 4096   /* largest handle the rows call serves: 64 KB of comb table per point, 256 MB */
#define C25519_PRECOMP_ROWS_AUTO 0
#define C25519_PRECOMP_ROWS_LANE 1            /* one lane per row  */
#define C25519_PRECOMP_ROWS_WAVE 2            /* one wave per row  */
#define C25519_PRECOMP_ROWS_LANE_WIDTH 16     /* AUTO: the lane route only for rows narrower than this ... */
#define C25519_PRECOMP_ROWS_LANE_MIN_ROWS 32768   /* ... and only from this many rows (measured: DESIGN.md section 3.15) */
int32_t c25519_precomp_msm_vartime_rows_dev(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *d_scalars /* m x w x 32, row-major */, uint64_t m, uint64_t w,
                                            int32_t route, int out_fmt, uint8_t *d_out /* m x (32 | 160) */);
int32_t c25519_precomp_msm_vartime_rows(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *scalars, uint64_t m, uint64_t w, int32_t route, int out_fmt,
                                        uint8_t *out);
/* how C25519_PRECOMP_ROWS_AUTO routes m rows of w terms: plan[0] the route (C25519_PRECOMP_ROWS_LANE or _WAVE), plan[1] the waves it launches.
 * Same bounds on m and m * w and the same error as the call.  Host arithmetic: no context, no GPU. */
int32_t c25519_precomp_msm_vartime_rows_plan(uint64_t m, uint64_t w, uint64_t plan[2]);
/* bytes of the handle's comb table: 0 until the first rows call has built it, 65536 per static point afterwards */
uint64_t c25519_precomp_rows_table_bytes(const c25519_precomp *p);

/* MANY MIXED multiscalar muls over ONE precomputation in one call:
 *   out[r] = sum_{j < w} static_scalars[r][j] * S_j + sum_{i in [dyn_off[r], dyn_off[r+1])} dyn_scalars[i] * dyn_points[i],   r < m
 * -- one VartimePrecomputedMultiscalarMul::vartime_mixed_multiscalar_mul (traits.rs:304-419, precomputed_straus.rs:29-127) per row: the
 * verification equation of a Bulletproofs range proof (2 * 64 + 2 static generators, 17 dynamic points A, S, T1, T2, V, L_i, R_i), of an
 * aggregated one, of a Schnorr / DLEQ / Pedersen-opening check (1 - 2 static, 1 - 3 dynamic).  Variable time: the scalars are public by
 * contract, as for c25519_msm_vartime.
 *   - static_scalars m x w x 32, row-major; dyn_scalars n_dyn x 32, dyn_points n_dyn x 32 | 160 in in_fmt, the rows' terms one after the other;
 *     out m x 32 | 160; ok m bytes (may be NULL): HOST pointers in the un-suffixed form, DEVICE pointers in the _dev form.  dyn_off is a HOST
 *     array of m + 1 offsets in both forms, as for c25519_msm_vartime_segments_dev: the lengths are public and the host cuts the passes by them.
 *   - each of these returns -(hipErrorInvalidValue) before any launch: what c25519_precomp_msm_vartime_rows refuses (w above c25519_precomp_len,
 *     precomputed_straus.rs:86; out_fmt outside 0 .. 2; an unknown route; m not below 2^32 - 1; m * w overflowing; a handle of more than
 *     C25519_PRECOMP_ROWS_MAX_POINTS points); offsets c25519_msm_vartime_segments refuses (dyn_off[0] != 0, dyn_off[m] != n_dyn, a decreasing
 *     pair, n_dyn not below 2^40); in_fmt and out_fmt of different groups (the pairing rule of c25519_msm_vartime_segments); and a row of more
 *     than C25519_MSM_SEGMENT_WAVE_MAX dynamic terms -- such a row belongs to c25519_precomp_msm_vartime, one call for it.
 *   - m == 0 returns C25519_OK and touches nothing; a row with w == 0 and no dynamic term is the identity with ok = 1.
 *   - a static or dynamic scalar with bit 255 set, anywhere, returns -(hipErrorInvalidValue) with the message of c25519_msm_vartime; scalars
 *     need not be reduced mod l.
 *   - ok[r] = 0 iff a dynamic point of row r does not decode (Option::None of that row alone; its output is unspecified); the call returns
 *     C25519_NONE iff any row has ok = 0 and C25519_OK otherwise, with or without an ok array.  RAW160 dynamic points are trusted.
 *   - both forms synchronise the context's stream once, at the end, to read the two verdict words.
 *   - every out[r] with ok[r] = 1 in format 0 or 1 is byte for byte what c25519_precomp_msm_vartime returns for that row alone; a RAW160
 *     output is the same point (equal under ct_eq), not the same limbs.
 * The comb table is the rows call's: the first mixed OR rows call on a handle builds it (65536 bytes per static point, see above), and
 * c25519_precomp_rows_table_bytes reports it as before.
 * How: the dynamic half of a row is Straus with one doubling chain shared by its terms (scalar_mul/straus.rs:159-200), over per-term tables
 * {1 .. 8} P built per pass as by c25519_msm_vartime_segments (1344 bytes per term; at most C25519_MSM_SEGMENT_PASS_TERMS dynamic terms are
 * resident at a time, more are cut into passes at row boundaries: one tables launch and one row launch per pass).  The static half needs no
 * doubling -- the comb records are already scaled by 16^k -- so it is added into the accumulator the window loop leaves behind: one
 * accumulator, one fold and one store per row, where the composition rows -> segments -> c25519_point_add_batch_dev takes three calls, three
 * synchronisations and two 160-byte round trips per row.  A row without dynamic terms skips the doubling chain.  Two routes
 * (route = C25519_PRECOMP_ROWS_LANE / _WAVE forces one; both are correct for every accepted shape):
 *   - WAVE: one wave per row; lane l takes dynamic terms l, l + 64, ... through the window loop, then window l of every static scalar.
 *   - LANE: one lane per row, 64 consecutive rows per wave: a wave costs what its longest row costs.
 *   C25519_PRECOMP_ROWS_AUTO (c25519_precomp_msm_vartime_mixed_rows_plan reports it), with t = w + the dynamic terms of the longest row: the
 *   wave route if w >= C25519_PRECOMP_ROWS_LANE_WIDTH; the rule of the rows call (lane iff m >= C25519_PRECOMP_ROWS_LANE_MIN_ROWS) if no row has
 *   a dynamic term -- the call is the rows call then; otherwise the lane route iff the longest row has at most
 *   C25519_PRECOMP_MIXED_LANE_DYN_MAX dynamic terms and m >= C25519_PRECOMP_MIXED_LANE_BASE_ROWS + C25519_PRECOMP_MIXED_LANE_ROWS_PER_TERM * t.
 *   Measured, not derived: with a dynamic term the wave route pays a whole doubling chain per row, so lanes win from far fewer rows than in
 *   the rows call, and a lane's gathers over long rows' tables lose to the wave route well below C25519_MSM_SEGMENT_DIRECT_MAX terms.
 * Measured by tools/precomp_mixed_numbers.py (profiles/precomp_mixed_numbers.txt): against the three
 * calls it replaces (rows -> segments -> c25519_point_add_batch_dev) and one c25519_precomp_msm_vartime per row, device-resident, ms:
 * 4096 rows of 130 + 17: 3.82 against 5.51 and 2030; 256 of 2050 + 40: 6.68 against 15.2 and 109; 64 of 2048 + 64: 6.67 against 19.4 and 27;
 * 131072 of 2 + 1: 2.38 against 2.31 and 42 500; 2^20 of 1 + 2: 18.3 against 18.6 and 337 000 -- LEVEL with the composition at those two;
 * 4096 of 2 + 1: 1.17 against 0.98 and 1310 -- x1.2 SLOWER than the composition.  Rows of one to three terms are the same lane work
 * either way: there the call saves the caller two calls, not time. */
#define C25519_PRECOMP_MIXED_LANE_DYN_MAX 16          /* AUTO: the lane route only if no row has more dynamic terms than this ... */
#define C25519_PRECOMP_MIXED_LANE_BASE_ROWS 1024      /* ... and only from BASE_ROWS + ROWS_PER_TERM * (w + longest row's dynamic terms) rows */
#define C25519_PRECOMP_MIXED_LANE_ROWS_PER_TERM 320   /*     (measured: DESIGN.md section 3.16) */
int32_t c25519_precomp_msm_vartime_mixed_rows_dev(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *d_static_scalars /* m x w x 32, row-major */, uint64_t m,
                                                  uint64_t w, const uint8_t *d_dyn_scalars /* n_dyn x 32 */, const uint8_t *d_dyn_points /* n_dyn x (32 | 160) */,
                                                  uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off /* m + 1 HOST offsets */, int32_t route, int out_fmt,
                                                  uint8_t *d_out /* m x (32 | 160) */, uint8_t *d_ok /* m, may be NULL */);
int32_t c25519_precomp_msm_vartime_mixed_rows(c25519_ctx *ctx, c25519_precomp *p, const uint8_t *static_scalars, uint64_t m, uint64_t w, const uint8_t *dyn_scalars,
                                              const uint8_t *dyn_points, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off, int32_t route, int out_fmt, uint8_t *out,
                                              uint8_t *ok);
/* how the mixed rows call treats m rows of w static scalars with these dynamic offsets: plan[0] the route C25519_PRECOMP_ROWS_AUTO takes,
 * plan[1] the waves of its row launches summed over the passes, plan[2] the passes, plan[3] the most dynamic terms in one pass.  Same
 * refusals and the same error as the call, as far as they depend on (m, w, dyn_off); n_dyn is dyn_off[m], read only once m is known to be
 * below 2^32 - 1.  Host arithmetic: no context, no GPU. */
int32_t c25519_precomp_msm_vartime_mixed_rows_plan(uint64_t m, uint64_t w, const uint64_t *dyn_off, uint64_t plan[4]);

/* The rows of the mixed rows call FOLDED into ONE multiscalar mul by a random linear combination: with a weight c_r per row, all on integers mod l,
 *   t_j = sum_r c_r * static_scalars[r][j]  (j < w),   d'_i = c_row(i) * dyn_scalars[i],   out = sum_j t_j * S_j + sum_i d'_i * dyn_points[i]
 * -- what a verifier runs on its common path: m verification equations hold iff (up to the weights' randomness) this ONE sum is the identity.
 * It is the fold of ed25519-dalek/src/batch.rs:207-233 (128-bit z_i, the scalars z_i * s_i and z_i * k_i mod l, one
 * VartimeMultiscalarMul::vartime_multiscalar_mul), offered for the equations of VartimePrecomputedMultiscalarMul::vartime_mixed_multiscalar_mul
 * (traits.rs:304-419, precomputed_straus.rs:29-127) instead of signatures only.  The per-row calls above stay what locates a bad row.
 *   - static_scalars m x w x 32, row-major; dyn_scalars n_dyn x 32; dyn_points n_dyn x 32 | 160 in in_fmt, the rows' terms one after the other;
 *     weights m x weight_bytes: HOST pointers in the un-suffixed form, DEVICE pointers (16-byte aligned) in the _dev form.  dyn_off is a HOST array
 *     of m + 1 offsets and out a HOST pointer (32 | 160 bytes) in BOTH forms, and both synchronise, as c25519_msm_vartime_dev does.
 *   - static scalars, dynamic scalars and 32-byte weights are ANY 32-byte little-endian integers: the products reduce them mod l, so -- unlike the
 *     sibling calls -- nothing is refused for bit 255; the scalars that reach the MSM are canonical by construction.  16-byte weights are 128-bit
 *     integers, the width of z_i in batch.rs.
 *   - p: the first w static points of the handle are used, w <= c25519_precomp_len(p); a handle of ANY size is accepted, because no comb table is
 *     involved (c25519_precomp_rows_table_bytes does not change).  p == NULL is allowed iff w == 0: the fold of c25519_msm_vartime_segments.
 *   - a row may have any number of dynamic terms (the rows end up in one MSM: C25519_MSM_SEGMENT_WAVE_MAX does not apply).
 *   - each of these returns -(hipErrorInvalidValue) before any launch: weight_bytes other than 16 or 32; out_fmt outside 0 .. 2; w above
 *     c25519_precomp_len (precomputed_straus.rs:86) or w != 0 without a handle; in_fmt and out_fmt of different groups (the pairing rule of
 *     c25519_msm_vartime_segments); dyn_off[0] != 0, a decreasing pair, dyn_off[m] != n_dyn, n_dyn not below 2^40; m not below 2^32 - 1; m * w
 *     overflowing.  m == 0 writes the identity.
 *   - the result in format 0 or 1 is byte for byte what c25519_precomp_msm_vartime returns for (t, d', dyn_points); a RAW160 output is the same
 *     point (equal under ct_eq), not the same limbs.  Returns C25519_NONE iff a dynamic point does not decode; out is then unspecified.
 * CAVEAT: reducing mod l changes the result by a small-order point when an Edwards input is not torsion-free -- the property of
 * ed25519_verify_batch (batch.rs:207-233 multiplies by z_i mod l as well).  The result is exact in the Ristretto group and for torsion-free
 * points.  The weights are the caller's randomness; the call is variable time, its scalars and weights are public by contract.
 * How: two small kernels of scalar arithmetic (28-bit limbs, l = 2^252 + c folded directly) -- the weighted column sums, lanes on consecutive
 * columns of a row and rows cut into slices so that about 512 blocks run whatever the shape (c25519_precomp_msm_vartime_mixed_rows_fold_plan),
 * and one lane per dynamic term -- then the MSM the library has: the static half over the handle's bucket table, the dynamic half through the
 * routed device-resident MSM (c25519_msm_partial_dev: small, mid or bucket path by n_dyn), added on the host.  c25519_phase_ms(ctx, 0, 0 | 1)
 * after the call: the column fold | the dynamic scaling.
 * Measured by tools/precomp_fold_numbers.py (profiles/precomp_fold_numbers.txt), device-resident, 16-byte weights, ms:
 * the call against c25519_precomp_msm_vartime_mixed_rows_dev on the same input and against the final MSM alone on pre-folded scalars:
 * 4096 rows of 130 + 17: 0.63 against 3.79 and 0.59 (the fold kernels 0.08); 256 of 2050 + 40: 0.45 against 6.68 and 0.44; 131072 of 2 + 1: 0.61
 * against 2.30 and 0.51; 2^20 of 1 + 2: 2.66 against 18.95 and 2.06 -- there 0.6 ms above the MSM alone, 0.29 of it the kernels, the rest the
 * upload of 8 MB of dyn_off; 64 of 2 + 1: 0.26 against 0.83 and 0.25.  The fold is the faster of the two calls from m = 1. */
int32_t c25519_precomp_msm_vartime_mixed_rows_fold_dev(c25519_ctx *ctx, const c25519_precomp *p, const uint8_t *d_static_scalars /* m x w x 32, row-major */, uint64_t m,
                                                       uint64_t w, const uint8_t *d_dyn_scalars /* n_dyn x 32 */, const uint8_t *d_dyn_points /* n_dyn x (32 | 160) */,
                                                       uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off /* m + 1 HOST offsets */,
                                                       const uint8_t *d_weights /* m x weight_bytes */, int32_t weight_bytes /* 16 | 32 */, int out_fmt,
                                                       uint8_t *out /* HOST, 32 | 160 */);
int32_t c25519_precomp_msm_vartime_mixed_rows_fold(c25519_ctx *ctx, const c25519_precomp *p, const uint8_t *static_scalars, uint64_t m, uint64_t w,
                                                   const uint8_t *dyn_scalars, const uint8_t *dyn_points, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off,
                                                   const uint8_t *weights, int32_t weight_bytes, int out_fmt, uint8_t *out);
/* the MSM the fold leaves behind and how the column fold is cut: plan[0] static terms of the final MSM (w), plan[1] its dynamic terms (dyn_off[m]),
 * plan[2] the row slices of the column fold, plan[3] the rows per slice (plan[2] * plan[3] >= m > (plan[2] - 1) * plan[3]).  Same refusals and the
 * same error as the call, as far as they depend on (m, w, dyn_off, weight_bytes); dyn_off[m] is read only once m is known to be below 2^32 - 1.
 * Host arithmetic: no context, no GPU. */
int32_t c25519_precomp_msm_vartime_mixed_rows_fold_plan(uint64_t m, uint64_t w, const uint64_t *dyn_off, int32_t weight_bytes, uint64_t plan[4]);

/* ---- regular-schedule multiscalar multiplication: MultiscalarMul::multiscalar_mul ------------------------
 * replaces backend::straus_multiscalar_mul (backend.rs:196 -> scalar_mul/straus.rs:103-144;
 * edwards.rs:966-1000).  One radix-16 fixed-window ladder per term (the schedule of variable_base.rs: identical
 * instruction stream for every input, every table lookup a full scan with selects, whatever the context's flags) and a
 * tree sum; staged scalars and per-lane tables are wiped.  HOST pointers; fmt as c25519_mul_batch. */
int32_t c25519_msm_consttime(c25519_ctx *ctx, const uint8_t *scalars, const uint8_t *points, uint64_t n, int in_fmt, int out_fmt, uint8_t *out);

/* ---- RistrettoPoint::double_and_compress_batch (ristretto.rs:564-648): out[i] = compress(2 * P_i) with one
 * shared inversion per lane-chunk.  in: n x 160 raw points; out: n x 32 CompressedRistretto. */
int32_t c25519_double_and_compress_batch_dev(c25519_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out);
int32_t c25519_double_and_compress_batch(c25519_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out);

/* ---- hash-to-group: points from bytes, one item per lane ----------------------------------------------------------------
 * Output formats: the Ristretto calls write C25519_FMT_RISTRETTO (n x 32) or C25519_FMT_RAW160 (n x 160, to feed
 * c25519_msm_vartime_dev / c25519_precomp_create without a round trip); the Edwards call writes C25519_FMT_EDWARDS_Y or
 * C25519_FMT_RAW160.  Any other out_fmt returns -(hipErrorInvalidValue).  n == 0 returns C25519_OK.
 * from_uniform_bytes and map_to_curve are constant-time in their inputs (selects only, no branch or address depends on a byte);
 * the hashing calls branch on message lengths only.
 * Messages as in ed25519_verify_batch: msgs concatenated, msg_off n+1 offsets; for the _dev forms msg_off must be
 * non-decreasing with msg_off[n] <= msgs_len, otherwise the call returns -(hipErrorInvalidValue) and no byte outside
 * [msgs, msgs + msgs_len) is read.  The hashing _dev forms synchronise the context's stream (they read that verdict back). */
/* RistrettoPoint::from_uniform_bytes (ristretto.rs:774): in: n x 64 bytes, two Elligator maps (ristretto/elligator.rs:15-52) and their sum. */
int32_t c25519_ristretto_from_uniform_bytes_batch_dev(c25519_ctx *ctx, const uint8_t *d_in64, uint64_t n, int out_fmt, uint8_t *d_out);
int32_t c25519_ristretto_from_uniform_bytes_batch(c25519_ctx *ctx, const uint8_t *in64, uint64_t n, int out_fmt, uint8_t *out);
/* RistrettoPoint::map_to_curve (ristretto/elligator.rs:62-68, RFC 9496 MAP): in: n x 32 bytes, bit 255 ignored, values >= p reduced. */
int32_t c25519_ristretto_map_to_curve_batch_dev(c25519_ctx *ctx, const uint8_t *d_in32, uint64_t n, int out_fmt, uint8_t *d_out);
int32_t c25519_ristretto_map_to_curve_batch(c25519_ctx *ctx, const uint8_t *in32, uint64_t n, int out_fmt, uint8_t *out);
/* RistrettoPoint::hash_from_bytes::<Sha512> (ristretto.rs:736-761): from_uniform_bytes(SHA-512(msg_i)). */
int32_t c25519_ristretto_hash_from_bytes_batch_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len, uint64_t n,
                                                   int out_fmt, uint8_t *d_out);
int32_t c25519_ristretto_hash_from_bytes_batch(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, int out_fmt, uint8_t *out);
/* EdwardsPoint::hash_to_curve::<Sha512> (mode C25519_H2C_RO, RFC 9380 edwards25519_XMD:SHA-512_ELL2_RO_) and
 * EdwardsPoint::encode_to_curve::<Sha512> (mode C25519_H2C_NU, ..._ELL2_NU_), edwards.rs:710-750: expand_message_xmd
 * (field.rs:440-490), hash_to_field (field.rs:397-428), Elligator 2 (montgomery.rs:276-363) and the map to edwards25519
 * (edwards.rs:651-690), the sum (RO), mul_by_cofactor.  dst: HOST pointer in both forms, ONE domain separator for the batch
 * (the reference's concatenated domain_sep), 1 .. 255 bytes, else C25519_DOMAIN_SEPARATOR_LENGTH. */
#define C25519_H2C_NU 0
#define C25519_H2C_RO 1
int32_t c25519_edwards_hash_to_curve_batch_dev(c25519_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msgs_len, uint64_t n,
                                               const uint8_t *dst, uint32_t dst_len, int mode, int out_fmt, uint8_t *d_out);
int32_t c25519_edwards_hash_to_curve_batch(c25519_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n,
                                           const uint8_t *dst, uint32_t dst_len, int mode, int out_fmt, uint8_t *out);

/* ---- Lizard (curve25519-dalek's `lizard` feature, D = Sha256): an injective 16-byte -> Ristretto encoding and its inverse ------
 * One item per lane, constant-time in the payload and the point (selects only).  in_fmt / out_fmt: C25519_FMT_RISTRETTO (n x 32)
 * or C25519_FMT_RAW160 (n x 160; a RAW160 input is trusted to be a point, as in the MSM, and is used as given: the slot order of
 * map_to_curve_inverse is that of this representative).  Any other format returns -(hipErrorInvalidValue); n == 0 returns C25519_OK. */
#define C25519_LIZARD_NONE 0          /* no unique Lizard preimage (lizard_decode returned None) */
#define C25519_LIZARD_OK 1
#define C25519_LIZARD_BAD_ENCODING 2  /* in_fmt RISTRETTO only: not a canonical Ristretto encoding */
/* RistrettoPoint::lizard_encode::<Sha256> (lizard/lizard_ristretto.rs:25-42): in n x 16 bytes, out n points. */
int32_t c25519_ristretto_lizard_encode_sha256_batch_dev(c25519_ctx *ctx, const uint8_t *d_data16, uint64_t n, int out_fmt, uint8_t *d_out);
int32_t c25519_ristretto_lizard_encode_sha256_batch(c25519_ctx *ctx, const uint8_t *data16, uint64_t n, int out_fmt, uint8_t *out);
/* RistrettoPoint::lizard_decode::<Sha256> (lizard/lizard_ristretto.rs:46-75), after CompressedRistretto::decompress for in_fmt RISTRETTO:
 * out16 n x 16 bytes (zero unless the status is C25519_LIZARD_OK), status n bytes C25519_LIZARD_*. */
int32_t c25519_ristretto_lizard_decode_sha256_batch_dev(c25519_ctx *ctx, const uint8_t *d_in, uint64_t n, int in_fmt, uint8_t *d_out16, uint8_t *d_status);
int32_t c25519_ristretto_lizard_decode_sha256_batch(c25519_ctx *ctx, const uint8_t *in, uint64_t n, int in_fmt, uint8_t *out16, uint8_t *status);
/* RistrettoPoint::map_to_curve_inverse (lizard/lizard_ristretto.rs:232-238): out512 n x 16 x 32 bytes, slot j of item i at
 * out512 + 512 i + 32 j (an undefined slot is all zero bytes); mask[i] bit j set when slot j is defined; ok[i] = 1 when the
 * encoding is valid (in_fmt RISTRETTO only: for RAW160 ok is not written and may be NULL). */
int32_t c25519_ristretto_map_to_curve_inverse_batch_dev(c25519_ctx *ctx, const uint8_t *d_in, uint64_t n, int in_fmt, uint8_t *d_out512, uint16_t *d_mask,
                                                        uint8_t *d_ok);
int32_t c25519_ristretto_map_to_curve_inverse_batch(c25519_ctx *ctx, const uint8_t *in, uint64_t n, int in_fmt, uint8_t *out512, uint16_t *mask, uint8_t *ok);

/* ---- MontgomeryPoint (montgomery.rs): the unclamped ladder, the fixed base and the map back to Edwards form ----------------------
 * One item per lane, constant-time in the scalar, the bits and the point (selects only).  u: n x 32 MontgomeryPoint bytes, decoded as
 * FieldElement::from_bytes (bit 255 ignored, values >= p accepted); out: n x 32 MontgomeryPoint bytes, the canonical u of the result,
 * all zero where the ladder ends at W = 0 (as_affine, montgomery.rs:409).  n == 0 returns C25519_OK. */
#define C25519_MONTGOMERY_MAX_BITS 512u
/* impl Mul<&Scalar> for &MontgomeryPoint (montgomery.rs:484-492): out[i] = u(k[i] * P_i) over bits 254..0 of k[i] as given -- no
 * clamping, no reduction; bit 255 is skipped, as bits_le().rev().skip(1) skips it.  k: n x 32. */
int32_t c25519_montgomery_mul_batch_dev(c25519_ctx *ctx, const uint8_t *d_k, const uint8_t *d_u, uint64_t n, uint8_t *d_out);
int32_t c25519_montgomery_mul_batch(c25519_ctx *ctx, const uint8_t *k, const uint8_t *u, uint64_t n, uint8_t *out);
/* MontgomeryPoint::mul_bits_be (montgomery.rs:183-211): the same ladder over nbits big-endian bits per item, packed MSB first into
 * ceil(nbits / 8) bytes (bits: n x ceil(nbits / 8); the padding bits of the last byte are ignored).  nbits is one value for the call,
 * 0 <= nbits <= C25519_MONTGOMERY_MAX_BITS, else -(hipErrorInvalidValue); nbits == 0 gives u = 0.  The running time depends on nbits only. */
int32_t c25519_montgomery_mul_bits_be_batch_dev(c25519_ctx *ctx, const uint8_t *d_bits, uint32_t nbits, const uint8_t *d_u, uint64_t n, uint8_t *d_out);
int32_t c25519_montgomery_mul_bits_be_batch(c25519_ctx *ctx, const uint8_t *bits, uint32_t nbits, const uint8_t *u, uint64_t n, uint8_t *out);
/* MontgomeryPoint::mul_base (montgomery.rs:144-146) = EdwardsPoint::mul_base(s).to_montgomery(), unclamped: the fixed-base kernels of
 * c25519_mul_base_batch (constant-time tables unless C25519_FLAG_VARTIME_TABLES) and the to_montgomery map.  scalars: n x 32. */
int32_t c25519_montgomery_mul_base_batch_dev(c25519_ctx *ctx, const uint8_t *d_scalars, uint64_t n, uint8_t *d_out);
int32_t c25519_montgomery_mul_base_batch(c25519_ctx *ctx, const uint8_t *scalars, uint64_t n, uint8_t *out);
/* MontgomeryPoint::to_edwards (montgomery.rs:239-268): y = (u - 1) / (u + 1), y_bytes[31] ^= signs[i] << 7 (in 8 bits: only bit 0 of
 * the sign counts), then CompressedEdwardsY::decompress.  signs: n bytes.  out_fmt C25519_FMT_EDWARDS_Y (n x 32, the compression of the
 * decompressed point: for u = 0 with sign 1 that is y without the sign bit) or C25519_FMT_RAW160 (n x 160); any other format returns
 * -(hipErrorInvalidValue).  status[i] = 1 for Some, 0 for None (u = -1, or u on the twist); a None item's output is all zero. */
int32_t c25519_montgomery_to_edwards_batch_dev(c25519_ctx *ctx, const uint8_t *d_u, const uint8_t *d_signs, uint64_t n, int out_fmt, uint8_t *d_out,
                                               uint8_t *d_status);
int32_t c25519_montgomery_to_edwards_batch(c25519_ctx *ctx, const uint8_t *u, const uint8_t *signs, uint64_t n, int out_fmt, uint8_t *out, uint8_t *status);

/* ---- the group law: add, sub, neg, mul_by_cofactor, eq / is_identity and segmented sums, one group per call --------------------
 * Formats: in_fmt / out_fmt must belong to one group -- in C25519_FMT_EDWARDS_Y -> out 0 or 2, in C25519_FMT_RISTRETTO -> out 1 or 2,
 * in C25519_FMT_RAW160 -> out 0, 1 or 2 (the group is the output's; RAW160 -> RAW160 is the same arithmetic in both groups).  Any
 * other pair returns -(hipErrorInvalidValue).  Compressed inputs are decoded as CompressedEdwardsY::decompress (ZIP-215) or
 * CompressedRistretto::decompress; a RAW160 input is trusted to be a point.  ok (may be NULL) is 1 where every input of the item decodes
 * (its output is unspecified otherwise), and the call returns C25519_NONE if any item fails to decode, as c25519_decompress_batch
 * does: the _dev forms with a compressed input synchronise the context's stream to read that verdict; with RAW160 input they do not.
 * n == 0 returns C25519_OK.  No branch and no address depends on point data. */
#define C25519_POINT_ADD 0
#define C25519_POINT_SUB 1
/* impl Add / Sub for EdwardsPoint (edwards.rs:808-835) and RistrettoPoint (ristretto.rs:852-880): out[i] = p[i] + q[i] (op
 * C25519_POINT_ADD) or p[i] - q[i] (C25519_POINT_SUB); p, q, out: n points each. */
int32_t c25519_point_add_batch_dev(c25519_ctx *ctx, const uint8_t *d_p, const uint8_t *d_q, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *d_out,
                                   uint8_t *d_ok);
int32_t c25519_point_add_batch(c25519_ctx *ctx, const uint8_t *p, const uint8_t *q, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *out, uint8_t *ok);
#define C25519_POINT_NEG 0
#define C25519_POINT_MUL_BY_COFACTOR 1      /* Edwards only: rejected when either format is C25519_FMT_RISTRETTO */
/* impl Neg (edwards.rs:853-875, ristretto.rs:897-907) and EdwardsPoint::mul_by_cofactor (edwards.rs:1365): out[i] = -p[i] or [8] p[i]. */
int32_t c25519_point_map_batch_dev(c25519_ctx *ctx, const uint8_t *d_p, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *d_out, uint8_t *d_ok);
int32_t c25519_point_map_batch(c25519_ctx *ctx, const uint8_t *p, uint64_t n, int op, int in_fmt, int out_fmt, uint8_t *out, uint8_t *ok);
/* eq[i] = 1 iff p[i] == q[i] in `group` (C25519_FMT_EDWARDS_Y: projective equality, ConstantTimeEq edwards.rs:501-512;
 * C25519_FMT_RISTRETTO: X1*Y2 == Y1*X2 || X1*X2 == Y1*Y2, ristretto.rs:815-830).  q == NULL compares with the identity
 * (is_identity, traits.rs:45 / ristretto.rs:1197).  A compressed in_fmt must equal group; RAW160 takes either group.  Points are compared
 * decoded, never as bytes; eq[i] = 0 where ok[i] = 0. */
int32_t c25519_point_eq_batch_dev(c25519_ctx *ctx, const uint8_t *d_p, const uint8_t *d_q, uint64_t n, int in_fmt, int group, uint8_t *d_eq, uint8_t *d_ok);
int32_t c25519_point_eq_batch(c25519_ctx *ctx, const uint8_t *p, const uint8_t *q, uint64_t n, int in_fmt, int group, uint8_t *eq, uint8_t *ok);
/* sums[s] = sum of points[seg_off[s] .. seg_off[s+1]) for s < m (impl Sum, edwards.rs:837-851, ristretto.rs:882-895).  seg_off: m + 1
 * non-decreasing u64 with seg_off[0] = 0 and seg_off[m] = n; an empty segment sums to the identity; ok[s] = 0 if a point of segment s
 * does not decode.  m must be below 2^32 - 1; m == 0 returns C25519_OK.  The host form checks the offsets (-(hipErrorInvalidValue)
 * otherwise); the _dev form takes d_seg_off on the device and TRUSTS it (it never copies the offsets to the host): offsets that break
 * the rule give unspecified sums, but no access outside the arrays.  Control flow depends on the offsets only. */
int32_t c25519_point_sum_segments_dev(c25519_ctx *ctx, const uint8_t *d_points, uint64_t n, int in_fmt, const uint64_t *d_seg_off, uint64_t m, int out_fmt,
                                      uint8_t *d_sums, uint8_t *d_ok);
int32_t c25519_point_sum_segments(c25519_ctx *ctx, const uint8_t *points, uint64_t n, int in_fmt, const uint64_t *seg_off, uint64_t m, int out_fmt,
                                  uint8_t *sums, uint8_t *ok);

/* ---- Scalar::invert_batch_alloc (scalar.rs:802-856): io[i] <- 1/io[i] mod l in place (HOST pointer; all inputs
 * must be canonical and non-zero, as in the reference); prod_inv (32 bytes, may be NULL) receives the product of
 * all inverses, the reference's return value. */
int32_t c25519_scalar_invert_batch(c25519_ctx *ctx, uint8_t *io, uint64_t n, uint8_t *prod_inv);

/* ---- diagnostics ----------------------------------------------------------------------------------
 * Integer-multiplier roofline probes: runs a dependent-free chain microbenchmark and
 * returns giga-operations per second.  which: 0 v_mad_u64_u32, 1 fe_mul (radix 2^25.5, this
 * engine), 2 fe_sq, 3 fe_mul written on 5 x u64 limbs with unsigned __int128 products (the
 * reference's literal layout, for the A/B in DESIGN.md), 4 v_add_u32, 5 v_mul_lo_u32. */
double c25519_microbench(c25519_ctx *ctx, int which, int iters);
/* Device field self-test: runs ONE field operation per element on the GPU, in the translation unit built with the
 * chained-carry multiplication (chain = 1: kernels.hip) or the ten-column one (chain = 0), and returns canonical bytes
 * (field.rs:368-450 to_bytes).  a_limbs / b_limbs: n x 10 u32 limbs at bit positions 0,26,51,...,230 (HOST pointers;
 * any magnitudes the operation's bound class admits, csrc/fe26.h); out: n x 32.  op: 0 a*b (a wide, b loose), 1 a^2
 * (loose), 2 1/a, 3 canonical encoding of a (wide), 4 a^((p-5)/8), 5 a-b (both loose), 6 weak reduction of a,
 * 7 (a-b)*(a+b) (both tight); 8-11 the lockstep multiplier of the bucket accumulation (csrc/fe26x.h; a wide, b loose):
 * 8 a*b and 9 b^2 out of one group of three products, 10 a*b and 11 b^2 out of one group of four; 12, 13 a*b out of the
 * first / the second slot of a lockstep pair (csrc/mid_long.h); 14 b[0] ? -a : a (a tight; b[0] = 0 or ~0: fe_cond_neg),
 * 15 a+b (both loose, fe_add_w), 16 2a+b (both tight, fe_add_lt).  Pins the device code generation against big integers
 * (field.rs:552-642). */
int32_t c25519_selftest_field(c25519_ctx *ctx, int op, int chain, const uint32_t *a_limbs, const uint32_t *b_limbs, uint64_t n, uint8_t *out);
/* Device point self-test: ONE point formula of csrc/ge26.h / fe26x.h / mid_long.h per row on the GPU, in either translation-unit
 * flavour (chain as above), on raw limbs: p_limbs n x 40 u32 = X Y Z T, q_limbs n x 40 u32 (the second operand in the form the op
 * names; may be NULL), aux n u32 (sign / flip / count; may be NULL) -- HOST pointers, tight limbs (csrc/fe26.h); out: n x 128 =
 * the canonical encodings of X Y Z T.  op: 0 2p; 1 2^aux p (aux 1..8); 2 p +- q through aniels_words_cneg + ge_madd (q = 24
 * canonical words y+x, y-x, 2dxy); 3 / 4 ge_madd_signed_p3 and its lockstep form (q = y+x, y-x, 2dxy limbs; aux & 1: subtract);
 * 5 / 6 ge_madd_lazy_p3 and its lockstep form (aux != 0: p changes sides first); 7 ge_from_aniels_signed; 8 p +- q through
 * ge_cached_cneg + ge_add_cached (q a point); 9 ge_add; 10 / 11 the signed and the lazy lockstep addition of a projective Niels
 * record (q = Y+X, Y-X, Z, 2dT); 12 sixteen lazy lockstep additions of q with the signs in bits 0..15 of aux, then the sign
 * resolution, as the bucket accumulation chains them; 13 -p; 14 byte 0 = ge_eq(p,q) | ge_is_identity(p) << 1 | ris_eq(p,q) << 2.
 * Compared coordinate by coordinate with big-integer formulas (curve_models.rs:365-494, edwards.rs:528-535, 1370-1380) by
 * tests/test_gpu_point.py. */
int32_t c25519_selftest_point(c25519_ctx *ctx, int op, int chain, const uint32_t *p_limbs /* n x 40: X Y Z T */, const uint32_t *q_limbs /* n x 40, may be NULL */,
                              const uint32_t *aux /* n, may be NULL */, uint64_t n, uint8_t *out /* n x 128: canonical X Y Z T */);
/* The same for the device SCALAR arithmetic mod l (csrc/sc28.h: ten 28-bit limbs, reduction by folding with l = 2^252 + c),
 * which replaces Scalar52 (u64/scalar.rs:66-320) inside the verify_batch / sign / per-signature-verify kernels.
 * a_words / b_words: n x 16 u32 per operand (HOST pointers; b may be NULL for the unary ops); out: n x 32 bytes.
 * op 0 from_bytes_mod_order_wide(a: 16 words) (scalar.rs:248, u64/scalar.rs:89-118); 1 a*b mod l, a = 5 and b = 10 raw 28-bit
 * limbs with a*b < 2^393 (z_i * s_i, z_i * h_i: batch.rs:225-233); 2 a*b mod l, 10 x 10 raw limbs with a*b < 2^512 (u64/scalar.rs:302;
 * signing.rs:899 k*a with the clamped a); 3 a+b and 4 -a on canonical operands (8 words each; u64/scalar.rs:161-207);
 * 5 out[0] = (a < l), the word-wise test behind from_canonical_bytes (scalar.rs:259-263); 6 words -> limbs -> words of a < 2^256;
 * 7 r + k*a as the signer chains them: k = a mod l (16 words), a = b[0..8] (unreduced, < 2^256), r = b[8..16] (canonical). */
int32_t c25519_selftest_scalar(c25519_ctx *ctx, int op, const uint32_t *a_words, const uint32_t *b_words, uint64_t n, uint8_t *out);
/* A read-only window on the device workspaces of a context and of its peer context, for tests/test_gpu_wipe.py: what a call on secrets leaves behind.
 * count: how many there are (every devbuf of the context, its flag words and its result slots; then the same of the peer, if one exists -- the list is
 * csrc/ctx.h ctx_workspaces, which c25519_ctx_trim and c25519_ctx_destroy share).  info: *name ("tmp_a", "peer.tmp_a", ...; valid until the next info call)
 * and *cap, the bytes allocated (0: not yet).  read: bytes [off, off + bytes) of workspace `which` into the HOST buffer out, after every stream of the
 * context and its peer has drained.  zero: the only write -- every workspace set to zero over its whole capacity; synchronises. */
int32_t c25519_debug_workspace_count(c25519_ctx *ctx);
int32_t c25519_debug_workspace_info(c25519_ctx *ctx, int which, const char **name, uint64_t *cap);
int32_t c25519_debug_workspace_read(c25519_ctx *ctx, int which, uint64_t off, uint64_t bytes, uint8_t *out);
int32_t c25519_debug_workspace_zero(c25519_ctx *ctx);
/* The window layout the MSM uses for n terms of RAW points (host arithmetic, no GPU needed; encoded inputs of 4096 .. 6143 terms and verify_batch choose widths of
 * their own -- every record carries the width it was made with): window k covers bits
 * [pos[k], pos[k] + wid[k]) of s' = s + addk (addk as 8 little-endian 32-bit words); all windows but the last two are
 * signed (digit = slice - 2^(wid-1)).  pos / wid need room for 56 entries.  Used by the CPU tests to check that the
 * digits always recompose the scalar. */
int32_t c25519_msm_geometry(uint64_t n, int32_t *c, int32_t *nwin, uint8_t *pos, uint8_t *wid, uint32_t *addk);
/* Which path serves a call (host arithmetic: no context, no GPU; the call itself routes with the same code).  kind 0: c25519_msm_vartime[_dev] over n points
 * of format in_fmt; kind 1: ed25519_verify_batch[_dev] of n signatures in the device z-mode (in_fmt is ignored).  host_pointers: the host-pointer entry
 * point; for kind 1 it only decides, by 2n + 1 > 32769 terms, whether the arrays go up pass by pass (then nothing is published) -- message lengths are not
 * looked at, and the host-pointer call's own route for at most 128 signatures (small path, published) is not reported here.  A first attempt on a
 * context whose peer context exists (two stream sets).
 * route[0] path: 0 nothing to do (n = 0), 1 small (csrc/small.hip), 2 mid (csrc/mid.hip), 3 the bucket pipeline; [1] window width; [2] passes; [3] terms
 * (kind 1: signatures) per pass; [4] 1 = the path's last kernel publishes the record to the host itself; [5] 1 = encoded points: records are made first;
 * [6] the term count the window layout is derived from. */
int32_t c25519_msm_route(int32_t kind, uint64_t n, int32_t in_fmt, int32_t host_pointers, int64_t route[7]);

#ifdef __cplusplus
}
#endif
#endif
