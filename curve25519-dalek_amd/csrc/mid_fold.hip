// MANY mixed multiscalar equations over ONE precomputed point set folded into ONE multiscalar multiplication by a random linear combination:
//   out = sum_{j < w} t_j * S_j + sum_i d'_i * P_i,   t_j = sum_r c_r * s[r][j] mod l,   d'_i = c_row(i) * d_i mod l
// -- the check a verifier runs on its common path (ed25519-dalek/src/batch.rs:207-233: 128-bit z_i, the scalars z_i * s_i and z_i * k_i mod l,
// one vartime_multiscalar_mul), for the rows of c25519_precomp_msm_vartime_mixed_rows.  DESIGN.md section 3.17.
//
//   c25519_precomp_msm_vartime_mixed_rows_fold_dev / c25519_precomp_msm_vartime_mixed_rows_fold / c25519_precomp_msm_vartime_mixed_rows_fold_plan
//
// The GPU work that is new here is scalar arithmetic (fold.h, on sc28.h); the one MSM it leaves behind runs through what the library has: the
// static half over the handle's bucket table (msm_merged_core), the dynamic half through the routed device-resident MSM
// (c25519_msm_partial_dev: small, mid or bucket path by n_dyn), the two sums added on the host as c25519_precomp_msm_vartime adds them.
//   k_mid_fold_part<W>   the column sums of the m x w scalar matrix, weighted.  A block of 256 lanes is a tile of tc columns (a power of two,
//                        at most 64) times 256 / tc row phases: lane (phase, col) walks rows phase, phase + ph, ... of the block's row slice, so
//                        that the lanes of one phase read consecutive 32-byte scalars of one row and share that row's weight; the phases are
//                        added through LDS (eight halving steps at most) and phase 0 stores the slice's partial t.  Grid: column tiles x row
//                        slices (fold_geom: about FOLD_BLOCKS blocks whatever the shape; m never reaches a grid dimension).
//   k_mid_fold_finish    the same tile over the SLICES of the partial sums, additions only -> t (not launched when there is one slice: the
//                        part kernel wrote t itself)
//   k_mid_fold_dyn<W>    one lane per dynamic term: its row by a binary search of the uploaded offsets (the last row whose offset is not above
//                        the term: empty rows and runs of equal offsets resolve to the owner), then one product
// <W>: 0 = 16-byte weights, 1 = 32-byte weights.  Sums mod l are exact in any order: there is no ordering machinery, no atomics, no waiting.
// Variable time: weights and scalars are public by contract (a *_vartime entry point).  Every index comes from the m, w and offsets the host
// validated.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include "msm_internal.h"
#include "devio.h"
#include "ctx.h"
#include "precomp.h"
#include "capi_util.h"
#include "ffi.h"
#include "fold.h"

using namespace c25519;

namespace c25519 {

// The phases of a block -> phase 0.  Lane t = phase * tc + col holds acc; sh: 256 x 8 words.  Every lane of the block calls it.
__device__ __forceinline__ sc28 fold_block_sum(sc28 acc, u32 t, u32 tc, u32 ph, u32 *sh) {
    const u32 phase = t / tc;
#pragma unroll 1
    for (u32 s = ph >> 1; s > 0; s >>= 1) {
        __syncthreads();                                    // (the readers of the previous step are done with sh)
        if (phase >= s && phase < 2 * s) {
            u32 w[8];
            sc28_to_words(acc, w);
            for (int q = 0; q < 8; q++) sh[t * 8 + q] = w[q];
        }
        __syncthreads();
        if (phase < s) {
            u32 w[8];
            for (int q = 0; q < 8; q++) w[q] = sh[(t + s * tc) * 8 + q];
            acc = fold_combine(acc, sc28_from_words(w));
        }
    }
    return acc;
}

template <int WB>
__device__ __forceinline__ fold_weight<WB> fold_weight_load(const uint8_t *__restrict__ wts, u64 r) {
    u32 w[8];
    if constexpr (WB == 16) {
        const uint4 a = reinterpret_cast<const uint4 *>(wts)[r];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    } else load8(wts, r, w);
    return fold_weight_from_words<WB>(w);
}

// Block (x, y): columns [x * tc, x * tc + tc) of rows [y * rows, min(m, y * rows + rows)) -> part[y][col] (32 canonical bytes each), tc = 1 << lg_tc.
// ss: m x w x 32, row-major; wts: m weights.  A lane whose column is past w carries zero through the block sum and stores nothing.
template <int W>
__global__ void __launch_bounds__(256) k_mid_fold_part(const uint8_t *__restrict__ ss, const uint8_t *__restrict__ wts, u32 m, u64 w, u32 lg_tc, u32 rows,
                                                       uint8_t *__restrict__ part) {
    constexpr int WB = W ? 32 : 16;
    __shared__ u32 sh[256 * 8];
    const u32 t = threadIdx.x, tc = 1u << lg_tc, ph = 256u >> lg_tc, phase = t >> lg_tc;
    const u64 col = (u64)blockIdx.x * tc + (t & (tc - 1u));
    const u64 r_lo = (u64)blockIdx.y * rows, r_hi = r_lo + rows < (u64)m ? r_lo + rows : (u64)m;
    sc28 acc = sc28_zero();
    if (col < w) {
#pragma unroll 1
        for (u64 r = r_lo + phase; r < r_hi; r += ph) {
            const fold_weight<WB> c = fold_weight_load<WB>(wts, r);
            u32 s[8];
            load8(ss, r * w + col, s);
            acc = fold_step<WB>(acc, c, s);
        }
    }
    acc = fold_block_sum(acc, t, tc, ph, sh);
    if (phase == 0 && col < w) {
        u32 o[8];
        sc28_to_words(acc, o);
        store8(part, (u64)blockIdx.y * w + col, o);
    }
}

// Block x: columns [x * tc, x * tc + tc) of the `slices` partial sums (slices x w x 32 canonical bytes) -> t (w x 32)
__global__ void __launch_bounds__(256) k_mid_fold_finish(const uint8_t *__restrict__ part, u32 slices, u64 w, u32 lg_tc, uint8_t *__restrict__ tsum) {
    __shared__ u32 sh[256 * 8];
    const u32 t = threadIdx.x, tc = 1u << lg_tc, ph = 256u >> lg_tc, phase = t >> lg_tc;
    const u64 col = (u64)blockIdx.x * tc + (t & (tc - 1u));
    sc28 acc = sc28_zero();
    if (col < w) {
#pragma unroll 1
        for (u32 y = phase; y < slices; y += ph) {
            u32 s[8];
            load8(part, (u64)y * w + col, s);
            acc = fold_combine(acc, sc28_from_words(s));
        }
    }
    acc = fold_block_sum(acc, t, tc, ph, sh);
    if (phase == 0 && col < w) {
        u32 o[8];
        sc28_to_words(acc, o);
        store8(tsum, col, o);
    }
}

// Lane i (grid-stride): out[i] = weight of the row that owns dynamic term i * ds[i] mod l.  off: m + 1 offsets, off[0] = 0, off[m] = n, non-decreasing, m >= 1.
template <int W>
__global__ void __launch_bounds__(256) k_mid_fold_dyn(const u64 *__restrict__ off, u32 m, const uint8_t *__restrict__ wts, const uint8_t *__restrict__ ds, u64 n,
                                                      uint8_t *__restrict__ out) {
    constexpr int WB = W ? 32 : 16;
    const u64 stride = (u64)gridDim.x * blockDim.x;
#pragma unroll 1
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        u32 lo = 0, hi = m;                                 // off[lo] <= i < off[hi]
        while (hi - lo > 1) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if (off[mid] <= i) lo = mid; else hi = mid;
        }
        const fold_weight<WB> c = fold_weight_load<WB>(wts, lo);
        u32 s[8], o[8];
        load8(ds, i, s);
        sc28_to_words(fold_scale<WB>(c, s), o);
        store8(out, i, o);
    }
}

}  // namespace c25519

// ---- host side ----------------------------------------------------------------------------------------------------------------
// The geometry of the column fold, from (m, w) alone: the tile is the smallest power of two of columns that holds w, at most 64 (a wave's
// width: wider rows take more tiles); the rows are cut into slices so that tiles x slices is about FOLD_BLOCKS blocks (two per CU), but no
// slice has fewer than four rows per phase -- below that the block sum costs more than the rows.
constexpr uint64_t FOLD_BLOCKS = 512;
struct fold_geom { uint32_t lg_tc = 0, tc = 1, ph = 256; uint64_t tiles = 0, slices = 0, rows = 0; };
static fold_geom fold_geometry(uint64_t m, uint64_t w) {
    fold_geom g;
    while (g.tc < 64 && g.tc < w) { g.tc <<= 1; g.lg_tc++; }
    g.ph = 256u >> g.lg_tc;
    g.tiles = (w + g.tc - 1) / g.tc;
    const uint64_t max_slices = std::max<uint64_t>(1, FOLD_BLOCKS / std::max<uint64_t>(1, g.tiles));
    g.rows = std::max<uint64_t>(4ull * g.ph, (m + max_slices - 1) / max_slices);
    g.slices = (m + g.rows - 1) / g.rows;
    return g;
}

static const off_msgs FOLD_OFF_MSGS = OFF_MSGS("precomp_msm_vartime_mixed_rows_fold", "dyn_off", "n_dyn", nullptr);
// what depends on (m, w, n_dyn, dyn_off, weight_bytes): the refusals the call and the plan share
static int32_t fold_check_shape(c25519_ctx *ctx, uint64_t m, uint64_t w, uint64_t n_dyn, const uint64_t *dyn_off, int32_t weight_bytes) {
    if (weight_bytes != 16 && weight_bytes != 32) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows_fold: weight_bytes must be 16 or 32");
    int32_t q;
    if ((q = check_offsets(ctx, FOLD_OFF_MSGS, n_dyn, dyn_off, m))) return q;
    if (w && m > UINT64_MAX / w) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows_fold: m * w overflows");
    return C25519_OK;
}

EXPORT int32_t c25519_precomp_msm_vartime_mixed_rows_fold_plan(uint64_t m, uint64_t w, const uint64_t *dyn_off, int32_t weight_bytes, uint64_t plan[4]) {
    const uint64_t n_dyn = offsets_end(dyn_off, m);
    const int32_t r = fold_check_shape(nullptr, m, w, n_dyn, dyn_off, weight_bytes);
    if (r) return r;
    const fold_geom g = fold_geometry(m, w);
    plan[0] = m ? w : 0; plan[1] = m ? n_dyn : 0; plan[2] = g.slices; plan[3] = g.rows;
    return C25519_OK;
}

// everything that is refused before any launch
static int32_t fold_check(c25519_ctx *ctx, const c25519_precomp *p, uint64_t m, uint64_t w, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off, int32_t weight_bytes,
                          int out_fmt) {
    if (out_fmt < 0 || out_fmt > 2) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows_fold: bad out_fmt");
    if (!p && w) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows_fold: static scalars need a handle");
    if (p && w > p->n) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows_fold: more static scalars per row than static points (precomputed_straus.rs:86)");
    if (!fmt_pair_ok(in_fmt, out_fmt)) return bad_arg(ctx, "precomp_msm_vartime_mixed_rows_fold: in_fmt and out_fmt must belong to one group");
    return fold_check_shape(ctx, m, w, n_dyn, dyn_off, weight_bytes);
}

// The fold's own entry of the phase ring (c25519_phase_ms: phase 0 the column fold, phase 1 the dynamic scaling) is taken before the MSMs run;
// a bucket-path MSM takes entries of its own behind it.  The fold's three events move to a fresh latest entry then, and the one they leave
// is marked as a pass without events (it answers -1), so that back = 0 is this call's fold whatever path the MSM took.
static void fold_ring_last(c25519_ctx *ctx, uint64_t call) {
    if (ctx->ncalls == call + 1) return;
    const int from = (int)(call % c25519_ctx::RING);
    hipEvent_t *mine = ctx->ring[from], *last = ctx_ring_item(ctx);
    if (last == mine) return;                               // (the ring went round: the entry is gone)
    for (int e = 0; e < 3; e++) std::swap(mine[e], last[e]);
    ctx->ring_kind[from] = 4;
}

// The whole call on device inputs; the arguments have been checked (fold_check) and m > 0.
static int32_t fold_run(c25519_ctx *ctx, const c25519_precomp *p, const uint8_t *d_ss, uint64_t m, uint64_t w, const uint8_t *d_ds, const uint8_t *d_dp, uint64_t n_dyn,
                        int in_fmt, const uint64_t *dyn_off, const uint8_t *d_wts, int32_t weight_bytes, int out_fmt, uint8_t *out) {
    hipStream_t st = ctx->stream;
    const fold_geom g = fold_geometry(m, w);
    // tmp_f: dyn_off (m + 1) | partial column sums (slices x w; none with one slice) | t (w) | d' (n_dyn); none of the MSM paths touches tmp_f
    ws_layout F;
    const size_t o_off = F.part((m + 1) * 8), o_part = F.part(g.slices > 1 ? g.slices * w * 32 : 0), o_t = F.part(w * 32), o_d = F.part(n_dyn * 32);
    int32_t r;
    if ((r = F.reserve(ctx, ctx->tmp_f, 256))) return r;
    uint8_t *d_part = F.at(o_part), *d_t = F.at(o_t), *d_dd = F.at(o_d);
    uint64_t *d_off = F.at<uint64_t>(o_off);
    const uint64_t call = ctx->ncalls;
    hipEvent_t *ring = ctx_ring_item(ctx);
    ctx->last_passes.clear();
    HIPCHK(hipEventRecord(ring[0], st));
    if (w) {
        ctx->kname[0] = "c25519::k_mid_fold_part (weighted column sums of the static scalar matrix mod l: lanes on columns, row phases added through LDS)";
        const dim3 grid((unsigned)g.tiles, (unsigned)g.slices);
        uint8_t *dst = g.slices > 1 ? d_part : d_t;
        if (weight_bytes == 16) hipLaunchKernelGGL(k_mid_fold_part<0>, grid, dim3(256), 0, st, d_ss, d_wts, (u32)m, w, g.lg_tc, (u32)g.rows, dst);
        else hipLaunchKernelGGL(k_mid_fold_part<1>, grid, dim3(256), 0, st, d_ss, d_wts, (u32)m, w, g.lg_tc, (u32)g.rows, dst);
        HIPCHK(hipGetLastError());
        if (g.slices > 1) {
            hipLaunchKernelGGL(k_mid_fold_finish, dim3((unsigned)g.tiles), dim3(256), 0, st, (const uint8_t *)d_part, (u32)g.slices, w, g.lg_tc, d_t);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipEventRecord(ring[1], st));
    if (n_dyn) {
        HIPCHK(hipMemcpyAsync(d_off, dyn_off, (m + 1) * 8, hipMemcpyHostToDevice, st));
        const dim3 grid((unsigned)std::min<uint64_t>((n_dyn + 255) / 256, 1u << 20));
        if (weight_bytes == 16) hipLaunchKernelGGL(k_mid_fold_dyn<0>, grid, dim3(256), 0, st, (const u64 *)d_off, (u32)m, d_wts, d_ds, n_dyn, d_dd);
        else hipLaunchKernelGGL(k_mid_fold_dyn<1>, grid, dim3(256), 0, st, (const u64 *)d_off, (u32)m, d_wts, d_ds, n_dyn, d_dd);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ring[2], st));
    // the one MSM over (t, d'): both halves synchronise the stream (the dynamic one after the upload of dyn_off has read the caller's array)
    ge_p3 R = ge_identity();
    if (w && (r = msm_merged_core(ctx, d_t, w, p->m, p->d_table, R))) { (void)hipStreamSynchronize(st); return r; }
    if (n_dyn) {
        uint8_t raw[160];
        if ((r = c25519_msm_partial_dev(ctx, d_dd, d_dp, n_dyn, in_fmt, raw))) { (void)hipStreamSynchronize(st); return r; }      // (C25519_NONE: a dynamic point does not decode)
        const ge_p3 Rd = host_from_raw160(raw);
        R = w ? ge_add(R, Rd) : Rd;
    }
    if (!w && !n_dyn) HIPCHK(hipStreamSynchronize(st));      // (rows without any term: the identity, and the host form's uploads are through)
    fold_ring_last(ctx, call);
    host_encode(R, out_fmt, out);
    return C25519_OK;
}

EXPORT int32_t c25519_precomp_msm_vartime_mixed_rows_fold_dev(c25519_ctx *ctx, const c25519_precomp *p, const uint8_t *d_static_scalars, uint64_t m, uint64_t w,
                                                              const uint8_t *d_dyn_scalars, const uint8_t *d_dyn_points, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off,
                                                              const uint8_t *d_weights, int32_t weight_bytes, int out_fmt, uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = fold_check(ctx, p, m, w, n_dyn, in_fmt, dyn_off, weight_bytes, out_fmt))) return r;
    if (m == 0) { host_encode(ge_identity(), out_fmt, out); return C25519_OK; }
    return fold_run(ctx, p, d_static_scalars, m, w, d_dyn_scalars, d_dyn_points, n_dyn, in_fmt, dyn_off, d_weights, weight_bytes, out_fmt, out);
}

EXPORT int32_t c25519_precomp_msm_vartime_mixed_rows_fold(c25519_ctx *ctx, const c25519_precomp *p, const uint8_t *static_scalars, uint64_t m, uint64_t w,
                                                          const uint8_t *dyn_scalars, const uint8_t *dyn_points, uint64_t n_dyn, int in_fmt, const uint64_t *dyn_off,
                                                          const uint8_t *weights, int32_t weight_bytes, int out_fmt, uint8_t *out) {
    HIPCHK(hipSetDevice(ctx->device));
    int32_t r;
    if ((r = fold_check(ctx, p, m, w, n_dyn, in_fmt, dyn_off, weight_bytes, out_fmt))) return r;
    if (m == 0) { host_encode(ge_identity(), out_fmt, out); return C25519_OK; }
    // tmp_a: static scalars | weights; tmp_b: dynamic scalars; tmp_c: dynamic points (the staging buffers of a host form; the MSM keeps to its own)
    const size_t pb = point_bytes(in_fmt), wb = (size_t)m * (size_t)weight_bytes;
    ws_layout A; A.part((size_t)(m * w) * 32);              // (the weights are the tail: not rounded, and 16 bytes behind it)
    if ((r = A.reserve(ctx, ctx->tmp_a, wb + 16)) || (r = ctx_reserve(ctx, ctx->tmp_b, n_dyn * 32 + 16)) || (r = ctx_reserve(ctx, ctx->tmp_c, n_dyn * pb + 16))) return r;
    ffi_small_begin(ctx);
    uint8_t *d_ss = A.at(0), *d_wts = A.at(A.bytes()), *d_ds = (uint8_t *)ctx->tmp_b.p, *d_dp = (uint8_t *)ctx->tmp_c.p;
    const struct { void *dst; const void *src; size_t bytes; } ups[4] = {{d_ss, static_scalars, (size_t)(m * w) * 32}, {d_wts, weights, wb}, {d_ds, dyn_scalars, n_dyn * 32},
                                                                         {d_dp, dyn_points, n_dyn * pb}};
    for (const auto &u : ups) {
        if (!u.bytes) continue;
        const hipError_t e = hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return c25519_fail(ctx, e, "hipMemcpyAsync(inputs)"); }
    }
    r = fold_run(ctx, p, d_ss, m, w, d_ds, d_dp, n_dyn, in_fmt, dyn_off, d_wts, weight_bytes, out_fmt, out);
    if (r < 0) (void)hipStreamSynchronize(ctx->stream);    // (an early error: the uploads may still be reading the caller's memory)
    ffi_small_end(ctx, (size_t)(m * w) * 32 + wb + n_dyn * (32 + pb) + (n_dyn ? (m + 1) * 8 : 0), 0);
    return r;
}
