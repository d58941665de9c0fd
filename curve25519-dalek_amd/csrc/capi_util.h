// Host-side plumbing of the extern "C" entry points (internal to libc25519hip.so): the export macro, the HIP status check,
// argument errors and the point-format helpers every entry-point file uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/c25519_hip.h"
#include "ctx.h"

#define EXPORT extern "C" __attribute__((visibility("default")))
#define HIPCHK(call)                                                \
    do {                                                            \
        hipError_t _e = (call);                                     \
        if (_e != hipSuccess) return c25519_fail(ctx, _e, #call);   \
    } while (0)

static inline unsigned div_up(uint64_t a, uint64_t b) { return (unsigned)((a + b - 1) / b); }
static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }       // the parts of a carved workspace
// The parts of ONE devbuf: each a multiple of 256 bytes, one behind the other in the order they are declared.  Declare every part, reserve
// once, then ask for typed pointers.
struct ws_layout {
    size_t off = 0;
    uint8_t *base = nullptr;
    size_t part(size_t bytes) { const size_t o = off; off += al256(bytes); return o; }      // -> its offset; a part of 0 bytes takes nothing
    size_t bytes(size_t slack = 0) const { return off + slack; }
    void bind(void *p) { base = (uint8_t *)p; }                                              // over memory that is reserved already
    int32_t reserve(c25519_ctx *ctx, devbuf &b, size_t slack = 0) { const int32_t r = ctx_reserve(ctx, b, bytes(slack)); bind(b.p); return r; }
    template <class T = uint8_t> T *at(size_t o) const { return (T *)(base + o); }
};

// a rejected argument: the message for c25519_last_error and the status every entry point returns for it.  (ctx may be null: the *_plan
// exports have none, and then only the status is returned)
static inline int32_t bad_arg(c25519_ctx *ctx, const char *what) { if (ctx) ctx->err = what; return -(int32_t)hipErrorInvalidValue; }

static inline size_t point_bytes(int fmt) { return fmt == C25519_FMT_RAW160 ? 160 : 32; }
static inline bool ris_fmt_ok(int fmt) { return fmt == C25519_FMT_RISTRETTO || fmt == C25519_FMT_RAW160; }
static inline bool ed_fmt_ok(int fmt) { return fmt == C25519_FMT_EDWARDS_Y || fmt == C25519_FMT_RAW160; }
// the format rule of a call that takes points of one group and returns points of the same: Edwards in (0) -> 0 or 2, Ristretto in (1) -> 1 or 2,
// RAW160 in (2) -> anything
static inline bool fmt_pair_ok(int in_fmt, int out_fmt) {
    if (in_fmt == C25519_FMT_EDWARDS_Y) return ed_fmt_ok(out_fmt);
    if (in_fmt == C25519_FMT_RISTRETTO) return ris_fmt_ok(out_fmt);
    return in_fmt == C25519_FMT_RAW160 && (ed_fmt_ok(out_fmt) || out_fmt == C25519_FMT_RISTRETTO);
}

// The offsets of a segmented call: m segments [off[s], off[s + 1]) over n items.  ctx->err keeps the pointer it is given, so every caller
// has its messages as literals (OFF_MSGS: the call's name, what it calls the offsets and the item count; too_long only where max_len is
// given).  In this order: m, n, (m = 0: nothing else), the ends, then segment by segment the order and the length.
struct off_msgs { const char *m, *n, *ends, *order, *too_long; };
#define OFF_MSGS(call, off, n, too_long)                                                                                          \
    { call ": m must be below 2^32 - 1", call ": " n " must be < 2^40", call ": " off " must run from 0 to " n, call ": " off " must be non-decreasing", too_long }
static inline int32_t check_offsets(c25519_ctx *ctx, const off_msgs &msg, uint64_t n, const uint64_t *off, uint64_t m, uint64_t max_len = ~0ull) {
    if (m >= 0xffffffffull) return bad_arg(ctx, msg.m);
    if (n >= (1ull << 40)) return bad_arg(ctx, msg.n);
    if (m == 0) return C25519_OK;
    if (!off || off[0] != 0 || off[m] != n) return bad_arg(ctx, msg.ends);
    for (uint64_t s = 0; s < m; s++) {
        if (off[s + 1] < off[s]) return bad_arg(ctx, msg.order);
        if (off[s + 1] - off[s] > max_len) return bad_arg(ctx, msg.too_long);
    }
    return C25519_OK;
}
// n as a *_plan export has it: off[m], read only after m has been bounded (check_offsets refuses the rest)
static inline uint64_t offsets_end(const uint64_t *off, uint64_t m) { return (m && m < 0xffffffffull && off) ? off[m] : 0; }

// two staging buffers of na / nb bytes (16 when empty)
static inline int32_t reserve2(c25519_ctx *ctx, devbuf &a, size_t na, devbuf &b, size_t nb) {
    int32_t r = ctx_reserve(ctx, a, na ? na : 16);
    return r ? r : ctx_reserve(ctx, b, nb ? nb : 16);
}
