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

// a rejected argument: the message for c25519_last_error and the status every entry point returns for it
static inline int32_t bad_arg(c25519_ctx *ctx, const char *what) { ctx->err = what; return -(int32_t)hipErrorInvalidValue; }

static inline size_t point_bytes(int fmt) { return fmt == C25519_FMT_RAW160 ? 160 : 32; }
static inline bool ris_fmt_ok(int fmt) { return fmt == C25519_FMT_RISTRETTO || fmt == C25519_FMT_RAW160; }
static inline bool ed_fmt_ok(int fmt) { return fmt == C25519_FMT_EDWARDS_Y || fmt == C25519_FMT_RAW160; }

// two staging buffers of na / nb bytes (16 when empty)
static inline int32_t reserve2(c25519_ctx *ctx, devbuf &a, size_t na, devbuf &b, size_t nb) {
    int32_t r = ctx_reserve(ctx, a, na ? na : 16);
    return r ? r : ctx_reserve(ctx, b, nb ? nb : 16);
}
