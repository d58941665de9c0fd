// The bucket route of c25519_msm_vartime_segments (mid_segb.hip) as mid_seg.hip sees it: the two constants of the header as the host reads
// them, the workspace of a bucket pass and the function that enqueues one.  DESIGN.md section 3.13.
#pragma once
#include <stdint.h>
#include <algorithm>
#include "straus.h"
#include "segb_digits.h"

static_assert(C25519_MSM_SEGMENT_BUCKET_MAX <= 65536, "a term index relative to its segment is kept in 16 bits");
static_assert(C25519_MSM_SEGMENT_BUCKET_MAX > C25519_MSM_SEGMENT_WAVE_MAX && C25519_MSM_SEGMENT_BUCKET_PASS_TERMS >= C25519_MSM_SEGMENT_BUCKET_MAX, "one segment always fits into a pass");

// (the tuning build reads other values, knobs.h; never above 65536, never below the wave maximum, where the route is empty)
static inline uint64_t seg_bucket_max() {
    static const uint64_t v = std::max<uint64_t>(std::min<uint64_t>((uint64_t)std::max<long long>(1, C25519_KNOB_LL("SEG_BUCKET_MAX", C25519_MSM_SEGMENT_BUCKET_MAX)), 65536), seg_wave_max());
    return v;
}
static inline uint64_t seg_bucket_pass_terms() {
    static const uint64_t v = std::max<uint64_t>((uint64_t)std::max<long long>(1, C25519_KNOB_LL("SEG_BUCKET_PASS_TERMS", C25519_MSM_SEGMENT_BUCKET_PASS_TERMS)), seg_bucket_max());
    return v;
}

// A bucket pass: nb segments with nt terms in all, term after term as records 0 .. nt - 1.  Its descriptor is 3 nb + 1 u64 words:
//   rec_off[0 .. nb] (the first record of segment k of the pass; rec_off[nb] = nt) | term0[0 .. nb) (its first term in the call) | sid[0 .. nb) (its index in the call)
static inline size_t segb_desc_words(uint64_t nb) { return (size_t)(3 * nb + 1); }

// The workspace of the route.  Per pass, where the Straus passes keep tables, digits and term ok bytes (the passes run one after the other on the
// stream, so the two kinds share the place):
//   records (160 bytes per term) | digits (32 per term, window-major) | term indices (32 x 2 per term, window-major) | term ok bytes |
//   window sums (32 x 160 per segment) | window ok bytes (32 per segment)
// and, for the whole call, the descriptors of all bucket passes.  Every part a multiple of 256 bytes.
struct segb_ws {
    ws_layout L;                                            // the parts of a pass
    size_t o_rec, o_dig, o_idx, o_tok, o_wsum, o_wok, b_desc;
    uint4 *rec = nullptr;
    uint8_t *dig = nullptr, *tok = nullptr, *wok = nullptr;
    uint16_t *idx = nullptr;
    uint32_t *wsum = nullptr;
    uint64_t *desc = nullptr;
    segb_ws(uint64_t maxt, uint64_t maxseg, size_t desc_words)
        : o_rec(L.part(maxt * 160)), o_dig(L.part(maxt * c25519::SEGB_WIN)), o_idx(L.part(maxt * c25519::SEGB_WIN * 2)), o_tok(L.part(maxt)),
          o_wsum(L.part(maxseg * c25519::SEGB_WIN * 160)), o_wok(L.part(maxseg * c25519::SEGB_WIN)), b_desc(al256(desc_words * 8)) {}
    size_t pass_bytes() const { return L.bytes(); }
    void bind(void *pass_base, void *desc_base) {
        L.bind(pass_base);
        rec = L.at<uint4>(o_rec); dig = L.at(o_dig); idx = L.at<uint16_t>(o_idx); tok = L.at(o_tok); wsum = L.at<uint32_t>(o_wsum); wok = L.at(o_wok);
        desc = (uint64_t *)desc_base;
    }
};

// The three launches of one bucket pass on ctx->stream: d_desc is the pass's descriptor (device), sums / okbuf the call's raw sums and ok bytes.
int32_t segb_enqueue_pass(c25519_ctx *ctx, int in_fmt, const uint8_t *d_scalars, const uint8_t *d_points, const segb_ws &ws, const uint64_t *d_desc, uint32_t nb, uint64_t nt,
                          uint8_t *sums, uint8_t *okbuf);
extern const char *const SEGB_KERNEL_NAME;
