// The per-level states of the device z-mode's hash tree (verify.hip k_ztree_first has the derivation), shared by the single-batch path
// (verify.hip) and the segmented one (verify_seg.hip).
#pragma once
#include <stdint.h>
#include "fe26.h"

namespace c25519 {
constexpr int ZTREE_MAX_LEVELS = 16;
struct ztree_ivs { u64 iv[ZTREE_MAX_LEVELS][8]; };       // iv[l]: the BLAKE2b state after TAG(l, ..)
}  // namespace c25519

// iv[l] for a tree over n signatures: host arithmetic (one BLAKE2b compression per level), verify.hip
void ztree_make_ivs(uint64_t n, c25519::ztree_ivs &ivs);
