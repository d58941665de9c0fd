// Host build of the per-lane transcript of the segmented verify_batch (csrc/transcript_dev.h is __host__ __device__).  Test-only: built by
// tests/test_transcript_dev_host.py into tests/host/libtranscriptdevhost.so, and -- with -DTRANSCRIPT_DEV_MAIN -- as a stand-alone program that
// compares it with the host path (csrc/transcript_host.h) for every length 0 .. 400 on exactly-sized heap buffers (run under ASan + UBSan).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../curve25519-dalek_amd/csrc/transcript_dev.h"

// hram n x 64, sigs n x 64 -> z16 n x 16, through an exactly-sized staging buffer as a lane of the kernel has it
static void dev_zs(const uint8_t *hram, const uint8_t *sigs, uint64_t n, uint8_t *z16) {
    if (!n) return;                                         // (the kernel's lanes skip empty segments)
    std::vector<uint64_t> h(n * 8), s(n * 8), z(n * 2), stage(c25519_trd::STAGE_WORDS, 0);
    memcpy(h.data(), hram, n * 64); memcpy(s.data(), sigs, n * 64);
    c25519_trd::prefix pre;
    c25519_trd::make_prefix(pre);
    c25519_trd::transcript_zs(pre, h.data(), s.data(), n, z.data(), stage.data());
    memcpy(z16, z.data(), n * 16);
}

extern "C" void h_transcript_dev_zs(const uint8_t *hram, const uint8_t *sigs, uint64_t n, uint8_t *z16) { dev_zs(hram, sigs, n, z16); }

#ifdef TRANSCRIPT_DEV_MAIN
#include "../../curve25519-dalek_amd/csrc/transcript_host.h"
int main() {
    for (uint64_t n = 0; n <= 400; n++) {
        std::vector<uint8_t> h(n * 64), s(n * 64), z(n * 16), want(n * 16);
        for (auto &x : h) x = (uint8_t)rand();
        for (auto &x : s) x = (uint8_t)rand();
        dev_zs(h.data(), s.data(), n, z.data());
        c25519_transcript_zs(h.data(), s.data(), n, want.data());
        if (n && memcmp(z.data(), want.data(), n * 16)) { printf("MISMATCH at n = %llu\n", (unsigned long long)n); return 1; }
    }
    printf("sanitized ok\n");
    return 0;
}
#endif
