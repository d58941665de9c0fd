// Stand-alone host program around csrc/segb_digits.h, the digit recoding of the segmented MSM's bucket route (csrc/mid_segb.hip): for every
// scalar of the file named on the command line (64 hex digits per line, little-endian bytes) it prints bit 255, then the 32 digits as the
// kernels take them out of the recoded words (k_mid_segb_front stores byte k of word k / 4; k_mid_segb_window reads it back with segb_digit),
// then the list (segb_slot) of every digit, -1 for a zero digit.  Test-only: built and run by tests/test_seg_msm_bucket_host.py, with the
// sanitizers, against Python integers.
#include "../../curve25519-dalek_amd/csrc/segb_digits.h"
#include <stdio.h>
#include <string.h>
using namespace c25519;

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: segb_digits_host FILE\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char line[256];
    while (fgets(line, sizeof line, f)) {
        if (strlen(line) < 64) continue;
        uint8_t b[32];
        for (int i = 0; i < 32; i++) {
            const int hi = hexval(line[2 * i]), lo = hexval(line[2 * i + 1]);
            if (hi < 0 || lo < 0) { fprintf(stderr, "bad hex\n"); fclose(f); return 2; }
            b[i] = (uint8_t)(16 * hi + lo);
        }
        u32 s[8];
        for (int i = 0; i < 8; i++) s[i] = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
        const bool top = segb_recode(s);
        printf("%d", top ? 1 : 0);
        int d[SEGB_WIN];
        for (int k = 0; k < SEGB_WIN; k++) {
            const uint8_t stored = (uint8_t)(s[k >> 2] >> (8 * (k & 3)));
            d[k] = segb_digit(stored, k);
            printf(" %d", d[k]);
        }
        for (int k = 0; k < SEGB_WIN; k++) printf(" %d", d[k] == 0 ? -1 : (int)segb_slot(d[k]));
        printf("\n");
    }
    fclose(f);
    printf("segb_digits_host ok\n");
    return 0;
}
