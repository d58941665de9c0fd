// Stand-alone host program around csrc/rows_digits.h, the digit recoding of the precomputed rows call (csrc/mid_rows.hip): for every scalar of
// the file named on the command line (64 hex digits per line, little-endian bytes) it prints bit 255 and the 64 digits, taken out of the recoded
// words in the two ways the kernels do it -- the lane kernel's walk (a nibble at a time, the words moving down after every eighth) and the wave
// kernel's pick (window l: word l / 8, nibble l % 8).  The two must agree.  Test-only: built and run by tests/test_precomp_rows_host.py, with
// the sanitizers, against Python integers.
#include "../../curve25519-dalek_amd/csrc/rows_digits.h"
#include <stdio.h>
#include <string.h>
using namespace c25519;

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: rows_digits_host FILE\n"); return 2; }
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
        const bool top = rows_recode(s);
        int pick[ROWS_WIN], walk[ROWS_WIN];
        for (int l = 0; l < ROWS_WIN; l++) {                 // k_mid_rows_wave
            const u32 word = (u32)l >> 3, shift = 4u * ((u32)l & 7u);
            u32 mine = s[0];
            for (u32 q = 1; q < 8; q++) mine = word == q ? s[q] : mine;
            pick[l] = rows_digit((mine >> shift) & 15u, l);
        }
        u32 cur = s[0];                                      // k_mid_rows_lane (consumes s)
        for (int k = 0; k < ROWS_WIN; k++) {
            const u32 nib = cur & 15u;
            cur >>= 4;
            if ((k & 7) == 7) {
                for (int q = 0; q < 7; q++) s[q] = s[q + 1];
                cur = s[0];
            }
            walk[k] = rows_digit(nib, k);
        }
        if (memcmp(pick, walk, sizeof pick) != 0) { printf("MISMATCH\n"); fclose(f); return 1; }
        printf("%d", top ? 1 : 0);
        for (int k = 0; k < ROWS_WIN; k++) printf(" %d", walk[k]);
        printf("\n");
    }
    fclose(f);
    printf("rows_digits_host ok\n");
    return 0;
}
