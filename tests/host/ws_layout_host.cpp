// Stand-alone host program around the workspace layouts of csrc: ws_layout (csrc/capi_util.h) and the two sized structs built on it,
// straus_ws (csrc/straus.h) and segb_ws (csrc/mid_segb.h).  Compiled for the host alone (no device code is generated, no GPU is opened);
// ctx_reserve is replaced by one that hands out a host buffer and notes what it was asked for.  Test-only: built and run by
// tests/test_ws_layout_host.py.
//   ws_layout_host parts SLACK BYTES...   one layout of the given parts: "offset pointer-offset" per part, then "bytes(0) bytes(SLACK) reserved"
//   ws_layout_host totals                 the totals of straus_ws / segb_ws over the shapes of tests/golden/ws_layout_totals.json, as that file has them
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../curve25519-dalek_amd/csrc/capi_util.h"
#include "../../curve25519-dalek_amd/csrc/straus.h"
#include "../../curve25519-dalek_amd/csrc/mid_segb.h"

static size_t g_reserved = 0;
static std::vector<uint8_t> g_mem;
int32_t ctx_reserve(c25519_ctx *, devbuf &b, size_t bytes) {
    g_reserved = bytes;
    g_mem.assign(bytes ? bytes : 1, 0);
    b.p = g_mem.data(); b.cap = bytes;
    return 0;
}

static int parts(int argc, char **argv) {
    const size_t slack = strtoull(argv[2], nullptr, 10);
    ws_layout L;
    std::vector<size_t> off;
    for (int i = 3; i < argc; i++) off.push_back(L.part(strtoull(argv[i], nullptr, 10)));
    devbuf buf;
    if (L.reserve(nullptr, buf, slack) != 0 || L.base != (uint8_t *)buf.p) return 1;
    for (size_t i = 0; i < off.size(); i++) {
        uint32_t *p = L.at<uint32_t>(off[i]);
        const size_t end = i + 1 < off.size() ? off[i + 1] : L.bytes();
        memset(p, 0xa5, end - off[i]);                      // (under the sanitizers: every byte of the part is inside the reservation)
        printf("%zu %zu\n", off[i], (size_t)((uint8_t *)p - (uint8_t *)buf.p));
    }
    printf("%zu %zu %zu\n", L.bytes(), L.bytes(slack), g_reserved);
    return 0;
}

static int totals() {
    const uint64_t ms[3] = {0, 1, 3}, ts[3] = {1, 64, 2049};
    const int fmts[2] = {C25519_FMT_EDWARDS_Y, C25519_FMT_RAW160};
    uint8_t caller_out[1], caller_ok[1];
    printf("{\n \"straus_ws\": [");
    bool first = true;
    for (uint64_t m : ms) for (uint64_t t : ts) for (int f : fmts) for (int ok = 0; ok < 2; ok++) {
        straus_ws ws(m, (size_t)m, t, f, ok != 0);
        // the parts of a pass lie behind the head, the whole is the two and 256 bytes; bound, the caller's arrays are used where the workspace has none
        if (ws.head_bytes() + ws.pass_bytes() + 256 != ws.bytes()) return 1;
        std::vector<uint8_t> mem(ws.bytes());
        ws.bind(mem.data(), caller_out, ok ? caller_ok : nullptr);
        if ((uint8_t *)ws.d_off != mem.data() || (uint8_t *)ws.tab != mem.data() + ws.head_bytes() || ws.tok + al256(t) + 256 != mem.data() + ws.bytes()) return 1;
        if ((ws.okbuf == caller_ok) != (ok != 0) || (ws.sums == caller_out) != (f == C25519_FMT_RAW160 || m == 0)) return 1;
        printf("%s\n  {\"m\": %llu, \"n_ids\": %llu, \"maxt\": %llu, \"out_fmt\": %d, \"caller_ok\": %d, \"bytes\": %zu}", first ? "" : ",", (unsigned long long)m,
               (unsigned long long)m, (unsigned long long)t, f, ok, ws.bytes());
        first = false;
    }
    printf("\n ],\n \"segb_ws\": [");
    first = true;
    for (uint64_t m : ms) for (uint64_t t : ts) {
        segb_ws bw(t, m, segb_desc_words(m));
        std::vector<uint8_t> mem(bw.pass_bytes() + bw.b_desc + 1);
        bw.bind(mem.data(), mem.data() + bw.pass_bytes());
        if ((uint8_t *)bw.rec != mem.data() || bw.wok + al256(m * c25519::SEGB_WIN) != (uint8_t *)bw.desc) return 1;
        printf("%s\n  {\"maxt\": %llu, \"maxseg\": %llu, \"desc_words\": %zu, \"pass_bytes\": %zu, \"desc_bytes\": %zu}", first ? "" : ",", (unsigned long long)t,
               (unsigned long long)m, segb_desc_words(m), bw.pass_bytes(), bw.b_desc);
        first = false;
    }
    printf("\n ]\n}\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "parts")) return parts(argc, argv);
    if (argc == 2 && !strcmp(argv[1], "totals")) return totals();
    fprintf(stderr, "usage: ws_layout_host parts SLACK BYTES... | totals\n");
    return 2;
}
