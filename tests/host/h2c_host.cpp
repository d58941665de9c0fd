// Host build of the hash-to-group device code (csrc/h2c.h is __host__ __device__) with bound checking enabled.
// Test-only: built by tests/test_h2c_host.py into tests/host/libh2chost.so.
#define C25519_CHECK_BOUNDS 1
#include "../../curve25519-dalek_amd/csrc/h2c.h"
#include <string.h>
using namespace c25519;

static feT load(const uint8_t b[32]) { u32 w[8]; memcpy(w, b, 32); return fe_from_words(w); }
static void store(uint8_t b[32], const feW &a) { u32 w[8]; fe_to_words(a, w); memcpy(b, w, 32); }
static void store_affine(uint8_t o[64], const ge_p3 &p) {      // x || y, canonical little-endian (the identity of a degenerate Z is caught by the caller)
    const feT zi = fe_invert(p.Z);
    store(o, fe_mul(p.X, zi)); store(o + 32, fe_mul(p.Y, zi));
}

extern "C" {
// RistrettoPoint::map_to_curve(in32).compress()
void h_ris_map(const uint8_t *in, uint8_t *o) { u32 w[8], c[8]; memcpy(w, in, 32); ris_compress(ris_map_words(w), c); memcpy(o, c, 32); }
// RistrettoPoint::from_uniform_bytes(in64).compress()
void h_ris_from_uniform(const uint8_t *in, uint8_t *o) {
    u32 a[8], b[8], c[8]; memcpy(a, in, 32); memcpy(b, in + 32, 32);
    ris_compress(ge_add(ris_map_words(a), ris_map_words(b)), c); memcpy(o, c, 32);
}
// RFC 9380 G.2.1: (xn, xd, y) canonical
void h_mont_elligator2(const uint8_t *u, uint8_t *o) { feT xn, xd, y; mont_elligator2(load(u), xn, xd, y); store(o, xn); store(o + 32, xd); store(o + 64, y); }
// EdwardsPoint::map_to_curve: affine x || y
void h_ed_map(const uint8_t *u, uint8_t *o) { store_affine(o, ed_h2c_map(load(u))); }
void h_xmd(const uint8_t *msg, uint64_t len, const uint8_t *dst, uint32_t dst_len, int count, uint8_t *o) { xmd_sha512(msg, len, dst, dst_len, count, o); }
void h_hash_to_field(const uint8_t *msg, uint64_t len, const uint8_t *dst, uint32_t dst_len, int count, uint8_t *o) {
    feT u[2]; hash_to_field(msg, len, dst, dst_len, count, u);
    for (int i = 0; i < count; i++) store(o + 32 * i, u[i]);
}
void h_fe_from_be48(const uint8_t *b, uint8_t *o) { store(o, fe_from_be48(b)); }
// hash_to_curve (ro = 1) / encode_to_curve (ro = 0): affine x || y, and the compressed Edwards y
void h_ed_hash_to_curve(const uint8_t *msg, uint64_t len, const uint8_t *dst, uint32_t dst_len, int ro, uint8_t *o) {
    const ge_p3 p = ed_hash_to_curve(msg, len, dst, dst_len, ro != 0);
    store_affine(o, p);
    const feT zi = fe_invert(p.Z);
    u32 w[8]; ge_affine_compress(fe_mul(p.X, zi), fe_mul(p.Y, zi), w); memcpy(o + 64, w, 32);
}
}
