// rs_index.hpp -- the strand-index code of the DNA format: systematic RS(8,4)
// over GF(16), the (15,11) code shortened by seven symbols (DESIGN.md sec.
// 8.5).  Header-only, no HIP needed: the same functions run on the host and,
// compiled by hipcc, inside the kernels of dna.hip.
//
// Conventions (pinned by the 18432 strands of original files/final_DNA.txt,
// tests/golden/index_fixtures.npz; MATLAB's rsenc/rsdec defaults):
//   field     GF(16), primitive polynomial x^4 + x + 1 (19), alpha = 2
//   generator g(x) = (x - alpha)(x - alpha^2)(x - alpha^3)(x - alpha^4)
//                  = x^4 + 13 x^3 + 12 x^2 + 8 x + 7
//   word      symbols c0..c7, c(x) = sum c_j x^(7-j): c0..c3 the 16-bit index
//             (most significant nibble first), c4..c7 = x^4 m(x) mod g(x)
//   packing   a word is one uint32_t, symbol j in bits 4 (7-j) .. 4 (7-j) + 3,
//             so the index is word >> 16 and the parity is word & 0xffff
//   bases     A/C/G/T = 0..3 (DNA2binary, def_func.py:97-117): symbol j is
//             nt 2j (high two bits) and nt 2j+1 (low two bits)
//
// Decoder: bounded distance, t = 2 (d = 5).  If a codeword lies within
// Hamming distance 2 of the received word it is returned with cnumerr = that
// distance; otherwise cnumerr = -1.  Closed form (Peterson): syndromes
// S1..S4; one error iff S1, S2 != 0, S2^2 = S1 S3 and S3^2 = S2 S4; else the
// 2 x 2 solve for the locator x^2 + s1 x + s2, its roots searched among the 15
// nonzero field elements, the error values from S1 and S2.  A locator on one
// of the seven shortened positions (exponent >= 8), a zero error value and a
// locator without two distinct roots are failures.
//
// The log / antilog tables are 16 nibbles each, held as 64-bit constants:
// a lookup is a shift and a mask, in registers on the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

namespace ldpc {
namespace rs {

constexpr int kPrefixNt = 16;  // 8 symbols, two bases each
// alpha^i at nibble i, i = 0..14: 1 2 4 8 3 6 12 11 5 10 7 14 15 13 9 (nibble 15 unused)
constexpr uint64_t kExp = 0x09DFE7A5BC638421ull;
// log_alpha(a) at nibble a, a = 1..15: 0 1 4 2 8 5 10 3 14 9 7 6 13 11 12 (nibble 0 unused)
constexpr uint64_t kLog = 0xCBD679E3A5824100ull;

RS_HD uint32_t gf_exp(uint32_t i) { return (uint32_t)(kExp >> (4 * i)) & 15u; }  // i < 15
RS_HD uint32_t gf_log(uint32_t a) { return (uint32_t)(kLog >> (4 * a)) & 15u; }  // a != 0
RS_HD uint32_t mod15(uint32_t s) { return s >= 15u ? s - 15u : s; }              // s < 30

RS_HD uint32_t gf_mul(uint32_t a, uint32_t b)
{
    const uint32_t p = gf_exp(mod15(gf_log(a) + gf_log(b)));
    return (a != 0u && b != 0u) ? p : 0u;
}

// a / b, b != 0
RS_HD uint32_t gf_div(uint32_t a, uint32_t b)
{
    const uint32_t p = gf_exp(mod15(gf_log(a) + 15u - gf_log(b)));
    return a != 0u ? p : 0u;
}

// a * alpha^k, k < 15
RS_HD uint32_t gf_mul_exp(uint32_t a, uint32_t k)
{
    const uint32_t p = gf_exp(mod15(gf_log(a) + k));
    return a != 0u ? p : 0u;
}

// The four parity symbols of a 16-bit index, c4 in the high nibble: the
// remainder of x^4 m(x) by g(x), one LFSR step per message symbol.
RS_HD uint32_t rs_index_encode(uint32_t index)
{
    uint32_t p3 = 0, p2 = 0, p1 = 0, p0 = 0;
    for (int j = 0; j < 4; j++) {
        const uint32_t fb = ((index >> (12 - 4 * j)) & 15u) ^ p3;
        p3 = p2 ^ gf_mul(fb, 13u);
        p2 = p1 ^ gf_mul(fb, 12u);
        p1 = p0 ^ gf_mul(fb, 8u);
        p0 = gf_mul(fb, 7u);
    }
    return (p3 << 12) | (p2 << 8) | (p1 << 4) | p0;
}

RS_HD uint32_t rs_index_codeword(uint32_t index) { return ((index & 0xffffu) << 16) | rs_index_encode(index & 0xffffu); }

// Decode a packed word.  Returns cnumerr (0, 1, 2 or -1); *corrected gets the
// codeword (the received word itself on failure).
RS_HD int rs_index_decode(uint32_t word, uint32_t* corrected)
{
    *corrected = word;
    uint32_t S1 = 0, S2 = 0, S3 = 0, S4 = 0;  // S_k = r(alpha^k), Horner from c0
    for (int j = 0; j < 8; j++) {
        const uint32_t r = (word >> (28 - 4 * j)) & 15u;
        S1 = gf_mul_exp(S1, 1u) ^ r;
        S2 = gf_mul_exp(S2, 2u) ^ r;
        S3 = gf_mul_exp(S3, 3u) ^ r;
        S4 = gf_mul_exp(S4, 4u) ^ r;
    }
    if ((S1 | S2 | S3 | S4) == 0u) return 0;
    if (S1 != 0u && S2 != 0u && gf_mul(S2, S2) == gf_mul(S1, S3) && gf_mul(S3, S3) == gf_mul(S2, S4)) {
        // one error e at x^d: S_k = e alpha^(k d)
        const uint32_t d = gf_log(gf_div(S2, S1));
        if (d >= 8u) return -1;
        *corrected = word ^ (gf_div(gf_mul(S1, S1), S2) << (4 * d));
        return 1;
    }
    // two errors: [S1 S2; S2 S3] [s2; s1] = [S3; S4], locators = roots of x^2 + s1 x + s2
    const uint32_t det = gf_mul(S1, S3) ^ gf_mul(S2, S2);
    if (det == 0u) return -1;
    const uint32_t s1 = gf_div(gf_mul(S1, S4) ^ gf_mul(S2, S3), det);
    const uint32_t s2 = gf_div(gf_mul(S2, S4) ^ gf_mul(S3, S3), det);
    if (s1 == 0u || s2 == 0u) return -1;  // a double root, or a zero locator
    uint32_t n = 0, da = 0, db = 0;       // roots alpha^da, alpha^db, da < db
    for (uint32_t i = 0; i < 15u; i++) {
        const uint32_t x = gf_exp(i);
        const bool root = (gf_mul(x, x) ^ gf_mul(s1, x) ^ s2) == 0u;
        da = (root && n == 0u) ? i : da;
        db = (root && n == 1u) ? i : db;
        n += root ? 1u : 0u;
    }
    if (n != 2u || db >= 8u) return -1;
    // e_a X_a + e_b X_b = S1, e_a X_a^2 + e_b X_b^2 = S2, X_a + X_b = s1
    const uint32_t Xa = gf_exp(da), Xb = gf_exp(db);
    const uint32_t ea = gf_div(S2 ^ gf_mul(S1, Xb), gf_mul(Xa, s1));
    const uint32_t eb = gf_div(S2 ^ gf_mul(S1, Xa), gf_mul(Xb, s1));
    if (ea == 0u || eb == 0u) return -1;
    *corrected = word ^ (ea << (4 * da)) ^ (eb << (4 * db));
    return 2;
}

// The first 16 bases of a read as a packed word.  false: the read is shorter
// than 16 or holds a character other than A, C, G, T (upper case) there.
RS_HD bool rs_prefix_pack(const uint8_t* p, int64_t len, uint32_t* word)
{
    if (len < kPrefixNt) return false;
    uint32_t w = 0;
    bool ok = true;
    for (int k = 0; k < kPrefixNt; k++) {
        const uint32_t c = p[k];
        const uint32_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u;
        ok = ok && (c == 'A' || c == 'C' || c == 'G' || c == 'T');
        w = (w << 2) | v;
    }
    *word = w;
    return ok;
}

// Base k (0..15) of a packed word as its ASCII letter.
RS_HD uint8_t rs_prefix_base(uint32_t word, int k)
{
    const uint32_t v = (word >> (30 - 2 * k)) & 3u;
    return (uint8_t)(0x54474341u >> (8 * v));  // "ACGT"
}

// One read: index (0..65535, or -1) and cnumerr (0, 1, 2 or -1).
RS_HD void rs_read_decode(const uint8_t* p, int64_t len, int32_t* index, int32_t* cnumerr)
{
    uint32_t w = 0, c = 0;
    int ne = -1;
    if (rs_prefix_pack(p, len, &w)) ne = rs_index_decode(w, &c);
    *cnumerr = ne;
    *index = ne < 0 ? -1 : (int32_t)(c >> 16);
}

}  // namespace rs
}  // namespace ldpc
