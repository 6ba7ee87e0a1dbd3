// rs_check.cpp -- TEST INFRASTRUCTURE: the strand-index codec
// (csrc/rs_index.hpp) under ASan + UBSan, as a stand-alone host program (no
// HIP).  tests/test_rs_index_san.py compiles it with g++ into a temporary
// directory and runs it:
//
//   rs_check
//
// * every one of the 65536 codewords decodes to itself with cnumerr 0;
// * for the codewords of index 0, 65535 and 0x1b14: all 120 single and all
//   6300 double symbol errors decode back with cnumerr 1 / 2;
// * edge-case reads, each in a heap buffer of exactly its length so that a
//   read past the end is an ASan report: lengths 0, 15, 16, 17, a prefix with
//   'N', '-', lower case, and a corrected prefix followed by a payload.
// Exit status 0 iff every check held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../dna-ldpc-codes_amd/csrc/rs_index.hpp"

using namespace ldpc::rs;

static int fails = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);         \
            fails++;                          \
        }                                     \
    } while (0)

static std::string prefix_of(uint32_t word)
{
    std::string s(kPrefixNt, '?');
    for (int k = 0; k < kPrefixNt; k++) s[(size_t)k] = (char)rs_prefix_base(word, k);
    return s;
}

// decode a read held in a heap buffer of exactly its length
static void decode_read(const std::string& s, int32_t* index, int32_t* cnumerr)
{
    std::vector<uint8_t> buf(s.begin(), s.end());
    rs_read_decode(buf.empty() ? nullptr : buf.data(), (int64_t)buf.size(), index, cnumerr);
}

int main()
{
    for (uint32_t i = 0; i < 65536u; i++) {
        uint32_t c = 0;
        const uint32_t w = rs_index_codeword(i);
        const int ne = rs_index_decode(w, &c);
        CHECK(ne == 0 && c == w && (w >> 16) == i, "codeword %u: cnumerr %d", i, ne);
    }
    const uint32_t picks[3] = {0u, 65535u, 0x1b14u};
    long singles = 0, doubles = 0;
    for (uint32_t idx : picks) {
        const uint32_t w = rs_index_codeword(idx);
        for (int p = 0; p < 8; p++) {
            for (uint32_t e = 1; e < 16; e++) {
                uint32_t c = 0;
                const int ne = rs_index_decode(w ^ (e << (4 * p)), &c);
                CHECK(ne == 1 && c == w, "index %u: single error %u at %d: cnumerr %d", idx, e, p, ne);
                singles++;
                for (int q = p + 1; q < 8; q++) {
                    for (uint32_t f = 1; f < 16; f++) {
                        const int n2 = rs_index_decode(w ^ (e << (4 * p)) ^ (f << (4 * q)), &c);
                        CHECK(n2 == 2 && c == w, "index %u: errors %u at %d, %u at %d: cnumerr %d", idx, e, p, f, q, n2);
                        doubles++;
                    }
                }
            }
        }
    }
    CHECK(singles == 3 * 120 && doubles == 3 * 6300, "error patterns: %ld singles, %ld doubles", singles, doubles);

    int32_t index = 0, ne = 0;
    const std::string good = prefix_of(rs_index_codeword(0x1b14u));
    decode_read("", &index, &ne);
    CHECK(index == -1 && ne == -1, "empty read: %d %d", index, ne);
    decode_read(good.substr(0, 15), &index, &ne);
    CHECK(index == -1 && ne == -1, "15-nt read: %d %d", index, ne);
    decode_read(good, &index, &ne);
    CHECK(index == 0x1b14 && ne == 0, "16-nt read: %d %d", index, ne);
    decode_read(good + "A", &index, &ne);
    CHECK(index == 0x1b14 && ne == 0, "17-nt read: %d %d", index, ne);
    for (const char bad : {'N', '-', 'a', 't', '\0'}) {
        for (int k : {0, 7, 15}) {
            std::string s = good;
            s[(size_t)k] = bad;
            decode_read(s + "ACGT", &index, &ne);
            CHECK(index == -1 && ne == -1, "character %d at %d: %d %d", (int)bad, k, index, ne);
        }
    }
    std::string two = good;  // two symbols wrong (nt 0 and nt 15), then a payload
    two[0] = two[0] == 'A' ? 'C' : 'A';
    two[15] = two[15] == 'G' ? 'T' : 'G';
    decode_read(two + std::string(136, 'C'), &index, &ne);
    CHECK(index == 0x1b14 && ne == 2, "two symbol errors: %d %d", index, ne);
    if (!fails) std::printf("rs_check ok: 65536 codewords, %ld single and %ld double errors\n", singles, doubles);
    return fails ? 1 : 0;
}
