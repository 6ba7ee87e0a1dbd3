// enc_check.cpp -- TEST INFRASTRUCTURE: the host encoder (csrc/gf2.hpp) and
// the graph loader under ASan + UBSan, as a stand-alone host program (no HIP).
// tests/test_encoder_san.py compiles it with g++ into a temporary directory
// and runs it on the .pchk files it is given:
//
//   enc_check <code.pchk>...
//
// For every file: build the encoder, check the positions (ascending, disjoint,
// K + rank = N), encode 70 seeded messages and require H c = 0 and the message
// bits at info_pos; a message byte of 2 must be refused.  A code with K = 0
// must give LDPC_ERR_UNSUPPORTED.  Exit status 0 iff every check held.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../dna-ldpc-codes_amd/csrc/gf2.hpp"
#include "../../dna-ldpc-codes_amd/csrc/graph.hpp"

static int fails = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);         \
            fails++;                          \
        }                                     \
    } while (0)

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; a++) {
        ldpc::HostGraph g;
        std::string msg;
        int rc = ldpc::load_pchk(argv[a], g, &msg);
        CHECK(rc == LDPC_OK, "%s: load: %s", argv[a], msg.c_str());
        if (rc) continue;
        ldpc::HostEncoder e;
        rc = ldpc::build_encoder(g, e, &msg);
        if (rc == LDPC_ERR_UNSUPPORTED && e.K == 0) {
            std::printf("%s: M %d N %d rank %d K 0 unsupported\n", argv[a], g.M, g.N, e.rank);
            continue;
        }
        CHECK(rc == LDPC_OK, "%s: build_encoder: %s", argv[a], msg.c_str());
        if (rc) continue;
        CHECK(e.K + e.rank == e.N && (int)e.info_pos.size() == e.K && (int)e.par_pos.size() == e.rank, "%s: sizes", argv[a]);
        std::vector<uint8_t> seen((size_t)e.N, 0);
        for (size_t k = 0; k < e.info_pos.size(); k++) {
            CHECK(k == 0 || e.info_pos[k] > e.info_pos[k - 1], "%s: info_pos order", argv[a]);
            seen[(size_t)e.info_pos[k]]++;
        }
        for (size_t k = 0; k < e.par_pos.size(); k++) {
            CHECK(k == 0 || e.par_pos[k] > e.par_pos[k - 1], "%s: par_pos order", argv[a]);
            seen[(size_t)e.par_pos[k]]++;
        }
        for (int j = 0; j < e.N; j++) CHECK(seen[(size_t)j] == 1, "%s: position %d covered %d times", argv[a], j, seen[(size_t)j]);
        const int64_t B = 70;
        std::vector<uint8_t> m((size_t)B * (size_t)e.K), cw((size_t)B * (size_t)e.N);
        uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(a + 1);
        for (auto& b : m) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            b = (uint8_t)((x >> 40) & 1);
        }
        rc = ldpc::encode_host(e, m.data(), B, cw.data(), &msg);
        CHECK(rc == LDPC_OK, "%s: encode_host: %s", argv[a], msg.c_str());
        int unsat = 0, wrong = 0;
        for (int64_t b = 0; b < B; b++) {
            unsat += ldpc::syndrome_host(g, cw.data() + (size_t)b * (size_t)e.N, nullptr);
            for (int k = 0; k < e.K; k++) wrong += cw[(size_t)b * (size_t)e.N + (size_t)e.info_pos[k]] != m[(size_t)b * (size_t)e.K + (size_t)k];
        }
        CHECK(unsat == 0, "%s: %d unsatisfied checks", argv[a], unsat);
        CHECK(wrong == 0, "%s: %d message bits not at their positions", argv[a], wrong);
        m[m.size() - 1] = 2;
        CHECK(ldpc::encode_host(e, m.data(), B, cw.data(), &msg) == LDPC_ERR_ARG, "%s: a byte of 2 was accepted", argv[a]);
        std::printf("%s: M %d N %d rank %d K %d ok\n", argv[a], g.M, g.N, e.rank, e.K);
    }
    return fails ? 1 : 0;
}
