// plan_check.cpp -- stand-alone check of csrc/engine_plan.hpp (no HIP): prints
// what plan_engine / resolve_schedule decide for the DNA code and a few
// synthetic graphs, one line per case.  tests/test_engine_plan.py builds it
// with ASan + UBSan and compares the lines with what Engine::init decided
// before the plan was a function of its own.
//   plan_check <golden .pchk>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "../../dna-ldpc-codes_amd/csrc/engine_plan.hpp"

using namespace ldpc;

static const size_t kFree = 200000000000ull;  // 200 GB free

static ldpc_schedule sched(int32_t set = 0, int32_t flags = 0)
{
    ldpc_schedule s{};
    s.flags_set = set;
    s.flags = flags;
    return s;
}

static void show(const char* name, const HostGraph& g, int algo, int64_t chunk, ldpc_schedule s, size_t free_bytes = kFree)
{
    const ldpc_schedule r = resolve_schedule(&s);
    const EnginePlan p = plan_engine(g, algo, chunk, r, free_bytes);
    if (p.error) {
        std::printf("%s: error=%s\n", name, p.error);
        return;
    }
    std::printf("%s: msa_c=%d cont=%d res=%d handover=%d nt=%d first_fp=%d no_drain=%d bad_lane=%d cpw=%d poll=%d syn=%d "
                "cap=%lld cap_tiles=%lld group=%lld c2v_tiles=%lld c2v_bytes=%zu\n",
                name, p.msa_c, p.cont, p.res, p.handover, p.nt_d, p.first_fp, p.debug_no_drain, p.debug_bad_lane, p.var_cpw,
                p.res_poll, p.syn_blocks, (long long)p.cap, (long long)p.cap_tiles, (long long)p.group_tiles,
                (long long)p.c2v_tiles, p.c2v_bytes);
}

static void show_sched(const char* name, ldpc_schedule s)
{
    const ldpc_schedule r = resolve_schedule(&s);
    std::printf("%s: set=%#x flags=%#x group=%d cpw=%d pool=%d poll=%d syn=%d reserved=%d\n", name, (unsigned)r.flags_set,
                (unsigned)r.flags, r.group_tiles, r.var_cpw, r.pool_tiles, r.poll_every, r.syn_blocks, r.reserved);
}

static HostGraph from_edges(int32_t M, int32_t N, const std::vector<int32_t>& rows, const std::vector<int32_t>& cols)
{
    HostGraph g;
    std::string msg;
    if (build_graph(M, N, rows.data(), cols.data(), (int64_t)rows.size(), g, &msg) != LDPC_OK) {
        std::fprintf(stderr, "build_graph: %s\n", msg.c_str());
        std::exit(2);
    }
    return g;
}

// A (dv, dc)-regular code with M = dv * Q rows and N = dc * Q columns: row
// block b holds each column once, in a pseudo-random order per block.
static HostGraph regular_graph(int32_t Q, int dv, int dc)
{
    const int32_t M = dv * Q, N = dc * Q;
    std::vector<int32_t> rows, cols, perm((size_t)N);
    uint64_t x = 88172645463325252ull;
    for (int b = 0; b < dv; b++) {
        std::iota(perm.begin(), perm.end(), 0);
        for (int32_t i = N - 1; i > 0; i--) {  // Fisher-Yates on xorshift64
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            std::swap(perm[(size_t)i], perm[(size_t)(x % (uint64_t)(i + 1))]);
        }
        for (int32_t i = 0; i < Q; i++)
            for (int k = 0; k < dc; k++) {
                rows.push_back(b * Q + i);
                cols.push_back(perm[(size_t)i * dc + k]);
            }
    }
    return from_edges(M, N, rows, cols);
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    HostGraph dna;
    std::string msg;
    if (load_pchk(argv[1], dna, &msg) != LDPC_OK) {
        std::fprintf(stderr, "load_pchk: %s\n", msg.c_str());
        return 2;
    }
    std::printf("dna: M=%d N=%d E=%lld dc=%d dv=%d bytes_per_codeword=%lld\n", dna.M, dna.N, (long long)dna.E, dna.dc_max,
                dna.dv_max, (long long)engine_bytes_per_codeword(dna));
    show("bp", dna, LDPC_ALGO_BP, 0, sched());
    show("msa", dna, LDPC_ALGO_MSA, 0, sched());
    show("bp chunk=320", dna, LDPC_ALGO_BP, 320, sched());
    show("bp chunk=320 resident", dna, LDPC_ALGO_BP, 320, sched(LDPC_SCHED_RESIDENT, LDPC_SCHED_RESIDENT));
    show("bp fixed", dna, LDPC_ALGO_BP, 0, sched(LDPC_SCHED_CONTINUOUS, 0));
    show("qmsa", dna, LDPC_ALGO_QMSA, 0, sched());
    show("gallager_a", dna, LDPC_ALGO_GALLAGER_A, 0, sched());
    show("gallager_b1", dna, LDPC_ALGO_GALLAGER_B1, 0, sched());
    show("gallager_b2", dna, LDPC_ALGO_GALLAGER_B2, 0, sched());
    show("bp no handover", dna, LDPC_ALGO_BP, 0, sched(LDPC_SCHED_HANDOVER, 0));
    show("bp chunk=4194304", dna, LDPC_ALGO_BP, 4194304, sched());
    show("bp chunk=4194240", dna, LDPC_ALGO_BP, 4194240, sched());
    show("bp little memory", dna, LDPC_ALGO_BP, 0, sched(), 10000000);
    show("msa little memory", dna, LDPC_ALGO_MSA, 0, sched(), 10000000);
    show("bp debug", dna, LDPC_ALGO_BP, 0,
         sched(LDPC_SCHED_DEBUG_NO_DRAIN | LDPC_SCHED_DEBUG_BAD_LANE, LDPC_SCHED_DEBUG_NO_DRAIN | LDPC_SCHED_DEBUG_BAD_LANE));

    const HostGraph big = regular_graph(512, 8, 72);  // N = 36 864
    std::printf("big: M=%d N=%d E=%lld dc=%d dv=%d regular=%d%d\n", big.M, big.N, (long long)big.E, big.dc_max, big.dv_max,
                big.regular_dc, big.regular_dv);
    show("big bp", big, LDPC_ALGO_BP, 0, sched());
    show("big bp resident", big, LDPC_ALGO_BP, 0, sched(LDPC_SCHED_RESIDENT, LDPC_SCHED_RESIDENT));
    show("big msa", big, LDPC_ALGO_MSA, 0, sched());

    {  // column 0 in 33 rows: no register bucket for the variable phase
        std::vector<int32_t> rows, cols;
        for (int i = 0; i < 40; i++) {
            if (i < 33) rows.push_back(i), cols.push_back(0);
            rows.push_back(i), cols.push_back(1 + i);
            rows.push_back(i), cols.push_back(41 + i % 9);
        }
        const HostGraph g = from_edges(40, 50, rows, cols);
        std::printf("dv33: dc=%d dv=%d\n", g.dc_max, g.dv_max);
        show("dv33 bp", g, LDPC_ALGO_BP, 0, sched());
    }
    {  // a row of degree 97, columns of degree <= 4
        std::vector<int32_t> rows, cols;
        for (int j = 0; j < 97; j++) rows.push_back(0), cols.push_back(j);
        for (int i = 1; i < 4; i++)
            for (int j = 0; j < 200; j += i + 2) rows.push_back(i), cols.push_back(j);
        const HostGraph g = from_edges(4, 200, rows, cols);
        std::printf("dc97: dc=%d dv=%d\n", g.dc_max, g.dv_max);
        show("dc97 bp", g, LDPC_ALGO_BP, 0, sched());
        show("dc97 msa", g, LDPC_ALGO_MSA, 0, sched());
    }
    {
        const HostGraph g = regular_graph(64, 4, 32);
        std::printf("reg4x32: M=%d N=%d E=%lld dc=%d dv=%d regular=%d%d pool_tiles=%d\n", g.M, g.N, (long long)g.E, g.dc_max,
                    g.dv_max, g.regular_dc, g.regular_dv, gen_pool_tiles(g));
        show("reg4x32 bp", g, LDPC_ALGO_BP, 0, sched());
        show("reg4x32 msa", g, LDPC_ALGO_MSA, 0, sched());
        ldpc_schedule s = sched();
        s.pool_tiles = 2;
        show("reg4x32 bp pool_tiles=2", g, LDPC_ALGO_BP, 0, s);
    }
    // Regular on one side only: a specialised kernel next to a generic one
    // (rows of degree 72 with other columns, columns of degree 8 with other rows).
    const auto mixed = [](const char* name, const HostGraph& g) {
        std::printf("%s: M=%d N=%d E=%lld dc=%d dv=%d regular=%d%d pool_tiles=%d\n", name, g.M, g.N, (long long)g.E,
                    g.dc_max, g.dv_max, g.regular_dc, g.regular_dv, gen_pool_tiles(g));
        const ldpc_schedule res = sched(LDPC_SCHED_RESIDENT, LDPC_SCHED_RESIDENT);
        const std::string n(name);
        show((n + " bp").c_str(), g, LDPC_ALGO_BP, 0, sched());
        show((n + " msa").c_str(), g, LDPC_ALGO_MSA, 0, sched());
        show((n + " bp resident").c_str(), g, LDPC_ALGO_BP, 0, res);
        show((n + " msa resident").c_str(), g, LDPC_ALGO_MSA, 0, res);
    };
    {
        const HostGraph g = regular_graph(5, 6, 72);  // N = 360: 32 does not divide it
        mixed("reg6x72", g);
        show("reg6x72 bp chunk=320", g, LDPC_ALGO_BP, 320, sched());
        show("reg6x72 bp chunk=320 resident", g, LDPC_ALGO_BP, 320, sched(LDPC_SCHED_RESIDENT, LDPC_SCHED_RESIDENT));
    }
    mixed("reg8x48", regular_graph(5, 8, 48));    // N = 240
    mixed("reg8x100", regular_graph(3, 8, 100));  // N = 300: rows past the last check bucket

    show_sched("null", ldpc_schedule{});
    show_sched("unknown bits", sched(0x7fffffff, 0x7fffffff & ~LDPC_SCHED_RESIDENT));
    ldpc_schedule s = sched(kResolved | kResChosen, 0);  // a caller's: re-resolved, the marks dropped
    s.group_tiles = 0;
    s.var_cpw = 5;
    s.pool_tiles = -3;
    s.poll_every = -1;
    s.syn_blocks = 1000;
    s.reserved = 7;
    show_sched("marked resolved", s);
    for (int cpw = 0; cpw <= 9; cpw++) {
        s = sched();
        s.var_cpw = cpw;
        std::printf("var_cpw %d -> %d\n", cpw, resolve_schedule(&s).var_cpw);
    }
    s = sched();
    s.syn_blocks = 256;
    s.group_tiles = -1;
    s.pool_tiles = 5;
    s.poll_every = 3;
    show_sched("kept", s);
    return 0;
}
