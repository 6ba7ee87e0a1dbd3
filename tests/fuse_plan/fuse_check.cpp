// fuse_check.cpp -- stand-alone check of the fused row block's eligibility
// (csrc/engine_plan.hpp: fuse_row_block_of, plan_engine's fuse_block; no HIP).
// tests/test_fuse_plan.py builds it and compares the lines.
//   fuse_check <name>=<.pchk> ...      (the name rs7 needs no file: RS-LDPC(7, 72, 8))
// One line per graph: the block search, then plan_engine's fuse_block for
//   bp        the defaults
//   cpw       BP with an explicit var_cpw (2)
//   msa       min-sum (fp64 messages, so the pool is resident)
//   grouped   BP, LDPC_SCHED_RESIDENT off
//   off       BP, LDPC_SCHED_FUSE_ROW_BLOCK off
//   on        BP, LDPC_SCHED_FUSE_ROW_BLOCK set on by the caller
#include <cstdio>
#include <cstring>
#include <string>

#include "../../dna-ldpc-codes_amd/csrc/engine_plan.hpp"

using namespace ldpc;

static int fuse(const HostGraph& g, int algo, int32_t set, int32_t flags, int32_t cpw = 0)
{
    ldpc_schedule s{};
    s.flags_set = set;
    s.flags = flags;
    s.var_cpw = cpw;
    const ldpc_schedule r = resolve_schedule(&s);
    const EnginePlan p = plan_engine(g, algo, 0, r, 200000000000ull);
    if (p.error) return -99;
    if (p.fuse_block >= 0 && !p.res) return -98;  // never outside the resident pool
    return p.fuse_block;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++) {
        const char* eq = std::strchr(argv[i], '=');
        const std::string name = eq ? std::string(argv[i], (size_t)(eq - argv[i])) : std::string(argv[i]);
        HostGraph g;
        std::string msg;
        const int rc = eq ? load_pchk(eq + 1, g, &msg) : build_rs_ldpc(7, 72, 8, g, nullptr, nullptr, &msg);
        if (rc != LDPC_OK) {
            std::fprintf(stderr, "%s: %s\n", name.c_str(), msg.c_str());
            return 2;
        }
        const int32_t F = LDPC_SCHED_FUSE_ROW_BLOCK, R = LDPC_SCHED_RESIDENT, C = LDPC_SCHED_MSA_COMPRESSED;
        std::printf("%s: M=%d N=%d block=%d bp=%d cpw=%d msa=%d grouped=%d off=%d on=%d\n", name.c_str(), g.M, g.N,
                    fuse_row_block_of(g), fuse(g, LDPC_ALGO_BP, 0, 0), fuse(g, LDPC_ALGO_BP, 0, 0, 2),
                    fuse(g, LDPC_ALGO_MSA, C, 0), fuse(g, LDPC_ALGO_BP, R, 0), fuse(g, LDPC_ALGO_BP, F, 0),
                    fuse(g, LDPC_ALGO_BP, F, F));
    }
    return 0;
}
