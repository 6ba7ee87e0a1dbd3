// engine_plan.hpp -- what an engine decides before it allocates anything: the
// resolved schedule and, from the graph, the algorithm, the chunk and the free
// device memory, which kernels run and how large every buffer is
// (plan_engine).  Pure host code, no HIP: tests/engine_plan/plan_check.cpp
// runs it on a CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/ldpc_amd.h"
#include "graph.hpp"

namespace ldpc {

// Defaults, each chosen by a same-process A/B on MI355X (profiles/r*/README.md).
constexpr int32_t kDefaultGroupTiles = 3;     // grouped schedule (tools/sweep.py)
constexpr int32_t kDefaultMsaGroupTiles = 8;  // compressed min-sum, 1024-lane pool: one tile per XCD (+2.7 %)
constexpr int32_t kDefaultVarCpw = 4;         // fp64 priors: +2.6-2.9 % over 1 column per wave
constexpr int32_t kDefaultVarCpwCoded = 2;    // coded priors, resident pool / compressed min-sum: +0.5 % / +1.9 %
                                              // over 4 (the grouped BP schedule stays at 4: 2 is 10 % slower)
constexpr int32_t kDefaultPoolTiles = 3;      // resident pool: 3 x 85 MB ~ the 256 MB Infinity Cache
constexpr int32_t kDefaultResPoll = 8;
constexpr int32_t kDefaultSynBlocks = 32;     // continuous-mode syndrome blocks per tile (config 5 +5-6 %)
constexpr int64_t kMsaPool = 1024;            // compressed min-sum lanes (scattered v2c stores: small pool)
constexpr int64_t kResAutoMaxTiles = 4;       // explicit pools above this: grouped unless RESIDENT is set

constexpr int32_t kDefaultFlags = LDPC_SCHED_NONTEMPORAL | LDPC_SCHED_CONTINUOUS | LDPC_SCHED_MSA_COMPRESSED |
                                  LDPC_SCHED_RESIDENT | LDPC_SCHED_FIRST_FROM_PRIOR | LDPC_SCHED_LR_TABLE |
                                  LDPC_SCHED_HANDOVER;
constexpr int32_t kAllFlags = kDefaultFlags | LDPC_SCHED_DEBUG_NO_DRAIN | LDPC_SCHED_DEBUG_BAD_LANE;

// flags_set bits of a resolved schedule, outside kAllFlags: resolved, and
// whether the caller chose the resident pool (the auto-disable rule for
// large explicit pools applies only when it did not).  A caller's bits
// outside kAllFlags are dropped, so no caller can mark a schedule resolved.
// kNoFuse: the caller turned LDPC_SCHED_FUSE_ROW_BLOCK off.  That flag is on
// by default, but a resolved schedule carries it as this mark and not in the
// low word: the resolved words of bits 0..15 are what they were before the
// flag existed (tests/test_engine_plan.py states them), and the rule above
// still holds.
constexpr int32_t kResolved = 1 << 30, kResChosen = 1 << 29, kNoFuse = 1 << 28;

// A caller's ldpc_schedule with every field resolved: flags_set covers all
// bits, zero fields replaced by the defaults (include/ldpc_amd.h).  Two
// resolved schedules compare equal iff they select the same engine.  The
// input is always treated as a caller's (bits outside LDPC_SCHED_* dropped).
inline ldpc_schedule resolve_schedule(const ldpc_schedule* s)
{
    ldpc_schedule r{};
    if (s) r = *s;
    const bool no_fuse = (r.flags_set & LDPC_SCHED_FUSE_ROW_BLOCK) && !(r.flags & LDPC_SCHED_FUSE_ROW_BLOCK);
    r.flags_set &= kAllFlags;
    r.flags = (kDefaultFlags & ~r.flags_set) | (r.flags & r.flags_set);
    r.flags &= kAllFlags;
    r.flags_set = kAllFlags | kResolved | ((r.flags_set & LDPC_SCHED_RESIDENT) ? kResChosen : 0) |
                  (no_fuse ? kNoFuse : 0);
    if (r.group_tiles == 0) r.group_tiles = -2;  // per-algorithm default, resolved by plan_engine
    // (3: compressed min-sum only; the fp64 variable kernels take 1, 2, 4 or
    // 8); -2: the default, chosen per decode by the prior's form (var_cpw_for)
    if (r.var_cpw < 1 || r.var_cpw > 8 || (r.var_cpw > 4 && r.var_cpw != 8)) r.var_cpw = -2;
    if (r.pool_tiles <= 0) r.pool_tiles = 0;  // the default, resolved by plan_engine (kDefaultPoolTiles / gen_pool_tiles)
    if (r.poll_every <= 0) r.poll_every = kDefaultResPoll;
    if (r.syn_blocks <= 0) r.syn_blocks = kDefaultSynBlocks;
    r.syn_blocks = std::min(r.syn_blocks, 256);
    r.reserved = 0;
    return r;
}
inline bool sched_flag(const ldpc_schedule& s, int bit) { return (s.flags & bit) != 0; }

// Degree buckets of the register-staged generic kernels (kernels.hpp
// k_check_gr / k_var_gr and their lane-pool forms), ascending.  Each list is
// stated here only: gen_bucket and the launches (dispatch) both run over it.
template <int... Ds>
using Buckets = std::integer_sequence<int, Ds...>;
using CheckBuckets = Buckets<8, 16, 32, 48, 64, 96>;
using VarBuckets = Buckets<4, 8, 12, 16, 24, 32>;

// the smallest bucket >= the graph's maximum degree, 0 when none holds it
// (the memory-staged *_gen kernels then run; no continuous mode without a
// variable bucket)
template <int... Ds>
inline int gen_bucket(int32_t dmax, Buckets<Ds...>)
{
    int b = 0;
    (void)((dmax <= Ds && (b = Ds, true)) || ...);
    return b;
}

// Default resident pool of a code other than the (8, 72)-regular one: as many
// tiles as keep the pool's messages + fp64 priors within the DNA pool's
// footprint (kDefaultPoolTiles x 85 MB ~ the 256 MB Infinity Cache).
constexpr double kGenPoolBytes = 226e6;
inline int32_t gen_pool_tiles(const HostGraph& g)
{
    const double per_tile = 64.0 * 8.0 * ((double)g.E + (double)g.N);
    return (int32_t)std::max(1.0, std::min(256.0, std::floor(kGenPoolBytes / std::max(per_tile, 1.0))));
}

// bytes of device memory per resident codeword
inline int64_t engine_bytes_per_codeword(const HostGraph& g)
{
    // v2c + c2v (E fp64 each) + prior (N fp64) + hard (N bits) + state
    return 2 * g.E * 8 + (int64_t)g.N * 8 + (g.N + 7) / 8 + 8;
}

// Layout constants of the compressed min-sum that the plan needs; the
// kernels' own (kernels.hpp TILE, MSA_REC_PLANES, MSA_ER_SHIFT) are checked
// against them in engine.hip.
constexpr int kTile = 64, kMsaRecPlanes = 4, kMsaErShift = 18;

// MSA-C scratch of `tiles` group tiles: record planes [tiles][M][4][64] fp64
// (m1, m2, n0, n1), then the meta words [tiles][M][64] u16
inline size_t msa_scratch_bytes(int64_t tiles, int32_t M)
{
    return (size_t)tiles * M * kTile * (kMsaRecPlanes * sizeof(double) + sizeof(uint16_t));
}

// The fused row block (LDPC_SCHED_FUSE_ROW_BLOCK) of a graph with dv row
// blocks of Q = M / dv rows: the first block a whose rows [aQ, (a+1)Q) hold
// every column exactly once, -1 when there is none.  Each row of that block
// then owns its dc columns: no other row of the block touches them.
inline int fuse_row_block_of(const HostGraph& g)
{
    const int dv = g.dv_max;
    if (dv <= 0 || g.M % dv != 0 || !g.regular_dc) return -1;
    const int32_t Q = g.M / dv;
    if ((int64_t)Q * g.dc_max != g.N) return -1;
    std::vector<uint8_t> seen((size_t)g.N);
    for (int a = 0; a < dv; a++) {
        std::fill(seen.begin(), seen.end(), (uint8_t)0);
        bool once = true;
        for (int64_t e = (int64_t)a * Q * g.dc_max; once && e < (int64_t)(a + 1) * Q * g.dc_max; e++) {
            uint8_t& c = seen[(size_t)g.col_idx[(size_t)e]];
            once = c == 0;
            c = 1;
        }
        if (once) return a;  // Q * dc = N distinct columns: all of them
    }
    return -1;
}

struct EnginePlan {
    bool msa_c = false;       // min-sum with compressed c2v (records + meta words, k_check_msa_c / k_var_msa_c)
    bool cont = false;        // continuous batching: refill lanes as codewords finish
    bool res = false;         // resident pool: a few tiles iterated in place, syndrome in the check kernel
    bool handover = false;    // res, (8,72)-regular: a lane is refilled during its codeword's last update (ResStep::last)
    int fuse_block = -1;      // res, (8,72)-regular BP: the row block whose check runs in the variable kernel
                              // (k_var_bp_fused; k_check_bp skips its messages), -1: none
    bool nt_d = false;        // nontemporal loads/stores of the v2c ("d") stream
    bool first_fp = false;    // single-fill BP: the first check reads the prior (k_check_bp_first)
    bool debug_no_drain = false;  // LDPC_SCHED_DEBUG_NO_DRAIN: the host ignores a drained pool
    bool debug_bad_lane = false;  // LDPC_SCHED_DEBUG_BAD_LANE: one lane records an out-of-range codeword index
    int var_cpw = 4;          // variable phase: columns per wave (-2: by the prior's form, var_cpw_for)
    int res_poll = 8;         // res: steps between occupancy polls
    int syn_blocks = 0;       // continuous grouped mode: k_syndrome_split blocks per tile
    int64_t cap = 0;          // codewords per pass / lane pool (multiple of 64)
    int64_t cap_tiles = 0;
    int64_t group_tiles = 0;  // tiles per check/variable launch; the scratch holds only one group
    int64_t c2v_tiles = 0;    // tiles of c2v scratch allocated (res: the pool's, in place)
    size_t c2v_bytes = 0;     // bytes of that scratch (res: none)
    const char* error = nullptr;  // not null: LDPC_ERR_ARG with this message, nothing else is valid
};

// Everything Engine::init decides.  `s` is resolved (resolve_schedule);
// chunk <= 0 sizes the engine from free_bytes (not read otherwise).
inline EnginePlan plan_engine(const HostGraph& g, int algo, int64_t chunk, const ldpc_schedule& s, size_t free_bytes)
{
    EnginePlan p;
    const bool int_algo = algo >= LDPC_ALGO_QMSA;
    const bool reg_72_8 = g.regular_dc && g.dc_max == 72 && g.regular_dv && g.dv_max == 8;
    // compressed min-sum: the packed column table carries edge ids (E < 2^18)
    p.msa_c = algo == LDPC_ALGO_MSA && reg_72_8 && g.N % 16 == 0 && g.E < ((int64_t)1 << kMsaErShift) &&
              sched_flag(s, LDPC_SCHED_MSA_COMPRESSED);
    // continuous mode: the specialised kernels, or any code whose column
    // degrees fit a register bucket of the generic continuous variable kernel
    // (k_var_gr_cont; its syndrome k_syndrome_split_gen)
    p.cont = sched_flag(s, LDPC_SCHED_CONTINUOUS) && !int_algo &&
             (reg_72_8 || (g.regular_dv && g.dv_max == 8) || gen_bucket(g.dv_max, VarBuckets{}) != 0);
    // resident pool: a few tiles whose whole state fits the
    // Infinity Cache, check->variable messages written over the variable->check
    // messages they are computed from (each row's / column's edges are read
    // into registers before its outputs are stored), no c2v scratch
    // (other codes: row and column degrees in register buckets, k_check_gr_res + k_var_gr_cont in place)
    const bool gen_res = !reg_72_8 && gen_bucket(g.dc_max, CheckBuckets{}) != 0 &&
                         gen_bucket(g.dv_max, VarBuckets{}) != 0;
    p.res = sched_flag(s, LDPC_SCHED_RESIDENT) && p.cont && !p.msa_c && ((reg_72_8 && g.N % 32 == 0) || gen_res);
    // by default the resident pool is the Infinity-Cache-sized one: a caller's
    // explicit larger pool (the host API's chunks, the DNA batch) runs the
    // grouped schedule (A/B, 272-codeword DNA batch at cap 320: 193k -> 250k cw/s)
    const bool res_chosen = (s.flags_set & kResChosen) != 0;
    if (p.res && !res_chosen && chunk > kResAutoMaxTiles * 64) p.res = false;
    // an (8, 72)-regular code larger than the DNA code: its default 3-tile pool
    // would overflow the Infinity Cache (RS(9,72,8), N = 36 864: 509 MB, 12 %
    // slower than the grouped schedule, profiles/r6/generic_codes.txt)
    if (p.res && !res_chosen && reg_72_8 && s.pool_tiles <= 0 &&
        64.0 * 8.0 * kDefaultPoolTiles * ((double)g.E + (double)g.N) > 1.15 * kGenPoolBytes)
        p.res = false;
    p.nt_d = sched_flag(s, LDPC_SCHED_NONTEMPORAL) && !p.res;  // the pool is meant to stay cached
    // hand-over: k_check_bp / k_check_msa<72, ., RES> + k_var_m in place only
    p.handover = sched_flag(s, LDPC_SCHED_HANDOVER) && p.res && reg_72_8 &&
                 (algo == LDPC_ALGO_BP || algo == LDPC_ALGO_MSA);
    // fused row block: k_var_bp_fused in place of k_var_m at its default
    // columns per wave (an explicit var_cpw keeps k_var_m)
    if (!(s.flags_set & kNoFuse) && p.res && reg_72_8 && algo == LDPC_ALGO_BP && s.var_cpw == -2)
        p.fuse_block = fuse_row_block_of(g);
    p.debug_no_drain = sched_flag(s, LDPC_SCHED_DEBUG_NO_DRAIN);
    p.debug_bad_lane = sched_flag(s, LDPC_SCHED_DEBUG_BAD_LANE);
    p.var_cpw = s.var_cpw;
    p.res_poll = s.poll_every;
    if (chunk <= 0) {
        // half of the free memory for the resident state, at most 16384 codewords;
        // compressed min-sum in continuous mode: a small lane pool (its scattered
        // v2c stores run ~45 % longer over a 19 GB pool than over 1.2 GB, A/B)
        const int64_t ptiles = s.pool_tiles > 0 ? s.pool_tiles : reg_72_8 ? kDefaultPoolTiles : gen_pool_tiles(g);
        const int64_t want = p.res ? 64 * ptiles : (p.msa_c && p.cont) ? kMsaPool : 16384;
        chunk = std::min<int64_t>(want, (int64_t)(free_bytes / 2) / engine_bytes_per_codeword(g));
    }
    p.cap = std::max<int64_t>(64, (chunk + 63) / 64 * 64);
    p.cap_tiles = p.cap / 64;
    if (p.cap_tiles > 65535) { p.error = "chunk too large (max 4194240 codewords)"; return p; }
    // group: tiles whose check->variable messages are live at once.  Small
    // groups keep c2v resident in the 256 MB Infinity Cache between the check
    // and the variable phase; the resident pool launches
    // each phase over the whole pool.
    int64_t group = s.group_tiles;
    if (group == -2) group = p.msa_c ? kDefaultMsaGroupTiles : kDefaultGroupTiles;
    p.group_tiles = (p.res || group <= 0 || group > p.cap_tiles) ? p.cap_tiles : group;
    if (p.cont) {
        // grouped continuous schedule: a separate syndrome launch spread over
        // several blocks per tile (the resident pool fuses it into the check)
        p.syn_blocks = p.res ? 0 : s.syn_blocks;
        // single fill (the DNA batch): step 0's refill stores only the prior and
        // step 1's check derives the first messages from it (k_check_bp_first)
        p.first_fp = !p.res && reg_72_8 && algo == LDPC_ALGO_BP && sched_flag(s, LDPC_SCHED_FIRST_FROM_PRIOR);
    }
    if (p.res) {
        p.c2v_tiles = p.cap_tiles;  // in place
    } else {
        // continuous mode's drain tail (< 1/32 occupancy) launches wider groups
        p.c2v_tiles = std::max<int64_t>(p.group_tiles, p.cont ? (p.cap_tiles + 3) / 4 : 0);
        const size_t E = (size_t)std::max<int64_t>(g.E, 1);
        p.c2v_bytes = p.msa_c ? msa_scratch_bytes(p.c2v_tiles, g.M) : (size_t)p.c2v_tiles * 64 * E * sizeof(double);
    }
    return p;
}

}  // namespace ldpc
