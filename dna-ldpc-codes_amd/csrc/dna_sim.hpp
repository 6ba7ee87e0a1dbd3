// dna_sim.hpp -- the sequencing channel: strands -> raw
// reads with substitutions, insertions and deletions, every draw a counter
// hash of (seed, read, stream, position), so a read depends on (seed, r) alone
// and a range of reads gives the same bytes however it is split.  Header-only
// host C++, no HIP: the body of ldpc_dna_sim_reads_host, the definition
// k_sim_reads (dna_sim_kernels.hpp) and synth.dna_raw_reads_hashed follow, and
// what tests/dna_sim_san/sim_check.cpp includes.  The draws themselves
// (LDPC_SIM_HD below) are compiled for both sides, so there is one statement
// of each.  Integers only: no floating point anywhere.
//
// Definition.  h(r, c, p) = splitmix64(((r << 24) | (c << 16) | p) ^ splitmix64(seed)),
// r < 2^40, stream c < 256, p < 2^16 (the keying of k_gen_bsc with a stream
// id); hi(x) = x >> 32, u(x) = x >> 11 (uniform in [0, 2^53)).
//   strand     (hi(h(r, 0, 0)) * S) >> 32
//   quality    q_val[i], i the largest index with q_lo[i] <= hi(h(r, 1, 0))
//   slot p     (p = 0 .. L) inserts iff u(h(r, 2, p)) < t_ins, the base
//              "ACGT"[(hi(h(r, 3, p)) * 4) >> 32]
//   base p     (p = 0 .. L - 1), e = u(h(r, 4, p)): deleted iff e < t_del,
//              substituted iff t_del <= e < t_del + t_sub by
//              "ACGT"[(b + 1 + ((hi(h(r, 5, p)) * 3) >> 32)) & 3], b the source
//              base's position in ACGT, else copied
//   read       for p = 0 .. L - 1: slot p's insertion, then base p unless
//              deleted; slot L's insertion last.  Length in [0, 2L + 1].
// Layout: read r - r0 starts at byte (r - r0) * stride(L); bytes of its slot
// beyond its length are not written.
#pragma once
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define LDPC_SIM_HD __host__ __device__ __forceinline__
#else
#define LDPC_SIM_HD inline
#endif

namespace ldpc {
namespace sim {

constexpr int32_t kMaxStrandNt = 399;           // 2L + 1 <= 800, the planner's read limit
constexpr int32_t kMaxQuals = 256;              // entries of the quality table
constexpr int64_t kOne = (int64_t)1 << 53;      // probability 1 as a threshold
constexpr int64_t kMaxRead = (int64_t)1 << 40;  // r0 + n_reads <= 2^40: the key holds r in 40 bits

enum : uint32_t { kStrand = 0, kQual = 1, kInsert = 2, kInsertBase = 3, kEvent = 4, kSubBase = 5 };  // stream ids

LDPC_SIM_HD uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// h(r, c, p) with seedmix = splitmix64(seed)
LDPC_SIM_HD uint64_t hash(uint64_t seedmix, uint64_t r, uint32_t c, uint32_t p)
{
    return splitmix64(((r << 24) | ((uint64_t)c << 16) | (uint64_t)p) ^ seedmix);
}

LDPC_SIM_HD uint8_t base_char(uint32_t k) { return (uint8_t)(0x54474341u >> (8 * (k & 3u))); }  // "ACGT"

// position in ACGT (a byte outside it reads as A: the strands are checked on the host)
LDPC_SIM_HD uint32_t base_pos(uint8_t c) { return c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u; }

LDPC_SIM_HD int64_t read_strand(uint64_t seedmix, uint64_t r, int32_t S)
{
    return (int64_t)(((hash(seedmix, r, kStrand, 0) >> 32) * (uint64_t)S) >> 32);
}

// index into the quality table: the largest i with q_lo[i] <= x (q_lo[0] = 0, so there is one)
LDPC_SIM_HD int32_t read_quality_index(uint64_t seedmix, uint64_t r, const uint32_t* q_lo, int32_t nq)
{
    const uint32_t x = (uint32_t)(hash(seedmix, r, kQual, 0) >> 32);
    int32_t lo = 0, hi = nq;  // first index with q_lo > x
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (q_lo[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// slot p: true when it inserts, *base the inserted character
LDPC_SIM_HD bool slot_inserts(uint64_t seedmix, uint64_t r, uint32_t p, uint64_t t_ins, uint8_t* base)
{
    if ((hash(seedmix, r, kInsert, p) >> 11) >= t_ins) return false;
    *base = base_char((uint32_t)(((hash(seedmix, r, kInsertBase, p) >> 32) * 4u) >> 32));
    return true;
}

// source base p with character c: false when deleted, else *out is the read's character
LDPC_SIM_HD bool base_kept(uint64_t seedmix, uint64_t r, uint32_t p, uint8_t c, uint64_t t_sub, uint64_t t_del,
                           uint8_t* out)
{
    const uint64_t e = hash(seedmix, r, kEvent, p) >> 11;
    if (e < t_del) return false;
    *out = c;
    if (e < t_del + t_sub)
        *out = base_char(base_pos(c) + 1u + (uint32_t)(((hash(seedmix, r, kSubBase, p) >> 32) * 3u) >> 32));
    return true;
}

// bytes between the starts of two reads: 2L + 1 rounded up to a multiple of 16; 0 for an L outside 1 .. 399
inline int64_t stride(int32_t L)
{
    if (L < 1 || L > kMaxStrandNt) return 0;
    return ((int64_t)2 * L + 1 + 15) / 16 * 16;
}

struct Args {
    const uint8_t* strands;  // [S][L] over ACGT
    int32_t S, L;
    uint64_t seed;
    int64_t r0, n;  // reads [r0, r0 + n)
    int64_t t_sub, t_ins, t_del;
    const int32_t* q_val;
    const uint32_t* q_lo;
    int32_t nq;
    uint8_t* reads;      // [n][stride(L)]
    int32_t* lengths;    // [n]
    int32_t* quals;      // [n]
    int32_t* strand_of;  // [n] or null
};

// The argument errors of the channel itself (every form, the trial's included); empty: none.
inline std::string check_channel(int32_t L, int64_t r0, int64_t n, int64_t t_sub, int64_t t_ins, int64_t t_del,
                                 const int32_t* q_val, const uint32_t* q_lo, int32_t nq)
{
    if (L < 1 || L > kMaxStrandNt) return "strand_nt must be in 1 .. 399 (a read of 2 * strand_nt + 1 bytes stays within 800)";
    if (r0 < 0 || n < 0 || r0 > kMaxRead || n > kMaxRead - r0) return "the reads must lie in [0, 2^40)";
    if (t_sub < 0 || t_ins < 0 || t_del < 0 || t_sub > kOne || t_ins > kOne || t_del > kOne || t_sub + t_del > kOne)
        return "thresholds must be in [0, 2^53] with t_sub + t_del <= 2^53";
    if (nq < 1 || nq > kMaxQuals || !q_val || !q_lo) return "the quality table needs 1 .. 256 entries";
    if (q_lo[0] != 0) return "q_lo[0] must be 0";
    for (int32_t i = 1; i < nq; i++)
        if (q_lo[i] < q_lo[i - 1]) return "q_lo must be ascending";
    return std::string();
}

// The strands: [S][L] over ACGT, S >= 1.
inline std::string check_strands(const uint8_t* strands, int64_t S, int32_t L)
{
    if (S < 1 || S > INT32_MAX || !strands) return "needs 1 .. 2^31 - 1 strands";
    if (L < 1 || L > kMaxStrandNt) return "strand_nt must be in 1 .. 399 (a read of 2 * strand_nt + 1 bytes stays within 800)";
    for (int64_t i = 0; i < S * (int64_t)L; i++) {
        const uint8_t c = strands[i];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T')
            return "strand " + std::to_string(i / L) + " holds a byte outside ACGT at position " + std::to_string(i % L);
    }
    return std::string();
}

// Every argument error of ldpc_dna_sim_reads_host / ldpc_dna_sim_reads, before anything else happens.
inline std::string check_args(const Args& a)
{
    std::string err = check_strands(a.strands, a.S, a.L);
    if (err.empty()) err = check_channel(a.L, a.r0, a.n, a.t_sub, a.t_ins, a.t_del, a.q_val, a.q_lo, a.nq);
    if (err.empty() && a.n > 0 && (!a.reads || !a.lengths || !a.quals)) err = "null reads, lengths or quals";
    if (err.empty() && a.n > INT64_MAX / stride(a.L)) err = "the reads overflow the address space";
    return err;
}

// The channel on one thread.  Returns an empty string or the argument error.
inline std::string reads_host(const Args& a)
{
    const std::string err = check_args(a);
    if (!err.empty()) return err;
    const uint64_t seedmix = splitmix64(a.seed);
    const uint64_t t_sub = (uint64_t)a.t_sub, t_ins = (uint64_t)a.t_ins, t_del = (uint64_t)a.t_del;
    const int64_t st = stride(a.L);
    for (int64_t i = 0; i < a.n; i++) {
        const uint64_t r = (uint64_t)(a.r0 + i);
        const int64_t s = read_strand(seedmix, r, a.S);
        const uint8_t* src = a.strands + (size_t)s * (size_t)a.L;
        uint8_t* dst = a.reads + (size_t)i * (size_t)st;
        int32_t len = 0;
        uint8_t c;
        for (int32_t p = 0; p <= a.L; p++) {
            if (slot_inserts(seedmix, r, (uint32_t)p, t_ins, &c)) dst[len++] = c;
            if (p < a.L && base_kept(seedmix, r, (uint32_t)p, src[p], t_sub, t_del, &c)) dst[len++] = c;
        }
        a.lengths[i] = len;
        a.quals[i] = a.q_val[read_quality_index(seedmix, r, a.q_lo, a.nq)];
        if (a.strand_of) a.strand_of[i] = (int32_t)s;
    }
    return std::string();
}

}  // namespace sim
}  // namespace ldpc
