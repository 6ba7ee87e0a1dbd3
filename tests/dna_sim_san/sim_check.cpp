// sim_check.cpp -- TEST INFRASTRUCTURE: the sequencing channel's host form
// (csrc/dna_sim.hpp) under ASan + UBSan, as a stand-alone host program (no
// HIP).  tests/test_dna_sim_san.py compiles it with g++ into a temporary
// directory and runs it:
//
//   sim_check
//
// Every input and every output lives in a heap buffer of exactly its size
// (strands [S][L], the tables [nq], reads [n][stride], lengths / quals /
// strand_of [n]), so a read or write past an end is an ASan report.  The
// cases are the corner rates on every shape of the Python tests -- nothing
// happens (the read is its strand), every base substituted (no byte equal),
// every slot inserts (2L + 1 bytes, the strand at the odd positions: the
// longest read fills its slot to the last defined byte), every base deleted
// (length 0), a mixed rate -- with the properties of the definition checked
// here (strand < S, quality from the table, prefix and split ranges, the last
// read range the key holds), and the argument errors, which must leave the
// outputs untouched.  Exit status 0 iff every check held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../dna-ldpc-codes_amd/csrc/dna_sim.hpp"

using namespace ldpc;

static int fails = 0, n_cases = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);          \
            fails++;                           \
        }                                      \
    } while (0)

template <class T>
static std::unique_ptr<T[]> heap(size_t n, T fill)
{
    std::unique_ptr<T[]> p(new T[n]);  // exactly n (n = 0: a valid pointer to nothing)
    for (size_t i = 0; i < n; i++) p[i] = fill;
    return p;
}

struct Run {
    int32_t S, L;
    int64_t n, st;
    std::unique_ptr<uint8_t[]> strands, reads;
    std::unique_ptr<int32_t[]> q_val, lengths, quals, strand_of;
    std::unique_ptr<uint32_t[]> q_lo;
    int32_t nq;
    std::string err;
};

static const int64_t kOne = sim::kOne;

static Run run(int32_t S, int32_t L, uint64_t seed, int64_t r0, int64_t n, int64_t t_sub, int64_t t_ins, int64_t t_del)
{
    Run r;
    r.S = S;
    r.L = L;
    r.n = n;
    r.st = sim::stride(L);
    r.strands = heap<uint8_t>((size_t)S * (size_t)L, 0);
    for (size_t i = 0; i < (size_t)S * (size_t)L; i++) r.strands[i] = (uint8_t)"ACGT"[sim::splitmix64(i * 977 + (uint64_t)S) & 3];
    r.nq = 5;
    r.q_val = heap<int32_t>(5, 0);
    r.q_lo = heap<uint32_t>(5, 0);
    const int32_t qv[5] = {33, 40, 53, 63, 70};
    const uint32_t ql[5] = {0u, 1u << 28, 1u << 30, 1u << 31, 0xf0000000u};
    for (int i = 0; i < 5; i++) {
        r.q_val[i] = qv[i];
        r.q_lo[i] = ql[i];
    }
    r.reads = heap<uint8_t>((size_t)(n * r.st), (uint8_t)'#');
    r.lengths = heap<int32_t>((size_t)n, -7);
    r.quals = heap<int32_t>((size_t)n, -7);
    r.strand_of = heap<int32_t>((size_t)n, -7);
    r.err = sim::reads_host(sim::Args{r.strands.get(), S, L, seed, r0, n, t_sub, t_ins, t_del, r.q_val.get(),
                                      r.q_lo.get(), r.nq, r.reads.get(), r.lengths.get(), r.quals.get(),
                                      r.strand_of.get()});
    return r;
}

// what holds of every read whatever the rates
static void check_common(const Run& r, const char* what)
{
    CHECK(r.err.empty(), "%s: %s", what, r.err.c_str());
    for (int64_t i = 0; i < r.n; i++) {
        const int32_t len = r.lengths[i], s = r.strand_of[i], q = r.quals[i];
        CHECK(len >= 0 && len <= 2 * r.L + 1, "%s: read %lld has length %d", what, (long long)i, len);
        CHECK(s >= 0 && s < r.S, "%s: read %lld has strand %d", what, (long long)i, s);
        CHECK(q == 33 || q == 40 || q == 53 || q == 63 || q == 70, "%s: read %lld has quality %d", what, (long long)i, q);
        for (int32_t j = 0; j < len && j <= 2 * r.L; j++) {
            const uint8_t c = r.reads[(size_t)(i * r.st + j)];
            CHECK(c == 'A' || c == 'C' || c == 'G' || c == 'T', "%s: read %lld byte %d is %d", what, (long long)i, j, c);
        }
        for (int64_t j = len; j < r.st; j++)  // nothing is written past the read
            CHECK(r.reads[(size_t)(i * r.st + j)] == '#', "%s: read %lld wrote byte %lld", what, (long long)i, (long long)j);
    }
}

static void shape(int32_t S, int32_t L, int64_t n)
{
    char what[96];
    std::snprintf(what, sizeof what, "S %d L %d n %lld", S, L, (long long)n);
    n_cases++;
    {  // nothing happens
        const Run r = run(S, L, 3, 0, n, 0, 0, 0);
        check_common(r, what);
        for (int64_t i = 0; i < n; i++)
            CHECK(r.lengths[i] == L && !std::memcmp(&r.reads[(size_t)(i * r.st)], &r.strands[(size_t)r.strand_of[i] * L], (size_t)L),
                  "%s: rate 0 read %lld is not its strand", what, (long long)i);
    }
    {  // every base substituted
        const Run r = run(S, L, 3, 0, n, kOne, 0, 0);
        check_common(r, what);
        for (int64_t i = 0; i < n; i++) {
            CHECK(r.lengths[i] == L, "%s: sub 1 length", what);
            for (int32_t p = 0; p < L && r.lengths[i] == L; p++)
                CHECK(r.reads[(size_t)(i * r.st + p)] != r.strands[(size_t)r.strand_of[i] * L + p], "%s: sub 1 kept a base", what);
        }
    }
    {  // every slot inserts
        const Run r = run(S, L, 3, 0, n, 0, kOne, 0);
        check_common(r, what);
        for (int64_t i = 0; i < n; i++) {
            CHECK(r.lengths[i] == 2 * L + 1, "%s: ins 1 length %d", what, r.lengths[i]);
            for (int32_t p = 0; p < L && r.lengths[i] == 2 * L + 1; p++)
                CHECK(r.reads[(size_t)(i * r.st + 2 * p + 1)] == r.strands[(size_t)r.strand_of[i] * L + p], "%s: ins 1 moved a base", what);
        }
    }
    {  // every base deleted; with every slot inserting, L + 1 bytes remain
        const Run r = run(S, L, 3, 0, n, 0, 0, kOne);
        check_common(r, what);
        for (int64_t i = 0; i < n; i++) CHECK(r.lengths[i] == 0, "%s: del 1 length %d", what, r.lengths[i]);
        const Run r2 = run(S, L, 3, 0, n, 0, kOne, kOne);
        check_common(r2, what);
        for (int64_t i = 0; i < n; i++) CHECK(r2.lengths[i] == L + 1, "%s: del 1 ins 1 length %d", what, r2.lengths[i]);
    }
    {  // mixed rates: prefix, split range, far range
        const int64_t t = kOne / 20;
        const Run whole = run(S, L, 9, 0, n, t, t, t);
        check_common(whole, what);
        const int64_t h = n / 3;
        const Run a = run(S, L, 9, 0, h, t, t, t), b = run(S, L, 9, h, n - h, t, t, t);
        check_common(a, what);
        check_common(b, what);
        for (int64_t i = 0; i < n; i++) {
            const Run& part = i < h ? a : b;
            const int64_t k = i < h ? i : i - h;
            CHECK(part.lengths[k] == whole.lengths[i] && part.quals[k] == whole.quals[i] &&
                      part.strand_of[k] == whole.strand_of[i] &&
                      !std::memcmp(&part.reads[(size_t)(k * part.st)], &whole.reads[(size_t)(i * whole.st)], (size_t)whole.st),
                  "%s: split range differs at read %lld", what, (long long)i);
        }
        const Run far = run(S, L, 9, sim::kMaxRead - n, n, t, t, t);  // the last reads the key holds
        check_common(far, what);
    }
}

static void errors()
{
    n_cases++;
    const int64_t t = kOne / 50;
    struct Bad { const char* what; int32_t S, L; int64_t r0, n, t_sub, t_ins, t_del; };
    const Bad bad[] = {
        {"no strands", 0, 24, 0, 4, t, t, t},          {"L 0", 3, 0, 0, 4, t, t, t},
        {"L 400", 3, 400, 0, 4, t, t, t},               {"negative r0", 3, 24, -1, 4, t, t, t},
        {"negative n", 3, 24, 0, -1, t, t, t},          {"r past 2^40", 3, 24, sim::kMaxRead - 3, 4, t, t, t},
        {"r0 huge", 3, 24, INT64_MAX, 4, t, t, t},      {"t_sub < 0", 3, 24, 0, 4, -1, t, t},
        {"t_ins < 0", 3, 24, 0, 4, t, -1, t},           {"t_del < 0", 3, 24, 0, 4, t, t, -1},
        {"t_sub > 1", 3, 24, 0, 4, kOne + 1, 0, 0},     {"t_ins > 1", 3, 24, 0, 4, 0, kOne + 1, 0},
        {"t_del > 1", 3, 24, 0, 4, 0, 0, kOne + 1},     {"sub + del > 1", 3, 24, 0, 4, kOne, 0, 1},
        {"thresholds huge", 3, 24, 0, 4, INT64_MAX, 0, INT64_MAX},
    };
    for (const Bad& b : bad) {
        const Run r = run(b.S > 0 ? b.S : 0, b.L > 0 && b.L <= 400 ? b.L : 0, 1, b.r0, b.n > 0 ? b.n : 0, 0, 0, 0);
        // (buffers of the right shape; the bad values go in here)
        const std::string err = sim::reads_host(sim::Args{r.strands.get(), b.S, b.L, 1, b.r0, b.n, b.t_sub, b.t_ins, b.t_del,
                                                          r.q_val.get(), r.q_lo.get(), r.nq, nullptr, nullptr, nullptr, nullptr});
        CHECK(!err.empty(), "%s: accepted", b.what);
    }
    // tables, strand bytes and null pointers, on buffers that must stay as they are
    Run r = run(3, 24, 1, 0, 4, 0, 0, 0);
    auto args = [&] {
        return sim::Args{r.strands.get(), 3, 24, 1, 0, 4, t, t, t, r.q_val.get(), r.q_lo.get(), r.nq,
                         r.reads.get(), r.lengths.get(), r.quals.get(), r.strand_of.get()};
    };
    for (int64_t i = 0; i < 4; i++) r.lengths[i] = -7;
    auto rejects = [&](sim::Args a, const char* what) {
        CHECK(!sim::reads_host(a).empty(), "%s: accepted", what);
        for (int64_t i = 0; i < 4; i++) CHECK(r.lengths[i] == -7, "%s: wrote before failing", what);
    };
    sim::Args a = args();
    a.strands = nullptr; rejects(a, "null strands");
    a = args(); a.q_val = nullptr; rejects(a, "null q_val");
    a = args(); a.q_lo = nullptr; rejects(a, "null q_lo");
    a = args(); a.nq = 0; rejects(a, "nq 0");
    a = args(); a.nq = 257; rejects(a, "nq 257");
    a = args(); a.reads = nullptr; rejects(a, "null reads");
    a = args(); a.lengths = nullptr; rejects(a, "null lengths");
    a = args(); a.quals = nullptr; rejects(a, "null quals");
    r.q_lo[0] = 1; rejects(args(), "q_lo[0] != 0"); r.q_lo[0] = 0;
    r.q_lo[3] = r.q_lo[2] - 1; rejects(args(), "descending q_lo"); r.q_lo[3] = 1u << 31;
    r.strands[3 * 24 - 1] = 'N'; rejects(args(), "strand byte N"); r.strands[3 * 24 - 1] = 'A';
    r.strands[0] = 'a'; rejects(args(), "strand byte a"); r.strands[0] = 'A';
    a = args(); a.strand_of = nullptr;
    CHECK(sim::reads_host(a).empty(), "null strand_of is allowed");
    a = args(); a.n = 0; a.reads = nullptr; a.lengths = nullptr; a.quals = nullptr;
    CHECK(sim::reads_host(a).empty(), "no reads need no outputs");
    CHECK(sim::stride(0) == 0 && sim::stride(1) == 16 && sim::stride(7) == 16 && sim::stride(8) == 32 &&
              sim::stride(152) == 320 && sim::stride(399) == 800 && sim::stride(400) == 0,
          "stride");
}

int main()
{
    const int32_t shapes[][2] = {{5, 1}, {7, 24}, {64, 64}, {100, 86}, {33, 152}, {3, 399}};
    const int64_t counts[] = {1, 63, 64, 65, 200};
    for (const auto& s : shapes)
        for (const int64_t n : counts) shape(s[0], s[1], n);
    errors();
    if (fails) {
        std::fprintf(stderr, "sim_check: %d checks failed\n", fails);
        return 1;
    }
    std::printf("sim_check ok: %d cases\n", n_cases);
    return 0;
}
