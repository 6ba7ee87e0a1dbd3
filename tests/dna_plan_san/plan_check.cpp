// plan_check.cpp -- TEST INFRASTRUCTURE: the read planner's host form
// (csrc/dna_plan.hpp, which brings star_align.hpp and rs_index.hpp) under
// ASan + UBSan, as a stand-alone host program (no HIP).
// tests/test_dna_plan_san.py compiles it with g++ into a temporary directory
// and runs it:
//
//   plan_check
//
// Every input and every output of a call lives in a heap buffer of exactly the
// size the contract gives it (seqs: the bytes the reads span, a null pointer
// for none; rows[max(n, 1)][nt], row_q[max(n, 1)], kind[S], row_ptr[S + 1],
// stats[9]), so a read or write past an end is an ASan report.  Rows from R on
// must keep the fill they were given.
// * no reads; no strands; reads whose index is no strand;
// * empty reads (quality 63: a '-' row, 64: the error), a single long and a
//   single short read, full-length reads in input order;
// * ragged strands with and without close pairs, with and without the aligner,
//   aligned widths equal to and different from payload_nt;
// * raw reads: prefixes made with rs_index.hpp, a read of 16 bytes (an empty
//   payload), shorter ones and a non-ACGT prefix (dropped);
// * the argument errors; the shared extent check of ragged reads
//   (ragged_reads.hpp) and the aligned-row rule (plan::aligned_row) on their own;
// * a dense case: 60 strands of 2..7 mutated reads, planned twice.
// Exit status 0 iff every check held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../dna-ldpc-codes_amd/csrc/dna_plan.hpp"

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

constexpr uint8_t kFill = 0xEE;

struct Out {
    std::string err;
    std::vector<int32_t> kind, row_q;
    std::vector<int64_t> row_ptr, stats;
    std::vector<std::string> rows;  // the R rows
};

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v)
{
    std::unique_ptr<T[]> p(v.empty() ? nullptr : new T[v.size()]);
    for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
    return p;
}

// One call.  index empty and raw = true: index_vals is null.
static Out run_plan(const std::vector<std::string>& reads, const std::vector<int32_t>& quals,
                const std::vector<int32_t>& index, bool raw, const std::vector<int32_t>& strands, int32_t nt,
                int32_t align)
{
    n_cases++;
    const int64_t n = (int64_t)reads.size();
    const int32_t S = (int32_t)strands.size();
    std::vector<uint8_t> bytes;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    for (const std::string& r : reads) {
        off.push_back((int64_t)bytes.size());
        len.push_back((int32_t)r.size());
        bytes.insert(bytes.end(), r.begin(), r.end());
    }
    auto h_seq = exact(bytes);
    auto h_off = exact(off);
    auto h_len = exact(len);
    auto h_q = exact(quals);
    auto h_idx = exact(index);
    auto h_str = exact(strands);
    const size_t cap = (size_t)(n > 0 ? n : 1);
    std::unique_ptr<int32_t[]> kind(S ? new int32_t[(size_t)S] : nullptr), row_q(new int32_t[cap]);
    std::unique_ptr<int64_t[]> row_ptr(new int64_t[(size_t)S + 1]), stats(new int64_t[plan::kNumStats]);
    std::unique_ptr<uint8_t[]> rows(new uint8_t[cap * (size_t)nt]);
    std::memset(rows.get(), kFill, cap * (size_t)nt);
    for (size_t i = 0; i < cap; i++) row_q[i] = -7;
    const plan::Args a{h_seq.get(), h_off.get(), h_len.get(), h_q.get(), n, raw ? nullptr : h_idx.get(), h_str.get(), S,
                       nt, align, kind.get(), row_ptr.get(), rows.get(), row_q.get(), stats.get()};
    Out o;
    o.err = plan::plan_host(a);
    if (!o.err.empty()) return o;
    o.kind.assign(kind.get(), kind.get() + S);
    o.row_ptr.assign(row_ptr.get(), row_ptr.get() + S + 1);
    o.stats.assign(stats.get(), stats.get() + plan::kNumStats);
    const int64_t R = o.row_ptr[(size_t)S];
    CHECK(o.row_ptr[0] == 0 && R >= 0 && R <= n && o.stats[plan::kStatRows] == R, "R = %lld of %lld reads", (long long)R,
          (long long)n);
    for (int32_t s = 0; s < S; s++) {
        CHECK(o.row_ptr[(size_t)s + 1] >= o.row_ptr[(size_t)s], "row_ptr falls at %d", s);
        CHECK(o.kind[(size_t)s] >= 0 && o.kind[(size_t)s] <= 3, "kind %d at %d", o.kind[(size_t)s], s);
        CHECK((o.kind[(size_t)s] == 0) == (o.row_ptr[(size_t)s + 1] == o.row_ptr[(size_t)s]), "kind 0 <=> no rows, at %d", s);
    }
    if (R < 0 || R > n) return o;
    for (int64_t r = 0; r < R; r++) o.rows.emplace_back((const char*)rows.get() + (size_t)r * (size_t)nt, (size_t)nt);
    o.row_q.assign(row_q.get(), row_q.get() + R);
    for (size_t b = (size_t)R * (size_t)nt; b < cap * (size_t)nt; b++)
        if (rows[b] != kFill) {
            CHECK(false, "byte %zu past the %lld rows was written", b, (long long)R);
            break;
        }
    for (size_t r = (size_t)R; r < cap; r++) CHECK(row_q[r] == -7, "row_q[%zu] past R was written", r);
    return o;
}

static std::string pad(const std::string& s, size_t nt) { return s + std::string(nt - s.size(), '-'); }

static std::string prefix_of(uint32_t index)
{
    const uint32_t w = rs::rs_index_codeword(index);
    std::string p;
    for (int k = 0; k < rs::kPrefixNt; k++) p.push_back((char)rs::rs_prefix_base(w, k));
    return p;
}

static uint64_t lcg_state = 12345;
static uint32_t rnd(uint32_t m)
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((lcg_state >> 33) % m);
}

static std::string random_read(size_t len)
{
    std::string s;
    for (size_t i = 0; i < len; i++) s.push_back("ACGT"[rnd(4)]);
    return s;
}

int main()
{
    const int32_t nt = 12;
    const std::vector<int32_t> st{3, 8, 20, 21};
    const std::string p = "ACGTTGCAACGG";  // nt bytes

    {  // no reads; no strands; an index that is no strand
        Out o = run_plan({}, {}, {}, false, st, nt, 1);
        CHECK(o.err.empty() && o.kind == std::vector<int32_t>(4, 0) && o.rows.empty(), "no reads");
        o = run_plan({p, p}, {60, 60}, {3, 8}, false, {}, nt, 1);
        CHECK(o.err.empty() && o.row_ptr == std::vector<int64_t>{0} && o.stats[plan::kStatValid] == 0, "no strands");
        o = run_plan({p, p, p}, {60, 61, 62}, {4, -1, 65536}, false, st, nt, 1);
        CHECK(o.err.empty() && o.rows.empty() && o.stats[plan::kStatValid] == 0, "foreign indices");
    }
    {  // single reads: empty, short, long; full-length reads in input order
        Out o = run_plan({"", "ACG", p + "TT", p, "AAAAAAAAAAAA"}, {63, 70, 50, 41, 42}, {3, 8, 20, 21, 21}, false, st, nt, 0);
        CHECK(o.err.empty() && o.kind == (std::vector<int32_t>{2, 2, 1, 1}), "single-read kinds");
        CHECK(o.rows == (std::vector<std::string>{pad("-", 12), pad("G", 12), p, p, "AAAAAAAAAAAA"}), "single-read rows");
        CHECK(o.row_q == (std::vector<int32_t>{63, 70, 50, 41, 42}), "single-read qualities");
        o = run_plan({"AAAAAAAAAAAA", "", p}, {42, 64, 41}, {21, 8, 21}, false, st, nt, 0);
        CHECK(o.err.find("empty read on strand 1 with quality > 63") == 0, "empty read of quality 64: '%s'", o.err.c_str());
        o = run_plan({"", ""}, {64, 64}, {8, 8}, false, st, nt, 1);  // two empty reads are a ragged strand, distance 0
        CHECK(o.err.empty() && o.kind[1] == 3 && o.rows == (std::vector<std::string>{pad("-", 12), pad("-", 12)}),
              "two empty reads");
    }
    {  // ragged strands
        const std::string far = "TTTTTTTTTTTTTTTTTTTTTTTTTTTTTT";  // 30 bytes: distance to p >= 18
        Out o = run_plan({p, far}, {60, 61}, {8, 8}, false, st, nt, 0);
        CHECK(o.err.empty() && o.kind[1] == 0 && o.rows.empty() && o.stats[plan::kStatPairs] == 1, "no close pair");
        o = run_plan({p, p.substr(0, 11)}, {60, 61}, {8, 8}, false, st, nt, 0);
        CHECK(o.err.find("need an aligner") != std::string::npos, "align = 0 with candidates: '%s'", o.err.c_str());
        o = run_plan({p.substr(0, 11), far, p}, {61, 62, 60}, {8, 8, 8}, false, st, nt, 1);
        CHECK(o.err.empty() && o.kind[1] == 1 && o.rows == (std::vector<std::string>{"ACGTTGCAAC-G", p}) &&
                  o.row_q == (std::vector<int32_t>{61, 60}),
              "aligned to payload_nt");
        CHECK(o.stats[plan::kStatPairs] == 3 && o.stats[plan::kStatAligned] == 1 && o.stats[plan::kStatAlignPairs] == 1,
              "aligned stats");
        o = run_plan({p + "GA", p, p.substr(0, 9) + "C"}, {67, 70, 40}, {20, 20, 20}, false, st, nt, 1);
        CHECK(o.err.empty() && o.kind[2] == 3 && o.rows == (std::vector<std::string>{pad("A", 12), pad("-", 12), pad("-", 12)}),
              "alignment wider than payload_nt");
    }
    {  // raw reads
        const std::string a = prefix_of(8), b = prefix_of(21);
        std::string bad = a;
        bad[2] = 'N';
        std::string one = b;
        one[5] = one[5] == 'A' ? 'C' : 'A';  // one symbol error
        Out o = run_plan({a + p, a, b.substr(0, 15), bad + p, one + p, b + p, ""}, {60, 61, 62, 63, 64, 65, 66}, {}, true, st,
                     nt, 1);
        // strand 8: p and an empty payload, distance 12 < 15 -> aligned to p's width
        CHECK(o.err.empty() && o.kind == (std::vector<int32_t>{0, 1, 0, 1}), "raw kinds");
        CHECK(o.rows == (std::vector<std::string>{p, pad("", 12), p, p}), "raw rows");
        CHECK(o.row_q == (std::vector<int32_t>{60, 61, 64, 65}), "raw qualities");
        CHECK(o.stats[plan::kStatCnumerr] == 3 && o.stats[plan::kStatCnumerr + 1] == 3 &&
                  o.stats[plan::kStatCnumerr + 2] == 1 && o.stats[plan::kStatCnumerr + 3] == 0,
              "cnumerr histogram");
    }
    {  // argument errors
        CHECK(!run_plan({p}, {60}, {3}, false, {3, 3}, nt, 1).err.empty(), "duplicate strands");
        CHECK(!run_plan({p}, {60}, {3}, false, {8, 3}, nt, 1).err.empty(), "unsorted strands");
        CHECK(!run_plan({p}, {60}, {3}, false, st, 0, 1).err.empty(), "payload_nt 0");
        int64_t total = 0;
        int32_t kind[1];
        int64_t row_ptr[2], off[1] = {0};
        int32_t len[1] = {-1}, q[1] = {0}, s1[1] = {3};
        uint8_t rows[12];
        plan::Args a{nullptr, off, len, q, 1, s1, s1, 1, nt, 1, kind, row_ptr, rows, q, nullptr};
        CHECK(plan::check_args(a, &total) == "negative or overflowing length/offset", "negative length");
        len[0] = 4;
        CHECK(plan::check_args(a, &total) == "null sequences", "null sequences");
        off[0] = INT64_MAX - 2;
        CHECK(plan::check_args(a, &total) == "negative or overflowing length/offset", "overflowing offset");
        a.n_reads = -1;
        CHECK(!plan::check_args(a, &total).empty(), "negative n_reads");
        a.n_reads = 1;
        off[0] = 0;
        a.row_ptr = nullptr;
        CHECK(!plan::check_args(a, &total).empty() && plan::check_args(a, &total, false).empty() == false, "null row_ptr");
        n_cases += 5;
    }
    {  // the extent check of ragged reads: arrays of exact size
        int64_t total = -1;
        int32_t max_len = -1;
        CHECK(ragged::check(nullptr, nullptr, nullptr, 0, &total).empty() && total == 0, "extent: n = 0");
        auto off = exact(std::vector<int64_t>{INT64_MAX, 4}), ovf = exact(std::vector<int64_t>{0, INT64_MAX - 2});
        auto len = exact(std::vector<int32_t>{0, 0}), len3 = exact(std::vector<int32_t>{1, 3}), neg = exact(std::vector<int32_t>{2, -1});
        CHECK(ragged::check(nullptr, off.get(), len.get(), 2, &total).empty() && total == 0,
              "extent: empty reads at large offsets span nothing");
        CHECK(ragged::extent(off.get(), len.get(), 2, &total, true, &max_len).empty() && total == INT64_MAX && max_len == 0,
              "extent: empty reads counted");
        uint8_t byte = 0;
        CHECK(ragged::check(&byte, ovf.get(), len3.get(), 2, &total) == "negative or overflowing length/offset",
              "extent: offset + length overflows");
        CHECK(ragged::check(&byte, off.get() + 1, neg.get(), 1, &total).empty() && total == 6, "extent: one read");
        CHECK(ragged::check(nullptr, off.get() + 1, neg.get(), 1, &total) == "null sequences", "extent: null sequences");
        CHECK(ragged::check(&byte, off.get(), neg.get(), 2, &total) == "negative or overflowing length/offset",
              "extent: negative length");
        CHECK(ragged::extent(ovf.get(), len3.get(), 1, &total, false, &max_len).empty() && total == 1 && max_len == 1,
              "extent: longest read");
        n_cases += 8;
    }
    {  // the aligned-row rule at width == nt, 0, nt - 1 and nt + 1: source and destination of exact size
        for (int64_t width : {(int64_t)nt, (int64_t)0, (int64_t)nt - 1, (int64_t)nt + 1}) {
            std::vector<uint8_t> src;
            for (int64_t j = 0; j < width; j++) src.push_back((uint8_t)('a' + j));
            auto row = exact(src);
            auto dst = exact(std::vector<uint8_t>((size_t)nt, (uint8_t)'-'));
            plan::aligned_row(row.get(), width, nt, dst.get());
            std::string want((size_t)nt, '-');
            if (width == nt) want.assign(src.begin(), src.end());
            else if (width > 0) want[0] = (char)src.back();
            CHECK(std::string((const char*)dst.get(), (size_t)nt) == want, "aligned_row at width %lld", (long long)width);
            n_cases++;
        }
    }
    {  // dense: 60 strands of 2..7 reads, mutated copies of a 40-nt payload, shuffled; twice the same
        const int32_t dnt = 40;
        std::vector<int32_t> strands, index, quals;
        std::vector<std::string> reads;
        for (int32_t s = 0; s < 60; s++) strands.push_back(100 + 7 * s);
        for (int32_t s = 0; s < 60; s++) {
            const std::string parent = random_read((size_t)dnt);
            const uint32_t k = 2 + rnd(6);
            for (uint32_t r = 0; r < k; r++) {
                std::string m = parent;
                for (uint32_t e = rnd(4); e > 0; e--) {
                    const uint32_t op = rnd(3), at = rnd((uint32_t)m.size());
                    if (op == 0) m[at] = "ACGT"[rnd(4)];
                    else if (op == 1) m.insert(m.begin() + at, "ACGT"[rnd(4)]);
                    else if (m.size() > 1) m.erase(m.begin() + at);
                }
                if (rnd(10) == 0) m = random_read(30 + rnd(20));
                reads.push_back(m);
                index.push_back(strands[(size_t)s]);
                quals.push_back(35 + (int32_t)rnd(40));
            }
        }
        for (size_t i = reads.size(); i > 1; i--) {
            const size_t j = rnd((uint32_t)i);
            std::swap(reads[i - 1], reads[j]);
            std::swap(index[i - 1], index[j]);
            std::swap(quals[i - 1], quals[j]);
        }
        const Out o1 = run_plan(reads, quals, index, false, strands, dnt, 1), o2 = run_plan(reads, quals, index, false, strands, dnt, 1);
        CHECK(o1.err.empty() && o1.kind == o2.kind && o1.row_ptr == o2.row_ptr && o1.rows == o2.rows && o1.row_q == o2.row_q,
              "dense case differs between two runs");
        CHECK(o1.stats[plan::kStatValid] == (int64_t)reads.size() && o1.stats[plan::kStatAligned] >= 10 &&
                  o1.stats[plan::kStatPairs] > o1.stats[plan::kStatAlignPairs],
              "dense stats: %lld valid, %lld aligned", (long long)o1.stats[0], (long long)o1.stats[2]);
        int seen[4] = {0, 0, 0, 0};
        for (int32_t kd : o1.kind) seen[kd]++;
        CHECK(seen[1] > 0 && seen[3] > 0, "dense kinds %d %d %d %d", seen[0], seen[1], seen[2], seen[3]);
    }
    if (fails) {
        std::fprintf(stderr, "plan_check: %d checks failed\n", fails);
        return 1;
    }
    std::printf("plan_check ok: %d cases\n", n_cases);
    return 0;
}
