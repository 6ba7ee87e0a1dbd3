// star_check.cpp -- TEST INFRASTRUCTURE: the centre-star aligner's host code
// (csrc/star_align.hpp) under ASan + UBSan, as a stand-alone host program (no
// HIP).  tests/test_star_align_san.py compiles it with g++ into a temporary
// directory and runs it:
//
//   star_check
//
// Every read lives in a heap buffer of exactly its length (an empty read is a
// null pointer) and every output row buffer has exactly k * width bytes, so a
// read or write past an end is an ASan report.
// * groups with empty reads and k = 1;
// * every single substitution, insertion and deletion of a 10-nt parent,
//   paired with the parent in both orders: distance 1, width 10 or 11, each
//   row without '-' is its read;
// * a group of five reads with ties, and one of two 700-nt reads.
// Exit status 0 iff every check held.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../dna-ldpc-codes_amd/csrc/star_align.hpp"

using namespace ldpc::star;

static int fails = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);          \
            fails++;                           \
        }                                      \
    } while (0)

struct Aligned {
    int64_t centre = 0, width = 0;
    std::vector<std::string> rows;
    std::vector<int64_t> dist;
};

// One group through group_scripts, merge_width and merge_rows, all buffers of exact size.
static Aligned align(const std::vector<std::string>& reads)
{
    const int64_t k = (int64_t)reads.size();
    std::vector<std::unique_ptr<uint8_t[]>> heap((size_t)k);
    std::vector<const uint8_t*> ptr((size_t)k, nullptr);
    std::vector<int64_t> len((size_t)k);
    for (int64_t a = 0; a < k; a++) {
        len[(size_t)a] = (int64_t)reads[(size_t)a].size();
        if (len[(size_t)a]) {
            heap[(size_t)a].reset(new uint8_t[(size_t)len[(size_t)a]]);
            for (int64_t q = 0; q < len[(size_t)a]; q++) heap[(size_t)a][(size_t)q] = (uint8_t)reads[(size_t)a][(size_t)q];
            ptr[(size_t)a] = heap[(size_t)a].get();
        }
    }
    std::vector<Script> scripts((size_t)k);
    Aligned r;
    r.centre = group_scripts(ptr.data(), len.data(), k, scripts.data());
    std::vector<RowScript> rows((size_t)k);
    for (int64_t a = 0; a < k; a++) {
        rows[(size_t)a] = RowScript{scripts[(size_t)a].at.data(), scripts[(size_t)a].cnt.data(), scripts[(size_t)a].ins.data()};
        r.dist.push_back(scripts[(size_t)a].dist);
    }
    const int64_t n = len[(size_t)r.centre];
    std::vector<int32_t> w;
    r.width = merge_width(rows.data(), k, r.centre, n, &w);
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)(k * r.width) + (k * r.width == 0 ? 1 : 0)]);
    merge_rows(rows.data(), k, r.centre, ptr[(size_t)r.centre], n, w, r.width, out.get());
    for (int64_t a = 0; a < k; a++)
        r.rows.emplace_back(reinterpret_cast<const char*>(out.get()) + a * r.width, (size_t)r.width);
    return r;
}

static std::string ungap(const std::string& s)
{
    std::string o;
    for (char c : s)
        if (c != '-') o.push_back(c);
    return o;
}

static void check_rows(const std::vector<std::string>& reads, const Aligned& r, const char* what)
{
    for (size_t a = 0; a < reads.size(); a++) {
        CHECK((int64_t)r.rows[a].size() == r.width, "%s: row %zu has %zu bytes, width %ld", what, a, r.rows[a].size(), (long)r.width);
        CHECK(ungap(r.rows[a]) == reads[a], "%s: row %zu '%s' is not read '%s'", what, a, r.rows[a].c_str(), reads[a].c_str());
    }
}

int main()
{
    // empty reads and k = 1
    Aligned r = align({""});
    CHECK(r.centre == 0 && r.width == 0 && r.rows[0].empty(), "one empty read");
    r = align({"ACGT"});
    CHECK(r.centre == 0 && r.width == 4 && r.rows[0] == "ACGT" && r.dist[0] == 0, "k = 1");
    r = align({"", ""});
    CHECK(r.centre == 0 && r.width == 0 && r.dist[1] == 0, "two empty reads");
    r = align({"", "ACGT"});
    CHECK(r.centre == 0 && r.width == 4 && r.rows[0] == "----" && r.rows[1] == "ACGT" && r.dist[1] == 4, "empty centre");
    r = align({"ACGT", ""});
    CHECK(r.centre == 0 && r.width == 4 && r.rows[0] == "ACGT" && r.rows[1] == "----" && r.dist[1] == 4, "empty read");
    r = align({"", "", "A"});
    CHECK(r.centre == 0 && r.width == 1 && r.rows[2] == "A" && r.rows[1] == "-", "two empty reads and one base");

    // the exhaustive single edits of a 10-nt parent, both orders
    const std::string parent = "ACGTTGCAAC";
    std::vector<std::string> variants;
    for (size_t p = 0; p < parent.size(); p++) {
        variants.push_back(parent.substr(0, p) + parent.substr(p + 1));
        for (char c : std::string("ACGT"))
            if (c != parent[p]) variants.push_back(parent.substr(0, p) + c + parent.substr(p + 1));
    }
    for (size_t p = 0; p <= parent.size(); p++)
        for (char c : std::string("ACGT")) variants.push_back(parent.substr(0, p) + c + parent.substr(p));
    long pairs = 0;
    for (const std::string& v : variants) {
        if (v == parent) continue;
        for (int order = 0; order < 2; order++) {
            const std::vector<std::string> reads = order ? std::vector<std::string>{v, parent} : std::vector<std::string>{parent, v};
            r = align(reads);
            check_rows(reads, r, "single edit");
            CHECK(r.centre == 0 && r.dist[0] == 0 && r.dist[1] == 1, "single edit '%s': distance %ld", v.c_str(), (long)r.dist[1]);
            const int64_t want = (int64_t)std::max(reads[0].size(), reads[1].size());
            CHECK(r.width == want, "single edit '%s': width %ld", v.c_str(), (long)r.width);
            CHECK(edit_distance(reinterpret_cast<const uint8_t*>(v.data()), (int64_t)v.size(),
                                reinterpret_cast<const uint8_t*>(parent.data()), (int64_t)parent.size()) == 1,
                  "edit_distance '%s'", v.c_str());
            pairs++;
        }
    }
    CHECK(pairs == 2 * (30 + 10 + 44), "%ld single-edit pairs", pairs);

    // ties, and two long reads
    std::vector<std::string> tie = {"GGGG", "AC", "CA", "AA", "CCA"};
    r = align(tie);
    check_rows(tie, r, "ties");
    // distance sums 16, 9, 8, 8, 9: reads 2 and 3 tie, the lower index wins
    CHECK(r.centre == 2, "ties: centre %ld", (long)r.centre);
    std::string a, b;
    uint32_t x = 12345u;
    for (int i = 0; i < 700; i++) {
        x = x * 1664525u + 1013904223u;
        a.push_back("ACGT"[x >> 30]);
    }
    b = a.substr(0, 100) + a.substr(103, 400) + "TT" + a.substr(503);
    r = align({a, b});
    check_rows({a, b}, r, "long reads");
    CHECK(r.dist[1] == 5 && r.width == 702, "long reads: distance %ld width %ld", (long)r.dist[1], (long)r.width);
    if (!fails) std::printf("star_check ok: %ld single-edit pairs\n", pairs);
    return fails ? 1 : 0;
}
