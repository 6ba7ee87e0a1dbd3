// star_align.hpp -- the centre-star multiple alignment of one group of reads
// (the place MUSCLE has in the reference,
// ex_decoder/decoder.py:201-207).  Header-only, no HIP needed: the host path
// of ldpc_dna_star_align[_host] and the comparator of the kernels in dna.hip.
//
// Definition.  A group is k >= 1 reads (any bytes, any length), in candidate
// order.
//   centre   the read with the smallest sum of Levenshtein distances (unit
//            cost) to the others, ties to the lowest index;
//   pair     read r (length m) against the centre c (length n): D[i][j] is the
//            Levenshtein table of r[:i], c[:j]; the traceback starts at (m, n)
//            and at each cell takes the first move that fits:
//              0 diagonal  i, j > 0 and D[i][j] = D[i-1][j-1] + (r[i-1] != c[j-1]):
//                          r[i-1] lands on centre position j-1;
//              1 up        i > 0 and D[i][j] = D[i-1][j] + 1: r[i-1] is an
//                          insertion in slot j, the gap before centre position j
//                          (slot n follows the last position);
//              2 left      centre position j-1 gets '-' in this row.
//            The move of a cell depends on the cell's three neighbours only, so
//            it is recorded (2 bits) while the table is filled, and the table
//            itself is never kept: two rows are.
//   script   what a pair's traceback leaves: at[n] (the read's byte on each
//            centre position, '-' for none), cnt[n + 1] (insertions per slot),
//            ins (the inserted bytes, slot by slot, read order) and the
//            distance D[m][n];
//   merge    slot width w[j] = the largest cnt[j] of any row; a row is, for
//            j = 0..n, its slot-j bytes left-justified and padded with '-' to
//            w[j], then (j < n) at[j]; the centre's own row has its bytes and
//            '-' in every slot; width = n + sum w[j]; rows in candidate order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define STAR_HD __host__ __device__ __forceinline__
#else
#define STAR_HD inline
#endif

namespace ldpc {
namespace star {

constexpr uint8_t kGap = '-';
enum : uint32_t { kDiag = 0, kUp = 1, kLeft = 2 };

// Levenshtein distance of a[0..la) and b[0..lb), two rows.
inline int64_t edit_distance(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb)
{
    std::vector<int64_t> row((size_t)lb + 1);
    for (int64_t j = 0; j <= lb; j++) row[(size_t)j] = j;
    for (int64_t i = 1; i <= la; i++) {
        const uint8_t ai = a[i - 1];
        int64_t diag = row[0], left = i;
        row[0] = i;
        for (int64_t j = 1; j <= lb; j++) {
            const int64_t up = row[(size_t)j];
            int64_t v = diag + (ai != b[j - 1] ? 1 : 0);
            if (up + 1 < v) v = up + 1;
            if (left + 1 < v) v = left + 1;
            row[(size_t)j] = v;
            diag = up;
            left = v;
        }
    }
    return row[(size_t)lb];
}

// A pair's script, as flat arrays (the layout the kernels write too).
struct Script {
    std::vector<uint8_t> at;   // [n]
    std::vector<int32_t> cnt;  // [n + 1]
    std::vector<uint8_t> ins;  // [sum cnt], slot by slot
    int64_t dist = 0;
};

// The traceback over recorded moves: `move(i, j)` gives the move of cell
// (i, j), i, j >= 1.  Writes at[n], cnt[n + 1] and the inserted bytes
// end-justified into ins_buf[0..m): they occupy ins_buf[m - t .. m), t = their
// number, which is returned.  Also the traceback of k_star_align_pairs: every
// index stays within at[n], cnt[n + 1], ins_buf[m] and r[m] whatever `move`
// returns (i or j falls by one each step; an unknown move counts as left).
template <class MoveFn>
STAR_HD int64_t walk(const uint8_t* r, int64_t m, int64_t n, MoveFn move, uint8_t* at, int32_t* cnt, uint8_t* ins_buf)
{
    int64_t i = m, j = n, wp = m;
    int32_t c = 0;
    while (i > 0 || j > 0) {
        const uint32_t mv = i == 0 ? (uint32_t)kLeft : j == 0 ? (uint32_t)kUp : move(i, j);
        if (mv == kUp) {
            ins_buf[--wp] = r[i - 1];
            c++;
            i--;
        } else {
            cnt[j] = c;
            c = 0;
            at[j - 1] = mv == kDiag ? r[i - 1] : kGap;
            if (mv == kDiag) i--;
            j--;
        }
    }
    cnt[0] = c;
    return m - wp;
}

// Read r against centre c: fill the table row by row, keep every cell's move
// (2 bits, 16 per word), walk it.
inline void pair_script(const uint8_t* r, int64_t m, const uint8_t* c, int64_t n, Script* s)
{
    const size_t wpr = (size_t)(n + 15) / 16;
    std::vector<uint32_t> moves((size_t)m * wpr, 0u);
    std::vector<int64_t> row((size_t)n + 1);
    for (int64_t j = 0; j <= n; j++) row[(size_t)j] = j;
    for (int64_t i = 1; i <= m; i++) {
        const uint8_t ri = r[i - 1];
        int64_t diag = row[0], left = i;
        row[0] = i;
        uint32_t* mrow = moves.data() + (size_t)(i - 1) * wpr;
        for (int64_t j = 1; j <= n; j++) {
            const int64_t up = row[(size_t)j];
            const int64_t sub = diag + (ri != c[j - 1] ? 1 : 0);
            int64_t v = sub;
            if (up + 1 < v) v = up + 1;
            if (left + 1 < v) v = left + 1;
            const uint32_t mv = v == sub ? kDiag : v == up + 1 ? kUp : kLeft;
            mrow[(size_t)(j - 1) >> 4] |= mv << (2 * ((j - 1) & 15));
            row[(size_t)j] = v;
            diag = up;
            left = v;
        }
    }
    s->dist = row[(size_t)n];
    s->at.assign((size_t)n, kGap);
    s->cnt.assign((size_t)n + 1, 0);
    std::vector<uint8_t> buf((size_t)m);
    const uint32_t* mv = moves.data();
    const int64_t t = walk(
        r, m, n,
        [mv, wpr](int64_t i, int64_t j) {
            return (mv[(size_t)(i - 1) * wpr + ((size_t)(j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u;
        },
        s->at.data(), s->cnt.data(), buf.data());
    s->ins.assign(buf.begin() + (ptrdiff_t)(m - t), buf.end());
}

// The centre of k reads from their distance matrix d[k][k] (row-major,
// symmetric, zero diagonal): smallest row sum, ties to the lowest index.
inline int64_t choose_centre(const int64_t* d, int64_t k)
{
    int64_t best = 0, best_sum = -1;
    for (int64_t a = 0; a < k; a++) {
        int64_t s = 0;
        for (int64_t b = 0; b < k; b++) s += d[a * k + b];
        if (best_sum < 0 || s < best_sum) {
            best = a;
            best_sum = s;
        }
    }
    return best;
}

// One row's view for the merge; the centre's own row has script = nullptr.
struct RowScript {
    const uint8_t* at = nullptr;   // [n]
    const int32_t* cnt = nullptr;  // [n + 1]
    const uint8_t* ins = nullptr;  // [sum cnt]
};

// Slot widths w[n + 1] of a group and its width n + sum w.
inline int64_t merge_width(const RowScript* rows, int64_t k, int64_t centre, int64_t n, std::vector<int32_t>* w)
{
    w->assign((size_t)n + 1, 0);
    for (int64_t a = 0; a < k; a++) {
        if (a == centre) continue;
        for (int64_t j = 0; j <= n; j++)
            if (rows[a].cnt[j] > (*w)[(size_t)j]) (*w)[(size_t)j] = rows[a].cnt[j];
    }
    int64_t width = n;
    for (int64_t j = 0; j <= n; j++) width += (*w)[(size_t)j];
    return width;
}

// Write the k rows (width bytes each, candidate order) to out.
inline void merge_rows(const RowScript* rows, int64_t k, int64_t centre, const uint8_t* c, int64_t n,
                       const std::vector<int32_t>& w, int64_t width, uint8_t* out)
{
    for (int64_t a = 0; a < k; a++) {
        uint8_t* o = out + (size_t)a * (size_t)width;
        const uint8_t* ins = rows[a].ins;
        for (int64_t j = 0; j <= n; j++) {
            const int32_t have = a == centre ? 0 : rows[a].cnt[j];
            for (int32_t q = 0; q < have; q++) *o++ = *ins++;
            for (int32_t q = have; q < w[(size_t)j]; q++) *o++ = kGap;
            if (j < n) *o++ = a == centre ? c[j] : rows[a].at[j];
        }
    }
}

// One group on the host.  reads[a] / lens[a], a < k (k >= 1).  Returns the
// centre; scripts[0..k) are filled (the centre's stays empty, dist 0).
inline int64_t group_scripts(const uint8_t* const* reads, const int64_t* lens, int64_t k, Script* scripts)
{
    for (int64_t a = 0; a < k; a++) scripts[a] = Script();
    int64_t centre = 0;
    if (k > 2) {  // k = 2: equal sums, the tie goes to read 0
        std::vector<int64_t> d((size_t)(k * k), 0);
        for (int64_t a = 0; a < k; a++)
            for (int64_t b = a + 1; b < k; b++)
                d[(size_t)(a * k + b)] = d[(size_t)(b * k + a)] = edit_distance(reads[a], lens[a], reads[b], lens[b]);
        centre = choose_centre(d.data(), k);
    }
    for (int64_t a = 0; a < k; a++)
        if (a != centre) pair_script(reads[a], lens[a], reads[centre], lens[centre], &scripts[a]);
    return centre;
}

}  // namespace star
}  // namespace ldpc
