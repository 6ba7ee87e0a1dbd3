// star_align.hpp -- the centre-star multiple alignment of one group of reads
// (the place MUSCLE has in the reference,
// ex_decoder/decoder.py:201-207).  Header-only, no HIP needed: the host path
// of ldpc_dna_star_align[_host], the comparator of the kernels in dna.hip, and
// (at the end) the device path's planning: which groups the kernel takes,
// their pairs packed into blocks and passes, the check of a returned script.
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

// --- the device path's planning (ldpc_dna_star_align, dna.hip): which groups
// k_star_align_pairs takes and how their (read, centre) pairs are laid out in
// blocks of lanes and passes over the workspace.  Plain arrays in and out.

constexpr int32_t kDevMaxLen = 800;  // the DP row and the centre of 64 lanes in LDS

// Workspace words of one lane-interleaved block: rows x words per row x 64 lanes.
inline int64_t block_words(int64_t m, int64_t wpr) { return m * wpr * 64; }
// Words of one table row against a centre of n bytes: 2 bits per cell.
inline int64_t words_per_row(int64_t n) { return (n + 15) / 16; }

// A group the device can take: two reads or more, none longer than kDevMaxLen.
inline bool device_eligible(const int32_t* len, int64_t k)
{
    bool ok = k >= 2;
    for (int64_t q = 0; q < k && ok; q++) ok = len[q] <= kDevMaxLen;
    return ok;
}

// The budget rule: a group with a pair whose own block (64 lanes x m rows x
// ceil(n / 16) words) is beyond the budget goes to the host.
inline bool within_budget(const int32_t* len, int64_t k, int64_t centre, int64_t budget_words)
{
    const int64_t wpr = words_per_row(len[centre]);
    for (int64_t q = 0; q < k; q++)
        if (q != centre && block_words(len[q], wpr) > budget_words) return false;
    return true;
}

// Pair p is read pr[p] against centre pc[p] (sequence numbers); its script goes
// to at_off[p] (n bytes; cnt at at_off[p] + p) and ins_off[p] (m bytes).  Block b
// is pairs blk_first[b] .. blk_first[b + 1], blk_wpr[b] words per table row,
// blk_words[b] workspace words.
struct PairBlocks {
    std::vector<int32_t> pr, pc, blk_wpr;
    std::vector<int64_t> at_off, ins_off, blk_first, blk_words;
    int64_t at_total = 0, ins_total = 0;
    int64_t n_host = 0;  // groups of two reads or more left to the host
    int32_t max_n = 0;   // longest centre
};

// The pairs of the groups with on_dev[g] set, group by group in read order, cut
// into blocks of at most 64 pairs whose max(m) * max(ceil(n / 16)) * 64 words
// fit the budget.  centre[g] is the centre's index inside group g.
inline PairBlocks pack_pairs(const int32_t* lengths, const int64_t* group_ptr, int64_t n_groups, const int64_t* centre,
                             const uint8_t* on_dev, int64_t budget_words)
{
    PairBlocks pb;
    int64_t cnt = 0, bm = 0, bw = 0;
    auto close_block = [&] {
        pb.blk_words.push_back(block_words(bm, bw));
        pb.blk_wpr.push_back((int32_t)bw);
        cnt = bm = bw = 0;
    };
    for (int64_t g = 0; g < n_groups; g++) {
        const int64_t g0 = group_ptr[g], k = group_ptr[g + 1] - g0;
        if (!on_dev[g]) {
            if (k >= 2) pb.n_host++;
            continue;
        }
        const int64_t c = g0 + centre[g], n = lengths[c], wpr = words_per_row(n);
        if ((int32_t)n > pb.max_n) pb.max_n = (int32_t)n;
        for (int64_t q = g0; q < g0 + k; q++) {
            if (q == c) continue;
            const int64_t m = lengths[q], nm = m > bm ? m : bm, nw = wpr > bw ? wpr : bw;
            if (cnt == 64 || (cnt > 0 && block_words(nm, nw) > budget_words)) close_block();
            if (cnt == 0) pb.blk_first.push_back((int64_t)pb.pr.size());
            cnt++;
            if (m > bm) bm = m;
            if (wpr > bw) bw = wpr;
            pb.pr.push_back((int32_t)q);
            pb.pc.push_back((int32_t)c);
            pb.at_off.push_back(pb.at_total);
            pb.ins_off.push_back(pb.ins_total);
            pb.at_total += n;
            pb.ins_total += m;
        }
    }
    if (cnt > 0) close_block();
    pb.blk_first.push_back((int64_t)pb.pr.size());
    return pb;
}

// The passes: runs of blocks whose pieces of the workspace fit the budget
// together.  Block b's piece starts at word blk_ws[b]; pass q is blocks
// pass_first[q] .. pass_first[q + 1]; the workspace needs ws_words words.
struct Passes {
    std::vector<int64_t> blk_ws, pass_first;
    int64_t ws_words = 0;
};

inline Passes cut_passes(const std::vector<int64_t>& blk_words, int64_t budget_words)
{
    Passes ps;
    const size_t nb = blk_words.size();
    ps.blk_ws.resize(nb);
    int64_t acc = 0;
    for (size_t b = 0; b < nb; b++) {
        if (b == 0 || acc + blk_words[b] > budget_words) {
            ps.pass_first.push_back((int64_t)b);
            acc = 0;
        }
        ps.blk_ws[b] = acc;
        acc += blk_words[b];
        if (acc > ps.ws_words) ps.ws_words = acc;
    }
    ps.pass_first.push_back((int64_t)nb);
    return ps;
}

// A script's cnt[n + 1] as the device returned it, for a read of m bytes: every
// entry in 0..m and their sum *t <= m (then ins holds its m - *t .. m).
inline bool script_consistent(const int32_t* cnt, int64_t m, int64_t n, int64_t* t)
{
    bool ok = true;
    *t = 0;
    for (int64_t j = 0; j <= n; j++) {
        ok = ok && cnt[j] >= 0 && cnt[j] <= m;
        *t += cnt[j];
    }
    return ok && *t <= m;
}

}  // namespace star
}  // namespace ldpc
