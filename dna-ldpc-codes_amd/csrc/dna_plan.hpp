// dna_plan.hpp -- the read planner: reads -> the
// kind / row_ptr / rows / row_q plan that ldpc_dna_llr consumes, i.e. the
// control flow of ex_decoder/decoder.py:103-497 that dna_llr.plan_llr mirrors
// in Python.  Header-only host C++, no HIP: the body of ldpc_dna_plan_host,
// the CPU-testable definition of the contract the kernels of
// dna_plan_kernels.hpp reproduce byte for byte, and what tests/dna_plan_san/plan_check.cpp includes.
//
// Contract.
//   reads     read i is seqs[offsets[i] .. offsets[i] + lengths[i]) with quality
//             quals[i].  With index_vals the read is its payload and
//             index_vals[i] its decoded index.  Without (raw reads) the first 16
//             bytes are the RS(8,4) index word (rs_index.hpp): reads with
//             cnumerr -1 are dropped, the payload is the bytes from 16 on
//             (dna_llr.split_reads);
//   grouping  strands[S] is strictly ascending; a read whose index is not in it
//             is dropped, the others are grouped per strand in input order (the
//             stable sort of decoder.py:116);
//   kinds     no reads 0; one read: 2 if shorter than payload_nt, else 1;
//             several reads all exactly payload_nt long: 1; otherwise ragged;
//   ragged    all pairs i < k of the strand's reads, Levenshtein distance each;
//             the candidates are the reads with a partner at distance < 15
//             (decoder.py:175), in input order; none: kind 0; otherwise the
//             candidates are one group of the centre-star aligner
//             (star_align.hpp); aligned width == payload_nt: kind 1 with the
//             aligned rows, any other width: kind 3, every row holding the last
//             byte of its aligned row ('-' for width 0) in byte 0.  align = 0
//             means "no aligner": a ragged strand with candidates is an error;
//   rows      payload_nt bytes each, prefilled with '-'; a plain kind-1 strand
//             copies each read's first payload_nt bytes; kind 2 puts the read's
//             last byte in byte 0 ('-' for an empty read; an empty read with
//             quality > 63 is an error); row_q is the row's read quality.
//             R = row_ptr[S] <= n_reads; rows from R on are not touched;
//   stats     int64[kNumStats] (may be null): see the enum below.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ragged_reads.hpp"
#include "rs_index.hpp"
#include "star_align.hpp"

namespace ldpc {
namespace plan {

constexpr int32_t kEdThreshold = 15;  // decoder.py:175 (temp < 15)
constexpr int32_t kQHigh = 63;        // decoder.py:247

enum : int {
    kStatValid = 0,       // reads valid after both filters (index decodes, index is a strand)
    kStatPairs = 1,       // Levenshtein pairs of the ragged strands
    kStatAligned = 2,     // ragged strands sent to the aligner
    kStatAlignPairs = 3,  // read-to-centre alignments (candidates - 1 per such strand)
    kStatRows = 4,        // R = row_ptr[S]
    kStatCnumerr = 5,     // [5..8]: reads with cnumerr -1, 0, 1, 2 (all 0 with index_vals)
    kNumStats = 9
};

struct Args {
    const uint8_t* seqs;
    const int64_t* offsets;
    const int32_t* lengths;
    const int32_t* quals;
    int64_t n_reads;
    const int32_t* index_vals;  // null: raw reads
    const int32_t* strands;
    int32_t n_strands;
    int32_t payload_nt;
    int32_t align;
    int32_t* kind;
    int64_t* row_ptr;
    uint8_t* rows;
    int32_t* row_q;
    int64_t* stats;
};

// The argument errors both forms report before any work; empty: none.
// *total = bytes of seqs the reads span.  plan_outputs = false: the caller
// takes no kind / row_ptr / rows / row_q (the fused call).
inline std::string check_args(const Args& a, int64_t* total, bool plan_outputs = true)
{
    *total = 0;
    if (a.n_reads < 0 || a.n_strands < 0 || a.payload_nt < 1) return "negative count or payload_nt < 1";
    if (a.n_strands > 0 && !a.strands) return "null strands";
    if (a.n_reads > 0 && (!a.offsets || !a.lengths || !a.quals)) return "null read arrays";
    if (plan_outputs && (!a.row_ptr || (a.n_strands > 0 && !a.kind) || (a.n_reads > 0 && (!a.rows || !a.row_q))))
        return "null kind, row_ptr, rows or row_q";
    for (int32_t s = 1; s < a.n_strands; s++)
        if (a.strands[s] <= a.strands[s - 1]) return "strands must be strictly ascending";
    return ragged::check(a.seqs, a.offsets, a.lengths, a.n_reads, total);
}

// What a candidate's aligned row (width bytes) leaves in its plan row dst[nt],
// prefilled with '-': the row when width == nt, for any other width its last
// byte in byte 0 (nothing for width 0).
inline void aligned_row(const uint8_t* row, int64_t width, int32_t nt, uint8_t* dst)
{
    if (width == nt) std::memcpy(dst, row, (size_t)nt);
    else if (width > 0) dst[0] = row[width - 1];
}

// Position of index value v in strands, or -1.
inline int32_t locate(const int32_t* strands, int32_t S, int32_t v)
{
    const int32_t* e = std::lower_bound(strands, strands + S, v);
    return (e != strands + S && *e == v) ? (int32_t)(e - strands) : -1;
}

// The whole planner on one thread.  Returns an empty string, or the message of
// an argument error (outputs are then unspecified).
inline std::string plan_host(const Args& a)
{
    int64_t total = 0;
    std::string err = check_args(a, &total);
    if (!err.empty()) return err;
    const int64_t n = a.n_reads;
    const int32_t S = a.n_strands, nt = a.payload_nt;
    int64_t st[kNumStats] = {0};

    // payload view of every read and its strand position
    std::vector<int64_t> poff((size_t)n);
    std::vector<int32_t> plen((size_t)n), pos((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        int32_t idx;
        poff[(size_t)i] = a.offsets[i];
        plen[(size_t)i] = a.lengths[i];
        if (a.index_vals) {
            idx = a.index_vals[i];
        } else {
            int32_t ne;
            rs::rs_read_decode(a.lengths[i] ? a.seqs + a.offsets[i] : nullptr, a.lengths[i], &idx, &ne);
            st[kStatCnumerr + 1 + ne]++;
            if (ne < 0) {
                pos[(size_t)i] = -1;
                continue;
            }
            poff[(size_t)i] += rs::kPrefixNt;
            plen[(size_t)i] -= rs::kPrefixNt;
        }
        pos[(size_t)i] = locate(a.strands, S, idx);
    }

    // segments: strand s holds ids[start[s] .. start[s + 1]), input order
    std::vector<int64_t> start((size_t)S + 1, 0);
    for (int64_t i = 0; i < n; i++)
        if (pos[(size_t)i] >= 0) start[(size_t)pos[(size_t)i] + 1]++;
    for (int32_t s = 0; s < S; s++) start[(size_t)s + 1] += start[(size_t)s];
    const int64_t n_valid = start[(size_t)S];
    std::vector<int64_t> ids((size_t)n_valid), cur(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < n; i++)
        if (pos[(size_t)i] >= 0) ids[(size_t)cur[(size_t)pos[(size_t)i]]++] = i;
    st[kStatValid] = n_valid;

    auto seq = [&](int64_t r) { return plen[(size_t)r] ? a.seqs + poff[(size_t)r] : (const uint8_t*)nullptr; };

    // classification; the candidates of ragged strands
    std::vector<int64_t> cand_ptr((size_t)S + 1, 0), cand;  // candidate read ids, strand by strand
    for (int32_t s = 0; s < S; s++) {
        const int64_t s0 = start[(size_t)s], k = start[(size_t)s + 1] - s0;
        cand_ptr[(size_t)s + 1] = (int64_t)cand.size();
        a.kind[s] = 0;
        if (k == 0) continue;
        if (k == 1) {
            a.kind[s] = plen[(size_t)ids[(size_t)s0]] < nt ? 2 : 1;
            continue;
        }
        bool all_full = true;
        for (int64_t q = 0; q < k; q++) all_full = all_full && plen[(size_t)ids[(size_t)(s0 + q)]] == nt;
        if (all_full) {
            a.kind[s] = 1;
            continue;
        }
        std::vector<uint8_t> close((size_t)k, 0);
        for (int64_t x = 0; x < k; x++)
            for (int64_t y = x + 1; y < k; y++) {
                const int64_t rx = ids[(size_t)(s0 + x)], ry = ids[(size_t)(s0 + y)];
                if (star::edit_distance(seq(rx), plen[(size_t)rx], seq(ry), plen[(size_t)ry]) < kEdThreshold)
                    close[(size_t)x] = close[(size_t)y] = 1;
            }
        st[kStatPairs] += k * (k - 1) / 2;
        for (int64_t q = 0; q < k; q++)
            if (close[(size_t)q]) cand.push_back(ids[(size_t)(s0 + q)]);
        cand_ptr[(size_t)s + 1] = (int64_t)cand.size();
        const int64_t nc = cand_ptr[(size_t)s + 1] - cand_ptr[(size_t)s];
        if (nc == 0) continue;  // kind 0
        if (!a.align) return "ragged strands need an aligner (align = 0)";
        a.kind[s] = 3;  // until the aligned width says 1
        st[kStatAligned]++;
        st[kStatAlignPairs] += nc - 1;
    }

    // row counts -> row_ptr
    a.row_ptr[0] = 0;
    for (int32_t s = 0; s < S; s++) {
        const int64_t nc = cand_ptr[(size_t)s + 1] - cand_ptr[(size_t)s];
        const int64_t rc = nc ? nc : a.kind[s] == 1 ? start[(size_t)s + 1] - start[(size_t)s] : a.kind[s] == 2 ? 1 : 0;
        a.row_ptr[s + 1] = a.row_ptr[s] + rc;
    }
    const int64_t R = a.row_ptr[S];
    st[kStatRows] = R;
    if (R > 0) std::memset(a.rows, star::kGap, (size_t)R * (size_t)nt);

    std::vector<const uint8_t*> rd;
    std::vector<int64_t> ln;
    std::vector<star::Script> scripts;
    std::vector<star::RowScript> rs_;
    std::vector<int32_t> w;
    std::vector<uint8_t> merged;
    for (int32_t s = 0; s < S; s++) {
        const int64_t r0 = a.row_ptr[s], c0 = cand_ptr[(size_t)s], nc = cand_ptr[(size_t)s + 1] - c0;
        if (nc > 0) {  // aligned strand
            rd.resize((size_t)nc);
            ln.resize((size_t)nc);
            scripts.assign((size_t)nc, star::Script());
            rs_.resize((size_t)nc);
            for (int64_t q = 0; q < nc; q++) {
                rd[(size_t)q] = seq(cand[(size_t)(c0 + q)]);
                ln[(size_t)q] = plen[(size_t)cand[(size_t)(c0 + q)]];
            }
            const int64_t c = star::group_scripts(rd.data(), ln.data(), nc, scripts.data());
            for (int64_t q = 0; q < nc; q++)
                rs_[(size_t)q] = star::RowScript{scripts[(size_t)q].at.data(), scripts[(size_t)q].cnt.data(),
                                                scripts[(size_t)q].ins.data()};
            const int64_t width = star::merge_width(rs_.data(), nc, c, ln[(size_t)c], &w);
            merged.resize((size_t)(nc * width));
            star::merge_rows(rs_.data(), nc, c, rd[(size_t)c], ln[(size_t)c], w, width, merged.data());
            a.kind[s] = width == nt ? 1 : 3;
            for (int64_t q = 0; q < nc; q++) {
                aligned_row(merged.data() + (size_t)(q * width), width, nt, a.rows + (size_t)(r0 + q) * (size_t)nt);
                a.row_q[r0 + q] = a.quals[cand[(size_t)(c0 + q)]];
            }
        } else if (a.kind[s] == 1) {
            const int64_t s0 = start[(size_t)s], k = start[(size_t)s + 1] - s0;
            for (int64_t q = 0; q < k; q++) {
                const int64_t r = ids[(size_t)(s0 + q)];
                std::memcpy(a.rows + (size_t)(r0 + q) * (size_t)nt, seq(r), (size_t)nt);  // plen >= nt here
                a.row_q[r0 + q] = a.quals[r];
            }
        } else if (a.kind[s] == 2) {
            const int64_t r = ids[(size_t)start[(size_t)s]];
            if (plen[(size_t)r] == 0 && a.quals[r] > kQHigh)
                return "empty read on strand " + std::to_string(s) + " with quality > 63 (the reference indexes its last bit)";
            if (plen[(size_t)r] > 0) a.rows[(size_t)r0 * (size_t)nt] = seq(r)[plen[(size_t)r] - 1];
            a.row_q[r0] = a.quals[r];
        }
    }
    if (a.stats) std::copy(st, st + kNumStats, a.stats);
    return std::string();
}

}  // namespace plan
}  // namespace ldpc
