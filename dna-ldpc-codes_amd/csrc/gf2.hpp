// gf2.hpp -- systematic LDPC encoding on the host: GF(2) construction of the
// encoder of a parity-check graph and the host encoder.
// Host-only, header-only, no HIP; bit vectors are packed in 64-bit words.
//
// Definition (include/ldpc_amd.h, ldpc_encoder_create).  For H (M x N):
//   parity positions: scanning columns j = N-1 .. 0, column j is one iff it is
//     linearly independent of the parity columns chosen so far (the greedy
//     basis in that order: r = rank(H) positions);
//   information positions: the other K = N - r columns;
//   encode(m) = the unique c with c[info_pos[k]] = m[k] and H c = 0.
//
// Mixed form: s = H_info m (sparse: the row parities of H over the
// information positions, CSR arrays), then c[par_pos[i]] = XOR_j T[i][j] s[j]
// with T an r x M bit matrix.  T is a left inverse of H_par on its column
// space: the elimination keeps the chosen columns as a fully reduced basis
// b_k (one pivot row p_k each, zero in every other pivot row) together with
// the combination C_k of chosen columns that b_k is.  Any s in the column
// space is XOR_k s[p_k] b_k, so the coefficient of chosen column i is
// XOR_k C_k[i] s[p_k]: T[i][p_k] = C_k[i], every other column of T is zero
// (a redundant row of H carries nothing the pivot rows do not).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ldpc_amd.h"
#include "graph.hpp"

namespace ldpc {

struct HostEncoder {
    int32_t M = 0, N = 0, K = 0, rank = 0;
    int32_t Mw = 0;                            // 64-bit words per row of T: ceil(M / 64)
    std::vector<int32_t> info_pos, par_pos;    // ascending
    std::vector<int32_t> row_ptr, col_idx;     // CSR of H (the graph may be freed)
    std::vector<uint64_t> T;                   // [rank][Mw], bit j of row i at word j / 64, bit j % 64
};

constexpr int64_t kEncoderMaxTBits = (int64_t)1 << 31;  // T above this: LDPC_ERR_UNSUPPORTED

inline int build_encoder(const HostGraph& g, HostEncoder& e, std::string* msg)
{
    const int32_t M = g.M, N = g.N;
    const size_t Mw = ((size_t)M + 63) / 64;
    const size_t Cw = ((size_t)(M < N ? M : N) + 63) / 64;  // rank <= min(M, N): words of a combination
    e.M = M;
    e.N = N;
    e.Mw = (int32_t)Mw;
    e.row_ptr = g.row_ptr;
    e.col_idx = g.col_idx;
    // (the rows of column j: edge_row of its CSC entries' CSR edge ids)
    std::vector<uint64_t> basis, comb;     // [rank][Mw], [rank][Cw]
    std::vector<int32_t> pivot_of_row((size_t)M, -1), pivot_row, chosen;
    std::vector<uint64_t> v(Mw), cv(Cw);
    for (int32_t j = N - 1; j >= 0; j--) {
        std::fill(v.begin(), v.end(), 0ull);
        std::fill(cv.begin(), cv.end(), 0ull);
        const int32_t q0 = g.col_ptr[j], q1 = g.col_ptr[j + 1];
        for (int32_t q = q0; q < q1; q++) {
            const int32_t i = g.edge_row[g.col_edge[q]];
            v[(size_t)i >> 6] ^= 1ull << (i & 63);
        }
        // reduce: a pivot row's bit is changed by its own basis vector only
        // (the basis is fully reduced), so the column's own entries decide
        for (int32_t q = q0; q < q1; q++) {
            const int32_t k = pivot_of_row[g.edge_row[g.col_edge[q]]];
            if (k < 0) continue;
            const uint64_t* b = &basis[(size_t)k * Mw];
            for (size_t w = 0; w < Mw; w++) v[w] ^= b[w];
            const uint64_t* c = &comb[(size_t)k * Cw];
            for (size_t w = 0; w < Cw; w++) cv[w] ^= c[w];
        }
        int32_t p = -1;
        for (size_t w = 0; w < Mw && p < 0; w++)
            if (v[w]) p = (int32_t)(w * 64 + (size_t)__builtin_ctzll(v[w]));
        if (p < 0) continue;  // dependent on the chosen columns: an information position
        const int32_t k = (int32_t)chosen.size();
        if ((int64_t)(k + 1) * (int64_t)(Mw * 64) > kEncoderMaxTBits) {
            if (msg) *msg = "encoder: the dense matrix T (rank x M bits) would exceed 2^31 bits";
            return LDPC_ERR_UNSUPPORTED;
        }
        cv[(size_t)k >> 6] ^= 1ull << (k & 63);
        for (int32_t l = 0; l < k; l++) {  // keep the basis fully reduced: clear row p everywhere else
            uint64_t* b = &basis[(size_t)l * Mw];
            if (!((b[(size_t)p >> 6] >> (p & 63)) & 1ull)) continue;
            for (size_t w = 0; w < Mw; w++) b[w] ^= v[w];
            uint64_t* c = &comb[(size_t)l * Cw];
            for (size_t w = 0; w < Cw; w++) c[w] ^= cv[w];
        }
        basis.insert(basis.end(), v.begin(), v.end());
        comb.insert(comb.end(), cv.begin(), cv.end());
        pivot_of_row[p] = k;
        pivot_row.push_back(p);
        chosen.push_back(j);
    }
    const int32_t r = (int32_t)chosen.size();
    e.rank = r;
    e.K = N - r;
    if (e.K == 0) {
        if (msg) *msg = "encoder: H has full column rank (K = N - rank = 0), there is nothing to encode";
        return LDPC_ERR_UNSUPPORTED;
    }
    // chosen[] descends; ascending parity index of chosen column i is r - 1 - i
    e.par_pos.assign(chosen.rbegin(), chosen.rend());
    e.info_pos.clear();
    e.info_pos.reserve((size_t)e.K);
    {
        size_t q = 0;
        for (int32_t j = 0; j < N; j++) {
            if (q < e.par_pos.size() && e.par_pos[q] == j) q++;
            else e.info_pos.push_back(j);
        }
    }
    e.T.assign((size_t)r * Mw, 0ull);
    for (int32_t k = 0; k < r; k++) {
        const int32_t p = pivot_row[k];
        const uint64_t* c = &comb[(size_t)k * Cw];
        for (int32_t i = 0; i < r; i++)
            if ((c[(size_t)i >> 6] >> (i & 63)) & 1ull) e.T[(size_t)(r - 1 - i) * Mw + ((size_t)p >> 6)] |= 1ull << (p & 63);
    }
    return LDPC_OK;
}

// msg [B][K] u8 (0 / 1) -> cw [B][N] u8.  LDPC_ERR_ARG (and *bad = the index
// of the first offending byte) when a message byte is neither 0 nor 1.
inline bool message_bytes_ok(const uint8_t* msg, size_t n, size_t* bad)
{
    for (size_t i = 0; i < n; i++)
        if (msg[i] > 1) {
            if (bad) *bad = i;
            return false;
        }
    return true;
}

// one codeword; s: Mw words of scratch
inline void encode_one(const HostEncoder& e, const uint8_t* m, uint8_t* c, uint64_t* s)
{
    std::memset(c, 0, (size_t)e.N);
    for (int32_t k = 0; k < e.K; k++) c[e.info_pos[k]] = m[k];
    std::memset(s, 0, (size_t)e.Mw * 8);
    for (int32_t i = 0; i < e.M; i++) {  // sparse step: s = H_info m
        unsigned p = 0;
        for (int32_t q = e.row_ptr[i]; q < e.row_ptr[i + 1]; q++) p ^= c[e.col_idx[q]];
        s[(size_t)i >> 6] |= (uint64_t)(p & 1u) << (i & 63);
    }
    for (int32_t i = 0; i < e.rank; i++) {  // dense step: parity of T[i] & s
        const uint64_t* t = &e.T[(size_t)i * (size_t)e.Mw];
        uint64_t a = 0;
        for (int32_t w = 0; w < e.Mw; w++) a ^= t[w] & s[w];
        c[e.par_pos[i]] = (uint8_t)(__builtin_popcountll(a) & 1);
    }
}

inline int encode_host(const HostEncoder& e, const uint8_t* msg, int64_t B, uint8_t* cw, std::string* err)
{
    size_t bad = 0;
    if (!message_bytes_ok(msg, (size_t)B * (size_t)e.K, &bad)) {
        if (err)
            *err = "message byte " + std::to_string(bad % (size_t)e.K) + " of message " + std::to_string(bad / (size_t)e.K) +
                   " is neither 0 nor 1";
        return LDPC_ERR_ARG;
    }
    std::vector<uint64_t> s((size_t)e.Mw);
    for (int64_t b = 0; b < B; b++) encode_one(e, msg + (size_t)b * (size_t)e.K, cw + (size_t)b * (size_t)e.N, s.data());
    return LDPC_OK;
}

}  // namespace ldpc
