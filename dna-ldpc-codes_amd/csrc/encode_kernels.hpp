// encode_kernels.hpp -- HIP kernels of the batched systematic encoder
// (gfx950, wave64; DESIGN.md sec. 8.4, host side and definition: gf2.hpp).
//
// 64 codewords form a tile, as in the decoder: w[tile][N] u64, bit l of a
// word = that position's bit of codeword 64 * tile + l (a ballot).  GF(2)
// arithmetic is order-free, so cross-lane XOR reductions are exact.
//
//   k_enc_pack   msg [B][K] u8 -> w at the information positions (the parity
//                positions are cleared by a memset before it)
//   k_enc_rows   s[tile][j] = parity of row j of H over w     (sparse step)
//   k_enc_dense  w[tile][par_pos[i]] = XOR_j T[i][j] s[tile][j] (dense step)
//   k_unpack_hard (kernels.hpp) w -> cw [B][N] u8
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"

namespace ldpc {
namespace dev {

constexpr int ENC_PACK_COLS = 256;  // message positions per k_enc_pack block (one row of them = 256 B)
// LDS row stride of the staged message bytes in dwords: 64 + 1, so that the
// 64 lanes of a wave, each reading its own codeword's row at the same
// column, fall on 64 different banks
constexpr int ENC_PACK_STRIDE = ENC_PACK_COLS / 4 + 1;
constexpr int ENC_DENSE_ROWS = 64;  // rows of T per k_enc_dense block (16 per wave)
// k_enc_dense keeps the tile's s (M x 8 B, zero-padded to whole words of T;
// 16 KB for the DNA code) in LDS up to this budget: the 64 KiB a block gets
// without opting in to more, which still lets two blocks share a CU's 160 KiB.
// Above it the kernel reads s from global memory (L2).
constexpr size_t ENC_DENSE_LDS_BYTES = 64 * 1024;

// grid (ceil(K / 256), tiles), 256 threads.  msg holds Bc rows of K bytes;
// vec4 != 0: every row starts 4-byte aligned (msg and K are multiples of 4).
__global__ __launch_bounds__(256) void k_enc_pack(const uint8_t* __restrict__ msg, const int32_t* __restrict__ info_pos,
                                                  uint64_t* __restrict__ w, int64_t Bc, int32_t K, int32_t N, int vec4)
{
    __shared__ uint32_t stage[TILE * ENC_PACK_STRIDE];
    const int64_t t = blockIdx.y;
    const int32_t k0 = (int32_t)blockIdx.x * ENC_PACK_COLS;
    const int wv = wave_id(), lane = lane_id();
    if (vec4) {
        // one 256-B row piece per wave instruction, 16 rows per wave
        const int32_t k = k0 + 4 * lane;
        for (int rr = 0; rr < TILE / 4; rr++) {
            const int r = wv * (TILE / 4) + rr;
            const int64_t b = t * TILE + r;
            uint32_t x = 0;
            if (b < Bc && k < K) x = *reinterpret_cast<const uint32_t*>(msg + (size_t)b * (size_t)K + (size_t)k);
            stage[r * ENC_PACK_STRIDE + lane] = x;
        }
    } else {
        uint8_t* sb = reinterpret_cast<uint8_t*>(stage);
        const int32_t k = k0 + (int32_t)threadIdx.x;
        for (int r = 0; r < TILE; r++) {
            const int64_t b = t * TILE + r;
            uint8_t x = 0;
            if (b < Bc && k < K) x = msg[(size_t)b * (size_t)K + (size_t)k];
            sb[r * (ENC_PACK_STRIDE * 4) + (int)threadIdx.x] = x;
        }
    }
    __syncthreads();
    // wave wv: message positions k0 + 64 wv + i, i < 64; lane l reads its own
    // codeword's bytes, the ballot of bit 0 is the word, lane i keeps word i
    uint64_t word = 0;
#pragma unroll 4
    for (int q = 0; q < TILE / 4; q++) {
        const uint32_t x = stage[lane * ENC_PACK_STRIDE + wv * (TILE / 4) + q];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint64_t m = __ballot((x >> (8 * c)) & 1u);
            if (lane == 4 * q + c) word = m;
        }
    }
    const int32_t k = k0 + wv * TILE + lane;
    if (k < K) w[(size_t)t * (size_t)N + (size_t)info_pos[k]] = word;
}

// grid (ceil(M / 4), tiles), 256 threads: one wave per row, the lanes split
// the row's entries (any row degree), XOR across the wave.
__global__ __launch_bounds__(256) void k_enc_rows(const uint64_t* __restrict__ w, const int32_t* __restrict__ row_ptr,
                                                  const int32_t* __restrict__ col_idx, uint64_t* __restrict__ s,
                                                  int32_t M, int32_t N)
{
    const int32_t row = (int32_t)blockIdx.x * 4 + wave_id();
    if (row >= M) return;
    const int64_t t = blockIdx.y;
    const int lane = lane_id();
    const uint64_t* wt = w + (size_t)t * (size_t)N;
    const int32_t e1 = row_ptr[row + 1];
    uint64_t p = 0;
    for (int32_t e = row_ptr[row] + lane; e < e1; e += TILE) p ^= wt[col_idx[e]];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p ^= shfl_xor_u64(p, off);
    if (lane == 0) s[(size_t)t * (size_t)M + (size_t)row] = p;
}

// grid (ceil(r / 64), tiles), 256 threads, Mw * 512 B of dynamic LDS when
// IN_LDS.  One wave per row i of T: lane l takes the columns j = 64 jw + l,
// whose bit is bit l of the wave-uniform word T[i][jw] (a scalar load).
template <bool IN_LDS>
__global__ __launch_bounds__(256) void k_enc_dense(const uint64_t* __restrict__ T, const uint64_t* __restrict__ s,
                                                   const int32_t* __restrict__ par_pos, uint64_t* __restrict__ w,
                                                   int32_t r, int32_t M, int32_t Mw, int32_t N)
{
    extern __shared__ uint64_t s_tile[];
    const int64_t t = blockIdx.y;
    const int lane = lane_id();
    const uint64_t* st = s + (size_t)t * (size_t)M;
    if (IN_LDS) {
        for (int32_t j = (int32_t)threadIdx.x; j < Mw * TILE; j += 256) s_tile[j] = j < M ? st[j] : 0ull;
        __syncthreads();
    }
    const int32_t i0 = (int32_t)blockIdx.x * ENC_DENSE_ROWS;
    const int32_t i1 = i0 + ENC_DENSE_ROWS < r ? i0 + ENC_DENSE_ROWS : r;
    for (int32_t i = i0 + wave_id(); i < i1; i += 4) {
        const uint64_t* Ti = T + (size_t)i * (size_t)Mw;
        uint64_t acc = 0;
        for (int32_t jw = 0; jw < Mw; jw++) {
            const uint64_t tw = Ti[jw];
            const int32_t j = jw * TILE + lane;
            uint64_t sv;
            if (IN_LDS) sv = s_tile[j];
            else sv = j < M ? st[j] : 0ull;
            if ((tw >> lane) & 1ull) acc ^= sv;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc ^= shfl_xor_u64(acc, off);
        if (lane == 0) w[(size_t)t * (size_t)N + (size_t)par_pos[i]] = acc;
    }
}

}  // namespace dev
}  // namespace ldpc
