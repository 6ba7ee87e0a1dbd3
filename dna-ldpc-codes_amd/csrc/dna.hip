// dna.hip -- the step before the decoder: per-strand
// read candidates -> the 272 x 18432 LLR matrix the first decode consumes,
// plus the pairwise edit distances that pick which ragged candidates go to
// the aligner, and the aligner itself (the centre-star alignment of
// star_align.hpp, DESIGN.md sec. 8.6: k_star_align_pairs; star_align_device
// keeps the uploads, the centre search, the pass loop and the downloads, the
// layout of the pairs is star_align.hpp's host code).
//
// Reference: ex_decoder/decoder.py:142-519 (the strand loop; count rule
// :266-320 and :442-497), def_func.py:10-26 (edit_dist), :97-117
// (DNA2binary).  The planner (dna_llr.plan_llr in Python; in the library
// dna_plan.hpp on the host and dna_plan_kernels.hpp on the GPU, included at
// the end of this file) classifies every strand into a
// `kind` and lays the candidates out as fixed-width rows; these kernels do
// the arithmetic:
//
//   kind 0  no LLRs              -> every bit int 0 (decoder.py:507-510 fill)
//   kind 1  count                -> bit b: (count0 - count1) * L over the rows,
//                                   bit 2*nt-1 skips rows with q < 53 and has
//                                   the one-vs-one tie rule (:290-299)
//   kind 2  one short candidate  -> only the last bit: +-L from the low bit of
//                                   the candidate's last base if q > 63 (:247-251)
//   kind 3  alignment failed     -> only the last bit: (count0 - count1) * L
//                                   over the failed rows' last bases with
//                                   q > 63 (:266-282)
//
// Bit values follow DNA2binary: A=00 C=01 G=10 T=11, any other character
// gives '2', which the count loop treats as a one (it tests == '0').
// Arithmetic is the reference's: (double)(c0 - c1) * L, +-2 * L, +-L.
//
// The two ends of the strand format (code: rs_index.hpp):
// k_rs_index_decode turns the 16-nt prefix of every raw read into its strand
// index (the reference's rs_dec.exe, decoder.py:59-92), k_strands_write lays
// codewords out as the strands that get synthesised (index prefix + payload,
// the format of original files/final_DNA.txt).
//
// The step after it, the trial loop of decoder.py:541-664 with the decoder
// input kept on the device (dna_trial.hpp): the kernels,
// the handle and the ldpc_trial_* entry points are dna_trial_kernels.hpp,
// included last.  The step before all of it, strands -> raw reads through a
// counter-hashed substitution / insertion / deletion channel (dna_sim.hpp,
// DESIGN.md sec. 8.9): dna_sim_kernels.hpp.
//
// Host code of this file and its three fragments: every kernel goes through
// launch() and every blocking copy down through download() (hip_own.hpp), the
// extent check of ragged reads is ragged_reads.hpp's, and dna_guard is the one
// bad_alloc guard of the entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/ldpc_amd.h"
#include "engine.hpp"
#include "dna_plan.hpp"
#include "dna_sim.hpp"
#include "dna_trial.hpp"
#include "host_decode.hpp"  // ldpc_graph
#include "ragged_reads.hpp"
#include "rs_index.hpp"
#include "star_align.hpp"

namespace ldpc {
namespace {

constexpr int kQSkip = 53;  // decoder.py:285 (i==271 and q < 53: skip)
constexpr int kQHigh = 63;  // decoder.py:247, :270, :292-295

// DNA2binary bit of character c: hi = first bit, else second bit.
// Returns true when the bit is '0'.
__device__ __forceinline__ bool bit_is_zero(uint8_t c, bool hi)
{
    if (hi) return c == 'A' || c == 'C';
    return c == 'A' || c == 'G';
}

// The count rule of one bit b = 2 * k + h of a strand of kind kd whose rows are
// r0 .. r1 - 1 (decoder.py:266-320, :442-497): *n = the count difference, the
// entry is *n * L; *is_int: the reference leaves an int 0.  Shared by
// k_dna_llr and k_dna_codes (dna_trial_kernels.hpp).
__device__ __forceinline__ void dna_bit_rule(int kd, int64_t r0, int64_t r1, const uint8_t* __restrict__ rows,
                                             const int32_t* __restrict__ row_q, int32_t nt, int32_t k, int h, int* n,
                                             bool* is_int)
{
    const int b = 2 * k + h, last_bit = 2 * nt - 1;
    *n = 0;
    *is_int = true;
    if (kd == 1) {
        int c0 = 0, c1 = 0, q0 = 0, q1 = 0;
        for (int64_t r = r0; r < r1; r++) {
            const int q = row_q[r];
            if (b == last_bit && q < kQSkip) continue;
            if (bit_is_zero(rows[r * nt + k], h == 0)) { c0++; q0 += q; }
            else { c1++; q1 += q; }
        }
        if (b == last_bit && c0 == 1 && c1 == 1) {
            if (q0 < kQSkip && q1 >= kQHigh) { *n = -2; *is_int = false; }
            else if (q0 >= kQHigh && q1 < kQSkip) { *n = 2; *is_int = false; }
        } else {
            *n = c0 - c1;
            *is_int = false;
        }
    } else if (kd == 2 && b == last_bit && r1 > r0) {
        if (row_q[r0] > kQHigh) {
            *n = bit_is_zero(rows[r0 * nt], false) ? 1 : -1;
            *is_int = false;
        }
    } else if (kd == 3 && b == last_bit) {
        int c0 = 0, c1 = 0;
        for (int64_t r = r0; r < r1; r++) {
            if (row_q[r] <= kQHigh) continue;
            if (bit_is_zero(rows[r * nt], false)) c0++;
            else c1++;
        }
        *n = c0 - c1;
        *is_int = false;
    }
}

// Every entry is k * L for an integer count difference k (decoder.py:297-314;
// the +-2L / +-L special cases included), so the kernel can hand the decoder
// its int8 codes directly (codes != nullptr): k saturated to [-127, 127], and
// *overflow set (a plain store of 1) when some |k| > 127.
__global__ void __launch_bounds__(256) k_dna_llr(const int32_t* __restrict__ kind, const int64_t* __restrict__ row_ptr,
                                                 const uint8_t* __restrict__ rows, const int32_t* __restrict__ row_q,
                                                 int32_t S, int32_t nt, double L, double* __restrict__ llr,
                                                 uint8_t* __restrict__ int_mask, int8_t* __restrict__ codes,
                                                 int32_t* __restrict__ overflow)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t k = blockIdx.y;  // nucleotide -> bits 2k, 2k+1
    if (s >= S) return;
    const int kd = kind[s];
    const int64_t r0 = row_ptr[s], r1 = row_ptr[s + 1];
    for (int h = 0; h < 2; h++) {
        const int b = 2 * k + h;
        int n;  // the count difference: the entry is n * L (0 for an int-0 entry)
        bool is_int;
        dna_bit_rule(kd, r0, r1, rows, row_q, nt, k, h, &n, &is_int);
        // (double)n * L: the reference's (count_0 - count_1) * math.log(...),
        // and 2.0 * L, L, -L for the special cases -- the same doubles
        llr[(size_t)b * S + s] = is_int ? 0.0 : (double)n * L;
        if (int_mask) int_mask[(size_t)b * S + s] = is_int;
        if (codes) {
            codes[(size_t)b * S + s] = (int8_t)max(-127, min(127, n));
            if (n > 127 || n < -127) *overflow = 1;
        }
    }
}

// Levenshtein distance, one pair per lane, the DP row and string b staged
// in LDS lane-interleaved (element j of lane l at j*64 + l).  Same
// recurrence as def_func.edit_dist: equal characters take the diagonal,
// otherwise 1 + min(diagonal, up, left).
__global__ void __launch_bounds__(64) k_edit_distance(const uint8_t* __restrict__ seqs,
                                                      const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ len,
                                                      const int32_t* __restrict__ pa, const int32_t* __restrict__ pb,
                                                      int64_t n_pairs, int32_t max_len, int32_t* __restrict__ dist)
{
    extern __shared__ uint8_t smem[];
    const int lane = threadIdx.x;
    uint16_t* row = reinterpret_cast<uint16_t*>(smem);
    uint8_t* bs = smem + sizeof(uint16_t) * 64 * (size_t)(max_len + 1);
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;
    if (p >= n_pairs) return;
    const uint8_t* a = seqs + off[pa[p]];
    const uint8_t* bg = seqs + off[pb[p]];
    const int la = len[pa[p]], lb = len[pb[p]];
    for (int j = 0; j < lb; j++) bs[j * 64 + lane] = bg[j];
    for (int j = 0; j <= lb; j++) row[j * 64 + lane] = (uint16_t)j;
    for (int i = 1; i <= la; i++) {
        const uint8_t ai = a[i - 1];
        uint16_t diag = row[lane];
        row[lane] = (uint16_t)i;
        uint16_t left = (uint16_t)i;
        for (int j = 1; j <= lb; j++) {
            const uint16_t up = row[j * 64 + lane];
            uint16_t v;
            if (ai == bs[(j - 1) * 64 + lane]) v = diag;
            else v = (uint16_t)(min(min(diag, up), left) + 1);
            row[j * 64 + lane] = v;
            diag = up;
            left = v;
        }
    }
    dist[p] = row[lb * 64 + lane];
}

// The pairwise step of the centre-star alignment (star_align.hpp, DESIGN.md
// sec. 8.6): one (read, centre) pair per lane, blocks of up to 64 pairs laid
// out by the host (pairs blk_first[b] .. blk_first[b + 1] belong to block b).
// The lane fills its Levenshtein table row by row as k_edit_distance does (DP
// row and centre lane-interleaved in LDS) and records every cell's traceback
// move, 2 bits, 16 cells per word: word q of table row i of lane l is
// ws[blk_ws[b] + ((i - 1) * blk_wpr[b] + q) * 64 + l], so the 64 lanes' stores
// of one word are one contiguous 256-byte piece.  The host sizes the block's
// piece of ws from the lengths it checked: rows <= the block's longest read,
// blk_wpr[b] >= ceil(n / 16) for every pair of the block.  The same lane then
// walks its moves back from (m, n) (star::walk: at most m + n steps, every
// index bounded by m and n whatever ws holds) and writes the pair's script:
// at[n] at at_off[p], cnt[n + 1] at at_off[p] + p, the inserted bytes
// end-justified in ins[ins_off[p] .. ins_off[p] + m), and the distance.
__global__ void __launch_bounds__(64) k_star_align_pairs(
    const uint8_t* __restrict__ seqs, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
    const int32_t* __restrict__ pr, const int32_t* __restrict__ pc, const int64_t* __restrict__ blk_first,
    const int64_t* __restrict__ blk_ws, const int32_t* __restrict__ blk_wpr, const int64_t* __restrict__ at_off,
    const int64_t* __restrict__ ins_off, int64_t blk0, int32_t max_n, uint32_t* ws, uint8_t* __restrict__ at,
    int32_t* __restrict__ cnt, uint8_t* __restrict__ ins, int32_t* __restrict__ dist)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t star_smem[];
    const int lane = threadIdx.x;
    uint16_t* row = reinterpret_cast<uint16_t*>(star_smem);
    uint8_t* cs = star_smem + sizeof(uint16_t) * 64 * (size_t)(max_n + 1);
    const int64_t b = blk0 + blockIdx.x;
    const int64_t p = blk_first[b] + lane;
    if (p >= blk_first[b + 1]) return;
    const uint8_t* r = seqs + off[pr[p]];
    const uint8_t* c = seqs + off[pc[p]];
    const int m = len[pr[p]], n = len[pc[p]];
    const int64_t wpr = blk_wpr[b];
    uint32_t* w = ws + blk_ws[b] + lane;
    for (int j = 0; j < n; j++) cs[j * 64 + lane] = c[j];
    for (int j = 0; j <= n; j++) row[j * 64 + lane] = (uint16_t)j;
    for (int i = 1; i <= m; i++) {
        const uint8_t ri = r[i - 1];
        uint32_t diag = row[lane];
        row[lane] = (uint16_t)i;
        uint32_t left = (uint32_t)i, word = 0;
        uint32_t* wrow = w + (int64_t)(i - 1) * wpr * 64;
        for (int j = 1; j <= n; j++) {
            const uint32_t up = row[j * 64 + lane];
            const uint32_t sub = diag + (ri != cs[(j - 1) * 64 + lane] ? 1u : 0u);
            const uint32_t v = min(sub, min(up, left) + 1u);
            const uint32_t mv = v == sub ? (uint32_t)star::kDiag : v == up + 1u ? (uint32_t)star::kUp
                                                                                : (uint32_t)star::kLeft;
            word |= mv << (2 * ((j - 1) & 15));
            if ((j & 15) == 0 || j == n) {
                wrow[(int64_t)((j - 1) >> 4) * 64] = word;
                word = 0;
            }
            row[j * 64 + lane] = (uint16_t)v;
            diag = up;
            left = v;
        }
    }
    dist[p] = row[n * 64 + lane];
    star::walk(
        r, (int64_t)m, (int64_t)n,
        [w, wpr](int64_t i, int64_t j) {
            return (w[((i - 1) * wpr + ((j - 1) >> 4)) * 64] >> (2 * ((j - 1) & 15))) & 3u;
        },
        at + at_off[p], cnt + at_off[p] + p, ins + ins_off[p]);
}

// One read per thread: the 16-nt prefix -> (index, cnumerr), rs_index.hpp.
// A read shorter than 16 is not touched.  No loop depends on the data; the
// field tables are two 64-bit constants, so nothing lives in scratch.
__global__ void __launch_bounds__(256) k_rs_index_decode(const uint8_t* __restrict__ seqs,
                                                         const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ len, int64_t n,
                                                         int32_t* __restrict__ index, int32_t* __restrict__ cnumerr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t idx, ne;
    rs::rs_read_decode(seqs + off[i], len[i], &idx, &ne);
    index[i] = idx;
    cnumerr[i] = ne;
}

constexpr int kStrTile = 64;     // strands per k_strands_write block (one per lane)
constexpr int kStrChunk = 256;   // bytes of every strand per block (blockIdx.y chunks a longer strand)
// LDS row stride of a staged strand in bytes: 64 + 1 dwords, so the 64 lanes
// of a wave, each writing its own strand's row at the same position, fall on
// 64 different banks
constexpr int kStrStride = kStrChunk + 4;
constexpr int64_t kStrMaxChunks = 65535;  // grid.y

__device__ __forceinline__ uint8_t base_of_bits(uint8_t hi, uint8_t lo)
{
    return (uint8_t)(0x54474341u >> (8 * (2 * (hi & 1) + (lo & 1))));  // "ACGT"
}

// The transpose codewords [n_cw][N] -> strands [N][16 + n_cw / 2], grid
// (ceil(N / 64), ceil(L / 256)), 256 threads.  Lane l owns strand j0 + l:
// every load is one 64-byte piece of a codeword row per wave (coalesced along
// N), wave 0 also encodes the index prefixes.  The block's tile is staged in
// LDS and written out along the strands: when the whole strand fits a chunk
// (the DNA code: 152 bytes) the block's 64 strands are one contiguous range
// that starts 4-byte aligned, written as dwords.  Lanes past N load nothing
// and their rows are never written.
__global__ void __launch_bounds__(256) k_strands_write(const uint8_t* __restrict__ cw,
                                                       const int32_t* __restrict__ index, int32_t n_cw, int64_t N,
                                                       uint8_t* __restrict__ out)
{
    __shared__ uint32_t tile32[kStrTile * kStrStride / 4];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tile32);
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const int64_t j0 = (int64_t)blockIdx.x * kStrTile;
    const int64_t j = j0 + lane;
    const int32_t L = rs::kPrefixNt + n_cw / 2;
    const int32_t c0 = (int32_t)blockIdx.y * kStrChunk;  // first strand byte of this chunk
    const int32_t W = L - c0 < kStrChunk ? L - c0 : kStrChunk;
    const int nvalid = N - j0 < kStrTile ? (int)(N - j0) : kStrTile;
    if (c0 == 0 && wv == 0 && j < N) {
        const uint32_t word = rs::rs_index_codeword((uint32_t)index[j]);
#pragma unroll
        for (int q = 0; q < rs::kPrefixNt / 4; q++) {
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) v |= (uint32_t)rs::rs_prefix_base(word, 4 * q + c) << (8 * c);
            tile32[lane * (kStrStride / 4) + q] = v;
        }
    }
    for (int32_t p = (c0 == 0 ? rs::kPrefixNt : 0) + wv; p < W; p += 4) {
        if (j < N) {
            const size_t k = (size_t)(c0 + p - rs::kPrefixNt);  // payload base: codeword rows 2k, 2k + 1
            const uint8_t hi = cw[(2 * k) * (size_t)N + (size_t)j];
            const uint8_t lo = cw[(2 * k + 1) * (size_t)N + (size_t)j];
            tile[lane * kStrStride + p] = base_of_bits(hi, lo);
        }
    }
    __syncthreads();
    const int32_t total = nvalid * W;
    if (W == L) {
        uint8_t* dst = out + (size_t)j0 * (size_t)L;
        const int32_t nwords = total / 4;
        for (int32_t f = (int32_t)threadIdx.x; f < nwords; f += 256) {
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int32_t b = 4 * f + c, l = b / L;
                v |= (uint32_t)tile[l * kStrStride + (b - l * L)] << (8 * c);
            }
            reinterpret_cast<uint32_t*>(dst)[f] = v;
        }
        for (int32_t b = 4 * nwords + (int32_t)threadIdx.x; b < total; b += 256) {
            const int32_t l = b / L;
            dst[b] = tile[l * kStrStride + (b - l * L)];
        }
    } else {
        for (int32_t f = (int32_t)threadIdx.x; f < total; f += 256) {
            const int32_t l = f / W, p = f - l * W;
            out[(size_t)(j0 + l) * (size_t)L + (size_t)(c0 + p)] = tile[l * kStrStride + p];
        }
    }
}

// k_edit_distance on device-resident buffers (the host-buffer entry point, the
// aligner's centres and the read planner): d_dist[p] for pairs whose indices
// the caller has checked, lengths <= max_len <= 800.
int launch_edit_distance(const uint8_t* d_seqs, const int64_t* d_off, const int32_t* d_len, const int32_t* d_pa,
                         const int32_t* d_pb, int64_t n_pairs, int32_t max_len, int32_t* d_dist)
{
    const size_t lds = (sizeof(uint16_t) * (size_t)(max_len + 1) + (size_t)max_len) * 64;
    return launch(k_edit_distance, dim3((unsigned)((n_pairs + 63) / 64)), dim3(64), lds, nullptr, d_seqs, d_off, d_len,
                  d_pa, d_pb, n_pairs, max_len, d_dist);
}

// k_dna_llr on a device-resident plan; d_mask, d_codes / d_overflow may be null.
int launch_dna_llr(const int32_t* d_kind, const int64_t* d_row_ptr, const uint8_t* d_rows, const int32_t* d_row_q,
                   int32_t n_strands, int32_t payload_nt, double llr_unit, double* d_llr, uint8_t* d_mask,
                   int8_t* d_codes, int32_t* d_overflow)
{
    dim3 grid((unsigned)((n_strands + 255) / 256), (unsigned)payload_nt);
    return launch(k_dna_llr, grid, dim3(256), 0, nullptr, d_kind, d_row_ptr, d_rows, d_row_q, n_strands, payload_nt,
                  llr_unit, d_llr, d_mask, d_codes, d_overflow);
}

// The one guard of the entry points that allocate host memory.
template <class F>
int dna_guard(const char* who, F&& f)
{
    try {
        return f();
    } catch (const std::bad_alloc&) {
        set_error(std::string(who) + ": out of host memory");
        return LDPC_ERR_DEVICE;
    }
}

}  // namespace
}  // namespace ldpc

using ldpc::set_error;

extern "C" {

int ldpc_dna_edit_distance(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, int64_t n_seqs,
                           const int32_t* pair_a, const int32_t* pair_b, int64_t n_pairs, int32_t* dist,
                           int32_t device)
{
    using namespace ldpc;
    constexpr int32_t kMaxLen = 800;  // 64 lanes x (801 x 2 B + 800 B) of LDS
    if (n_seqs < 0 || n_pairs < 0 || (n_pairs > 0 && (!pair_a || !pair_b || !dist || !offsets || !lengths))) {
        set_error("ldpc_dna_edit_distance: bad arguments");
        return LDPC_ERR_ARG;
    }
    if (n_pairs == 0) return LDPC_OK;
    int64_t total = 0;
    int32_t max_len = 0;
    // (the pair and length checks come before the null check here, and empty reads count into total)
    const std::string err = ragged::extent(offsets, lengths, n_seqs, &total, true, &max_len);
    if (!err.empty()) {
        set_error("ldpc_dna_edit_distance: " + err);
        return LDPC_ERR_ARG;
    }
    for (int64_t p = 0; p < n_pairs; p++) {
        if (pair_a[p] < 0 || pair_a[p] >= n_seqs || pair_b[p] < 0 || pair_b[p] >= n_seqs) {
            set_error("ldpc_dna_edit_distance: pair index out of range");
            return LDPC_ERR_ARG;
        }
    }
    if (max_len > kMaxLen) {
        set_error("ldpc_dna_edit_distance: sequences longer than 800 are not supported");
        return LDPC_ERR_UNSUPPORTED;
    }
    if (total > 0 && !seqs) {
        set_error("ldpc_dna_edit_distance: null sequences");
        return LDPC_ERR_ARG;
    }
    if (int rc = select_device("ldpc_dna_edit_distance", device)) return rc;
    dev_ptr<uint8_t> ds;
    dev_ptr<int64_t> doff;
    dev_ptr<int32_t> dlen, da, db, dd;
    int rc;
    if ((rc = upload(ds, seqs, (size_t)total)) || (rc = upload(doff, offsets, (size_t)n_seqs)) ||
        (rc = upload(dlen, lengths, (size_t)n_seqs)) || (rc = upload(da, pair_a, (size_t)n_pairs)) ||
        (rc = upload(db, pair_b, (size_t)n_pairs)) || (rc = dev_alloc(dd, (size_t)n_pairs)) ||
        (rc = launch_edit_distance(ds.get(), doff.get(), dlen.get(), da.get(), db.get(), n_pairs, max_len, dd.get())))
        return rc;
    return download(dist, dd.get(), (size_t)n_pairs);
}

int ldpc_dna_index_encode(const int32_t* index, int64_t n, uint8_t* prefix)
{
    if (n < 0 || (n > 0 && (!index || !prefix))) {
        set_error("ldpc_dna_index_encode: bad arguments");
        return LDPC_ERR_ARG;
    }
    for (int64_t i = 0; i < n; i++) {
        if (index[i] < 0 || index[i] > 0xffff) {
            set_error("ldpc_dna_index_encode: index " + std::to_string(i) + " is outside 0..65535");
            return LDPC_ERR_ARG;
        }
    }
    for (int64_t i = 0; i < n; i++) {
        const uint32_t word = ldpc::rs::rs_index_codeword((uint32_t)index[i]);
        for (int k = 0; k < ldpc::rs::kPrefixNt; k++)
            prefix[(size_t)i * ldpc::rs::kPrefixNt + k] = ldpc::rs::rs_prefix_base(word, k);
    }
    return LDPC_OK;
}

// Shared argument check of the two index decoders; *total = bytes of seqs the reads span.
static int index_decode_args(const char* who, const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths,
                             int64_t n, const int32_t* index, const int32_t* cnumerr, int64_t* total)
{
    *total = 0;
    if (n < 0 || (n > 0 && (!offsets || !lengths || !index || !cnumerr))) {
        set_error(std::string(who) + ": bad arguments");
        return LDPC_ERR_ARG;
    }
    const std::string err = ldpc::ragged::check(seqs, offsets, lengths, n, total);
    if (!err.empty()) {
        set_error(std::string(who) + ": " + err);
        return LDPC_ERR_ARG;
    }
    return LDPC_OK;
}

int ldpc_dna_index_decode_host(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, int64_t n,
                               int32_t* index, int32_t* cnumerr)
{
    int64_t total = 0;
    if (int rc = index_decode_args("ldpc_dna_index_decode_host", seqs, offsets, lengths, n, index, cnumerr, &total))
        return rc;
    for (int64_t i = 0; i < n; i++)
        ldpc::rs::rs_read_decode(lengths[i] ? seqs + offsets[i] : nullptr, lengths[i], &index[i], &cnumerr[i]);
    return LDPC_OK;
}

int ldpc_dna_index_decode(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, int64_t n,
                          int32_t* index, int32_t* cnumerr, int32_t device)
{
    using namespace ldpc;
    int64_t total = 0;
    if (int rc = index_decode_args("ldpc_dna_index_decode", seqs, offsets, lengths, n, index, cnumerr, &total))
        return rc;
    if (n == 0) return LDPC_OK;
    if (n > (int64_t)INT32_MAX * 256) {
        set_error("ldpc_dna_index_decode: too many reads for one call");
        return LDPC_ERR_UNSUPPORTED;
    }
    if (int rc = select_device("ldpc_dna_index_decode", device)) return rc;
    dev_ptr<uint8_t> ds;
    dev_ptr<int64_t> doff;
    dev_ptr<int32_t> dlen, di, dc;
    int rc;
    if ((rc = upload(ds, seqs, (size_t)total)) || (rc = upload(doff, offsets, (size_t)n)) ||
        (rc = upload(dlen, lengths, (size_t)n)) || (rc = dev_alloc(di, (size_t)n)) || (rc = dev_alloc(dc, (size_t)n)) ||
        (rc = launch(k_rs_index_decode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, ds.get(), doff.get(),
                     dlen.get(), n, di.get(), dc.get())) ||
        (rc = download(index, di.get(), (size_t)n)))
        return rc;
    return download(cnumerr, dc.get(), (size_t)n);
}

// Shared argument check of the two strand writers.
static int strands_args(const char* who, const uint8_t* codewords, int32_t n_cw, int64_t N, const int32_t* index,
                        const uint8_t* out)
{
    if (n_cw < 2 || n_cw % 2 || N < 0 || (N > 0 && (!codewords || !index || !out))) {
        set_error(std::string(who) + ": bad arguments (n_cw must be even and >= 2)");
        return LDPC_ERR_ARG;
    }
    if (N > INT64_MAX / n_cw) {
        set_error(std::string(who) + ": n_cw * N bytes overflow the address space");
        return LDPC_ERR_ARG;
    }
    for (int64_t j = 0; j < N; j++) {
        if (index[j] < 0 || index[j] > 0xffff) {
            set_error(std::string(who) + ": index " + std::to_string(j) + " is outside 0..65535");
            return LDPC_ERR_ARG;
        }
    }
    return LDPC_OK;
}

int ldpc_dna_strands_host(const uint8_t* codewords, int32_t n_cw, int64_t N, const int32_t* index, uint8_t* out)
{
    if (int rc = strands_args("ldpc_dna_strands_host", codewords, n_cw, N, index, out)) return rc;
    const size_t L = (size_t)ldpc::rs::kPrefixNt + (size_t)n_cw / 2;
    for (int64_t j = 0; j < N; j++) {
        const uint32_t word = ldpc::rs::rs_index_codeword((uint32_t)index[j]);
        for (int k = 0; k < ldpc::rs::kPrefixNt; k++) out[(size_t)j * L + k] = ldpc::rs::rs_prefix_base(word, k);
    }
    // row pairs outermost: the codeword rows are read in order, once
    for (size_t k = 0; k < (size_t)n_cw / 2; k++) {
        const uint8_t* hi = codewords + (2 * k) * (size_t)N;
        const uint8_t* lo = hi + (size_t)N;
        for (int64_t j = 0; j < N; j++)
            out[(size_t)j * L + ldpc::rs::kPrefixNt + k] = (uint8_t)("ACGT"[2 * (hi[j] & 1) + (lo[j] & 1)]);
    }
    return LDPC_OK;
}

int ldpc_dna_strands(const uint8_t* codewords, int32_t n_cw, int64_t N, const int32_t* index, uint8_t* out,
                     int32_t device)
{
    using namespace ldpc;
    if (int rc = strands_args("ldpc_dna_strands", codewords, n_cw, N, index, out)) return rc;
    if (N == 0) return LDPC_OK;
    const int64_t L = rs::kPrefixNt + n_cw / 2;
    const int64_t chunks = (L + kStrChunk - 1) / kStrChunk;
    if (chunks > kStrMaxChunks || N > (int64_t)INT32_MAX * kStrTile || N > INT64_MAX / L) {
        set_error("ldpc_dna_strands: shape too large for one call");
        return LDPC_ERR_UNSUPPORTED;
    }
    if (int rc = select_device("ldpc_dna_strands", device)) return rc;
    dev_ptr<uint8_t> dcw, dout;
    dev_ptr<int32_t> di;
    int rc;
    if ((rc = upload(dcw, codewords, (size_t)n_cw * (size_t)N)) || (rc = upload(di, index, (size_t)N)) ||
        (rc = dev_alloc(dout, (size_t)N * (size_t)L)) ||
        (rc = launch(k_strands_write, dim3((unsigned)((N + kStrTile - 1) / kStrTile), (unsigned)chunks), dim3(256), 0,
                     nullptr, dcw.get(), di.get(), n_cw, N, dout.get())))
        return rc;
    return download(out, dout.get(), (size_t)N * (size_t)L);
}

}  // extern "C"

// --- the centre-star alignment (star_align.hpp) ---------
namespace {

using namespace ldpc;

constexpr int64_t kStarMaxGroup = 32768;           // reads per group (the host keeps a k x k distance matrix)
constexpr int64_t kStarDefaultWs = 256ll << 20;    // workspace_bytes = 0

struct StarCall {
    const uint8_t* seqs;
    const int64_t* offsets;
    const int32_t* lengths;
    int64_t n_seqs;
    const int64_t* group_ptr;
    int64_t n_groups;
    int32_t* center;
    int32_t* width;
    int64_t* out_ptr;
    uint8_t* out;
    int64_t out_capacity;
    int64_t* out_needed;
    int32_t* dist;
    std::vector<uint8_t>* out_vec = nullptr;  // internal callers: sized to the rows and filled instead of out
};

// What both entry points gather before the merge: the centre of every group
// (index inside the group), and per sequence its script and distance to the centre.
struct StarScripts {
    std::vector<int64_t> centre;
    std::vector<star::RowScript> rows;
    std::vector<int32_t> dist;
    std::vector<star::Script> host;  // the scripts made on the host, by sequence
};

int star_args(const std::string& who, const StarCall& a)
{
    if (a.n_seqs < 0 || a.n_groups < 0 || a.out_capacity < 0 || (a.n_seqs > 0 && (!a.offsets || !a.lengths)) ||
        (a.n_groups > 0 && (!a.group_ptr || !a.center || !a.width || !a.out_ptr)) || (a.out_capacity > 0 && !a.out)) {
        set_error(who + ": bad arguments");
        return LDPC_ERR_ARG;
    }
    if (a.out_needed) *a.out_needed = 0;
    int64_t total = 0;
    const std::string err = ldpc::ragged::check(a.seqs, a.offsets, a.lengths, a.n_seqs, &total);
    if (!err.empty()) {
        set_error(who + ": " + err);
        return LDPC_ERR_ARG;
    }
    if (a.n_groups == 0 ? a.n_seqs != 0 : (a.group_ptr[0] != 0 || a.group_ptr[a.n_groups] != a.n_seqs)) {
        set_error(who + ": group_ptr must run from 0 to n_seqs");
        return LDPC_ERR_ARG;
    }
    for (int64_t g = 0; g < a.n_groups; g++) {
        if (a.group_ptr[g + 1] < a.group_ptr[g] || a.group_ptr[g + 1] > a.n_seqs) {
            set_error(who + ": group_ptr is not monotone");
            return LDPC_ERR_ARG;
        }
        if (a.group_ptr[g + 1] - a.group_ptr[g] > kStarMaxGroup) {
            set_error(who + ": more than " + std::to_string(kStarMaxGroup) + " reads in one group");
            return LDPC_ERR_ARG;
        }
    }
    return LDPC_OK;
}

const uint8_t* star_seq(const StarCall& a, int64_t i) { return a.lengths[i] ? a.seqs + a.offsets[i] : nullptr; }

// One group on the host (star::group_scripts) into s.
void star_group_host(const StarCall& a, int64_t g, StarScripts* s)
{
    const int64_t g0 = a.group_ptr[g], k = a.group_ptr[g + 1] - g0;
    if (k == 0) return;
    std::vector<const uint8_t*> rd((size_t)k);
    std::vector<int64_t> ln((size_t)k);
    for (int64_t q = 0; q < k; q++) {
        rd[(size_t)q] = star_seq(a, g0 + q);
        ln[(size_t)q] = a.lengths[g0 + q];
    }
    s->centre[(size_t)g] = star::group_scripts(rd.data(), ln.data(), k, s->host.data() + g0);
    for (int64_t q = 0; q < k; q++) {
        const star::Script& sc = s->host[(size_t)(g0 + q)];
        s->rows[(size_t)(g0 + q)] = star::RowScript{sc.at.data(), sc.cnt.data(), sc.ins.data()};
        s->dist[(size_t)(g0 + q)] = (int32_t)sc.dist;
    }
}

// The merge: widths and out_ptr first, then (if the buffer holds them) the rows.
int star_finish(const std::string& who, const StarCall& a, const StarScripts& s)
{
    std::vector<int32_t> w;
    int64_t total = 0;
    for (int64_t g = 0; g < a.n_groups; g++) {
        const int64_t g0 = a.group_ptr[g], k = a.group_ptr[g + 1] - g0;
        a.out_ptr[g] = total;
        a.center[g] = k ? (int32_t)s.centre[(size_t)g] : -1;
        a.width[g] = 0;
        if (k == 0) continue;
        const int64_t n = a.lengths[g0 + s.centre[(size_t)g]];
        const int64_t wd = star::merge_width(s.rows.data() + g0, k, s.centre[(size_t)g], n, &w);
        if (wd > INT32_MAX || (wd > 0 && k > (INT64_MAX - total) / wd)) {
            set_error(who + ": the aligned rows overflow the output sizes");
            return LDPC_ERR_ARG;
        }
        a.width[g] = (int32_t)wd;
        total += k * wd;
    }
    if (a.n_groups > 0) a.out_ptr[a.n_groups] = total;
    if (a.out_needed) *a.out_needed = total;
    if (a.dist) std::copy(s.dist.begin(), s.dist.end(), a.dist);
    uint8_t* out = a.out;
    if (a.out_vec) {
        a.out_vec->resize((size_t)total);
        out = a.out_vec->data();
    } else if (total > a.out_capacity) {
        set_error(who + ": the output buffer holds " + std::to_string(a.out_capacity) + " bytes, the rows need " +
                  std::to_string(total));
        return LDPC_ERR_ARG;
    }
    for (int64_t g = 0; g < a.n_groups; g++) {
        const int64_t g0 = a.group_ptr[g], k = a.group_ptr[g + 1] - g0;
        if (k == 0) continue;
        const int64_t c = s.centre[(size_t)g], n = a.lengths[g0 + c];
        const int64_t wd = star::merge_width(s.rows.data() + g0, k, c, n, &w);
        star::merge_rows(s.rows.data() + g0, k, c, star_seq(a, g0 + c), n, w, wd, out + a.out_ptr[g]);
    }
    return LDPC_OK;
}

void star_scripts_init(const StarCall& a, StarScripts* s)
{
    s->centre.assign((size_t)a.n_groups, 0);
    s->rows.assign((size_t)a.n_seqs, star::RowScript());
    s->dist.assign((size_t)a.n_seqs, 0);
    s->host.assign((size_t)a.n_seqs, star::Script());
}

int star_align_host(const StarCall& a)
{
    const std::string who = "ldpc_dna_star_align_host";
    if (int rc = star_args(who, a)) return rc;
    StarScripts s;
    star_scripts_init(a, &s);
    for (int64_t g = 0; g < a.n_groups; g++) star_group_host(a, g, &s);
    return star_finish(who, a, s);
}

// The reads, resident for the device aligner; seqs is the caller's copy or own_seqs.
struct StarDev {
    dev_ptr<uint8_t> own_seqs;
    const uint8_t* seqs = nullptr;
    dev_ptr<int64_t> off;
    dev_ptr<int32_t> len;
};

// The centres of the on-device groups of more than two reads: k_edit_distance
// on all in-group pairs (k = 2: the tie goes to read 0, s->centre stays 0).
int star_centres(const StarCall& a, const std::vector<uint8_t>& on_dev, const StarDev& d, int32_t max_len, StarScripts* s)
{
    std::vector<int32_t> pa, pb;
    for (int64_t g = 0; g < a.n_groups; g++) {
        const int64_t g0 = a.group_ptr[g], k = a.group_ptr[g + 1] - g0;
        if (!on_dev[(size_t)g] || k <= 2) continue;
        for (int64_t x = 0; x < k; x++)
            for (int64_t y = x + 1; y < k; y++) {
                pa.push_back((int32_t)(g0 + x));
                pb.push_back((int32_t)(g0 + y));
            }
    }
    const size_t np = pa.size();
    if (np == 0) return LDPC_OK;
    std::vector<int32_t> dist(np);
    dev_ptr<int32_t> da, db, dd;
    int rc;
    if ((rc = upload(da, pa)) || (rc = upload(db, pb)) || (rc = dev_alloc(dd, np)) ||
        (rc = launch_edit_distance(d.seqs, d.off.get(), d.len.get(), da.get(), db.get(), (int64_t)np, max_len,
                                   dd.get())) ||
        (rc = download(dist.data(), dd.get(), np)))
        return rc;
    const int32_t* dp = dist.data();
    std::vector<int64_t> dm;
    for (int64_t g = 0; g < a.n_groups; g++) {
        const int64_t k = a.group_ptr[g + 1] - a.group_ptr[g];
        if (!on_dev[(size_t)g] || k <= 2) continue;
        dm.assign((size_t)(k * k), 0);
        for (int64_t x = 0; x < k; x++)
            for (int64_t y = x + 1; y < k; y++) dm[(size_t)(x * k + y)] = dm[(size_t)(y * k + x)] = *dp++;
        s->centre[(size_t)g] = star::choose_centre(dm.data(), k);
    }
    return LDPC_OK;
}

// The scripts of the packed pairs as k_star_align_pairs leaves them.
struct StarPairsOut {
    std::vector<uint8_t> at, ins;
    std::vector<int32_t> cnt, dist;
};

// k_star_align_pairs over the packed pairs, one launch per pass, and its outputs to the host.
int star_run_pairs(const star::PairBlocks& pb, const star::Passes& ps, const StarDev& d, StarPairsOut* h)
{
    const size_t P = pb.pr.size(), n_at = (size_t)pb.at_total, n_ins = (size_t)pb.ins_total;
    h->at.resize(n_at);
    h->ins.resize(n_ins);
    h->cnt.resize(n_at + P);
    h->dist.resize(P);
    if (P == 0) return LDPC_OK;
    dev_ptr<int32_t> dpr, dpc, dbp, dcnt, ddist;
    dev_ptr<int64_t> dbf, dbw, dao, dio;
    dev_ptr<uint32_t> dws;
    dev_ptr<uint8_t> dat, dins;
    int rc;
    if ((rc = upload(dpr, pb.pr)) || (rc = upload(dpc, pb.pc)) || (rc = upload(dbf, pb.blk_first)) ||
        (rc = upload(dbw, ps.blk_ws)) || (rc = upload(dbp, pb.blk_wpr)) || (rc = upload(dao, pb.at_off)) ||
        (rc = upload(dio, pb.ins_off)) || (rc = dev_alloc(dws, (size_t)ps.ws_words)) || (rc = dev_alloc(dat, n_at)) ||
        (rc = dev_alloc(dcnt, n_at + P)) || (rc = dev_alloc(dins, n_ins)) || (rc = dev_alloc(ddist, P)))
        return rc;
    const size_t lds = (sizeof(uint16_t) * (size_t)(pb.max_n + 1) + (size_t)pb.max_n) * 64;
    for (size_t q = 0; q + 1 < ps.pass_first.size(); q++) {
        const int64_t b0 = ps.pass_first[q], nb = ps.pass_first[q + 1] - b0;
        if ((rc = launch(k_star_align_pairs, dim3((unsigned)nb), dim3(64), lds, nullptr, d.seqs, d.off.get(), d.len.get(),
                         dpr.get(), dpc.get(), dbf.get(), dbw.get(), dbp.get(), dao.get(), dio.get(), b0, pb.max_n,
                         dws.get(), dat.get(), dcnt.get(), dins.get(), ddist.get())))
            return rc;
    }
    if ((rc = download(h->at.data(), dat.get(), n_at)) || (rc = download(h->cnt.data(), dcnt.get(), n_at + P)) ||
        (rc = download(h->ins.data(), dins.get(), n_ins)))
        return rc;
    return download(h->dist.data(), ddist.get(), P);
}

// dev_seqs (may be null): a.seqs already resident on `device` (the read planner's reads).
// The planning (which groups, blocks, passes) is star_align.hpp's; here are the
// uploads, the centre search, the pass loop and the downloads.
int star_align_device(const StarCall& a, int32_t device, int64_t workspace_bytes, int64_t* stats,
                      const std::string& who = "ldpc_dna_star_align", const uint8_t* dev_seqs = nullptr)
{
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (int rc = star_args(who, a)) return rc;
    if (workspace_bytes < 0) {
        set_error(who + ": negative workspace_bytes");
        return LDPC_ERR_ARG;
    }
    if (a.n_seqs > INT32_MAX) {
        set_error(who + ": too many sequences for one call");
        return LDPC_ERR_UNSUPPORTED;
    }
    StarScripts s;
    star_scripts_init(a, &s);
    if (a.n_groups == 0) return star_finish(who, a, s);
    int rc;
    if ((rc = select_device(who.c_str(), device))) return rc;
    const int64_t budget_words = (workspace_bytes ? workspace_bytes : kStarDefaultWs) / 4;

    // the groups the device takes, and the bytes of seqs they span
    std::vector<uint8_t> on_dev((size_t)a.n_groups, 0);
    int64_t seq_bytes = 0;
    int32_t max_len = 0;
    for (int64_t g = 0; g < a.n_groups; g++) {
        const int64_t g0 = a.group_ptr[g], k = a.group_ptr[g + 1] - g0;
        on_dev[(size_t)g] = star::device_eligible(a.lengths + g0, k);
        if (!on_dev[(size_t)g]) continue;
        for (int64_t q = g0; q < g0 + k; q++) {
            max_len = std::max(max_len, a.lengths[q]);
            if (a.lengths[q]) seq_bytes = std::max<int64_t>(seq_bytes, a.offsets[q] + a.lengths[q]);
        }
    }
    StarDev d;
    if ((!dev_seqs && (rc = upload(d.own_seqs, a.seqs, (size_t)seq_bytes))) ||
        (rc = upload(d.off, a.offsets, (size_t)a.n_seqs)) || (rc = upload(d.len, a.lengths, (size_t)a.n_seqs)))
        return rc;
    d.seqs = dev_seqs ? dev_seqs : d.own_seqs.get();
    if ((rc = star_centres(a, on_dev, d, max_len, &s))) return rc;
    for (int64_t g = 0; g < a.n_groups; g++) {
        const int64_t g0 = a.group_ptr[g], k = a.group_ptr[g + 1] - g0;
        if (on_dev[(size_t)g]) on_dev[(size_t)g] = star::within_budget(a.lengths + g0, k, s.centre[(size_t)g], budget_words);
    }

    const star::PairBlocks pb = star::pack_pairs(a.lengths, a.group_ptr, a.n_groups, s.centre.data(), on_dev.data(),
                                                 budget_words);
    const star::Passes ps = star::cut_passes(pb.blk_words, budget_words);
    const int64_t P = (int64_t)pb.pr.size();
    StarPairsOut h;
    if ((rc = star_run_pairs(pb, ps, d, &h))) return rc;
    for (int64_t p = 0; p < P; p++) {
        const int64_t q = pb.pr[(size_t)p], m = a.lengths[q], n = a.lengths[pb.pc[(size_t)p]];
        const int32_t* cnt = h.cnt.data() + pb.at_off[(size_t)p] + p;
        int64_t t = 0;
        if (!star::script_consistent(cnt, m, n, &t)) {
            set_error(who + ": a device script is inconsistent with its read");
            return LDPC_ERR_DEVICE;
        }
        s.rows[(size_t)q] = star::RowScript{h.at.data() + pb.at_off[(size_t)p], cnt, h.ins.data() + pb.ins_off[(size_t)p] + m - t};
        s.dist[(size_t)q] = h.dist[(size_t)p];
    }
    for (int64_t g = 0; g < a.n_groups; g++)
        if (!on_dev[(size_t)g]) star_group_host(a, g, &s);
    if (stats) {
        stats[0] = pb.n_host;
        stats[1] = (int64_t)ps.pass_first.size() - 1;
        stats[2] = P;
    }
    return star_finish(who, a, s);
}

}  // namespace

extern "C" {

int ldpc_dna_star_align_host(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, int64_t n_seqs,
                             const int64_t* group_ptr, int64_t n_groups, int32_t* center, int32_t* width,
                             int64_t* out_ptr, uint8_t* out, int64_t out_capacity, int64_t* out_needed, int32_t* dist)
{
    const StarCall a{seqs, offsets, lengths, n_seqs, group_ptr, n_groups, center, width,
                     out_ptr, out, out_capacity, out_needed, dist};
    return dna_guard("ldpc_dna_star_align_host", [&] { return star_align_host(a); });
}

int ldpc_dna_star_align(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, int64_t n_seqs,
                        const int64_t* group_ptr, int64_t n_groups, int32_t* center, int32_t* width, int64_t* out_ptr,
                        uint8_t* out, int64_t out_capacity, int64_t* out_needed, int32_t* dist, int32_t device,
                        int64_t workspace_bytes, int64_t* stats)
{
    const StarCall a{seqs, offsets, lengths, n_seqs, group_ptr, n_groups, center, width,
                     out_ptr, out, out_capacity, out_needed, dist};
    return dna_guard("ldpc_dna_star_align", [&] { return star_align_device(a, device, workspace_bytes, stats); });
}

}  // extern "C"

// --- the read planner (dna_plan.hpp) --------------------
#include "dna_plan_kernels.hpp"

namespace {

ldpc::plan::Args plan_args(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, const int32_t* quals,
                           int64_t n_reads, const int32_t* index_vals, const int32_t* strands, int32_t n_strands,
                           int32_t payload_nt, int32_t align, int32_t* kind, int64_t* row_ptr, uint8_t* rows,
                           int32_t* row_q, int64_t* stats)
{
    return ldpc::plan::Args{seqs, offsets, lengths, quals, n_reads, index_vals, strands, n_strands,
                            payload_nt, align, kind, row_ptr, rows, row_q, stats};
}

// k_dna_llr on a device-resident plan, and its outputs to the host.
int llr_from_plan(const ldpc::PlanDev& pd, int32_t n_strands, int32_t payload_nt, double llr_unit, double* llr,
                  uint8_t* int_mask, int8_t* codes, int32_t* codes_exact)
{
    using namespace ldpc;
    const size_t out_n = (size_t)2 * payload_nt * n_strands;
    dev_ptr<double> dl;
    dev_ptr<uint8_t> dm;   // null unless int_mask
    dev_ptr<int8_t> dc;    // null unless codes, with dov
    dev_ptr<int32_t> dov;
    const int32_t zero = 0;
    int rc;
    if ((rc = dev_alloc(dl, out_n)) || (int_mask && (rc = dev_alloc(dm, out_n))) ||
        (codes && ((rc = dev_alloc(dc, out_n)) || (rc = upload(dov, &zero, 1)))))
        return rc;
    if ((rc = launch_dna_llr(pd.kind.get(), pd.row_ptr.get(), pd.rows.get(), pd.row_q.get(), n_strands, payload_nt,
                             llr_unit, dl.get(), dm.get(), dc.get(), dov.get())))
        return rc;
    if ((rc = download(llr, dl.get(), out_n)) || (int_mask && (rc = download(int_mask, dm.get(), out_n)))) return rc;
    if (codes) {
        int32_t ov = 0;
        if ((rc = download(codes, dc.get(), out_n)) || (rc = download(&ov, dov.get(), 1))) return rc;
        *codes_exact = ov ? 0 : 1;
    }
    return LDPC_OK;
}

// the LLRs of a plan made on the host
int dna_llr(int32_t n_strands, const int32_t* kind, const int64_t* row_ptr, const uint8_t* rows, const int32_t* row_q,
            int32_t payload_nt, double llr_unit, double* llr, uint8_t* int_mask, int8_t* codes, int32_t* codes_exact,
            int32_t device)
{
    using namespace ldpc;
    if (n_strands < 0 || payload_nt < 1 || !kind || !row_ptr || !llr || (codes && !codes_exact)) {
        set_error("ldpc_dna_llr: bad arguments");
        return LDPC_ERR_ARG;
    }
    if (codes_exact) *codes_exact = 1;
    if (n_strands == 0) return LDPC_OK;
    const int64_t R = row_ptr[n_strands];
    if (R < 0 || R > INT64_MAX / payload_nt || row_ptr[0] != 0 || (R > 0 && (!rows || !row_q))) {
        set_error("ldpc_dna_llr: bad row_ptr / rows");
        return LDPC_ERR_ARG;
    }
    for (int32_t s = 0; s < n_strands; s++) {
        if (row_ptr[s + 1] < row_ptr[s] || kind[s] < 0 || kind[s] > 3) {
            set_error("ldpc_dna_llr: row_ptr not monotone or kind out of range");
            return LDPC_ERR_ARG;
        }
    }
    int rc;
    if ((rc = select_device("ldpc_dna_llr", device))) return rc;
    PlanDev pd;
    pd.R = R;
    if ((rc = upload(pd.kind, kind, (size_t)n_strands)) || (rc = upload(pd.row_ptr, row_ptr, (size_t)n_strands + 1)) ||
        (rc = upload(pd.rows, rows, (size_t)R * payload_nt)) || (rc = upload(pd.row_q, row_q, (size_t)R)))
        return rc;
    return llr_from_plan(pd, n_strands, payload_nt, llr_unit, llr, int_mask, codes, codes_exact);
}

int reads_llr(const ldpc::plan::Args& a, int32_t device, int64_t workspace_bytes, double llr_unit, double* llr,
              uint8_t* int_mask, int8_t* codes, int32_t* codes_exact)
{
    using namespace ldpc;
    const std::string who = "ldpc_dna_reads_llr";
    if (!llr || (codes && !codes_exact)) {
        set_error(who + ": bad arguments");
        return LDPC_ERR_ARG;
    }
    PlanDev pd;
    if (int rc = plan_device(who, a, false, device, workspace_bytes, &pd)) return rc;
    if (codes_exact) *codes_exact = 1;
    if (a.n_strands == 0) return LDPC_OK;
    return llr_from_plan(pd, a.n_strands, a.payload_nt, llr_unit, llr, int_mask, codes, codes_exact);
}

}  // namespace

extern "C" {

int ldpc_dna_llr(int32_t n_strands, const int32_t* kind, const int64_t* row_ptr, const uint8_t* rows,
                 const int32_t* row_q, int32_t payload_nt, double llr_unit, double* llr, uint8_t* int_mask,
                 int32_t device)
{
    return dna_llr(n_strands, kind, row_ptr, rows, row_q, payload_nt, llr_unit, llr, int_mask, nullptr, nullptr,
                   device);
}

int ldpc_dna_llr_codes(int32_t n_strands, const int32_t* kind, const int64_t* row_ptr, const uint8_t* rows,
                       const int32_t* row_q, int32_t payload_nt, double llr_unit, double* llr, uint8_t* int_mask,
                       int8_t* codes, int32_t* codes_exact, int32_t device)
{
    return dna_llr(n_strands, kind, row_ptr, rows, row_q, payload_nt, llr_unit, llr, int_mask, codes, codes_exact,
                   device);
}

int ldpc_dna_plan_host(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, const int32_t* quals,
                       int64_t n_reads, const int32_t* index_vals, const int32_t* strands, int32_t n_strands,
                       int32_t payload_nt, int32_t align, int32_t* kind, int64_t* row_ptr, uint8_t* rows,
                       int32_t* row_q, int64_t* stats)
{
    return ldpc::dna_guard("ldpc_dna_plan_host", [&]() -> int {
        const std::string err = ldpc::plan::plan_host(plan_args(seqs, offsets, lengths, quals, n_reads, index_vals,
                                                                strands, n_strands, payload_nt, align, kind, row_ptr,
                                                                rows, row_q, stats));
        if (err.empty()) return LDPC_OK;
        set_error("ldpc_dna_plan_host: " + err);
        return LDPC_ERR_ARG;
    });
}

int ldpc_dna_plan(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, const int32_t* quals,
                  int64_t n_reads, const int32_t* index_vals, const int32_t* strands, int32_t n_strands,
                  int32_t payload_nt, int32_t align, int32_t device, int64_t workspace_bytes, int32_t* kind,
                  int64_t* row_ptr, uint8_t* rows, int32_t* row_q, int64_t* stats)
{
    return ldpc::dna_guard("ldpc_dna_plan", [&] {
        ldpc::PlanDev pd;
        return ldpc::plan_device("ldpc_dna_plan", plan_args(seqs, offsets, lengths, quals, n_reads, index_vals, strands,
                                                            n_strands, payload_nt, align, kind, row_ptr, rows, row_q,
                                                            stats),
                                 true, device, workspace_bytes, &pd);
    });
}

int ldpc_dna_reads_llr(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, const int32_t* quals,
                       int64_t n_reads, const int32_t* index_vals, const int32_t* strands, int32_t n_strands,
                       int32_t payload_nt, int32_t align, int32_t device, int64_t workspace_bytes, double llr_unit,
                       double* llr, uint8_t* int_mask, int8_t* codes, int32_t* codes_exact, int32_t* kind,
                       int64_t* stats)
{
    return ldpc::dna_guard("ldpc_dna_reads_llr", [&] {
        return reads_llr(plan_args(seqs, offsets, lengths, quals, n_reads, index_vals, strands, n_strands, payload_nt,
                                   align, kind, nullptr, nullptr, nullptr, stats),
                         device, workspace_bytes, llr_unit, llr, int_mask, codes, codes_exact);
    });
}

}  // extern "C"

// --- the sequencing channel (dna_sim.hpp) ---------------
#include "dna_sim_kernels.hpp"

// --- the trial handle (dna_trial.hpp) -------------------
#include "dna_trial_kernels.hpp"
