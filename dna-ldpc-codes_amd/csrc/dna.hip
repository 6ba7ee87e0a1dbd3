// dna.hip -- the step before the decoder: per-strand
// read candidates -> the 272 x 18432 LLR matrix the first decode consumes,
// plus the pairwise edit distances that pick which ragged candidates go to
// the aligner.
//
// Reference: ex_decoder/decoder.py:142-519 (the strand loop; count rule
// :266-320 and :442-497), def_func.py:10-26 (edit_dist), :97-117
// (DNA2binary).  The host mirror (dna_llr.py) classifies every strand into a
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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ldpc_amd.h"
#include "engine.hpp"
#include "rs_index.hpp"

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
    const int last_bit = 2 * nt - 1;
    for (int h = 0; h < 2; h++) {
        const int b = 2 * k + h;
        int n = 0;  // the count difference: the entry is n * L (0 for an int-0 entry)
        bool is_int = true;
        if (kd == 1) {
            int c0 = 0, c1 = 0, q0 = 0, q1 = 0;
            for (int64_t r = r0; r < r1; r++) {
                const int q = row_q[r];
                if (b == last_bit && q < kQSkip) continue;
                if (bit_is_zero(rows[r * nt + k], h == 0)) { c0++; q0 += q; }
                else { c1++; q1 += q; }
            }
            if (b == last_bit && c0 == 1 && c1 == 1) {
                if (q0 < kQSkip && q1 >= kQHigh) { n = -2; is_int = false; }
                else if (q0 >= kQHigh && q1 < kQSkip) { n = 2; is_int = false; }
            } else {
                n = c0 - c1;
                is_int = false;
            }
        } else if (kd == 2 && b == last_bit && r1 > r0) {
            if (row_q[r0] > kQHigh) {
                n = bit_is_zero(rows[r0 * nt], false) ? 1 : -1;
                is_int = false;
            }
        } else if (kd == 3 && b == last_bit) {
            int c0 = 0, c1 = 0;
            for (int64_t r = r0; r < r1; r++) {
                if (row_q[r] <= kQHigh) continue;
                if (bit_is_zero(rows[r * nt], false)) c0++;
                else c1++;
            }
            n = c0 - c1;
            is_int = false;
        }
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

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T* as() { return static_cast<T*>(p); }
};

int dev_copy_in(DevBuf& d, const void* src, size_t bytes)
{
    LDPC_HIP(hipMalloc(&d.p, std::max<size_t>(bytes, 16)));
    if (bytes) LDPC_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return LDPC_OK;
}

}  // namespace
}  // namespace ldpc

using ldpc::set_error;

static int dna_llr(int32_t n_strands, const int32_t* kind, const int64_t* row_ptr, const uint8_t* rows,
                   const int32_t* row_q, int32_t payload_nt, double llr_unit, double* llr, uint8_t* int_mask,
                   int8_t* codes, int32_t* codes_exact, int32_t device)
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
    int ndev = 0;
    LDPC_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        set_error("ldpc_dna_llr: no such device");
        return LDPC_ERR_DEVICE;
    }
    LDPC_HIP(hipSetDevice(device));
    const size_t out_n = (size_t)2 * payload_nt * n_strands;
    DevBuf dk, dp, dr, dq, dl, dm, dc, dov;
    int rc;
    if ((rc = dev_copy_in(dk, kind, sizeof(int32_t) * n_strands))) return rc;
    if ((rc = dev_copy_in(dp, row_ptr, sizeof(int64_t) * ((size_t)n_strands + 1)))) return rc;
    if ((rc = dev_copy_in(dr, rows, (size_t)R * payload_nt))) return rc;
    if ((rc = dev_copy_in(dq, row_q, sizeof(int32_t) * (size_t)R))) return rc;
    LDPC_HIP(hipMalloc(&dl.p, sizeof(double) * out_n));
    if (int_mask) LDPC_HIP(hipMalloc(&dm.p, out_n));
    if (codes) {
        const int32_t zero = 0;
        LDPC_HIP(hipMalloc(&dc.p, out_n));
        if ((rc = dev_copy_in(dov, &zero, sizeof zero))) return rc;
    }
    dim3 grid((unsigned)((n_strands + 255) / 256), (unsigned)payload_nt);
    hipLaunchKernelGGL(k_dna_llr, grid, dim3(256), 0, 0, dk.as<int32_t>(), dp.as<int64_t>(), dr.as<uint8_t>(),
                       dq.as<int32_t>(), n_strands, payload_nt, llr_unit, dl.as<double>(),
                       int_mask ? dm.as<uint8_t>() : nullptr, codes ? dc.as<int8_t>() : nullptr,
                       codes ? dov.as<int32_t>() : nullptr);
    LDPC_HIP(hipGetLastError());
    LDPC_HIP(hipMemcpy(llr, dl.p, sizeof(double) * out_n, hipMemcpyDeviceToHost));
    if (int_mask) LDPC_HIP(hipMemcpy(int_mask, dm.p, out_n, hipMemcpyDeviceToHost));
    if (codes) {
        int32_t ov = 0;
        LDPC_HIP(hipMemcpy(codes, dc.p, out_n, hipMemcpyDeviceToHost));
        LDPC_HIP(hipMemcpy(&ov, dov.p, sizeof ov, hipMemcpyDeviceToHost));
        *codes_exact = ov ? 0 : 1;
    }
    return LDPC_OK;
}


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
    for (int64_t i = 0; i < n_seqs; i++) {
        if (lengths[i] < 0 || offsets[i] < 0 || offsets[i] > INT64_MAX - lengths[i]) {
            set_error("ldpc_dna_edit_distance: negative or overflowing length/offset");
            return LDPC_ERR_ARG;
        }
        total = std::max<int64_t>(total, offsets[i] + lengths[i]);
        max_len = std::max(max_len, lengths[i]);
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
    int ndev = 0;
    LDPC_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        set_error("ldpc_dna_edit_distance: no such device");
        return LDPC_ERR_DEVICE;
    }
    LDPC_HIP(hipSetDevice(device));
    DevBuf ds, doff, dlen, da, db, dd;
    int rc;
    if ((rc = dev_copy_in(ds, seqs, (size_t)total))) return rc;
    if ((rc = dev_copy_in(doff, offsets, sizeof(int64_t) * (size_t)n_seqs))) return rc;
    if ((rc = dev_copy_in(dlen, lengths, sizeof(int32_t) * (size_t)n_seqs))) return rc;
    if ((rc = dev_copy_in(da, pair_a, sizeof(int32_t) * (size_t)n_pairs))) return rc;
    if ((rc = dev_copy_in(db, pair_b, sizeof(int32_t) * (size_t)n_pairs))) return rc;
    LDPC_HIP(hipMalloc(&dd.p, sizeof(int32_t) * (size_t)n_pairs));
    const size_t lds = (sizeof(uint16_t) * (size_t)(max_len + 1) + (size_t)max_len) * 64;
    const unsigned blocks = (unsigned)((n_pairs + 63) / 64);
    hipLaunchKernelGGL(k_edit_distance, dim3(blocks), dim3(64), lds, 0, ds.as<uint8_t>(), doff.as<int64_t>(),
                       dlen.as<int32_t>(), da.as<int32_t>(), db.as<int32_t>(), n_pairs, max_len, dd.as<int32_t>());
    LDPC_HIP(hipGetLastError());
    LDPC_HIP(hipMemcpy(dist, dd.p, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyDeviceToHost));
    return LDPC_OK;
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
    for (int64_t i = 0; i < n; i++) {
        if (lengths[i] < 0 || offsets[i] < 0 || offsets[i] > INT64_MAX - lengths[i]) {
            set_error(std::string(who) + ": negative or overflowing length/offset");
            return LDPC_ERR_ARG;
        }
        if (lengths[i] > 0) *total = std::max<int64_t>(*total, offsets[i] + lengths[i]);
    }
    if (*total > 0 && !seqs) {
        set_error(std::string(who) + ": null sequences");
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        set_error("ldpc_dna_index_decode: no such device");
        return LDPC_ERR_DEVICE;
    }
    LDPC_HIP(hipSetDevice(device));
    DevBuf ds, doff, dlen, di, dc;
    int rc;
    if ((rc = dev_copy_in(ds, seqs, (size_t)total))) return rc;
    if ((rc = dev_copy_in(doff, offsets, sizeof(int64_t) * (size_t)n))) return rc;
    if ((rc = dev_copy_in(dlen, lengths, sizeof(int32_t) * (size_t)n))) return rc;
    LDPC_HIP(hipMalloc(&di.p, sizeof(int32_t) * (size_t)n));
    LDPC_HIP(hipMalloc(&dc.p, sizeof(int32_t) * (size_t)n));
    hipLaunchKernelGGL(k_rs_index_decode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ds.as<uint8_t>(),
                       doff.as<int64_t>(), dlen.as<int32_t>(), n, di.as<int32_t>(), dc.as<int32_t>());
    LDPC_HIP(hipGetLastError());
    LDPC_HIP(hipMemcpy(index, di.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    LDPC_HIP(hipMemcpy(cnumerr, dc.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return LDPC_OK;
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        set_error("ldpc_dna_strands: no such device");
        return LDPC_ERR_DEVICE;
    }
    LDPC_HIP(hipSetDevice(device));
    DevBuf dcw, di, dout;
    int rc;
    if ((rc = dev_copy_in(dcw, codewords, (size_t)n_cw * (size_t)N))) return rc;
    if ((rc = dev_copy_in(di, index, sizeof(int32_t) * (size_t)N))) return rc;
    LDPC_HIP(hipMalloc(&dout.p, (size_t)N * (size_t)L));
    hipLaunchKernelGGL(k_strands_write, dim3((unsigned)((N + kStrTile - 1) / kStrTile), (unsigned)chunks), dim3(256),
                       0, 0, dcw.as<uint8_t>(), di.as<int32_t>(), n_cw, N, dout.as<uint8_t>());
    LDPC_HIP(hipGetLastError());
    LDPC_HIP(hipMemcpy(out, dout.p, (size_t)N * (size_t)L, hipMemcpyDeviceToHost));
    return LDPC_OK;
}

}  // extern "C"
