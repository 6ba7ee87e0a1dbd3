// dna_plan_kernels.hpp -- the read planner on the GPU:
// the kernels and the host driver of ldpc_dna_plan / ldpc_dna_reads_llr.
// Included by dna.hip after its own kernels (k_rs_index_decode,
// k_edit_distance, k_dna_llr) and the device aligner, which the driver reuses
// on device-resident buffers.  The contract is dna_plan.hpp's; plan::plan_host
// is the comparator and the outputs are the same bytes.
//
// Stages (every index loaded from device memory is range-checked before use;
// a failed check sets PlanCtl::bad and the call fails with LDPC_ERR_DEVICE):
//   k_plan_locate      read -> payload view, strand position (binary search),
//                      per-strand counts and "not all payload_nt" flags
//   k_plan_scan        single-block exclusive scan (counts -> segment starts,
//                      pair counts -> pair starts, row counts -> row_ptr, ...)
//   k_plan_place       scatter of read ids into their segment, any order
//   k_plan_sort        rank sort of every segment: input order, whatever order
//                      the scatter's atomics retired in; 8 lanes per strand
//   k_plan_classify    strand -> kind, pair count, provisional row count
//   k_plan_pairs       pair p -> (a, b), the i < k row-major order of
//                      np.triu_indices, as positions of the sorted read list
//   k_edit_distance    (dna.hip) the distances
//   k_plan_close       reads with a partner at distance < 15
//   k_plan_cand_count / k_plan_cand_fill   the candidate list of every ragged
//                      strand: the aligner's groups, group s = strand s
//   k_plan_check_src / k_plan_cand_len / k_plan_cand_gather   only when the reads
//                      are device-resident already (PlanSrc):
//                      the range check of the reads, and the candidates packed
//                      for the one copy down the aligner's host merge needs
//   star_align_device  (dna.hip) on the resident reads; the merge is host code
//   k_plan_rows        one wave per row: rows, row_q, the kinds of aligned strands
#pragma once

namespace ldpc {
namespace {

constexpr int32_t kPlanMaxLen = 800;  // k_edit_distance's limit
constexpr int kPlanScanThreads = 1024;

struct PlanCtl {
    unsigned long long hist[4];  // cnumerr -1, 0, 1, 2
    int32_t max_ragged_len;      // longest read of a ragged strand
    int32_t long_read;           // lowest read id longer than kPlanMaxLen on a ragged strand
    int32_t empty_strand;        // lowest strand whose single read is empty with quality > 63
    int32_t bad;                 // an index failed its range check
};

__global__ void __launch_bounds__(256) k_plan_locate(const int32_t* __restrict__ index_vals,
                                                     const int32_t* __restrict__ cnumerr,
                                                     const int64_t* __restrict__ off, const int32_t* __restrict__ len,
                                                     int64_t n, const int32_t* __restrict__ strands, int32_t S,
                                                     int32_t nt, int32_t* __restrict__ pos, int64_t* __restrict__ poff,
                                                     int32_t* __restrict__ plen, int32_t* __restrict__ cnt,
                                                     int32_t* __restrict__ notfull, PlanCtl* __restrict__ ctl)
{
    __shared__ unsigned int hist[4];
    if (threadIdx.x < 4) hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        int64_t o = off[i];
        int32_t l = len[i], p = -1;
        bool valid = true;
        if (cnumerr) {  // raw reads: the prefix decoded by k_rs_index_decode
            const int32_t ne = cnumerr[i];
            atomicAdd(&hist[ne < 0 || ne > 2 ? 0 : ne + 1], 1u);
            valid = ne >= 0 && ne <= 2 && l >= rs::kPrefixNt;
            if (valid) {
                o += rs::kPrefixNt;
                l -= rs::kPrefixNt;
            }
        }
        if (valid) {
            const int32_t v = index_vals[i];
            int32_t lo = 0, hi = S;  // lower bound
            while (lo < hi) {
                const int32_t mid = lo + (hi - lo) / 2;
                if (strands[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            if (lo < S && strands[lo] == v) p = lo;
        }
        pos[i] = p;
        poff[i] = o;
        plen[i] = l;
        if (p >= 0) {
            atomicAdd(&cnt[p], 1);
            if (l != nt) atomicOr(&notfull[p], 1);
        }
    }
    __syncthreads();
    if (cnumerr && threadIdx.x < 4 && hist[threadIdx.x]) atomicAdd(&ctl->hist[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

// Exclusive scan of in[0..n) into out[0..n], out[n] = the total; one block.
// Thread t sums a contiguous chunk, the 1024 chunk sums are scanned in LDS.
template <class T>
__global__ void __launch_bounds__(kPlanScanThreads) k_plan_scan(const T* __restrict__ in, int64_t n,
                                                                int64_t* __restrict__ out)
{
    __shared__ int64_t sh[kPlanScanThreads];
    const int t = threadIdx.x;
    const int64_t chunk = (n + kPlanScanThreads - 1) / kPlanScanThreads;
    const int64_t b = t * chunk < n ? t * chunk : n, e = b + chunk < n ? b + chunk : n;
    int64_t own = 0;
    for (int64_t i = b; i < e; i++) own += (int64_t)in[i];
    sh[t] = own;
    __syncthreads();
    for (int d = 1; d < kPlanScanThreads; d <<= 1) {
        const int64_t v = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    int64_t acc = sh[t] - own;
    for (int64_t i = b; i < e; i++) {
        out[i] = acc;
        acc += (int64_t)in[i];
    }
    if (t == kPlanScanThreads - 1) out[n] = sh[t];
}

__global__ void __launch_bounds__(256) k_plan_place(const int32_t* __restrict__ pos, int64_t n, int32_t S,
                                                    const int64_t* __restrict__ start, int32_t* __restrict__ cursor,
                                                    int32_t* __restrict__ tmp_ids, PlanCtl* __restrict__ ctl)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t p = pos[i];
    if (p < 0) return;
    if (p >= S) {
        ctl->bad = 1;
        return;
    }
    const int64_t s0 = start[p], s1 = start[p + 1];
    const int64_t d = s0 + atomicAdd(&cursor[p], 1);
    if (s0 < 0 || d >= s1 || s1 > n) {
        ctl->bad = 1;
        return;
    }
    tmp_ids[d] = (int32_t)i;
}

// 8 lanes per strand: element e of the segment goes to the slot given by the
// number of smaller ids (ids are distinct), so the segment ends in input
// order.  Also lays the payload views out in that order (the "local" read
// list pair indices refer to).
__global__ void __launch_bounds__(256) k_plan_sort(const int32_t* __restrict__ tmp_ids,
                                                   const int64_t* __restrict__ start, int32_t S, int64_t n,
                                                   const int64_t* __restrict__ poff, const int32_t* __restrict__ plen,
                                                   int32_t* __restrict__ ids, int64_t* __restrict__ soff,
                                                   int32_t* __restrict__ slen, PlanCtl* __restrict__ ctl)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t s = g >> 3;
    const int sub = (int)(g & 7);
    if (s >= S) return;
    const int64_t s0 = start[s], k = start[s + 1] - s0;
    if (s0 < 0 || k < 0 || s0 + k > n) {
        ctl->bad = 1;
        return;
    }
    for (int64_t e = sub; e < k; e += 8) {
        const int32_t v = tmp_ids[s0 + e];
        if (v < 0 || v >= n) {
            ctl->bad = 1;
            continue;
        }
        int64_t rank = 0;
        for (int64_t j = 0; j < k; j++) rank += tmp_ids[s0 + j] < v ? 1 : 0;
        ids[s0 + rank] = v;
        soff[s0 + rank] = poff[v];
        slen[s0 + rank] = plen[v];
    }
}

// One strand per thread.  A ragged strand keeps kind 0 until its candidates
// are known; npairs > 0 marks it.
__global__ void __launch_bounds__(256) k_plan_classify(const int64_t* __restrict__ start, int32_t S, int64_t n,
                                                       const int32_t* __restrict__ notfull,
                                                       const int32_t* __restrict__ ids, const int32_t* __restrict__ slen,
                                                       const int32_t* __restrict__ quals, int32_t nt,
                                                       int32_t* __restrict__ kind, int64_t* __restrict__ npairs,
                                                       int64_t* __restrict__ rowcnt, PlanCtl* __restrict__ ctl)
{
    const int32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const int64_t s0 = start[s], k = start[s + 1] - s0;
    int32_t kd = 0;
    int64_t np = 0, rc = 0;
    if (s0 < 0 || k < 0 || s0 + k > n) {
        ctl->bad = 1;
    } else if (k == 1) {
        const int32_t l = slen[s0], r = ids[s0];
        kd = l < nt ? 2 : 1;
        rc = 1;
        if (l == 0 && r >= 0 && r < n && quals[r] > kQHigh) atomicMin(&ctl->empty_strand, s);
    } else if (k > 1 && !notfull[s]) {
        kd = 1;
        rc = k;
    } else if (k > 1) {
        np = k * (k - 1) / 2;
        for (int64_t q = s0; q < s0 + k; q++) {
            const int32_t l = slen[q];
            atomicMax(&ctl->max_ragged_len, l);
            if (l > kPlanMaxLen) atomicMin(&ctl->long_read, ids[q]);
        }
    }
    kind[s] = kd;
    npairs[s] = np;
    rowcnt[s] = rc;
}

// Largest s in [0, S) with ptr[s] <= v, for a non-decreasing ptr[0..S] with
// ptr[0] <= v < ptr[S].
__device__ __forceinline__ int32_t plan_segment_of(const int64_t* __restrict__ ptr, int32_t S, int64_t v)
{
    int32_t lo = 0, hi = S;  // first index in [0, S] with ptr > v
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

__global__ void __launch_bounds__(256) k_plan_pairs(const int64_t* __restrict__ pair_start,
                                                    const int64_t* __restrict__ start, int32_t S, int64_t n_valid,
                                                    int64_t P, int32_t* __restrict__ pa, int32_t* __restrict__ pb,
                                                    PlanCtl* __restrict__ ctl)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    int32_t a = 0, b = 0;  // a defined pair whatever the checks say: position 0 against itself
    const int32_t s = plan_segment_of(pair_start, S, p);
    bool ok = s >= 0 && s < S;
    if (ok) {
        const int64_t s0 = start[s], k = start[s + 1] - s0;
        int64_t t = p - pair_start[s];
        ok = s0 >= 0 && k >= 2 && s0 + k <= n_valid && t >= 0 && t < k * (k - 1) / 2;
        if (ok) {
            int64_t i = 0;  // row i of the strict upper triangle holds k - 1 - i pairs
            while (t >= k - 1 - i) {
                t -= k - 1 - i;
                i++;
            }
            a = (int32_t)(s0 + i);
            b = (int32_t)(s0 + i + 1 + t);
        }
    }
    if (!ok) ctl->bad = 1;
    pa[p] = a;
    pb[p] = b;
}

__global__ void __launch_bounds__(256) k_plan_close(const int32_t* __restrict__ pa, const int32_t* __restrict__ pb,
                                                    const int32_t* __restrict__ dist, int64_t P, int64_t n_valid,
                                                    uint8_t* __restrict__ close, PlanCtl* __restrict__ ctl)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || dist[p] >= plan::kEdThreshold) return;
    const int32_t a = pa[p], b = pb[p];
    if (a < 0 || a >= n_valid || b < 0 || b >= n_valid) {
        ctl->bad = 1;
        return;
    }
    close[a] = 1;  // the same value from every writer
    close[b] = 1;
}

__global__ void __launch_bounds__(256) k_plan_cand_count(const int64_t* __restrict__ start, int32_t S, int64_t n_valid,
                                                         const int64_t* __restrict__ npairs,
                                                         const uint8_t* __restrict__ close,
                                                         int64_t* __restrict__ ncand, int64_t* __restrict__ rowcnt)
{
    const int32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    int64_t nc = 0;
    if (npairs[s] > 0) {
        const int64_t s0 = start[s], s1 = start[s + 1];
        if (s0 >= 0 && s1 <= n_valid)
            for (int64_t q = s0; q < s1; q++) nc += close[q] ? 1 : 0;
        rowcnt[s] = nc;
    }
    ncand[s] = nc;
}

__global__ void __launch_bounds__(256) k_plan_cand_fill(const int64_t* __restrict__ start, int32_t S, int64_t n_valid,
                                                        const int64_t* __restrict__ cand_ptr, int64_t C,
                                                        const uint8_t* __restrict__ close,
                                                        const int32_t* __restrict__ ids, int32_t* __restrict__ cand_ids,
                                                        PlanCtl* __restrict__ ctl)
{
    const int32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    int64_t c = cand_ptr[s];
    const int64_t c1 = cand_ptr[s + 1];
    if (c1 == c) return;
    const int64_t s0 = start[s], s1 = start[s + 1];
    if (c < 0 || c1 > C || s0 < 0 || s1 > n_valid) {
        ctl->bad = 1;
        return;
    }
    for (int64_t q = s0; q < s1 && c < c1; q++)
        if (close[q]) cand_ids[c++] = ids[q];
}

// One wave per row (4 rows per block at a time, grid-stride): the lanes find
// the row's strand in row_ptr, then write the payload_nt bytes together --
// dwords when payload_nt is a multiple of 4 (136: 34 lanes, one 136-byte
// contiguous piece), bytes otherwise.  Sources: the uploaded aligned rows
// (strands with candidates; lane 0 of the strand's first row also sets the
// kind from the aligned width), the read's first payload_nt bytes (plain
// kind 1), the read's last byte (kind 2).
__global__ void __launch_bounds__(256) k_plan_rows(
    const int64_t* __restrict__ row_ptr, int32_t S, int64_t R, const int64_t* __restrict__ start, int64_t n_valid,
    int64_t n, const int64_t* __restrict__ cand_ptr, int64_t C, const int32_t* __restrict__ cand_ids,
    const uint8_t* __restrict__ arows, const int32_t* __restrict__ width, const uint8_t* __restrict__ seqs,
    const int64_t* __restrict__ soff, const int32_t* __restrict__ slen, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ quals, int32_t nt, int32_t* __restrict__ kind, uint8_t* __restrict__ rows,
    int32_t* __restrict__ row_q, PlanCtl* __restrict__ ctl)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < R; r += n_waves) {
        const int32_t s = plan_segment_of(row_ptr, S, r);
        if (s < 0 || s >= S) {
            ctl->bad = 1;
            continue;
        }
        const int64_t k = r - row_ptr[s], c0 = cand_ptr[s], nc = cand_ptr[s + 1] - c0;
        const uint8_t* src = nullptr;  // bytes [0, have) come from src, the rest are '-'
        int32_t have = 0, q = 0;
        if (nc > 0) {
            const int64_t c = c0 + k;
            const int32_t id = (c >= 0 && c < C) ? cand_ids[c] : -1;
            if (id < 0 || id >= n) {
                ctl->bad = 1;
                continue;
            }
            src = arows + (size_t)c * (size_t)nt;
            have = nt;
            q = quals[id];
            if (k == 0 && lane == 0) kind[s] = width[s] == nt ? 1 : 3;
        } else {
            const int64_t p = start[s] + k;
            const int32_t id = (p >= 0 && p < n_valid) ? ids[p] : -1;
            if (id < 0 || id >= n) {
                ctl->bad = 1;
                continue;
            }
            q = quals[id];
            const int32_t l = slen[p];
            if (kind[s] == 1) {
                src = seqs + soff[p];
                have = l < nt ? l : nt;
            } else if (l > 0) {  // kind 2: the last byte
                src = seqs + soff[p] + (l - 1);
                have = 1;
            }
        }
        uint8_t* dst = rows + (size_t)r * (size_t)nt;
        if ((nt & 3) == 0) {
            for (int32_t j = lane * 4; j < nt; j += 256) {
                uint32_t v = 0;
#pragma unroll
                for (int c = 0; c < 4; c++) v |= (uint32_t)(j + c < have ? src[j + c] : star::kGap) << (8 * c);
                *reinterpret_cast<uint32_t*>(dst + j) = v;
            }
        } else {
            for (int32_t j = lane; j < nt; j += 64) dst[j] = j < have ? src[j] : star::kGap;
        }
        if (lane == 0) row_q[r] = q;
    }
}

unsigned plan_blocks(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

// What stays on the device after the planner, for the fused call.
struct PlanDev {
    dev_ptr<int32_t> kind, row_q;
    dev_ptr<int64_t> row_ptr;
    dev_ptr<uint8_t> rows;
    int64_t R = 0;
};

// Reads that are on the device already (the sequencing channel's, DESIGN.md
// sec. 8.9), in place of the four uploads: seqs holds seq_bytes bytes, the
// arrays n_reads entries.  `bad` (may be null) is the producer's flag word.
struct PlanSrc {
    const uint8_t* seqs;
    const int64_t* offsets;
    const int32_t* lengths;
    const int32_t* quals;
    int64_t seq_bytes;
    const int32_t* bad;
};

// The check of device-resident reads that plan::check_args makes of host ones:
// every read inside seqs.  Also folds the producer's flag word in.
__global__ void __launch_bounds__(256) k_plan_check_src(const int64_t* __restrict__ off, const int32_t* __restrict__ len,
                                                        int64_t n, int64_t seq_bytes, const int32_t* __restrict__ src_bad,
                                                        PlanCtl* __restrict__ ctl)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && src_bad && *src_bad) ctl->bad = 1;
    if (i >= n) return;
    const int64_t o = off[i], l = len[i];
    if (l < 0 || o < 0 || o > seq_bytes || l > seq_bytes - o) ctl->bad = 1;
}

// Candidate c of device-resident reads: its payload length (the read's bytes
// from `skip` on), 0 and the flag when the read id or the length fails its check.
__global__ void __launch_bounds__(256) k_plan_cand_len(const int32_t* __restrict__ cand_ids, int64_t C, int64_t n,
                                                       const int32_t* __restrict__ len, int32_t skip,
                                                       int32_t* __restrict__ clen, PlanCtl* __restrict__ ctl)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int32_t id = cand_ids[c];
    int32_t l = 0;
    if (id < 0 || id >= n || len[id] < skip || len[id] - skip > kPlanMaxLen) ctl->bad = 1;
    else l = len[id] - skip;
    clen[c] = l;
}

// One wave per candidate (4 per block): its payload bytes, packed at coff[c]
// of a buffer of T = coff[C] bytes.  The source range was checked by
// k_plan_check_src, the id and length by k_plan_cand_len (clen is its output);
// both are checked again here, with the destination range.
__global__ void __launch_bounds__(256) k_plan_cand_gather(const int32_t* __restrict__ cand_ids, int64_t C, int64_t n,
                                                          const uint8_t* __restrict__ seqs,
                                                          const int64_t* __restrict__ off, int64_t seq_bytes,
                                                          int32_t skip, const int64_t* __restrict__ coff,
                                                          const int32_t* __restrict__ clen, int64_t T,
                                                          uint8_t* __restrict__ out, PlanCtl* __restrict__ ctl)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    const int32_t id = cand_ids[c];
    if (id < 0 || id >= n) {
        if (lane == 0) ctl->bad = 1;
        return;
    }
    const int64_t o = off[id], d = coff[c], l = clen[c];
    if (l < 0 || o < 0 || o > seq_bytes - skip - l || d < 0 || d > T - l) {
        if (lane == 0) ctl->bad = 1;
        return;
    }
    for (int64_t j = lane; j < l; j += 64) out[d + j] = seqs[o + skip + j];
}

// The device planner.  Host outputs of `a` that are null are skipped (the
// fused call passes none but kind / stats).  With `src` the reads are the
// device-resident ones (a.seqs / offsets / lengths / quals are not read): the
// aligner's merge, the one host consumer of read bytes, gets the candidates
// packed by k_plan_cand_gather and copied down, nothing else crosses.
int plan_device(const std::string& who, const plan::Args& a, bool host_outputs, int32_t device,
                int64_t workspace_bytes, PlanDev* pd, const PlanSrc* src = nullptr)
{
    int64_t total = 0;
    {
        plan::Args host = a;
        if (src && host.n_reads > 0) host.n_reads = 0;  // no host reads to check
        const std::string err = plan::check_args(host, &total, host_outputs);
        if (!err.empty()) {
            set_error(who + ": " + err);
            return LDPC_ERR_ARG;
        }
    }
    if (workspace_bytes < 0) {
        set_error(who + ": negative workspace_bytes");
        return LDPC_ERR_ARG;
    }
    const int64_t n = a.n_reads;
    const int32_t S = a.n_strands, nt = a.payload_nt;
    if (n > INT32_MAX - 1024) {
        set_error(who + ": too many reads for one call");
        return LDPC_ERR_UNSUPPORTED;
    }
    if (a.stats) std::fill(a.stats, a.stats + plan::kNumStats, 0);
    if (S == 0) {
        if (host_outputs) a.row_ptr[0] = 0;
        pd->R = 0;
        return LDPC_OK;
    }
    if (int rc = select_device(who.c_str(), device)) return rc;

    const size_t nn = (size_t)std::max<int64_t>(n, 1), SS = (size_t)S;
    dev_ptr<uint8_t> dseq;
    dev_ptr<int64_t> doff, dpoff, dstart, dsoff, dnp, drc, dpstart, dncand, dcptr;
    dev_ptr<int32_t> dlen, dq, dstr, div, dne, dpos, dplen, dcnt, dtmp, dids, dslen;
    dev_ptr<PlanCtl> dctl;
    int rc;
    if (!src) {
        if ((rc = upload(dseq, a.seqs, (size_t)total))) return rc;
        if ((rc = upload(doff, a.offsets, (size_t)n))) return rc;
        if ((rc = upload(dlen, a.lengths, (size_t)n))) return rc;
        if ((rc = upload(dq, a.quals, (size_t)n))) return rc;
    }
    const uint8_t* d_seq = src ? src->seqs : dseq.get();
    const int64_t* d_off = src ? src->offsets : doff.get();
    const int32_t* d_len = src ? src->lengths : dlen.get();
    const int32_t* d_q = src ? src->quals : dq.get();
    if ((rc = upload(dstr, a.strands, SS))) return rc;
    PlanCtl ctl{};
    ctl.long_read = INT32_MAX;
    ctl.empty_strand = INT32_MAX;
    if ((rc = upload(dctl, &ctl, 1))) return rc;
    if (src) {  // before any kernel follows an offset
        if (src->seq_bytes < 0 || (n > 0 && (!src->seqs || !src->offsets || !src->lengths || !src->quals))) {
            set_error(who + ": bad device-resident reads");
            return LDPC_ERR_ARG;
        }
        int32_t bad = 0;
        hipLaunchKernelGGL(k_plan_check_src, dim3(plan_blocks(n, 256)), dim3(256), 0, 0, d_off, d_len, n,
                           src->seq_bytes, src->bad, dctl.get());
        LDPC_HIP(hipGetLastError());
        LDPC_HIP(hipMemcpy(&bad, &dctl.get()->bad, sizeof bad, hipMemcpyDeviceToHost));
        if (bad) {
            set_error(who + ": the device-resident reads failed their range check");
            return LDPC_ERR_DEVICE;
        }
    }
    if (a.index_vals) {
        if ((rc = upload(div, a.index_vals, (size_t)n))) return rc;
    } else {
        if ((rc = dev_alloc(div, nn))) return rc;
        if ((rc = dev_alloc(dne, nn))) return rc;
        if (n > 0) {
            hipLaunchKernelGGL(k_rs_index_decode, dim3(plan_blocks(n, 256)), dim3(256), 0, 0, d_seq,
                               d_off, d_len, n, div.get(), dne.get());
            LDPC_HIP(hipGetLastError());
        }
    }
    if ((rc = dev_alloc(dpos, nn))) return rc;
    if ((rc = dev_alloc(dpoff, nn))) return rc;
    if ((rc = dev_alloc(dplen, nn))) return rc;
    if ((rc = dev_alloc(dtmp, nn))) return rc;
    if ((rc = dev_alloc(dids, nn))) return rc;
    if ((rc = dev_alloc(dsoff, nn))) return rc;
    if ((rc = dev_alloc(dslen, nn))) return rc;
    if ((rc = dev_alloc(dcnt, SS * 3))) return rc;  // counts, not-full flags, scatter cursors
    LDPC_HIP(hipMemset(dcnt.get(), 0, sizeof(int32_t) * SS * 3));
    int32_t* d_cnt = dcnt.get();
    int32_t* d_notfull = d_cnt + SS;
    int32_t* d_cursor = d_cnt + 2 * SS;
    if ((rc = dev_alloc(dstart, (SS + 1)))) return rc;
    if ((rc = dev_alloc(dpstart, (SS + 1)))) return rc;
    if ((rc = dev_alloc(dcptr, (SS + 1)))) return rc;
    if ((rc = dev_alloc(pd->row_ptr, (SS + 1)))) return rc;
    if ((rc = dev_alloc(dnp, SS))) return rc;
    if ((rc = dev_alloc(drc, SS))) return rc;
    if ((rc = dev_alloc(dncand, SS))) return rc;
    if ((rc = dev_alloc(pd->kind, SS))) return rc;
    PlanCtl* d_ctl = dctl.get();
    const dim3 b256(256), per_read(plan_blocks(n, 256)), per_strand(plan_blocks(S, 256));

    if (n > 0) {
        hipLaunchKernelGGL(k_plan_locate, per_read, b256, 0, 0, div.get(),
                           a.index_vals ? nullptr : dne.get(), d_off, d_len, n,
                           dstr.get(), S, nt, dpos.get(), dpoff.get(), dplen.get(),
                           d_cnt, d_notfull, d_ctl);
        LDPC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_plan_scan<int32_t>, dim3(1), dim3(kPlanScanThreads), 0, 0, d_cnt, (int64_t)S,
                       dstart.get());
    LDPC_HIP(hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(k_plan_place, per_read, b256, 0, 0, dpos.get(), n, S, dstart.get(), d_cursor,
                           dtmp.get(), d_ctl);
        LDPC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_plan_sort, dim3(plan_blocks((int64_t)S * 8, 256)), b256, 0, 0, dtmp.get(),
                       dstart.get(), S, n, dpoff.get(), dplen.get(), dids.get(),
                       dsoff.get(), dslen.get(), d_ctl);
    LDPC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_plan_classify, per_strand, b256, 0, 0, dstart.get(), S, n, d_notfull,
                       dids.get(), dslen.get(), d_q, nt, pd->kind.get(),
                       dnp.get(), drc.get(), d_ctl);
    LDPC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_plan_scan<int64_t>, dim3(1), dim3(kPlanScanThreads), 0, 0, dnp.get(), (int64_t)S,
                       dpstart.get());
    LDPC_HIP(hipGetLastError());

    int64_t n_valid = 0, P = 0;
    LDPC_HIP(hipMemcpy(&ctl, dctl.get(), sizeof ctl, hipMemcpyDeviceToHost));
    LDPC_HIP(hipMemcpy(&n_valid, dstart.get() + S, sizeof n_valid, hipMemcpyDeviceToHost));
    LDPC_HIP(hipMemcpy(&P, dpstart.get() + S, sizeof P, hipMemcpyDeviceToHost));
    if (ctl.bad || n_valid < 0 || n_valid > n || P < 0) {
        set_error(who + ": the device plan is inconsistent");
        return LDPC_ERR_DEVICE;
    }
    if (ctl.empty_strand != INT32_MAX) {
        set_error(who + ": empty read on strand " + std::to_string(ctl.empty_strand) +
                  " with quality > 63 (the reference indexes its last bit)");
        return LDPC_ERR_ARG;
    }
    if (ctl.long_read != INT32_MAX) {
        set_error(who + ": read " + std::to_string(ctl.long_read) + " on a ragged strand is longer than " +
                  std::to_string(kPlanMaxLen) + " bytes (ldpc_dna_plan_host has no such limit)");
        return LDPC_ERR_ARG;
    }
    if (P > (int64_t)INT32_MAX * 64) {
        set_error(who + ": too many distance pairs for one call");
        return LDPC_ERR_UNSUPPORTED;
    }

    // distances, close reads, candidates
    dev_ptr<int32_t> dpa, dpb, ddist, dcand, dwidth;
    dev_ptr<uint8_t> dclose, darows;
    if ((rc = dev_alloc(dclose, (size_t)std::max<int64_t>(n_valid, 16)))) return rc;
    LDPC_HIP(hipMemset(dclose.get(), 0, (size_t)std::max<int64_t>(n_valid, 16)));
    if (P > 0) {
        if ((rc = dev_alloc(dpa, (size_t)P))) return rc;
        if ((rc = dev_alloc(dpb, (size_t)P))) return rc;
        if ((rc = dev_alloc(ddist, (size_t)P))) return rc;
        hipLaunchKernelGGL(k_plan_pairs, dim3(plan_blocks(P, 256)), b256, 0, 0, dpstart.get(),
                           dstart.get(), S, n_valid, P, dpa.get(), dpb.get(), d_ctl);
        LDPC_HIP(hipGetLastError());
        if ((rc = launch_edit_distance(d_seq, dsoff.get(), dslen.get(), dpa.get(),
                                       dpb.get(), P, std::max(ctl.max_ragged_len, 0), ddist.get())))
            return rc;
        hipLaunchKernelGGL(k_plan_close, dim3(plan_blocks(P, 256)), b256, 0, 0, dpa.get(), dpb.get(),
                           ddist.get(), P, n_valid, dclose.get(), d_ctl);
        LDPC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_plan_cand_count, per_strand, b256, 0, 0, dstart.get(), S, n_valid, dnp.get(),
                       dclose.get(), dncand.get(), drc.get());
    LDPC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_plan_scan<int64_t>, dim3(1), dim3(kPlanScanThreads), 0, 0, dncand.get(), (int64_t)S,
                       dcptr.get());
    LDPC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_plan_scan<int64_t>, dim3(1), dim3(kPlanScanThreads), 0, 0, drc.get(), (int64_t)S,
                       pd->row_ptr.get());
    LDPC_HIP(hipGetLastError());
    int64_t C = 0, R = 0;
    LDPC_HIP(hipMemcpy(&C, dcptr.get() + S, sizeof C, hipMemcpyDeviceToHost));
    LDPC_HIP(hipMemcpy(&R, pd->row_ptr.get() + S, sizeof R, hipMemcpyDeviceToHost));
    if (C < 0 || C > n_valid || R < 0 || R > n_valid) {
        set_error(who + ": the device plan is inconsistent");
        return LDPC_ERR_DEVICE;
    }

    // the aligner: group s = the candidates of strand s (empty for most strands)
    int64_t n_aligned = 0;
    std::vector<int32_t> width((size_t)S, 0);
    if ((rc = dev_alloc(dcand, (size_t)C))) return rc;
    if (C > 0) {
        if (!a.align) {
            set_error(who + ": ragged strands need an aligner (align = 0)");
            return LDPC_ERR_ARG;
        }
        hipLaunchKernelGGL(k_plan_cand_fill, per_strand, b256, 0, 0, dstart.get(), S, n_valid,
                           dcptr.get(), C, dclose.get(), dids.get(), dcand.get(), d_ctl);
        LDPC_HIP(hipGetLastError());
        std::vector<int64_t> cptr((size_t)S + 1), coff((size_t)C), out_ptr((size_t)S + 1);
        std::vector<int32_t> cand((size_t)C), clen((size_t)C), centre((size_t)S);
        std::vector<uint8_t> out;
        LDPC_HIP(hipMemcpy(cptr.data(), dcptr.get(), sizeof(int64_t) * (SS + 1), hipMemcpyDeviceToHost));
        LDPC_HIP(hipMemcpy(cand.data(), dcand.get(), sizeof(int32_t) * (size_t)C, hipMemcpyDeviceToHost));
        const int64_t skip = a.index_vals ? 0 : rs::kPrefixNt;
        if (cptr[0] != 0 || cptr[(size_t)S] != C) {
            set_error(who + ": the device plan is inconsistent");
            return LDPC_ERR_DEVICE;
        }
        std::vector<uint8_t> cseq;     // device source: the candidates' payloads, packed
        dev_ptr<uint8_t> dcseq;
        const uint8_t* star_seqs = a.seqs;
        const uint8_t* d_star_seqs = d_seq;
        if (!src) {
            for (int64_t c = 0; c < C; c++) {
                const int32_t r = cand[(size_t)c];
                if (r < 0 || r >= n || a.lengths[r] < skip) {
                    set_error(who + ": the device plan is inconsistent");
                    return LDPC_ERR_DEVICE;
                }
                coff[(size_t)c] = a.offsets[r] + skip;
                clen[(size_t)c] = (int32_t)(a.lengths[r] - skip);
            }
        } else {
            dev_ptr<int32_t> dclen;
            dev_ptr<int64_t> dcoff;
            int64_t T = 0;
            if ((rc = dev_alloc(dclen, (size_t)C)) || (rc = dev_alloc(dcoff, (size_t)C + 1))) return rc;
            hipLaunchKernelGGL(k_plan_cand_len, dim3(plan_blocks(C, 256)), b256, 0, 0, dcand.get(), C, n, d_len,
                               (int32_t)skip, dclen.get(), d_ctl);
            LDPC_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_plan_scan<int32_t>, dim3(1), dim3(kPlanScanThreads), 0, 0, dclen.get(), C,
                               dcoff.get());
            LDPC_HIP(hipGetLastError());
            LDPC_HIP(hipMemcpy(&T, dcoff.get() + C, sizeof T, hipMemcpyDeviceToHost));
            if (T < 0 || T > C * (int64_t)kPlanMaxLen) {
                set_error(who + ": the device plan is inconsistent");
                return LDPC_ERR_DEVICE;
            }
            if ((rc = dev_alloc(dcseq, (size_t)T))) return rc;
            hipLaunchKernelGGL(k_plan_cand_gather, dim3(plan_blocks(C, 4)), b256, 0, 0, dcand.get(), C, n, d_seq,
                               d_off, src->seq_bytes, (int32_t)skip, dcoff.get(), dclen.get(), T, dcseq.get(), d_ctl);
            LDPC_HIP(hipGetLastError());
            cseq.resize((size_t)T);
            LDPC_HIP(hipMemcpy(coff.data(), dcoff.get(), sizeof(int64_t) * (size_t)C, hipMemcpyDeviceToHost));
            LDPC_HIP(hipMemcpy(clen.data(), dclen.get(), sizeof(int32_t) * (size_t)C, hipMemcpyDeviceToHost));
            if (T > 0) LDPC_HIP(hipMemcpy(cseq.data(), dcseq.get(), (size_t)T, hipMemcpyDeviceToHost));
            LDPC_HIP(hipMemcpy(&ctl, dctl.get(), sizeof ctl, hipMemcpyDeviceToHost));
            if (ctl.bad) {
                set_error(who + ": the device plan is inconsistent");
                return LDPC_ERR_DEVICE;
            }
            star_seqs = cseq.data();
            d_star_seqs = dcseq.get();
        }
        StarCall sc{star_seqs, coff.data(), clen.data(), C, cptr.data(), (int64_t)S, centre.data(), width.data(),
                    out_ptr.data(), nullptr, 0, nullptr, nullptr};
        sc.out_vec = &out;
        if ((rc = star_align_device(sc, device, workspace_bytes, nullptr, who, d_star_seqs))) return rc;
        // the rows to upload: the aligned row (width == payload_nt), else its last byte in byte 0
        std::vector<uint8_t> arows((size_t)C * (size_t)nt, star::kGap);
        for (int32_t s = 0; s < S; s++) {
            const int64_t c0 = cptr[(size_t)s], nc = cptr[(size_t)s + 1] - c0, w = width[(size_t)s];
            if (nc == 0) continue;
            n_aligned++;
            for (int64_t q = 0; q < nc; q++) {
                const uint8_t* row = out.data() + out_ptr[(size_t)s] + q * w;
                uint8_t* dst = arows.data() + (size_t)(c0 + q) * (size_t)nt;
                if (w == nt) std::copy(row, row + nt, dst);
                else if (w > 0) dst[0] = row[w - 1];
            }
        }
        if ((rc = upload(darows, arows.data(), arows.size()))) return rc;
    }
    if ((rc = upload(dwidth, width.data(), SS))) return rc;

    if ((rc = dev_alloc(pd->rows, (size_t)R * (size_t)nt))) return rc;
    if ((rc = dev_alloc(pd->row_q, (size_t)R))) return rc;
    if (R > 0) {
        hipLaunchKernelGGL(k_plan_rows, dim3((unsigned)std::min<int64_t>((R + 3) / 4, 2048)), b256, 0, 0,
                           pd->row_ptr.get(), S, R, dstart.get(), n_valid, n, dcptr.get(), C,
                           dcand.get(), darows.get(), dwidth.get(), d_seq,
                           dsoff.get(), dslen.get(), dids.get(), d_q, nt,
                           pd->kind.get(), pd->rows.get(), pd->row_q.get(), d_ctl);
        LDPC_HIP(hipGetLastError());
    }
    LDPC_HIP(hipMemcpy(&ctl, dctl.get(), sizeof ctl, hipMemcpyDeviceToHost));
    if (ctl.bad) {
        set_error(who + ": the device plan is inconsistent");
        return LDPC_ERR_DEVICE;
    }
    pd->R = R;
    if (a.kind) LDPC_HIP(hipMemcpy(a.kind, pd->kind.get(), sizeof(int32_t) * SS, hipMemcpyDeviceToHost));
    if (host_outputs) {
        LDPC_HIP(hipMemcpy(a.row_ptr, pd->row_ptr.get(), sizeof(int64_t) * (SS + 1), hipMemcpyDeviceToHost));
        if (R > 0) {
            LDPC_HIP(hipMemcpy(a.rows, pd->rows.get(), (size_t)R * (size_t)nt, hipMemcpyDeviceToHost));
            LDPC_HIP(hipMemcpy(a.row_q, pd->row_q.get(), sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost));
        }
    }
    if (a.stats) {
        a.stats[plan::kStatValid] = n_valid;
        a.stats[plan::kStatPairs] = P;
        a.stats[plan::kStatAligned] = n_aligned;
        a.stats[plan::kStatAlignPairs] = C - n_aligned;
        a.stats[plan::kStatRows] = R;
        for (int k = 0; k < 4; k++) a.stats[plan::kStatCnumerr + k] = (int64_t)ctl.hist[k];
    }
    return LDPC_OK;
}

}  // namespace
}  // namespace ldpc
