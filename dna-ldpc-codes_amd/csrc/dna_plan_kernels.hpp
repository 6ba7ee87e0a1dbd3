// dna_plan_kernels.hpp -- the read planner on the GPU:
// the kernels and the host driver of ldpc_dna_plan / ldpc_dna_reads_llr,
// plan_device: a list of stages (plan_source .. plan_outputs, after the
// kernels) over one work struct, PlanWork.
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
//                      and the rows it leaves in the plan are plan::aligned_row's
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

// What plan_device keeps from stage to stage: the call, the device buffers
// that live to its end (PlanDev's outlive it) and the control words read back.
struct PlanWork {
    const std::string& who;
    const plan::Args& a;
    const PlanSrc* src;
    PlanDev* pd;
    int32_t device;
    int64_t workspace_bytes;
    int64_t n;  // reads
    int32_t S, nt;
    dim3 per_read, per_strand;
    // the reads: uploads (own_*) or the PlanSrc's
    dev_ptr<uint8_t> own_seq;
    dev_ptr<int64_t> own_off;
    dev_ptr<int32_t> own_len, own_q;
    const uint8_t* seq = nullptr;
    const int64_t* off = nullptr;
    const int32_t* len = nullptr;
    const int32_t* q = nullptr;
    dev_ptr<int32_t> strands, index, cnumerr;
    dev_ptr<PlanCtl> dctl;
    // per read: strand position and payload view; then the same in segment order
    dev_ptr<int32_t> pos, plen, tmp, ids, slen;
    dev_ptr<int64_t> poff, soff;
    // per strand: counts, not-full flags, scatter cursors ([3][S]); segment, pair and candidate starts
    dev_ptr<int32_t> cnt;
    dev_ptr<int64_t> start, pstart, cptr, npairs, rowcnt, ncand;
    dev_ptr<uint8_t> close, arows;
    dev_ptr<int32_t> cand, width;
    PlanCtl ctl{};
    int64_t n_valid = 0, P = 0, C = 0, R = 0, n_aligned = 0;
    std::vector<int32_t> h_width;  // aligned width per strand

    int32_t* notfull() const { return cnt.get() + S; }
    int32_t* cursor() const { return cnt.get() + 2 * (size_t)S; }
    int inconsistent() const
    {
        set_error(who + ": the device plan is inconsistent");
        return LDPC_ERR_DEVICE;
    }
};

template <class T>
int plan_scan(const T* in, int64_t n, int64_t* out)
{
    return launch(k_plan_scan<T>, dim3(1), dim3(kPlanScanThreads), 0, nullptr, in, n, out);
}

// The reads on the device (uploads, or the PlanSrc after its range check), the
// strand list and the control block.
int plan_source(PlanWork& w, int64_t total)
{
    const plan::Args& a = w.a;
    const PlanSrc* src = w.src;
    int rc;
    if (!src && ((rc = upload(w.own_seq, a.seqs, (size_t)total)) || (rc = upload(w.own_off, a.offsets, (size_t)w.n)) ||
                 (rc = upload(w.own_len, a.lengths, (size_t)w.n)) || (rc = upload(w.own_q, a.quals, (size_t)w.n))))
        return rc;
    w.seq = src ? src->seqs : w.own_seq.get();
    w.off = src ? src->offsets : w.own_off.get();
    w.len = src ? src->lengths : w.own_len.get();
    w.q = src ? src->quals : w.own_q.get();
    w.ctl.long_read = INT32_MAX;
    w.ctl.empty_strand = INT32_MAX;
    if ((rc = upload(w.strands, a.strands, (size_t)w.S)) || (rc = upload(w.dctl, &w.ctl, 1))) return rc;
    if (!src) return LDPC_OK;
    // before any kernel follows an offset
    if (src->seq_bytes < 0 || (w.n > 0 && (!src->seqs || !src->offsets || !src->lengths || !src->quals))) {
        set_error(w.who + ": bad device-resident reads");
        return LDPC_ERR_ARG;
    }
    int32_t bad = 0;
    if ((rc = launch(k_plan_check_src, w.per_read, dim3(256), 0, nullptr, w.off, w.len, w.n, src->seq_bytes, src->bad,
                     w.dctl.get())) ||
        (rc = download(&bad, &w.dctl.get()->bad, 1)))
        return rc;
    if (bad) {
        set_error(w.who + ": the device-resident reads failed their range check");
        return LDPC_ERR_DEVICE;
    }
    return LDPC_OK;
}

// Index values (the caller's, or k_rs_index_decode's), then locate, scan,
// place and sort: strand s holds ids[start[s] .. start[s + 1]) in input order.
int plan_segments(PlanWork& w)
{
    const plan::Args& a = w.a;
    const int64_t n = w.n;
    const int32_t S = w.S;
    const size_t nn = (size_t)std::max<int64_t>(n, 1), SS = (size_t)S;
    const dim3 b256(256);
    int rc;
    if (a.index_vals) {
        if ((rc = upload(w.index, a.index_vals, (size_t)n))) return rc;
    } else if ((rc = dev_alloc(w.index, nn)) || (rc = dev_alloc(w.cnumerr, nn)) ||
               (n > 0 && (rc = launch(k_rs_index_decode, w.per_read, b256, 0, nullptr, w.seq, w.off, w.len, n,
                                      w.index.get(), w.cnumerr.get())))) {
        return rc;
    }
    if ((rc = dev_alloc(w.pos, nn)) || (rc = dev_alloc(w.poff, nn)) || (rc = dev_alloc(w.plen, nn)) ||
        (rc = dev_alloc(w.tmp, nn)) || (rc = dev_alloc(w.ids, nn)) || (rc = dev_alloc(w.soff, nn)) ||
        (rc = dev_alloc(w.slen, nn)) || (rc = dev_alloc(w.cnt, SS * 3)))
        return rc;
    LDPC_HIP(hipMemset(w.cnt.get(), 0, sizeof(int32_t) * SS * 3));
    if ((rc = dev_alloc(w.start, SS + 1)) || (rc = dev_alloc(w.pstart, SS + 1)) || (rc = dev_alloc(w.cptr, SS + 1)) ||
        (rc = dev_alloc(w.pd->row_ptr, SS + 1)) || (rc = dev_alloc(w.npairs, SS)) || (rc = dev_alloc(w.rowcnt, SS)) ||
        (rc = dev_alloc(w.ncand, SS)) || (rc = dev_alloc(w.pd->kind, SS)))
        return rc;
    if (n > 0 && (rc = launch(k_plan_locate, w.per_read, b256, 0, nullptr, w.index.get(), w.cnumerr.get(), w.off, w.len, n,
                              w.strands.get(), S, w.nt, w.pos.get(), w.poff.get(), w.plen.get(), w.cnt.get(),
                              w.notfull(), w.dctl.get())))
        return rc;
    if ((rc = plan_scan(w.cnt.get(), (int64_t)S, w.start.get()))) return rc;
    if (n > 0 && (rc = launch(k_plan_place, w.per_read, b256, 0, nullptr, w.pos.get(), n, S, w.start.get(), w.cursor(),
                              w.tmp.get(), w.dctl.get())))
        return rc;
    return launch(k_plan_sort, dim3(plan_blocks((int64_t)S * 8, 256)), b256, 0, nullptr, w.tmp.get(), w.start.get(), S, n,
                  w.poff.get(), w.plen.get(), w.ids.get(), w.soff.get(), w.slen.get(), w.dctl.get());
}

// Kinds, pair counts and provisional row counts; then the first look at the
// control words: n_valid, P and what the kernels flagged.
int plan_classify(PlanWork& w)
{
    const std::string& who = w.who;
    const int32_t S = w.S;
    int rc;
    if ((rc = launch(k_plan_classify, w.per_strand, dim3(256), 0, nullptr, w.start.get(), S, w.n, w.notfull(),
                     w.ids.get(), w.slen.get(), w.q, w.nt, w.pd->kind.get(), w.npairs.get(), w.rowcnt.get(),
                     w.dctl.get())) ||
        (rc = plan_scan(w.npairs.get(), (int64_t)S, w.pstart.get())) || (rc = download(&w.ctl, w.dctl.get(), 1)) ||
        (rc = download(&w.n_valid, w.start.get() + S, 1)) || (rc = download(&w.P, w.pstart.get() + S, 1)))
        return rc;
    if (w.ctl.bad || w.n_valid < 0 || w.n_valid > w.n || w.P < 0) return w.inconsistent();
    if (w.ctl.empty_strand != INT32_MAX) {
        set_error(who + ": empty read on strand " + std::to_string(w.ctl.empty_strand) +
                  " with quality > 63 (the reference indexes its last bit)");
        return LDPC_ERR_ARG;
    }
    if (w.ctl.long_read != INT32_MAX) {
        set_error(who + ": read " + std::to_string(w.ctl.long_read) + " on a ragged strand is longer than " +
                  std::to_string(kPlanMaxLen) + " bytes (ldpc_dna_plan_host has no such limit)");
        return LDPC_ERR_ARG;
    }
    if (w.P > (int64_t)INT32_MAX * 64) {
        set_error(who + ": too many distance pairs for one call");
        return LDPC_ERR_UNSUPPORTED;
    }
    return LDPC_OK;
}

// The pairs of the ragged strands, their distances, and the reads with a close partner.
int plan_close_reads(PlanWork& w)
{
    const int64_t P = w.P;
    const size_t n_close = (size_t)std::max<int64_t>(w.n_valid, 16);
    const dim3 b256(256), per_pair(plan_blocks(P, 256));
    int rc;
    if ((rc = dev_alloc(w.close, n_close))) return rc;
    LDPC_HIP(hipMemset(w.close.get(), 0, n_close));
    if (P == 0) return LDPC_OK;
    dev_ptr<int32_t> pa, pb, dist;
    if ((rc = dev_alloc(pa, (size_t)P)) || (rc = dev_alloc(pb, (size_t)P)) || (rc = dev_alloc(dist, (size_t)P)) ||
        (rc = launch(k_plan_pairs, per_pair, b256, 0, nullptr, w.pstart.get(), w.start.get(), w.S, w.n_valid, P, pa.get(),
                     pb.get(), w.dctl.get())) ||
        (rc = launch_edit_distance(w.seq, w.soff.get(), w.slen.get(), pa.get(), pb.get(), P,
                                   std::max(w.ctl.max_ragged_len, 0), dist.get())))
        return rc;
    return launch(k_plan_close, per_pair, b256, 0, nullptr, pa.get(), pb.get(), dist.get(), P, w.n_valid, w.close.get(),
                  w.dctl.get());
}

// Candidates per strand, candidate starts and row_ptr; C and R; the candidate list.
int plan_candidates(PlanWork& w)
{
    const int32_t S = w.S;
    const dim3 b256(256);
    int rc;
    if ((rc = launch(k_plan_cand_count, w.per_strand, b256, 0, nullptr, w.start.get(), S, w.n_valid, w.npairs.get(),
                     w.close.get(), w.ncand.get(), w.rowcnt.get())) ||
        (rc = plan_scan(w.ncand.get(), (int64_t)S, w.cptr.get())) ||
        (rc = plan_scan(w.rowcnt.get(), (int64_t)S, w.pd->row_ptr.get())) ||
        (rc = download(&w.C, w.cptr.get() + S, 1)) || (rc = download(&w.R, w.pd->row_ptr.get() + S, 1)))
        return rc;
    if (w.C < 0 || w.C > w.n_valid || w.R < 0 || w.R > w.n_valid) return w.inconsistent();
    if ((rc = dev_alloc(w.cand, (size_t)w.C))) return rc;
    if (w.C == 0) return LDPC_OK;
    if (!w.a.align) {
        set_error(w.who + ": ragged strands need an aligner (align = 0)");
        return LDPC_ERR_ARG;
    }
    return launch(k_plan_cand_fill, w.per_strand, b256, 0, nullptr, w.start.get(), S, w.n_valid, w.cptr.get(), w.C,
                  w.close.get(), w.ids.get(), w.cand.get(), w.dctl.get());
}

// The aligner's view of the candidates of host reads: offsets and lengths into a.seqs.
int plan_cands_host(const PlanWork& w, const std::vector<int32_t>& cand, int64_t skip, std::vector<int64_t>* coff,
                    std::vector<int32_t>* clen)
{
    for (int64_t c = 0; c < w.C; c++) {
        const int32_t r = cand[(size_t)c];
        if (r < 0 || r >= w.n || w.a.lengths[r] < skip) return w.inconsistent();
        (*coff)[(size_t)c] = w.a.offsets[r] + skip;
        (*clen)[(size_t)c] = (int32_t)(w.a.lengths[r] - skip);
    }
    return LDPC_OK;
}

// ... and of device-resident reads: the candidates' payloads packed by
// k_plan_cand_gather into *dcseq, and copied down into *cseq for the host merge.
int plan_cands_device(PlanWork& w, int64_t skip, std::vector<int64_t>* coff, std::vector<int32_t>* clen,
                      std::vector<uint8_t>* cseq, dev_ptr<uint8_t>* dcseq)
{
    const int64_t C = w.C;
    const dim3 b256(256);
    dev_ptr<int32_t> dclen;
    dev_ptr<int64_t> dcoff;
    int64_t T = 0;
    int rc;
    if ((rc = dev_alloc(dclen, (size_t)C)) || (rc = dev_alloc(dcoff, (size_t)C + 1)) ||
        (rc = launch(k_plan_cand_len, dim3(plan_blocks(C, 256)), b256, 0, nullptr, w.cand.get(), C, w.n, w.len,
                     (int32_t)skip, dclen.get(), w.dctl.get())) ||
        (rc = plan_scan(dclen.get(), C, dcoff.get())) || (rc = download(&T, dcoff.get() + C, 1)))
        return rc;
    if (T < 0 || T > C * (int64_t)kPlanMaxLen) return w.inconsistent();
    cseq->resize((size_t)T);
    if ((rc = dev_alloc(*dcseq, (size_t)T)) ||
        (rc = launch(k_plan_cand_gather, dim3(plan_blocks(C, 4)), b256, 0, nullptr, w.cand.get(), C, w.n, w.seq, w.off,
                     w.src->seq_bytes, (int32_t)skip, dcoff.get(), dclen.get(), T, dcseq->get(), w.dctl.get())) ||
        (rc = download(coff->data(), dcoff.get(), (size_t)C)) || (rc = download(clen->data(), dclen.get(), (size_t)C)) ||
        (rc = download(cseq->data(), dcseq->get(), (size_t)T)) || (rc = download(&w.ctl, w.dctl.get(), 1)))
        return rc;
    return w.ctl.bad ? w.inconsistent() : LDPC_OK;
}

// The aligner: group s = the candidates of strand s (empty for most strands);
// its rows become the planner's (plan::aligned_row) and go up for k_plan_rows.
int plan_align(PlanWork& w)
{
    const int32_t S = w.S, nt = w.nt;
    const int64_t C = w.C, skip = w.a.index_vals ? 0 : rs::kPrefixNt;
    std::vector<int64_t> cptr((size_t)S + 1), coff((size_t)C), out_ptr((size_t)S + 1);
    std::vector<int32_t> cand((size_t)C), clen((size_t)C), centre((size_t)S);
    std::vector<uint8_t> out, cseq;  // cseq / dcseq, device source: the candidates' payloads, packed
    dev_ptr<uint8_t> dcseq;
    int rc;
    if ((rc = download(cptr.data(), w.cptr.get(), (size_t)S + 1)) || (rc = download(cand.data(), w.cand.get(), (size_t)C)))
        return rc;
    if (cptr[0] != 0 || cptr[(size_t)S] != C) return w.inconsistent();
    if ((rc = w.src ? plan_cands_device(w, skip, &coff, &clen, &cseq, &dcseq) : plan_cands_host(w, cand, skip, &coff, &clen)))
        return rc;
    StarCall sc{w.src ? cseq.data() : w.a.seqs, coff.data(), clen.data(), C, cptr.data(), (int64_t)S, centre.data(),
                w.h_width.data(), out_ptr.data(), nullptr, 0, nullptr, nullptr};
    sc.out_vec = &out;
    if ((rc = star_align_device(sc, w.device, w.workspace_bytes, nullptr, w.who, w.src ? dcseq.get() : w.seq))) return rc;
    std::vector<uint8_t> arows((size_t)C * (size_t)nt, star::kGap);
    for (int32_t s = 0; s < S; s++) {
        const int64_t c0 = cptr[(size_t)s], nc = cptr[(size_t)s + 1] - c0, wd = w.h_width[(size_t)s];
        if (nc == 0) continue;
        w.n_aligned++;
        for (int64_t q = 0; q < nc; q++)
            plan::aligned_row(out.data() + out_ptr[(size_t)s] + q * wd, wd, nt, arows.data() + (size_t)(c0 + q) * (size_t)nt);
    }
    return upload(w.arows, arows);
}

// k_plan_rows: rows and row_q, and the kinds of the aligned strands; the last look at the flag.
int plan_rows(PlanWork& w)
{
    PlanDev* pd = w.pd;
    const int64_t R = w.R;
    int rc;
    if ((rc = upload(w.width, w.h_width)) || (rc = dev_alloc(pd->rows, (size_t)R * (size_t)w.nt)) ||
        (rc = dev_alloc(pd->row_q, (size_t)R)) ||
        (R > 0 && (rc = launch(k_plan_rows, dim3((unsigned)std::min<int64_t>((R + 3) / 4, 2048)), dim3(256), 0, nullptr,
                               pd->row_ptr.get(), w.S, R, w.start.get(), w.n_valid, w.n, w.cptr.get(), w.C, w.cand.get(),
                               w.arows.get(), w.width.get(), w.seq, w.soff.get(), w.slen.get(), w.ids.get(), w.q, w.nt,
                               pd->kind.get(), pd->rows.get(), pd->row_q.get(), w.dctl.get()))) ||
        (rc = download(&w.ctl, w.dctl.get(), 1)))
        return rc;
    if (w.ctl.bad) return w.inconsistent();
    pd->R = R;
    return LDPC_OK;
}

// The host outputs the caller asked for, and the stats.
int plan_outputs(const PlanWork& w, bool host_outputs)
{
    const plan::Args& a = w.a;
    const PlanDev& pd = *w.pd;
    const size_t SS = (size_t)w.S, R = (size_t)w.R;
    int rc;
    if (a.kind && (rc = download(a.kind, pd.kind.get(), SS))) return rc;
    if (host_outputs && ((rc = download(a.row_ptr, pd.row_ptr.get(), SS + 1)) ||
                         (rc = download(a.rows, pd.rows.get(), R * (size_t)w.nt)) ||
                         (rc = download(a.row_q, pd.row_q.get(), R))))
        return rc;
    if (a.stats) {
        a.stats[plan::kStatValid] = w.n_valid;
        a.stats[plan::kStatPairs] = w.P;
        a.stats[plan::kStatAligned] = w.n_aligned;
        a.stats[plan::kStatAlignPairs] = w.C - w.n_aligned;
        a.stats[plan::kStatRows] = w.R;
        for (int k = 0; k < 4; k++) a.stats[plan::kStatCnumerr + k] = (int64_t)w.ctl.hist[k];
    }
    return LDPC_OK;
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
    if (a.n_reads > INT32_MAX - 1024) {
        set_error(who + ": too many reads for one call");
        return LDPC_ERR_UNSUPPORTED;
    }
    if (a.stats) std::fill(a.stats, a.stats + plan::kNumStats, 0);
    if (a.n_strands == 0) {
        if (host_outputs) a.row_ptr[0] = 0;
        pd->R = 0;
        return LDPC_OK;
    }
    int rc;
    if ((rc = select_device(who.c_str(), device))) return rc;
    PlanWork w{who, a, src, pd, device, workspace_bytes, a.n_reads, a.n_strands, a.payload_nt,
               dim3(plan_blocks(a.n_reads, 256)), dim3(plan_blocks(a.n_strands, 256))};
    w.h_width.assign((size_t)w.S, 0);
    if ((rc = plan_source(w, total)) || (rc = plan_segments(w)) || (rc = plan_classify(w)) ||
        (rc = plan_close_reads(w)) || (rc = plan_candidates(w)) || (w.C > 0 && (rc = plan_align(w))) ||
        (rc = plan_rows(w)))
        return rc;
    return plan_outputs(w, host_outputs);
}

}  // namespace
}  // namespace ldpc
