// dna_sim_kernels.hpp -- the sequencing channel on the GPU (DESIGN.md sec.
// 8.9): k_sim_reads and the ldpc_dna_sim_* entry points.  Included by dna.hip,
// whose launch() / download() helpers (hip_own.hpp) the host code uses.
// The definition and the draws are dna_sim.hpp's (sim::reads_host is the
// comparator, the bytes are the same).
#pragma once

namespace ldpc {
namespace {

constexpr int kSimWaves = 4;  // reads per block, one wave each

// One wave per read, lanes over positions in chunks of 64: lane l of chunk c0
// owns slot p = c0 + l and source base p.  Two ballots give every lane the
// number of bytes the lanes below it write ("slot inserts", "base kept"); `off`,
// the bytes of the chunks before, is the same in every lane.  A lane writes at
// most two bytes, its insertion and then its base, at off + those counts; the
// last position is 2L < stride, so every store stays inside the read's slot.
// Lane 0 writes length, quality, strand and (offsets != null) the read's byte
// offset i * stride, the planner's `offsets`.  No LDS, no atomics.  The strand
// index is < S by construction; a read whose index fails the check anyway gets
// length 0 and sets *bad.
__global__ void __launch_bounds__(64 * kSimWaves) k_sim_reads(
    const uint8_t* __restrict__ strands, int32_t S, int32_t L, uint64_t seedmix, int64_t r0, int64_t n, uint64_t t_sub,
    uint64_t t_ins, uint64_t t_del, const int32_t* __restrict__ q_val, const uint32_t* __restrict__ q_lo, int32_t nq,
    int64_t stride, uint8_t* __restrict__ reads, int64_t* __restrict__ offsets, int32_t* __restrict__ lengths,
    int32_t* __restrict__ quals, int32_t* __restrict__ strand_of, int32_t* __restrict__ bad)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t i = (int64_t)blockIdx.x * kSimWaves + (threadIdx.x >> 6);  // the same in the whole wave
    if (i >= n) return;
    const uint64_t r = (uint64_t)(r0 + i);
    const int64_t s = sim::read_strand(seedmix, r, S);
    const bool ok = s >= 0 && s < S;
    int32_t off = 0;
    if (ok) {
        const uint8_t* __restrict__ src = strands + (size_t)s * (size_t)L;
        uint8_t* __restrict__ dst = reads + (size_t)i * (size_t)stride;
        const uint64_t below = (1ull << lane) - 1ull;
        for (int32_t c0 = 0; c0 <= L; c0 += 64) {
            const int32_t p = c0 + lane;
            uint8_t ins_c = 0, base_c = 0;
            const bool ins = p <= L && sim::slot_inserts(seedmix, r, (uint32_t)p, t_ins, &ins_c);
            const bool kept = p < L && sim::base_kept(seedmix, r, (uint32_t)p, src[p], t_sub, t_del, &base_c);
            const uint64_t mi = __ballot(ins), mk = __ballot(kept);
            int32_t pos = off + __popcll(mi & below) + __popcll(mk & below);
            if (ins) dst[pos++] = ins_c;
            if (kept) dst[pos] = base_c;
            off += __popcll(mi) + __popcll(mk);
        }
    }
    if (lane == 0) {
        const int32_t qi = sim::read_quality_index(seedmix, r, q_lo, nq);
        const bool q_ok = qi >= 0 && qi < nq;
        if (!ok || !q_ok) *bad = 1;
        lengths[i] = off;
        quals[i] = q_ok ? q_val[qi] : 0;
        if (strand_of) strand_of[i] = ok ? (int32_t)s : -1;
        if (offsets) offsets[i] = i * stride;
    }
}

// k_sim_reads on device-resident buffers, on the null stream.  The arguments
// have passed sim::check_channel; 1 <= n <= INT32_MAX.
int launch_sim_reads(const uint8_t* d_strands, int32_t S, int32_t L, uint64_t seed, int64_t r0, int64_t n,
                     int64_t t_sub, int64_t t_ins, int64_t t_del, const int32_t* d_q_val, const uint32_t* d_q_lo,
                     int32_t nq, uint8_t* d_reads, int64_t* d_offsets, int32_t* d_lengths, int32_t* d_quals,
                     int32_t* d_strand_of, int32_t* d_bad)
{
    return launch(k_sim_reads, dim3((unsigned)((n + kSimWaves - 1) / kSimWaves)), dim3(64 * kSimWaves), 0, nullptr,
                  d_strands, S, L, sim::splitmix64(seed), r0, n, (uint64_t)t_sub, (uint64_t)t_ins, (uint64_t)t_del,
                  d_q_val, d_q_lo, nq, sim::stride(L), d_reads, d_offsets, d_lengths, d_quals, d_strand_of, d_bad);
}

int sim_reads_device(const sim::Args& a, int32_t device)
{
    const std::string who = "ldpc_dna_sim_reads";
    const std::string err = sim::check_args(a);
    if (!err.empty()) {
        set_error(who + ": " + err);
        return LDPC_ERR_ARG;
    }
    if (a.n > INT32_MAX) {
        set_error(who + ": too many reads for one call");
        return LDPC_ERR_UNSUPPORTED;
    }
    if (a.n == 0) return LDPC_OK;
    int rc;
    if ((rc = select_device(who.c_str(), device))) return rc;
    const size_t n = (size_t)a.n, bytes = n * (size_t)sim::stride(a.L);
    dev_ptr<uint8_t> dstr, dreads;
    dev_ptr<int32_t> dqv, dlen, dq, dso, dbad;
    dev_ptr<uint32_t> dql;
    const int32_t zero = 0;
    if ((rc = upload(dstr, a.strands, (size_t)a.S * (size_t)a.L)) || (rc = upload(dqv, a.q_val, (size_t)a.nq)) ||
        (rc = upload(dql, a.q_lo, (size_t)a.nq)) || (rc = dev_alloc(dreads, bytes)) || (rc = dev_alloc(dlen, n)) ||
        (rc = dev_alloc(dq, n)) || (a.strand_of && (rc = dev_alloc(dso, n))) || (rc = upload(dbad, &zero, 1)))
        return rc;
    // (bytes past a read's length are not written: a defined value for the copy down)
    LDPC_HIP(hipMemset(dreads.get(), 0, bytes));
    if ((rc = launch_sim_reads(dstr.get(), a.S, a.L, a.seed, a.r0, a.n, a.t_sub, a.t_ins, a.t_del, dqv.get(),
                               dql.get(), a.nq, dreads.get(), nullptr, dlen.get(), dq.get(), dso.get(), dbad.get())))
        return rc;
    int32_t bad = 0;
    if ((rc = download(&bad, dbad.get(), 1))) return rc;
    if (bad) {
        set_error(who + ": a strand or quality index failed its range check");
        return LDPC_ERR_DEVICE;
    }
    if ((rc = download(a.reads, dreads.get(), bytes)) || (rc = download(a.lengths, dlen.get(), n)) ||
        (rc = download(a.quals, dq.get(), n)))
        return rc;
    return a.strand_of ? download(a.strand_of, dso.get(), n) : LDPC_OK;
}

}  // namespace
}  // namespace ldpc

extern "C" {

int64_t ldpc_dna_sim_stride(int32_t strand_nt) { return ldpc::sim::stride(strand_nt); }

int ldpc_dna_sim_reads_host(const uint8_t* strands, int32_t n_strands, int32_t strand_nt, uint64_t seed, int64_t r0,
                            int64_t n_reads, int64_t t_sub, int64_t t_ins, int64_t t_del, const int32_t* q_val,
                            const uint32_t* q_lo, int32_t nq, uint8_t* reads, int32_t* lengths, int32_t* quals,
                            int32_t* strand_of)
{
    const std::string err = ldpc::sim::reads_host(ldpc::sim::Args{strands, n_strands, strand_nt, seed, r0, n_reads,
                                                                  t_sub, t_ins, t_del, q_val, q_lo, nq, reads,
                                                                  lengths, quals, strand_of});
    if (err.empty()) return LDPC_OK;
    set_error("ldpc_dna_sim_reads_host: " + err);
    return LDPC_ERR_ARG;
}

int ldpc_dna_sim_reads(const uint8_t* strands, int32_t n_strands, int32_t strand_nt, uint64_t seed, int64_t r0,
                       int64_t n_reads, int64_t t_sub, int64_t t_ins, int64_t t_del, const int32_t* q_val,
                       const uint32_t* q_lo, int32_t nq, uint8_t* reads, int32_t* lengths, int32_t* quals,
                       int32_t* strand_of, int32_t device)
{
    return ldpc::sim_reads_device(ldpc::sim::Args{strands, n_strands, strand_nt, seed, r0, n_reads, t_sub, t_ins,
                                                  t_del, q_val, q_lo, nq, reads, lengths, quals, strand_of},
                                  device);
}

}  // extern "C"
