// engine.hpp -- internal interface between the C ABI and the HIP engine.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ldpc_amd.h"
#include "engine_plan.hpp"  // resolve_schedule, plan_engine: what an engine decides before it allocates
#include "graph.hpp"
#include "hip_own.hpp"  // set_error, LDPC_HIP, the owning handles
#include "kargs.hpp"

namespace ldpc {

// K_UNCOUNTED: launches outside the per-class statistics (Sampler::launch)
enum KClass { K_UNCOUNTED = -1, K_CHECK = 0, K_VAR = 1, K_SYN = 2, K_INIT = 3, K_FINAL = 4, K_OTHER = 5, K_NCLASS = 6 };

// A buffer allocated on first use: ensure(n) leaves at least n elements.  One
// that must grow is replaced once stream `s` has drained (a decode still
// running may read the old one).
template <typename T>
int alloc_n(dev_ptr<T>& p, size_t n) { return dev_alloc(p, n); }
template <typename T>
int alloc_n(pinned_ptr<T>& p, size_t n) { return pinned_alloc(p, n); }
template <typename P>
struct Lazy {
    P p;
    size_t n = 0;
    auto get() const { return p.get(); }
    int ensure(size_t want, hipStream_t s)
    {
        if (p && n >= want) return LDPC_OK;
        if (p) LDPC_HIP(hipStreamSynchronize(s));
        p.reset();
        n = 0;
        if (int rc = alloc_n(p, want)) return rc;
        n = want;
        return LDPC_OK;
    }
};

// The graph on the device.
struct DeviceGraph {
    dev_ptr<int32_t> row_ptr, col_idx, col_ptr, col_edge;
    dev_ptr<int32_t> col_idx_T;  // [dc][M] for regular rows (syndrome gathers)
    dev_ptr<uint32_t> col_er;    // [E] (row << 18) | edge id of CSC position q (MSA-C record lookups)
    dev_ptr<int32_t> row_pos;    // [E] v2c position of CSR edge e (MSA-C: v2c in column order)
    int32_t msa_pa = 8, msa_pb = 1;  // MSA-C: edge s of column j at j * msa_pa + s * msa_pb
    int build(const HostGraph& g, bool msa_c);
};

// The lane pool of the continuous schedules: which lane holds which codeword,
// the claim counter, the syndrome step's words, and the two host-visible
// words (occupancy polls, device faults).
struct LanePool {
    static constexpr int kRing = 8, kLag = 2;
    dev_ptr<uint64_t> fresh, occ;          // [tile] lane masks (ContState)
    dev_ptr<int64_t> lane_b;               // [tile*64]
    dev_ptr<int32_t> lane_n;               // [tile*64]
    dev_ptr<unsigned long long> ctr;       // [0] claim counter, [1..kRing] occupancy ring
    // occupancy polls without copies or events: poll q's counter is
    // ctr[1 + q % kRing]; the device writes tag(q) << 40 | occupied lanes to
    // h_poll[q % kRing] (pinned, device-mapped at d_poll) and the host waits on it
    uint64_t poll_seq = 0;
    pinned_ptr<unsigned long long> h_poll;
    unsigned long long* d_poll = nullptr;
    // device fault word (kargs.hpp kFaultTag): pinned, device-mapped at d_fault
    pinned_ptr<unsigned long long> h_fault;
    unsigned long long* d_fault = nullptr;
    dev_ptr<unsigned long long> unsat;     // [tile] syndrome words of the step
    dev_ptr<unsigned int> done;            // [tile] syndrome / check blocks arrived
    dev_ptr<uint64_t> fin;                 // [tile] lanes finished at the step
    dev_ptr<int64_t> fin_b;                // [tile*64] their codeword index
    dev_ptr<int32_t> fin_n;                // [tile*64] their iteration count
    // handover: [0, cap_tiles) last, [cap_tiles, 2 cap_tiles) pend, [2 cap_tiles, 3 cap_tiles) the pending
    // plane's syndrome words; the pending codewords' indices; the second ballot plane [tile][N]
    dev_ptr<uint64_t> ho;
    dev_ptr<int64_t> pend_b;
    dev_ptr<uint64_t> hard_fin;

    int build(const EnginePlan& p, int32_t N);
    void poll_arm(dev::ContState& cs, uint64_t q) const;
    int poll_wait(uint64_t q, unsigned long long* occ, hipStream_t stream);
    // LDPC_ERR_DEVICE (and the message) once a kernel has reported a fault;
    // the word is cleared, so each fault is reported once
    int check_fault();
    void clear_faults();
};

// The one launch path, and the profile behind ldpc_engine_profile / _stats:
// HIP events on every `stride`-th launch of a class.
struct Sampler {
    int stride = 0;
    int64_t launches[K_NCLASS] = {0}, sampled[K_NCLASS] = {0};
    double ms[K_NCLASS] = {0};
    std::vector<std::pair<Event, Event>> live[K_NCLASS];  // recorded, not yet read
    std::vector<Event> pool;

    // Launch `kernel` on s as launch number launches[c]++ of class c
    // (K_UNCOUNTED: outside the statistics, never sampled); owning handles
    // among the arguments are passed as their pointers.  engine.hip only.
    template <typename F, typename... A>
    int launch(int c, hipStream_t s, F kernel, dim3 grid, dim3 block, const A&... args);
    // the live samples into ms (the stream has been waited for)
    int collect();
    void reset(int new_stride);
    void snapshot(ldpc_kernel_stats* out) const;

  private:
    Event get_event();
};

// One decode's arguments (Engine::decode / decode_codes list them in this order).
struct DecodeCall {
    const double* in = nullptr;    // [B][N] fp64 of in_kind, or
    const int8_t* codes = nullptr; // [B][N] int8 codes of the engine's prior table (continuous schedules)
    int in_kind = LDPC_IN_LLR;
    int32_t N = 0;
    int64_t B = 0;
    int32_t max_iter = 0;
    uint8_t* hard = nullptr;       // [B][N]
    double* post = nullptr;        // [B][N]
    int post_kind = LDPC_POST_LLR;
    int32_t* iters = nullptr;      // [B]
    uint8_t* valid = nullptr;      // [B]
    int64_t tie_base = 0;          // index of codeword 0 in the caller's whole batch (the integer decoders' tie hash)
    // codewords b0 .. b0 + Bc - 1 of this call
    DecodeCall slice(int64_t b0, int64_t Bc) const
    {
        DecodeCall c = *this;
        const size_t o = (size_t)b0 * (size_t)N;
        c.B = Bc;
        c.in = in ? in + o : nullptr;
        c.codes = codes ? codes + o : nullptr;
        c.hard = hard ? hard + o : nullptr;
        c.post = post ? post + o : nullptr;
        c.iters = iters ? iters + b0 : nullptr;
        c.valid = valid ? valid + b0 : nullptr;
        c.tie_base = tie_base + b0;
        return c;
    }
};

struct Engine {
    const HostGraph* g = nullptr;
    int device = 0;
    int algo = LDPC_ALGO_BP;
    ldpc_schedule sched{};  // resolved (resolve_schedule)
    EnginePlan p;           // what init decided (plan_engine); not modified afterwards
    // Declared before everything that may be in use on it, so destroyed after it.
    Stream stream;
    DeviceGraph dg;
    LanePool lp;
    Sampler sampler;
    // decoder state.  Messages: v2c, and the check->variable scratch of one
    // tile group (c2v_buf) -- empty in the resident pool, whose check->variable
    // messages are written over v2c: c2v() is the one or the other
    dev_ptr<double> v2c, c2v_buf;
    dev_ptr<double> prior;
    dev_ptr<uint8_t> d_sgn;  // msa_c: [tile][N][64] sign bits of the v2c each column last stored
    dev_ptr<uint64_t> hard, active;
    dev_ptr<int32_t> iters;
    dev_ptr<uint8_t> valid;
    Lazy<dev_ptr<double>> post_t;  // [tiles][N][64] per-iteration posterior
    // coded input (decode_codes): the lanes' int8 prior codes [tiles][N][64],
    // the prior table (256 fp64, code + 128), its last uploaded contents (an
    // unchanged table is not re-sent), and the fp64 staging of schedules
    // without coded kernels (the largest pass seen)
    Lazy<dev_ptr<int8_t>> pcode;
    Lazy<dev_ptr<double>> d_ptab;
    Lazy<pinned_ptr<double>> h_ptab;
    bool ptab_valid = false;
    Lazy<dev_ptr<double>> d_expand;
    // integer decoders (LDPC_ALGO_QMSA / GALLAGER_*): int32 views of v2c, c2v, prior
    int32_t q_precision = 6, q_beta = 0;
    double q_step = 0.5;
    uint64_t tie_seed = 0;

    ~Engine();
    // schedule: a caller's (resolved here), or with `resolved` one that
    // resolve_schedule already returned (the host API's slots)
    int init(const HostGraph* graph, int dev, int algorithm, int64_t chunk, const ldpc_schedule* schedule,
             bool resolved = false);
    double* c2v() const { return p.res ? v2c.get() : c2v_buf.get(); }
    // tie_base: the index of codeword 0 in the caller's whole batch (the host
    // API's chunks; the integer decoders' tie hash keys on it)
    int decode(const double* d_in, int in_kind, int64_t B, int32_t max_iter, uint8_t* d_hard, double* d_post,
               int post_kind, int32_t* d_iters, uint8_t* d_valid, int64_t tie_base = 0);
    // coded input: d_codes [B][N] int8 on device, h_table[256] (host) the
    // channel value of code k at k + 128, of kind table_kind (LDPC_IN_LLR or,
    // BP only, LDPC_IN_LR); BP takes the host exp of an LLR table.  d_stage
    // (optional, >= min(cap, B) x N fp64): where schedules without coded
    // kernels expand a pass to fp64 (else an engine buffer)
    int decode_codes(const int8_t* d_codes, const double* h_table, int table_kind, int64_t B, int32_t max_iter,
                     uint8_t* d_hard, double* d_post, int post_kind, int32_t* d_iters, uint8_t* d_valid,
                     double* d_stage = nullptr, int64_t tie_base = 0);
    int set_params(int32_t precision, double step, int32_t beta, uint64_t seed);
    int gen_bsc(double* d_out, int out_kind, int64_t b0, int64_t B, const uint8_t* d_cw, int32_t n_cw, uint64_t seed,
                double p, double llr_mag);
    // the same channel as int8 codes: +1 for a received 0, -1 for a 1
    int gen_bsc_codes(int8_t* d_out, int64_t b0, int64_t B, const uint8_t* d_cw, int32_t n_cw, uint64_t seed, double p);
    // the error-rate simulation's kernels (channel_sim_kernels.hpp, DESIGN.md
    // sec. 8.11) on the engine's stream: message bits d_msg [B][K] of frames
    // [b0, b0 + B); channel codes d_codes [B][N] of the codewords d_cw under
    // the thresholds d_thr[254]; per-frame error records d_rec [B] (d_mask
    // [N] the information positions, d_raw[256] chan::raw_table's bytes)
    int sim_messages(uint8_t* d_msg, int32_t K, int64_t b0, int64_t B, uint64_t seed);
    int channel_codes(const uint8_t* d_cw, int8_t* d_codes, int64_t b0, int64_t B, uint64_t seed, const uint64_t* d_thr);
    int frame_errors(const uint8_t* d_hard, const uint8_t* d_cw, const int8_t* d_codes, const uint8_t* d_mask,
                     const uint8_t* d_raw, const int32_t* d_iters, const uint8_t* d_valid, int64_t B,
                     ldpc_ber_record* d_rec);
    // wait for the engine's stream, then LanePool::check_fault
    int sync();
    // ldpc_engine_profile / ldpc_engine_stats: wait for the stream and read the
    // live samples, then reset the statistics and set the stride / copy them out
    int profile(int stride);
    int stats(ldpc_kernel_stats* out);
    // LDPC_SCHED_* bits in effect (ldpc_engine_info)
    int32_t flags() const;
    // out[i] = table[code[i] + 128] for i < n on stream s
    int expand_lr(const int8_t* d_code, const double* d_table, double* d_out, int64_t n, hipStream_t s);
    // out[i] bit r = in[8 i + r] for i < nbytes on the engine stream (host-API hard-bit copy)
    int pack_bits(const uint8_t* d_in, uint8_t* d_out, int64_t nbytes);

  private:
    int collect_stats();
    int decode(const DecodeCall& c);
    // continuous batching; on an error the queued steps are drained and the
    // fault words cleared before returning (each fault is reported once)
    int run_cont(const DecodeCall& c);
    int run_cont_steps(const DecodeCall& c);
    // fixed passes: c.B <= cap codewords, the fp64 decoders / the integer ones
    int run_chunk(const DecodeCall& c);
    int run_chunk_int(const DecodeCall& c);
    template <typename Init, typename Check, typename Var, typename Final>
    int fixed_pass(const DecodeCall& c, Init&& init, Check&& check, Var&& var, Final&& finalize);
    int probe(int probes);
    int time_candidates(int probes, std::vector<dev_ptr<double>>& cand, size_t* best);
    int time_steps(double* pool, unsigned gt, hipEvent_t e0, hipEvent_t e1, float* ms);
    // a launch of class c on the engine's stream (Sampler::launch)
    template <typename F, typename... A>
    int launch(int c, F kernel, dim3 grid, dim3 block, const A&... args);
    // check / variable phase of tiles t0 .. t0+gt-1.  rstep: the resident
    // pool's step (in-place check + fused syndrome), nullptr: the plain check
    // kernel.  timing: the placement probe's launches (K_UNCOUNTED)
    int launch_check(double* scratch, int64_t t0, unsigned gt, const dev::ResStep* rstep, bool timing = false);
    int launch_var(double* scratch, int64_t t0, unsigned gt, double* pt, const dev::Refill& rf, bool timing = false);
    int var_cpw_for(const dev::Refill& rf) const;
};

// Device copy of an encoder (gf2.hpp HostEncoder), uploaded once per
// (encoder, device) by capi.cpp.
struct EncoderDev {
    int32_t M = 0, N = 0, K = 0, rank = 0, Mw = 0;
    int32_t* info_pos = nullptr;  // [K]
    int32_t* par_pos = nullptr;   // [rank]
    int32_t* row_ptr = nullptr;   // [M+1]
    int32_t* col_idx = nullptr;   // [E]
    uint64_t* T = nullptr;        // [rank][Mw]
};

// Encode passes hold at most this many 64-codeword tiles (16 384 codewords;
// the DNA code's ballot words of a pass: 38 MB, L2 / Infinity Cache resident).
constexpr int64_t kEncPassTiles = 256;
// 64-bit words of workspace for passes of `tiles` tiles: w [tiles][N] + s [tiles][M]
inline size_t encode_workspace_words(const EncoderDev& d, int64_t tiles) { return (size_t)tiles * ((size_t)d.N + (size_t)d.M); }
// Enqueue the encode of d_msg [B][K] u8 (bit 0 of each byte) into d_cw
// [B][N] u8 on `stream`, in passes of ws_tiles <= kEncPassTiles tiles through
// the workspace ws (encode_workspace_words(d, ws_tiles)).  Asynchronous.
int encode_launch(const EncoderDev& d, hipStream_t stream, const uint8_t* d_msg, int64_t B, uint8_t* d_cw, uint64_t* ws,
                  int64_t ws_tiles);

}  // namespace ldpc
