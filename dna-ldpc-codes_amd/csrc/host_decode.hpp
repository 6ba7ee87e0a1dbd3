// host_decode.hpp -- the host-buffer decode behind ldpc_decode and
// ldpc_decode_codes (host_decode.cpp), and the graph handle that keeps its
// device contexts between calls.
#pragma once
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/ldpc_amd.h"
#include "engine.hpp"
#include "graph.hpp"
#include "hip_own.hpp"

namespace ldpc {

class Workers;  // persistent host threads of a slot (host_decode.cpp)

// One staging half: the pinned and device buffers of one chunk in flight, the
// code table that goes with it, and the events that order its three legs.
struct Stage {
    size_t rows = 0, N = 0;  // capacity in codewords, code length
    pinned_ptr<double> h_in, h_post;
    pinned_ptr<uint8_t> h_hard, h_valid;
    pinned_ptr<uint8_t> h_hbits;  // hard bits packed 8 per byte (N % 8 == 0)
    pinned_ptr<int32_t> h_iters;
    pinned_ptr<int8_t> h_code;    // code table path: one byte per LLR
    dev_ptr<double> d_in, d_post;
    dev_ptr<uint8_t> d_hard, d_valid, d_hbits;
    dev_ptr<int32_t> d_iters;
    dev_ptr<int8_t> d_code;
    std::vector<double> table;    // [256] LLR (or, BP, LR: table_kind) of code k at k + 128
    int table_kind = LDPC_IN_LLR;
    bool coded = false;           // the staging buffer holds codes (else fp64 input)
    Event h2d, dec, d2h;          // input on the device; decoded (and packed); outputs on the host

    int init(size_t rows_, size_t N_, bool codes);
    int want_codes();  // code staging of the integer decoders (ldpc_decode_codes): on first use
    int want_post();   // posterior staging: on the first call that asks for it
};

// One reusable device context for host-buffer decodes: an engine plus two
// staging halves of `xfer` codewords each, so that the host-side exp and the
// PCIe copies of one chunk overlap the decode of the previous one.  The
// engine decodes each chunk through its lane pool (pool codewords, 0: its own
// choice -- the resident pool for BP), by continuous refill when the chunk is
// larger.
struct Slot {
    std::unique_ptr<Engine> eng;  // (first: released last)
    int device = 0, algo = 0;
    int64_t pool = 0, xfer = 0;
    ldpc_schedule sched{};  // resolved (ldpc::resolve_schedule): the engine's schedule
    Stream copy, copy_out;  // H2D / D2H streams (the engine computes on its own)
    Stage stage[2];
    std::unique_ptr<Workers> workers;

    Slot();
    // waits for both copy streams and the engine's stream, then the members
    // release themselves (a slot is dropped on an error, with work queued)
    ~Slot();
};

// The channel input of a host-buffer decode: fp64 LLRs (ldpc_decode) or int8
// codes with their 256-entry table (ldpc_decode_codes).
struct HostInput {
    const double* llr = nullptr;
    const int8_t* codes = nullptr;
    const double* table = nullptr;
    int table_kind = LDPC_IN_LLR;
};

}  // namespace ldpc

struct ldpc_graph {
    ldpc::HostGraph h;
    std::mutex mu;
    std::vector<std::unique_ptr<ldpc::Slot>> free_slots;

    // a slot with the same lane pool (0: the engine's own) and staging for
    // at least `xfer` codewords per chunk
    // (small: any small-batch pool of at least `pool` lanes will do -- the
    // extra tiles stay empty -- so calls of varying small sizes share one)
    std::unique_ptr<ldpc::Slot> take(int device, int algo, int64_t pool, int64_t xfer, bool small,
                                     const ldpc_schedule& sched);
    void give(std::unique_ptr<ldpc::Slot> s);
};

namespace ldpc {

int host_decode(const ldpc_graph* g, const HostInput& in, int64_t B, int32_t max_iter, int32_t algo,
                uint8_t* hard_out, double* post_out, int32_t* iters_out, uint8_t* valid_out, const ldpc_opts* opts);

}  // namespace ldpc
