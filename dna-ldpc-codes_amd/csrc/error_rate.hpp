// error_rate.hpp -- the error-rate loop: the control
// flow of the reference's Run_Simulation / Check_End (DNA_main.cpp:756-914),
// encode -> channel -> decode -> count per frame, until `frames` frames or
// until the frame-error count reaches a target.  Header-only host C++, no HIP:
// the body of ldpc_ber_run_host and of the device handle's ldpc_ber_run
// (channel_sim_kernels.hpp), and what tests/channel_sim_san/chan_check.cpp
// includes.
//
// The loop is stated over "run this range": a callable
//     int run_range(int64_t b0, int64_t B, ldpc_ber_record* records)
// that produces the records of frames [b0, b0 + B) (LDPC_OK or an error code
// that ends the run).  Frames are taken in index order, a batch at a time; a
// batch runs whole, and the records are accumulated only up to the cut, so the
// result is the sequential loop's whatever the batch size.
//
// Stop rule (Check_End).  frames > 0: exactly `frames` frames.  frames == 0:
// the run ends after the frame at which the count of frame errors (frames
// with bit_err > 0) reaches target_frame_err >= 1, and after max_frames >= 1
// frames at the latest.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ldpc_amd.h"
#include "channel_sim.hpp"

namespace ldpc {
namespace ber {

// The argument errors of every run; empty: none.
inline std::string check_run(int64_t batch, int32_t max_iter, int64_t frames, int64_t target_frame_err,
                             int64_t max_frames, const ldpc_ber_result* out)
{
    if (!out) return "null result";
    if (batch < 1) return "batch must be >= 1";
    if (max_iter < 0) return "max_iter must be >= 0";
    if (frames < 0 || target_frame_err < 0 || max_frames < 0) return "negative frames, target_frame_err or max_frames";
    if (frames == 0 && (target_frame_err < 1 || max_frames < 1))
        return "frames == 0 needs target_frame_err >= 1 and max_frames >= 1";
    if (std::max(frames, max_frames) > chan::kMaxFrame) return "the frames must lie in [0, 2^40)";
    if (out->iter_hist && out->n_hist < max_iter + 1) return "the histogram needs max_iter + 1 bins";
    return std::string();
}

// One frame's record into the totals.  False: an iteration count outside 0 .. max_iter.
inline bool accumulate(const ldpc_ber_record& r, int32_t max_iter, ldpc_ber_result* out)
{
    if (r.iters < 0 || r.iters > max_iter) return false;
    out->frames++;
    out->bit_err += r.bit_err;
    out->info_err += r.info_err;
    out->frame_err += r.bit_err > 0;
    out->undetected += r.bit_err > 0 && r.valid;  // DNA_main.cpp:871-874
    out->detected += !r.valid;
    out->raw_bit_err += r.raw_err;
    out->raw_frame_err += r.raw_err > 0;          // DNA_main.cpp:830-834
    out->erased += r.erased;
    out->iter_sum += r.iters;
    if (out->iter_hist) out->iter_hist[r.iters]++;
    return true;
}

// The loop.  *out keeps its iter_hist / n_hist; every counter is reset.  *err
// gets the message of an argument error or of a bad record.
template <class RunRange>
int run(RunRange&& run_range, int64_t batch, int32_t max_iter, int64_t frames, int64_t target_frame_err,
        int64_t max_frames, ldpc_ber_result* out, std::string* err)
{
    *err = check_run(batch, max_iter, frames, target_frame_err, max_frames, out);
    if (!err->empty()) return LDPC_ERR_ARG;
    int64_t* hist = out->iter_hist;
    const int32_t n_hist = out->n_hist;
    *out = ldpc_ber_result{};
    out->iter_hist = hist;
    out->n_hist = n_hist;
    if (hist) std::fill(hist, hist + (max_iter + 1), (int64_t)0);
    const int64_t limit = frames > 0 ? frames : max_frames;
    std::vector<ldpc_ber_record> rec((size_t)std::min(batch, limit));
    for (int64_t b0 = 0; b0 < limit; b0 += batch) {
        const int64_t B = std::min(batch, limit - b0);
        if (int rc = run_range(b0, B, rec.data())) return rc;
        for (int64_t i = 0; i < B; i++) {
            if (!accumulate(rec[(size_t)i], max_iter, out)) {
                *err = "frame " + std::to_string(b0 + i) + " reports an iteration count outside 0 .. max_iter";
                return LDPC_ERR_DEVICE;
            }
            if (frames == 0 && out->frame_err >= target_frame_err) return LDPC_OK;  // the cut: the rest is dropped
        }
    }
    return LDPC_OK;
}

// "Run this range" on host buffers, one thread: the codewords from `encode`
//     int encode(int64_t b0, int64_t B, uint8_t* cw)      -- cw [B][N]
// (zero == true: the zero codeword, encode is not called), chan::codes_host,
// the caller's decoder
//     int decode(const int8_t* codes, int64_t b0, int64_t B, uint8_t* hard, int32_t* iters, uint8_t* valid)
// and chan::frame_errors_host.  Every buffer holds exactly B rows.
template <class Encode, class Decode>
struct HostRange {
    int32_t N;
    bool zero;
    Encode encode;
    Decode decode;
    const uint64_t* thr;
    uint64_t seed;
    const uint8_t* info_mask;  // [N] or null
    uint8_t raw[256];
    std::string* err;

    int operator()(int64_t b0, int64_t B, ldpc_ber_record* rec)
    {
        const size_t mat = (size_t)B * (size_t)N;
        std::vector<uint8_t> cw(mat, 0), hard(mat, 0), valid((size_t)B, 0);
        std::vector<int8_t> codes(mat, 0);
        std::vector<int32_t> iters((size_t)B, 0);
        if (!zero)
            if (int rc = encode(b0, B, cw.data())) return rc;
        *err = chan::codes_host(zero ? nullptr : cw.data(), N, b0, B, seed, thr, codes.data());
        if (!err->empty()) return LDPC_ERR_ARG;
        if (int rc = decode(codes.data(), b0, B, hard.data(), iters.data(), valid.data())) {
            *err = "the decoder callback failed";
            return rc;
        }
        *err = chan::frame_errors_host(hard.data(), zero ? nullptr : cw.data(), codes.data(), N, B, info_mask, raw,
                                       iters.data(), valid.data(), rec);
        return err->empty() ? LDPC_OK : LDPC_ERR_ARG;
    }
};

template <class Encode, class Decode>
HostRange<Encode, Decode> host_range(int32_t N, bool zero, Encode encode, Decode decode, const uint64_t* thr,
                                     const double* table, int32_t table_kind, uint64_t seed, const uint8_t* info_mask,
                                     std::string* err)
{
    HostRange<Encode, Decode> h{N, zero, encode, decode, thr, seed, info_mask, {0}, err};
    chan::raw_table(table, table_kind, h.raw);
    return h;
}

}  // namespace ber
}  // namespace ldpc
