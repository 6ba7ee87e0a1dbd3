// channel_sim.hpp -- the transmission channel of the error-rate simulation
// (DESIGN.md sec. 8.11): a symmetric memoryless channel with at most 255
// outputs, given as data, every draw a counter hash of (seed, frame, bit).
// Header-only host C++, no HIP: the body of ldpc_channel_codes_host and
// ldpc_frame_errors_host, the definition k_channel_codes / k_sim_messages /
// k_frame_errors (channel_sim_kernels.hpp) and synth.channel_codes follow, and
// what tests/channel_sim_san/chan_check.cpp includes.  The draws (LDPC_SIM_HD)
// are compiled for both sides, so there is one statement of each.  Integers
// only: no floating point in the channel itself.
//
// Definition.  thr[254]: u64 thresholds, non-decreasing, each <= 2^53.  For
// frame b < 2^40 and bit j < 2^24:
//   u    = splitmix64(((b << 24) | j) ^ splitmix64(seed ^ kStream)) >> 11
//   k0   = -127 + #{i : u >= thr[i]}
//   code = cw[b][j] ? -k0 : k0                    (int8, -127 .. 127)
// kStream keeps the channel's stream apart from the messages', whose bit k of
// frame b is the low bit of splitmix64(((b << 24) | k) ^ splitmix64(seed))
// (synth.random_messages).  A code's channel value is table[code + 128]
// (ldpc_decode_codes); the tables of the AWGN, BSC and BEC channels are made
// on the host (synth.awgn_channel / bsc_channel / bec_channel).
//
// Per frame the error counter (frame_errors_host, k_frame_errors) writes one
// record: bits where hard != cw over all N positions and over the information
// positions (a byte mask), raw channel errors by the reference's rule
// (DNA_main.cpp:1711-1748: value >= 0 reads as 0, anything else, a NaN
// included, as 1; over all N positions), erased bits (code == 0), and the
// decoder's iteration count and valid flag.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/ldpc_amd.h"
#include "dna_sim.hpp"  // LDPC_SIM_HD, sim::splitmix64

namespace ldpc {
namespace chan {

constexpr uint64_t kStream = 0x4348414e4e454c31ull;  // "CHANNEL1"
constexpr int32_t kThr = 254;                        // thresholds: 255 levels
constexpr int32_t kThrPad = 256;                     // the padded copy the search reads (2 KB)
constexpr uint64_t kOne = (uint64_t)1 << 53;         // probability 1 as a threshold
constexpr int64_t kMaxFrame = (int64_t)1 << 40;      // b0 + B <= 2^40: the key holds b in 40 bits
constexpr int32_t kMaxN = 1 << 24;                   // N < 2^24: the key holds j in 24 bits

LDPC_SIM_HD uint64_t channel_key(uint64_t seed) { return sim::splitmix64(seed ^ kStream); }
LDPC_SIM_HD uint64_t message_key(uint64_t seed) { return sim::splitmix64(seed); }

// u of (frame b, bit j), uniform in [0, 2^53); key = channel_key(seed)
LDPC_SIM_HD uint64_t draw(uint64_t key, uint64_t b, uint32_t j)
{
    return sim::splitmix64(((b << 24) | (uint64_t)j) ^ key) >> 11;
}

// bit k of the message of frame b; key = message_key(seed)
LDPC_SIM_HD uint8_t message_bit(uint64_t key, uint64_t b, uint32_t k)
{
    return (uint8_t)(sim::splitmix64(((b << 24) | (uint64_t)k) ^ key) & 1u);
}

// pad[kThrPad] from thr[kThr]: the thresholds, then entries no u reaches
template <class T>
LDPC_SIM_HD void pad_entry(const uint64_t* thr, T* pad, int32_t i)
{
    pad[i] = i < kThr ? thr[i] : ~(uint64_t)0;
}

// #{i < 254 : u >= thr[i]} for non-decreasing thr, by an 8-step binary search
// without branches over the padded copy: pos counts the entries known to be
// <= u, and entry pos + step - 1 <= 254 decides the next step (entries 254 and
// 255 are above every u, so pos ends <= 254).
LDPC_SIM_HD int32_t level(const uint64_t* pad, uint64_t u)
{
    int32_t pos = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int32_t step = 128; step >= 1; step >>= 1) pos += pad[pos + step - 1] <= u ? step : 0;
    return pos;
}

// the code of one bit: cw_bit is the transmitted bit
LDPC_SIM_HD int8_t code_of(const uint64_t* pad, uint64_t key, uint64_t b, uint32_t j, uint8_t cw_bit)
{
    const int32_t k0 = level(pad, draw(key, b, j)) - 127;
    return (int8_t)((cw_bit & 1u) ? -k0 : k0);
}

// raw[256]: the reference's hard reading of a channel value (DNA_main.cpp:1726-1741):
// LLR >= 0 (a likelihood ratio: >= 1) reads as 0, anything else, a NaN included, as 1
inline void raw_table(const double* table, int32_t table_kind, uint8_t* raw)
{
    const double zero = table_kind == LDPC_IN_LR ? 1.0 : 0.0;
    for (int i = 0; i < 256; i++) raw[i] = table[i] >= zero ? 0 : 1;
}

// The argument errors of the channel itself (every form); empty: none.
inline std::string check_channel(const uint64_t* thr, int64_t N, int64_t b0, int64_t B)
{
    if (!thr) return "null thresholds";
    if (N < 1 || N >= kMaxN) return "N must be in 1 .. 2^24 - 1 (the key holds the bit in 24 bits)";
    if (b0 < 0 || B < 0 || b0 > kMaxFrame || B > kMaxFrame - b0) return "the frames must lie in [0, 2^40)";
    if (B > INT64_MAX / 8 / N) return "B * N bytes overflow the address space";
    for (int32_t i = 0; i < kThr; i++) {
        if (thr[i] > kOne) return "a threshold is above 2^53";
        if (i && thr[i] < thr[i - 1]) return "the thresholds must be non-decreasing";
    }
    return std::string();
}

// The channel on one thread: codes [B][N] of frames [b0, b0 + B); cw [B][N]
// (bit 0 of each byte) or null: the zero codeword.
inline std::string codes_host(const uint8_t* cw, int32_t N, int64_t b0, int64_t B, uint64_t seed, const uint64_t* thr,
                              int8_t* codes)
{
    const std::string err = check_channel(thr, N, b0, B);
    if (!err.empty()) return err;
    if (B > 0 && !codes) return "null codes";
    uint64_t pad[kThrPad];
    for (int32_t i = 0; i < kThrPad; i++) pad_entry(thr, pad, i);
    const uint64_t key = channel_key(seed);
    for (int64_t i = 0; i < B; i++)
        for (int32_t j = 0; j < N; j++) {
            const size_t at = (size_t)i * (size_t)N + (size_t)j;
            codes[at] = code_of(pad, key, (uint64_t)(b0 + i), (uint32_t)j, cw ? cw[at] : (uint8_t)0);
        }
    return std::string();
}

// Message bits [B][K] of frames [b0, b0 + B) (synth.random_messages).
inline void messages_host(int32_t K, int64_t b0, int64_t B, uint64_t seed, uint8_t* msg)
{
    const uint64_t key = message_key(seed);
    for (int64_t i = 0; i < B; i++)
        for (int32_t k = 0; k < K; k++) msg[(size_t)i * (size_t)K + (size_t)k] = message_bit(key, (uint64_t)(b0 + i), (uint32_t)k);
}

// The error counter on one thread.  hard / codes [B][N]; cw [B][N] or null
// (zeros); info_mask [N] (1 at an information position) or null (every
// position); raw[256] from raw_table; iters / valid [B] or null (read as 0).
inline std::string frame_errors_host(const uint8_t* hard, const uint8_t* cw, const int8_t* codes, int32_t N, int64_t B,
                                     const uint8_t* info_mask, const uint8_t* raw, const int32_t* iters,
                                     const uint8_t* valid, ldpc_ber_record* rec)
{
    if (N < 1 || N >= kMaxN || B < 0 || B > INT64_MAX / 8 / N) return "N must be in 1 .. 2^24 - 1 and B >= 0";
    if (B > 0 && (!hard || !codes || !raw || !rec)) return "null hard, codes, table or records";
    for (int64_t i = 0; i < B; i++) {
        ldpc_ber_record r{};
        for (int32_t j = 0; j < N; j++) {
            const size_t at = (size_t)i * (size_t)N + (size_t)j;
            const uint8_t c = cw ? (uint8_t)(cw[at] & 1u) : (uint8_t)0;
            const int32_t d = (hard[at] & 1u) != c;
            r.bit_err += d;
            r.info_err += d & (info_mask ? (int32_t)(info_mask[j] & 1u) : 1);
            r.raw_err += raw[(int32_t)codes[at] + 128] != c;
            r.erased += codes[at] == 0;
        }
        r.iters = iters ? iters[i] : 0;
        r.valid = valid ? (int32_t)(valid[i] != 0) : 0;
        rec[i] = r;
    }
    return std::string();
}

}  // namespace chan
}  // namespace ldpc
