// channel_sim_kernels.hpp -- the error-rate simulation on the GPU (DESIGN.md
// sec. 8.11): k_sim_messages, k_channel_codes, k_frame_errors, the Engine
// methods that launch them (class K_OTHER of the kernel statistics), the
// ldpc_ber handle and the entry points of include/ldpc_amd.h's section
// "Error-rate simulation".  Included by engine.hip.  The definition and the
// draws are channel_sim.hpp's (chan::codes_host / frame_errors_host are the
// comparators, the bytes are the same); the loop is error_rate.hpp's.
#pragma once

#include "channel_sim.hpp"
#include "error_rate.hpp"
#include "host_decode.hpp"  // ldpc_graph

namespace ldpc {
namespace dev {

constexpr int kChanThreads = 256;
constexpr uint64_t kLowBits = 0x0101010101010101ull;

// Message bits [B][K] of frames [b0, b0 + B), K * B = total bytes.  The matrix
// is taken flat: a thread owns bytes [8t, 8t + 8) -- eight consecutive bits of
// one frame, or across a row end the last bits of one and the first of the
// next -- and stores them as one aligned 64-bit word; the thread that holds
// the end of the matrix stores its bytes one by one.
__global__ void __launch_bounds__(kChanThreads) k_sim_messages(uint8_t* __restrict__ msg, int32_t K, int64_t b0,
                                                               int64_t total, uint64_t key)
{
    const int64_t i0 = ((int64_t)blockIdx.x * kChanThreads + threadIdx.x) * 8;
    if (i0 >= total) return;
    uint64_t b = (uint64_t)(b0 + i0 / K);
    int32_t k = (int32_t)(i0 % K);
    const int n = total - i0 < 8 ? (int)(total - i0) : 8;
    uint64_t w = 0;
    for (int c = 0; c < n; c++) {
        w |= (uint64_t)chan::message_bit(key, b, (uint32_t)k) << (8 * c);
        if (++k == K) { k = 0; b++; }
    }
    if (n == 8) *reinterpret_cast<uint64_t*>(msg + i0) = w;
    else
        for (int c = 0; c < n; c++) msg[i0 + c] = (uint8_t)(w >> (8 * c));
}

// Codes [B][N] of frames [b0, b0 + B) from the codeword bytes cw [B][N], flat
// as k_sim_messages: one aligned 64-bit load of eight codeword bytes, eight
// draws, one aligned 64-bit store; the end of the matrix byte by byte.  The
// thresholds (padded, chan::pad_entry) sit in LDS, 2 KB; chan::level is the
// 8-step search without branches.
__global__ void __launch_bounds__(kChanThreads) k_channel_codes(const uint8_t* __restrict__ cw,
                                                                int8_t* __restrict__ codes, int32_t N, int64_t b0,
                                                                int64_t total, uint64_t key,
                                                                const uint64_t* __restrict__ thr)
{
    __shared__ uint64_t pad[chan::kThrPad];
    for (int i = (int)threadIdx.x; i < chan::kThrPad; i += kChanThreads) chan::pad_entry(thr, pad, i);
    __syncthreads();
    const int64_t i0 = ((int64_t)blockIdx.x * kChanThreads + threadIdx.x) * 8;
    if (i0 >= total) return;
    uint64_t b = (uint64_t)(b0 + i0 / N);
    int32_t j = (int32_t)(i0 % N);
    const int n = total - i0 < 8 ? (int)(total - i0) : 8;
    uint64_t c8 = 0, w = 0;
    if (n == 8) c8 = *reinterpret_cast<const uint64_t*>(cw + i0);
    else
        for (int c = 0; c < n; c++) c8 |= (uint64_t)cw[i0 + c] << (8 * c);
    for (int c = 0; c < n; c++) {
        const int8_t code = chan::code_of(pad, key, b, (uint32_t)j, (uint8_t)(c8 >> (8 * c)));
        w |= (uint64_t)(uint8_t)code << (8 * c);
        if (++j == N) { j = 0; b++; }
    }
    if (n == 8) *reinterpret_cast<uint64_t*>(codes + i0) = w;
    else
        for (int c = 0; c < n; c++) codes[i0 + c] = (int8_t)(w >> (8 * c));
}

// The error counter.  One rule picks the shape: a frame of N <= kWaveFrameMaxN
// bits is counted by one wave (four frames per block), a longer one by a whole
// block.
constexpr int32_t kWaveFrameMaxN = 2048;

// the four counts of positions [j, j + n) of one frame, n <= 8; Words: n == 8
// and the row is 8-byte aligned, so every array is read as one 64-bit word
template <bool Words>
__device__ __forceinline__ void count_piece(const uint8_t* __restrict__ hard, const uint8_t* __restrict__ cw,
                                            const int8_t* __restrict__ codes, const uint8_t* __restrict__ mask,
                                            const uint8_t* raw, int32_t j, int n, uint64_t* be_ie, uint64_t* re_er)
{
    uint64_t h = 0, c = 0, k = 0, m = 0;
    if (Words) {
        h = *reinterpret_cast<const uint64_t*>(hard + j);
        c = *reinterpret_cast<const uint64_t*>(cw + j);
        k = *reinterpret_cast<const uint64_t*>(codes + j);
        m = *reinterpret_cast<const uint64_t*>(mask + j);
    } else {
        for (int q = 0; q < n; q++) {
            h |= (uint64_t)hard[j + q] << (8 * q);
            c |= (uint64_t)cw[j + q] << (8 * q);
            k |= (uint64_t)(uint8_t)codes[j + q] << (8 * q);
            m |= (uint64_t)mask[j + q] << (8 * q);
        }
    }
    c &= kLowBits;
    const uint64_t d = (h ^ c) & kLowBits;
    uint64_t r = 0;  // the raw reading of the eight codes, one bit per byte
    uint32_t erased = 0;
    for (int q = 0; q < n; q++) {
        const uint32_t code = (uint32_t)(k >> (8 * q)) & 0xffu;  // the int8 code's byte
        r |= (uint64_t)raw[(code + 128u) & 0xffu] << (8 * q);    // table index code + 128 of the signed code
        erased += code == 0u;
    }
    *be_ie += (uint64_t)__popcll(d) | ((uint64_t)__popcll(d & m) << 32);
    *re_er += (uint64_t)__popcll((r ^ c) & kLowBits) | ((uint64_t)erased << 32);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// Block: one frame per block (256 threads, waves combined through LDS), else
// one frame per wave.  The counts travel as two packed 64-bit sums (each count
// < 2^24).  One lane writes the record with plain stores.
template <bool Block, bool Words>
__global__ void __launch_bounds__(kChanThreads) k_frame_errors(
    const uint8_t* __restrict__ hard, const uint8_t* __restrict__ cw, const int8_t* __restrict__ codes,
    const uint8_t* __restrict__ mask, const uint8_t* __restrict__ raw_tab, const int32_t* __restrict__ iters,
    const uint8_t* __restrict__ valid, int32_t N, int64_t B, ldpc_ber_record* __restrict__ rec)
{
    __shared__ uint8_t raw[256];
    __shared__ uint64_t part[2][kChanThreads / 64];
    raw[threadIdx.x] = raw_tab[threadIdx.x];
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const int64_t f = Block ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (kChanThreads / 64) + wv;
    const bool live = f < B;  // (the same in a whole wave; a block of the Block shape is all live)
    uint64_t a = 0, e = 0;
    if (live) {
        const size_t row = (size_t)f * (size_t)N;
        const int32_t t = Block ? (int32_t)threadIdx.x : lane, nt = Block ? kChanThreads : 64;
        const int32_t full = Words ? N / 8 * 8 : 0;
        for (int32_t j = 8 * t; j < full; j += 8 * nt)
            count_piece<true>(hard + row, cw + row, codes + row, mask, raw, j, 8, &a, &e);
        for (int32_t j = full + 8 * t; j < N; j += 8 * nt)
            count_piece<false>(hard + row, cw + row, codes + row, mask, raw, j, N - j < 8 ? N - j : 8, &a, &e);
    }
    a = wave_sum(a);
    e = wave_sum(e);
    if (Block) {
        if (lane == 0) { part[0][wv] = a; part[1][wv] = e; }
        __syncthreads();
        if (threadIdx.x != 0) return;
        a = e = 0;
        for (int q = 0; q < kChanThreads / 64; q++) { a += part[0][q]; e += part[1][q]; }
    } else if (lane != 0 || !live) {
        return;
    }
    ldpc_ber_record r;
    r.bit_err = (int32_t)(uint32_t)a;
    r.info_err = (int32_t)(a >> 32);
    r.raw_err = (int32_t)(uint32_t)e;
    r.erased = (int32_t)(e >> 32);
    r.iters = iters[f];
    r.valid = valid[f] != 0;
    rec[f] = r;
}

}  // namespace dev

int Engine::sim_messages(uint8_t* d_msg, int32_t K, int64_t b0, int64_t B, uint64_t seed)
{
    const int64_t total = B * K;
    if (total <= 0) return LDPC_OK;
    LDPC_HIP(hipSetDevice(device));
    const int64_t blocks = ((total + 7) / 8 + dev::kChanThreads - 1) / dev::kChanThreads;
    return launch(K_OTHER, dev::k_sim_messages, dim3((unsigned)blocks), dim3(dev::kChanThreads), d_msg, K, b0, total,
                  chan::message_key(seed));
}

int Engine::channel_codes(const uint8_t* d_cw, int8_t* d_codes, int64_t b0, int64_t B, uint64_t seed,
                          const uint64_t* d_thr)
{
    const int64_t total = B * g->N;
    if (total <= 0) return LDPC_OK;
    LDPC_HIP(hipSetDevice(device));
    const int64_t blocks = ((total + 7) / 8 + dev::kChanThreads - 1) / dev::kChanThreads;
    return launch(K_OTHER, dev::k_channel_codes, dim3((unsigned)blocks), dim3(dev::kChanThreads), d_cw, d_codes,
                  (int32_t)g->N, b0, total, chan::channel_key(seed), d_thr);
}

int Engine::frame_errors(const uint8_t* d_hard, const uint8_t* d_cw, const int8_t* d_codes, const uint8_t* d_mask,
                         const uint8_t* d_raw, const int32_t* d_iters, const uint8_t* d_valid, int64_t B,
                         ldpc_ber_record* d_rec)
{
    if (B <= 0) return LDPC_OK;
    LDPC_HIP(hipSetDevice(device));
    const int32_t N = (int32_t)g->N;
    const bool block = N > dev::kWaveFrameMaxN, words = N % 8 == 0;  // (hipMalloc's bases are 256-byte aligned)
    const dim3 grid((unsigned)(block ? B : (B + dev::kChanThreads / 64 - 1) / (dev::kChanThreads / 64)));
    const dim3 th(dev::kChanThreads);
    if (block)
        return words ? launch(K_OTHER, dev::k_frame_errors<true, true>, grid, th, d_hard, d_cw, d_codes, d_mask, d_raw,
                              d_iters, d_valid, N, B, d_rec)
                     : launch(K_OTHER, dev::k_frame_errors<true, false>, grid, th, d_hard, d_cw, d_codes, d_mask, d_raw,
                              d_iters, d_valid, N, B, d_rec);
    return words ? launch(K_OTHER, dev::k_frame_errors<false, true>, grid, th, d_hard, d_cw, d_codes, d_mask, d_raw,
                          d_iters, d_valid, N, B, d_rec)
                 : launch(K_OTHER, dev::k_frame_errors<false, false>, grid, th, d_hard, d_cw, d_codes, d_mask, d_raw,
                          d_iters, d_valid, N, B, d_rec);
}

}  // namespace ldpc

// The handle: everything a batch needs on the device, allocated once.
struct ldpc_ber {
    const ldpc::HostGraph* g = nullptr;
    const ldpc_encoder* enc = nullptr;  // null: the zero codeword
    int32_t device = 0, N = 0, K = 0;
    int64_t batch = 0;
    ldpc::Engine eng;
    ldpc::dev_ptr<uint8_t> msg, cw, hard, valid, mask, raw;
    ldpc::dev_ptr<int8_t> codes;
    ldpc::dev_ptr<int32_t> iters;
    ldpc::dev_ptr<uint64_t> thr;
    ldpc::dev_ptr<ldpc_ber_record> rec;
    ldpc::pinned_ptr<ldpc_ber_record> h_rec;
    ldpc::pinned_ptr<uint64_t> h_thr;  // staging of thr[254] and raw[256]
    ldpc::pinned_ptr<uint8_t> h_raw;

    ~ldpc_ber()
    {
        (void)hipSetDevice(device);
        if (eng.stream) (void)hipStreamSynchronize(eng.stream.get());
    }
};

namespace ldpc {
namespace {

constexpr int64_t kBerPoolMax = 1024;          // as ldpc_trial: batches up to here get a lane pool of their size
constexpr int64_t kBerMaxBatch = 1 << 20;

int ber_create(const ldpc_graph* g, const ldpc_encoder* enc, int32_t device, int32_t algo,
               const ldpc_schedule* schedule, int64_t batch, std::unique_ptr<ldpc_ber>& out)
{
    const std::string who = "ldpc_ber_create: ";
    if (!g) { set_error(who + "null graph"); return LDPC_ERR_ARG; }
    const int64_t N = g->h.N;
    if (N < 1 || N >= chan::kMaxN) { set_error(who + "N must be in 1 .. 2^24 - 1"); return LDPC_ERR_ARG; }
    if (batch < 1 || batch > kBerMaxBatch || batch > INT64_MAX / 8 / N) {
        set_error(who + "batch must be in 1 .. 2^20");
        return LDPC_ERR_ARG;
    }
    auto h = std::make_unique<ldpc_ber>();
    h->g = &g->h;
    h->enc = enc;
    h->device = device;
    h->N = (int32_t)N;
    h->batch = batch;
    std::vector<uint8_t> mask((size_t)N, enc ? 0 : 1);
    if (enc) {
        int32_t eN = 0, K = 0;
        int rc = ldpc_encoder_info(enc, &eN, &K, nullptr, nullptr, nullptr);
        if (rc) return rc;
        if (eN != N) { set_error(who + "the encoder is of another code length"); return LDPC_ERR_ARG; }
        std::vector<int32_t> info((size_t)K);
        if ((rc = ldpc_encoder_info(enc, nullptr, nullptr, nullptr, info.data(), nullptr))) return rc;
        for (const int32_t j : info) mask[(size_t)j] = 1;
        h->K = K;
    }
    int rc;
    if ((rc = select_device("ldpc_ber_create", device))) return rc;
    // the lane pool: the schedule's pool_tiles when set, else as ldpc_trial sizes it
    const int64_t pool = schedule && schedule->pool_tiles > 0 ? (int64_t)64 * schedule->pool_tiles
                         : batch <= kBerPoolMax               ? (batch + 63) / 64 * 64
                                                              : 0;
    if ((rc = h->eng.init(h->g, device, algo, pool, schedule))) return rc;
    // (+ 8: the matrices are read and written as 64-bit words up to their last whole word)
    const size_t n = (size_t)batch, mat = n * (size_t)N + 8;
    if ((rc = dev_alloc(h->msg, n * (size_t)h->K + 8)) || (rc = dev_alloc(h->cw, mat)) ||
        (rc = dev_alloc(h->codes, mat)) || (rc = dev_alloc(h->hard, mat)) || (rc = dev_alloc(h->valid, n)) ||
        (rc = dev_alloc(h->iters, n)) || (rc = dev_alloc(h->rec, n)) || (rc = upload(h->mask, mask)) ||
        (rc = dev_alloc(h->raw, 256)) || (rc = dev_alloc(h->thr, (size_t)chan::kThr)) ||
        (rc = pinned_alloc(h->h_rec, n)) || (rc = pinned_alloc(h->h_thr, (size_t)chan::kThr)) ||
        (rc = pinned_alloc(h->h_raw, 256)))
        return rc;
    LDPC_HIP(hipMemset(h->cw.get(), 0, mat));  // the zero codeword, when there is no encoder
    LDPC_HIP(hipMemset(h->hard.get(), 0, mat));
    LDPC_HIP(hipMemset(h->codes.get(), 0, mat));
    out = std::move(h);
    return LDPC_OK;
}

// thr and the raw table of `table` to the device, on the engine's stream
// (the stream is idle: every call of the handle ends with a sync).
int ber_tables(ldpc_ber& h, const uint64_t* thr, const double* table, int32_t table_kind)
{
    hipStream_t s = h.eng.stream.get();
    if (thr) {
        std::copy(thr, thr + chan::kThr, h.h_thr.get());
        LDPC_HIP(hipMemcpyAsync(h.thr.get(), h.h_thr.get(), sizeof(uint64_t) * chan::kThr, hipMemcpyHostToDevice, s));
    }
    chan::raw_table(table, table_kind, h.h_raw.get());
    LDPC_HIP(hipMemcpyAsync(h.raw.get(), h.h_raw.get(), 256, hipMemcpyHostToDevice, s));
    return LDPC_OK;
}

// One batch, B <= batch: the records of frames [b0, b0 + B) into rec (host).
int ber_batch(ldpc_ber& h, const double* table, int32_t table_kind, uint64_t seed, int64_t b0, int64_t B,
              int32_t max_iter, ldpc_ber_record* rec)
{
    int rc;
    hipStream_t s = h.eng.stream.get();
    if (h.enc) {
        if ((rc = h.eng.sim_messages(h.msg.get(), h.K, b0, B, seed))) return rc;
        if ((rc = ldpc_encoder_encode_device(h.enc, h.device, (void*)s, h.msg.get(), B, h.cw.get()))) return rc;
    }
    if ((rc = h.eng.channel_codes(h.cw.get(), h.codes.get(), b0, B, seed, h.thr.get()))) return rc;
    if ((rc = h.eng.decode_codes(h.codes.get(), table, table_kind, B, max_iter, h.hard.get(), nullptr, LDPC_POST_LLR,
                                 h.iters.get(), h.valid.get(), nullptr, b0)))
        return rc;
    if ((rc = h.eng.frame_errors(h.hard.get(), h.cw.get(), h.codes.get(), h.mask.get(), h.raw.get(), h.iters.get(),
                                 h.valid.get(), B, h.rec.get())))
        return rc;
    LDPC_HIP(hipMemcpyAsync(h.h_rec.get(), h.rec.get(), sizeof(ldpc_ber_record) * (size_t)B, hipMemcpyDeviceToHost, s));
    if ((rc = h.eng.sync())) return rc;
    std::copy(h.h_rec.get(), h.h_rec.get() + B, rec);
    return LDPC_OK;
}

int ber_check(const std::string& who, ldpc_ber* h, const uint64_t* thr, const double* table, int32_t table_kind,
              int64_t b0, int64_t B, int32_t max_iter)
{
    if (!h || !table) { set_error(who + "null handle or table"); return LDPC_ERR_ARG; }
    if (table_kind != LDPC_IN_LLR && table_kind != LDPC_IN_LR) { set_error(who + "bad table_kind"); return LDPC_ERR_ARG; }
    if (max_iter < 0) { set_error(who + "max_iter must be >= 0"); return LDPC_ERR_ARG; }
    const std::string err = chan::check_channel(thr, h->N, b0, B);
    if (!err.empty()) { set_error(who + err); return LDPC_ERR_ARG; }
    return LDPC_OK;
}

int ber_run_range(ldpc_ber* h, const uint64_t* thr, const double* table, int32_t table_kind, uint64_t seed, int64_t b0,
                  int64_t B, int32_t max_iter, ldpc_ber_record* out)
{
    if (int rc = ber_check("ldpc_ber_run_range: ", h, thr, table, table_kind, b0, B, max_iter)) return rc;
    if (B > 0 && !out) { set_error("ldpc_ber_run_range: null records"); return LDPC_ERR_ARG; }
    if (B == 0) return LDPC_OK;
    LDPC_HIP(hipSetDevice(h->device));
    if (int rc = ber_tables(*h, thr, table, table_kind)) return rc;
    for (int64_t o = 0; o < B; o += h->batch)
        if (int rc = ber_batch(*h, table, table_kind, seed, b0 + o, std::min(h->batch, B - o), max_iter, out + o))
            return rc;
    return LDPC_OK;
}

int ber_run(ldpc_ber* h, const uint64_t* thr, const double* table, int32_t table_kind, uint64_t seed, int32_t max_iter,
            int64_t frames, int64_t target, int64_t max_frames, ldpc_ber_result* out)
{
    const std::string who = "ldpc_ber_run: ";
    if (int rc = ber_check(who, h, thr, table, table_kind, 0, 0, max_iter)) return rc;
    std::string err = ber::check_run(h->batch, max_iter, frames, target, max_frames, out);
    if (!err.empty()) { set_error(who + err); return LDPC_ERR_ARG; }
    LDPC_HIP(hipSetDevice(h->device));
    if (int rc = ber_tables(*h, thr, table, table_kind)) return rc;
    const int rc = ber::run(
        [&](int64_t b0, int64_t B, ldpc_ber_record* rec) {
            return ber_batch(*h, table, table_kind, seed, b0, B, max_iter, rec);
        },
        h->batch, max_iter, frames, target, max_frames, out, &err);
    if (rc && !err.empty()) set_error(who + err);
    return rc;
}

int ber_frame_errors(ldpc_ber* h, const uint8_t* hard, const uint8_t* cw, const int8_t* codes, const double* table,
                     int32_t table_kind, const int32_t* iters, const uint8_t* valid, int64_t B, ldpc_ber_record* out)
{
    const std::string who = "ldpc_ber_frame_errors: ";
    if (!h || !hard || !codes || !table || !out) { set_error(who + "null argument"); return LDPC_ERR_ARG; }
    if (B < 1 || B > h->batch) { set_error(who + "B must be in 1 .. batch"); return LDPC_ERR_ARG; }
    LDPC_HIP(hipSetDevice(h->device));
    hipStream_t s = h->eng.stream.get();
    const size_t mat = (size_t)B * (size_t)h->N;
    if (int rc = ber_tables(*h, nullptr, table, table_kind)) return rc;
    LDPC_HIP(hipMemcpyAsync(h->hard.get(), hard, mat, hipMemcpyHostToDevice, s));
    LDPC_HIP(hipMemcpyAsync(h->codes.get(), codes, mat, hipMemcpyHostToDevice, s));
    if (cw) LDPC_HIP(hipMemcpyAsync(h->cw.get(), cw, mat, hipMemcpyHostToDevice, s));
    else LDPC_HIP(hipMemsetAsync(h->cw.get(), 0, mat, s));
    if (iters) LDPC_HIP(hipMemcpyAsync(h->iters.get(), iters, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, s));
    else LDPC_HIP(hipMemsetAsync(h->iters.get(), 0, sizeof(int32_t) * (size_t)B, s));
    if (valid) LDPC_HIP(hipMemcpyAsync(h->valid.get(), valid, (size_t)B, hipMemcpyHostToDevice, s));
    else LDPC_HIP(hipMemsetAsync(h->valid.get(), 0, (size_t)B, s));
    LDPC_HIP(hipStreamSynchronize(s));  // the caller's buffers are free whichever way the call ends
    int rc = h->eng.frame_errors(h->hard.get(), h->cw.get(), h->codes.get(), h->mask.get(), h->raw.get(),
                                 h->iters.get(), h->valid.get(), B, h->rec.get());
    if (!rc) {
        LDPC_HIP(hipMemcpyAsync(h->h_rec.get(), h->rec.get(), sizeof(ldpc_ber_record) * (size_t)B, hipMemcpyDeviceToHost, s));
        rc = h->eng.sync();
    }
    if (!rc) std::copy(h->h_rec.get(), h->h_rec.get() + B, out);
    // a handle without an encoder relies on cw being zeros
    if (!h->enc && cw) {
        LDPC_HIP(hipMemsetAsync(h->cw.get(), 0, mat, s));
        LDPC_HIP(hipStreamSynchronize(s));
    }
    return rc;
}

}  // namespace
}  // namespace ldpc

extern "C" {

int ldpc_channel_codes_host(const uint8_t* cw, int32_t N, int64_t b0, int64_t B, uint64_t seed, const uint64_t* thr,
                            int8_t* codes)
{
    const std::string err = ldpc::chan::codes_host(cw, N, b0, B, seed, thr, codes);
    if (err.empty()) return LDPC_OK;
    ldpc::set_error("ldpc_channel_codes_host: " + err);
    return LDPC_ERR_ARG;
}

int ldpc_frame_errors_host(const uint8_t* hard, const uint8_t* cw, const int8_t* codes, int32_t N, int64_t B,
                           const uint8_t* info_mask, const double* table, int32_t table_kind, const int32_t* iters,
                           const uint8_t* valid, ldpc_ber_record* records)
{
    if (!table || (table_kind != LDPC_IN_LLR && table_kind != LDPC_IN_LR)) {
        ldpc::set_error("ldpc_frame_errors_host: null table or bad table_kind");
        return LDPC_ERR_ARG;
    }
    uint8_t raw[256];
    ldpc::chan::raw_table(table, table_kind, raw);
    const std::string err = ldpc::chan::frame_errors_host(hard, cw, codes, N, B, info_mask, raw, iters, valid, records);
    if (err.empty()) return LDPC_OK;
    ldpc::set_error("ldpc_frame_errors_host: " + err);
    return LDPC_ERR_ARG;
}

int ldpc_ber_run_host(int32_t N, const ldpc_encoder* enc, ldpc_ber_decode_fn decode, void* user, const uint64_t* thr,
                      const double* table, int32_t table_kind, uint64_t seed, int64_t batch, int32_t max_iter,
                      int64_t frames, int64_t target_frame_err, int64_t max_frames, ldpc_ber_result* result)
{
    using namespace ldpc;
    const std::string who = "ldpc_ber_run_host: ";
    if (!decode || !table || (table_kind != LDPC_IN_LLR && table_kind != LDPC_IN_LR)) {
        set_error(who + "null decoder or table, or bad table_kind");
        return LDPC_ERR_ARG;
    }
    std::string err = chan::check_channel(thr, N, 0, 0);
    if (err.empty()) err = ber::check_run(batch, max_iter, frames, target_frame_err, max_frames, result);
    if (!err.empty()) { set_error(who + err); return LDPC_ERR_ARG; }
    try {
        std::vector<uint8_t> mask, msg;
        int32_t K = 0;
        if (enc) {
            int32_t eN = 0;
            if (int rc = ldpc_encoder_info(enc, &eN, &K, nullptr, nullptr, nullptr)) return rc;
            if (eN != N) { set_error(who + "the encoder is of another code length"); return LDPC_ERR_ARG; }
            std::vector<int32_t> info((size_t)K);
            if (int rc = ldpc_encoder_info(enc, nullptr, nullptr, nullptr, info.data(), nullptr)) return rc;
            mask.assign((size_t)N, 0);
            for (const int32_t j : info) mask[(size_t)j] = 1;
        }
        auto encode = [&](int64_t b0, int64_t B, uint8_t* cw) {
            msg.resize((size_t)B * (size_t)K);
            chan::messages_host(K, b0, B, seed, msg.data());
            return ldpc_encode_host(enc, msg.data(), B, cw);
        };
        auto dec = [&](const int8_t* codes, int64_t b0, int64_t B, uint8_t* hard, int32_t* iters, uint8_t* valid) {
            return decode(user, codes, table, table_kind, b0, B, max_iter, hard, iters, valid);
        };
        auto range = ber::host_range(N, enc == nullptr, encode, dec, thr, table, table_kind, seed,
                                     enc ? mask.data() : nullptr, &err);
        const int rc = ber::run(range, batch, max_iter, frames, target_frame_err, max_frames, result, &err);
        if (rc && !err.empty()) set_error(who + err);
        return rc;
    } catch (const std::bad_alloc&) {
        set_error(who + "out of host memory");
        return LDPC_ERR_DEVICE;
    }
}

ldpc_ber* ldpc_ber_create(const ldpc_graph* g, const ldpc_encoder* enc, int32_t device, int32_t algo,
                          const ldpc_schedule* schedule, int64_t batch, int* err)
{
    std::unique_ptr<ldpc_ber> h;
    int rc;
    try {
        rc = ldpc::ber_create(g, enc, device, algo, schedule, batch, h);
    } catch (const std::bad_alloc&) {
        ldpc::set_error("ldpc_ber_create: out of host memory");
        rc = LDPC_ERR_DEVICE;
    }
    if (err) *err = rc;
    return rc ? nullptr : h.release();
}

void ldpc_ber_free(ldpc_ber* h) { delete h; }

int ldpc_ber_set_params(ldpc_ber* h, int32_t msa_precision, double msa_step, int32_t msa_offset, uint64_t tie_seed)
{
    if (!h) { ldpc::set_error("ldpc_ber_set_params: null handle"); return LDPC_ERR_ARG; }
    return h->eng.set_params(msa_precision, msa_step, msa_offset, tie_seed);
}

int ldpc_ber_run_range(ldpc_ber* h, const uint64_t* thr, const double* table, int32_t table_kind, uint64_t seed,
                       int64_t b0, int64_t B, int32_t max_iter, ldpc_ber_record* records_out)
{
    return ldpc::ber_run_range(h, thr, table, table_kind, seed, b0, B, max_iter, records_out);
}

int ldpc_ber_run(ldpc_ber* h, const uint64_t* thr, const double* table, int32_t table_kind, uint64_t seed,
                 int32_t max_iter, int64_t frames, int64_t target_frame_err, int64_t max_frames,
                 ldpc_ber_result* result)
{
    try {
        return ldpc::ber_run(h, thr, table, table_kind, seed, max_iter, frames, target_frame_err, max_frames, result);
    } catch (const std::bad_alloc&) {
        ldpc::set_error("ldpc_ber_run: out of host memory");
        return LDPC_ERR_DEVICE;
    }
}

int ldpc_ber_read(ldpc_ber* h, int64_t B, uint8_t* cw, int8_t* codes, uint8_t* hard)
{
    if (!h || B < 0 || B > h->batch) { ldpc::set_error("ldpc_ber_read: null handle, or B outside 0 .. batch"); return LDPC_ERR_ARG; }
    LDPC_HIP(hipSetDevice(h->device));
    LDPC_HIP(hipStreamSynchronize(h->eng.stream.get()));
    const size_t mat = (size_t)B * (size_t)h->N;
    if (cw && mat) LDPC_HIP(hipMemcpy(cw, h->cw.get(), mat, hipMemcpyDeviceToHost));
    if (codes && mat) LDPC_HIP(hipMemcpy(codes, h->codes.get(), mat, hipMemcpyDeviceToHost));
    if (hard && mat) LDPC_HIP(hipMemcpy(hard, h->hard.get(), mat, hipMemcpyDeviceToHost));
    return LDPC_OK;
}

int ldpc_ber_frame_errors(ldpc_ber* h, const uint8_t* hard, const uint8_t* cw, const int8_t* codes,
                          const double* table, int32_t table_kind, const int32_t* iters, const uint8_t* valid,
                          int64_t B, ldpc_ber_record* records)
{
    return ldpc::ber_frame_errors(h, hard, cw, codes, table, table_kind, iters, valid, B, records);
}

int ldpc_ber_profile(ldpc_ber* h, int32_t stride)
{
    if (!h) { ldpc::set_error("ldpc_ber_profile: null handle"); return LDPC_ERR_ARG; }
    return h->eng.profile(stride);
}

int ldpc_ber_stats(ldpc_ber* h, ldpc_kernel_stats* out)
{
    if (!h || !out) { ldpc::set_error("ldpc_ber_stats: null argument"); return LDPC_ERR_ARG; }
    return h->eng.stats(out);
}

}  // extern "C"
