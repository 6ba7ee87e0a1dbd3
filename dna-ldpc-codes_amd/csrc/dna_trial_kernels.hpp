// dna_trial_kernels.hpp -- the trial handle: the kernels
// and the device backend of dna_trial.hpp's control flow, and the ldpc_trial_*
// entry points.  Included at the end of dna.hip, which has the planner
// (plan_device), the count rule (dna_bit_rule) and the entry points' guard
// (dna_guard) it reuses; kernels are started with launch() (hip_own.hpp).
//
// Everything of a run is enqueued on the engine's stream, the planner excepted:
// its kernels run on the null stream, and the engine's stream waits for an
// event recorded there before the code kernel starts.  Every index loaded from
// device memory is range-checked before use; a failed check sets the handle's
// flag word and the call fails with LDPC_ERR_DEVICE.
//
// ldpc_trial_run_sim puts the sequencing channel's kernel
// (k_sim_reads, dna_sim_kernels.hpp) on the null stream ahead of the planner,
// which then reads the handle's device-resident reads instead of uploads.
//
//   k_dna_codes      k_dna_llr's count rule, int8 codes and the overflow word only
//   k_trial_stats    one pass over hard, codes and truth: errors per row,
//                    re_decode per column, integer atomics only
//   k_trial_gather   rows of the code matrix -> the contiguous batch of a second decode
//   k_trial_scatter  rows of a second decode's hard bits -> their rows of hard
// and, for speculated second decodes (ldpc_trial_set_speculation),
//   k_trial_absmax       the largest |code| of the failed rows
//   k_trial_gather_spec  a failed row -> its k shifted copies in the batch, read once
#pragma once

namespace ldpc {
namespace {

// k_dna_llr without the fp64 matrix and the mask: thread (strand s, nucleotide
// k) writes the codes of bits 2k and 2k + 1 with the same rule and the same
// saturation, so the bytes are k_dna_llr's codes.
__global__ void __launch_bounds__(256) k_dna_codes(const int32_t* __restrict__ kind,
                                                   const int64_t* __restrict__ row_ptr,
                                                   const uint8_t* __restrict__ rows,
                                                   const int32_t* __restrict__ row_q, int32_t S, int32_t nt,
                                                   int8_t* __restrict__ codes, int32_t* __restrict__ overflow)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t k = blockIdx.y;
    if (s >= S) return;
    const int kd = kind[s];
    const int64_t r0 = row_ptr[s], r1 = row_ptr[s + 1];
    for (int h = 0; h < 2; h++) {
        int n;
        bool is_int;
        dna_bit_rule(kd, r0, r1, rows, row_q, nt, k, h, &n, &is_int);
        codes[(size_t)(2 * k + h) * S + s] = (int8_t)max(-127, min(127, n));
        if (n > 127 || n < -127) *overflow = 1;
    }
}

constexpr int kStatCols = 4;     // columns per thread (one 4-byte load of each matrix when N % 4 == 0)
constexpr int kStatRows = 16;    // rows per block
constexpr int kStatThreads = 256;

// 4 bytes of row `p` from column c0: one dword when `vec` (N % 4 == 0, so every
// row starts 4-byte aligned), else the bytes below N one by one (others 0).
__device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ p, int64_t c0, int32_t N, bool vec)
{
    if (vec) return *reinterpret_cast<const uint32_t*>(p + c0);
    uint32_t v = 0;
    for (int c = 0; c < kStatCols; c++)
        if (c0 + c < N) v |= (uint32_t)p[c0 + c] << (8 * c);
    return v;
}

// Block (x, y): columns [x * 1024, x * 1024 + 1024), batch rows [y * 16, y * 16
// + 16).  Batch row k is row k of hard [B][N]; its codes and truth are row
// rows[k] (rows null: k) of codes / truth [n_rows][N].  errors[k] += number of
// hard != truth (truth null: left alone), re_decode[j] += hard != (code < 0)
// (re_decode null: left alone).  Column sums stay in registers over the row
// loop; a row's count is reduced over the wave, one atomic per wave.
__global__ void __launch_bounds__(kStatThreads) k_trial_stats(const uint8_t* __restrict__ hard,
                                                              const int8_t* __restrict__ codes,
                                                              const uint8_t* __restrict__ truth,
                                                              const int32_t* __restrict__ rows, int32_t B,
                                                              int32_t n_rows, int32_t N, int32_t* __restrict__ errors,
                                                              int32_t* __restrict__ re_decode,
                                                              int32_t* __restrict__ bad)
{
    const bool vec = (N & 3) == 0;
    const int64_t c0 = ((int64_t)blockIdx.x * kStatThreads + threadIdx.x) * kStatCols;
    const bool live = c0 < N;  // with vec, c0 + 4 <= N as well
    const int32_t k0 = (int32_t)blockIdx.y * kStatRows;
    const int32_t k1 = k0 + kStatRows < B ? k0 + kStatRows : B;
    int32_t col[kStatCols] = {0, 0, 0, 0};
    for (int32_t k = k0; k < k1; k++) {  // (k and i are the same for the whole block)
        const int32_t i = rows ? rows[k] : k;
        if (i < 0 || i >= n_rows) {
            if (threadIdx.x == 0) *bad = 1;
            continue;
        }
        int32_t e = 0;
        if (live) {
            const uint32_t h = load4(hard + (size_t)k * N, c0, N, vec);
            if (re_decode) {
                const uint32_t cd = load4(reinterpret_cast<const uint8_t*>(codes) + (size_t)i * N, c0, N, vec);
#pragma unroll
                for (int c = 0; c < kStatCols; c++)
                    col[c] += ((h >> (8 * c)) & 0xffu) != ((cd >> (8 * c + 7)) & 1u);  // the code's sign bit
            }
            if (truth) {
                const uint32_t d = h ^ load4(truth + (size_t)i * N, c0, N, vec);
#pragma unroll
                for (int c = 0; c < kStatCols; c++) e += ((d >> (8 * c)) & 0xffu) != 0;
            }
        }
        if (truth) {
            for (int o = 32; o > 0; o >>= 1) e += __shfl_down(e, o, 64);
            if ((threadIdx.x & 63) == 0 && e) atomicAdd(&errors[k], e);
        }
    }
    if (live && re_decode)
        for (int c = 0; c < kStatCols; c++)
            if (c0 + c < N && col[c]) atomicAdd(&re_decode[c0 + c], col[c]);
}

constexpr int kCopyThreads = 256;
constexpr int kCopyBytes = 16;  // per thread

// Bytes [x * 4096, x * 4096 + 4096) of one row: 16 per thread, as one uint4
// when `vec` (N % 16 == 0 and both matrices 16-byte aligned, so every row is),
// else byte by byte.
__device__ __forceinline__ void copy_row_piece(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int32_t N,
                                               bool vec)
{
    const int64_t o = ((int64_t)blockIdx.x * kCopyThreads + threadIdx.x) * kCopyBytes;
    if (o >= N) return;
    if (vec) {
        *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(src + o);
        return;
    }
    for (int c = 0; c < kCopyBytes && o + c < N; c++) dst[o + c] = src[o + c];
}

// out[k] = src[rows[k]] for k = blockIdx.y < F; src has n_rows rows.
__global__ void __launch_bounds__(kCopyThreads) k_trial_gather(const uint8_t* __restrict__ src,
                                                               const int32_t* __restrict__ rows, int32_t n_rows,
                                                               int32_t N, int32_t vec, uint8_t* __restrict__ out,
                                                               int32_t* __restrict__ bad)
{
    const int32_t k = (int32_t)blockIdx.y, i = rows[k];
    if (i < 0 || i >= n_rows) {
        if (threadIdx.x == 0) *bad = 1;
        return;
    }
    copy_row_piece(src + (size_t)i * N, out + (size_t)k * N, N, vec != 0);
}

// dst[rows[pos[q]]] = batch[pos[q]] for q = blockIdx.y; batch has F rows, dst n_rows.
__global__ void __launch_bounds__(kCopyThreads) k_trial_scatter(const uint8_t* __restrict__ batch,
                                                                const int32_t* __restrict__ rows,
                                                                const int32_t* __restrict__ pos, int32_t F,
                                                                int32_t n_rows, int32_t N, int32_t vec,
                                                                uint8_t* __restrict__ dst, int32_t* __restrict__ bad)
{
    const int32_t k = pos[blockIdx.y];
    if (k < 0 || k >= F) {
        if (threadIdx.x == 0) *bad = 1;
        return;
    }
    const int32_t i = rows[k];
    if (i < 0 || i >= n_rows) {
        if (threadIdx.x == 0) *bad = 1;
        return;
    }
    copy_row_piece(batch + (size_t)k * N, dst + (size_t)i * N, N, vec != 0);
}

// The 16 code bytes of a thread of the copy grid, from byte o of a row: one
// uint4 when `vec`, else the bytes below N one by one (others 0).
__device__ __forceinline__ void load16(const uint8_t* __restrict__ row, int64_t o, int32_t N, bool vec, uint32_t w[4])
{
    if (vec) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + o);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        return;
    }
    for (int d = 0; d < 4; d++) w[d] = 0;
#pragma unroll
    for (int c = 0; c < kCopyBytes; c++)
        if (o + c < N) w[c >> 2] |= (uint32_t)row[o + c] << (8 * (c & 3));
}

// The largest |code| of 16 code bytes, as int32 (-128 gives 128).
__device__ __forceinline__ int32_t absmax16(const uint32_t w[4])
{
    int32_t m = 0;
#pragma unroll
    for (int c = 0; c < kCopyBytes; c++) {
        const int32_t v = (int32_t)(int8_t)(w[c >> 2] >> (8 * (c & 3)));
        m = max(m, v < 0 ? -v : v);
    }
    return m;
}

// *out = max(*out, the largest |code| of row rows[blockIdx.y]) (rows of codes
// [n_rows][N]; blockIdx.y < F; *out starts at 0): a wave's maximum by
// shuffles, one atomic per wave with a non-zero value.
__global__ void __launch_bounds__(kCopyThreads) k_trial_absmax(const uint8_t* __restrict__ codes,
                                                               const int32_t* __restrict__ rows, int32_t n_rows,
                                                               int32_t N, int32_t vec, int32_t* __restrict__ out,
                                                               int32_t* __restrict__ bad)
{
    const int32_t i = rows[blockIdx.y];  // (the same for the whole block)
    if (i < 0 || i >= n_rows) {
        if (threadIdx.x == 0) *bad = 1;
        return;
    }
    const int64_t o = ((int64_t)blockIdx.x * kCopyThreads + threadIdx.x) * kCopyBytes;
    int32_t m = 0;
    if (o < N) {
        uint32_t w[4];
        load16(codes + (size_t)i * N, o, N, vec != 0, w);
        m = absmax16(w);
    }
    for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_down(m, d, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// The packed batch of a speculated second decode:
// out[j * F + f] = src[rows[f]] with K + j * (2K + 1) - 128 added to every
// code, for f = blockIdx.y < F and j < k; out has at least k * F rows.  A
// thread loads its 16 bytes once and stores them k times.  The add is per
// byte, on packed dwords without a carry between bytes.  |code| > K cannot
// occur when K is the rows' maximum; it would pick a wrong slice of the table,
// so it is checked and reported as *bad = 2.
__global__ void __launch_bounds__(kCopyThreads) k_trial_gather_spec(const uint8_t* __restrict__ src,
                                                                    const int32_t* __restrict__ rows, int32_t F,
                                                                    int32_t k, int32_t K, int32_t n_rows, int32_t N,
                                                                    int32_t vec, uint8_t* __restrict__ out,
                                                                    int32_t* __restrict__ bad)
{
    const int32_t f = (int32_t)blockIdx.y, i = rows[f];
    if (i < 0 || i >= n_rows) {
        if (threadIdx.x == 0) *bad = 1;
        return;
    }
    const int64_t o = ((int64_t)blockIdx.x * kCopyThreads + threadIdx.x) * kCopyBytes;
    if (o >= N) return;
    uint32_t w[4];
    load16(src + (size_t)i * N, o, N, vec != 0, w);
    if (absmax16(w) > K) *bad = 2;
    for (int32_t j = 0; j < k; j++) {
        const uint32_t s = (uint32_t)((K + j * (2 * K + 1) - 128) & 0xff) * 0x01010101u;
        uint32_t r[4];
#pragma unroll
        for (int d = 0; d < 4; d++)  // bytes of w + bytes of s, mod 256 each
            r[d] = ((w[d] & 0x7f7f7f7fu) + (s & 0x7f7f7f7fu)) ^ ((w[d] ^ s) & 0x80808080u);
        uint8_t* dst = out + ((size_t)j * F + f) * N + o;
        if (vec) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int c = 0; c < kCopyBytes; c++)
                if (o + c < N) dst[c] = (uint8_t)(r[c >> 2] >> (8 * (c & 3)));
        }
    }
}

}  // namespace
}  // namespace ldpc

// The handle: everything a run needs on the device, allocated once.
struct ldpc_trial {
    const ldpc::HostGraph* g = nullptr;
    int32_t device = 0, algo = 0, n_cw = 0, N = 0;
    bool genie = false;
    int32_t B = 0, F = 0;      // rows of the current run; rows of its last second-decode batch
    ldpc::Engine eng;
    ldpc::Event planned;       // null stream -> engine stream
    ldpc::dev_ptr<uint8_t> truth, hard, valid, bhard, bvalid;
    ldpc::dev_ptr<int8_t> codes, bcodes;
    ldpc::dev_ptr<int32_t> iters, biters, errors, re_decode, rows, pos;
    ldpc::dev_ptr<int32_t> ctl;  // [0] a failed range check, [1] the code kernel's overflow word
    bool batch = false;          // the last decode went to bhard / bvalid
    // speculated second decodes (ldpc_trial_set_speculation)
    int32_t steps = 0;           // 0: off
    int64_t cap = 0;             // rows of the batch buffers: n_cw, or ceil64(n_cw) once speculation was enabled
    ldpc::dev_ptr<int32_t> kmax; // k_trial_absmax's word (allocated when speculation is first enabled)
    ldpc_trial_counters counters{};  // of the last run
    // the sequencing channel (ldpc_trial_set_strands / ldpc_trial_run_sim): the strands, uploaded once, and
    // the reads of the last run, grown on demand and reused
    int32_t strand_nt = 0;       // 0: no strands set
    ldpc::dev_ptr<uint8_t> strands, sim_reads;
    ldpc::dev_ptr<int64_t> sim_off;
    ldpc::dev_ptr<int32_t> sim_len, sim_q, sim_qval, sim_bad;
    ldpc::dev_ptr<uint32_t> sim_qlo;
    size_t sim_cap_reads = 0, sim_cap_bytes = 0;

    ~ldpc_trial()
    {
        (void)hipSetDevice(device);
        if (eng.stream) (void)hipStreamSynchronize(eng.stream.get());
    }
};

namespace ldpc {
namespace {

constexpr int64_t kTrialPoolMax = 1024;  // host_decode.cpp's kExplicitPoolMax: shards up to here get a pool of their size

// The device backend of trial::run.
struct TrialDev {
    ldpc_trial& t;
    hipStream_t s;
    explicit TrialDev(ldpc_trial& tr) : t(tr), s(tr.eng.stream.get()) {}
    bool has_truth() const { return t.genie; }
    bool vec16() const { return t.N % 16 == 0; }  // (hipMalloc's bases are 256-byte aligned)
    // the flag word, after the stream has been waited for
    int check_flag(const char* what)
    {
        int32_t bad = 0;
        LDPC_HIP(hipMemcpyAsync(&bad, t.ctl.get(), sizeof bad, hipMemcpyDeviceToHost, s));
        if (int rc = t.eng.sync()) return rc;
        if (bad) {
            set_error(std::string(bad == 2 ? "ldpc_trial: a code is larger than the rows' maximum in "
                                           : "ldpc_trial: a row index failed its range check in ") + what);
            return LDPC_ERR_DEVICE;
        }
        return LDPC_OK;
    }
    dim3 copy_grid(int64_t rows) const
    {
        return dim3((unsigned)(((int64_t)t.N + kCopyThreads * kCopyBytes - 1) / (kCopyThreads * kCopyBytes)),
                    (unsigned)rows);
    }
    int absmax(const int32_t* rows, int64_t F, int32_t* K)
    {
        LDPC_HIP(hipMemcpyAsync(t.rows.get(), rows, sizeof(int32_t) * (size_t)F, hipMemcpyHostToDevice, s));
        LDPC_HIP(hipMemsetAsync(t.kmax.get(), 0, sizeof(int32_t), s));
        if (int rc = launch(k_trial_absmax, copy_grid(F), dim3(kCopyThreads), 0, s,
                            reinterpret_cast<const uint8_t*>(t.codes.get()), t.rows.get(), t.B, t.N, (int32_t)vec16(),
                            t.kmax.get(), t.ctl.get()))
            return rc;
        LDPC_HIP(hipMemcpyAsync(K, t.kmax.get(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
        return check_flag("k_trial_absmax");
    }
    int decode_spec(const int32_t* rows, int64_t F, int64_t k, int32_t K, const double* table, int32_t max_iter)
    {
        const int64_t B = k * F;
        if (B > t.cap) {  // (k * F <= lanes64(F) <= ceil64(n_cw) by the rule)
            set_error("ldpc_trial: a speculated batch exceeds the handle's batch buffers");
            return LDPC_ERR_ARG;
        }
        t.batch = true;
        t.F = (int32_t)B;
        LDPC_HIP(hipMemcpyAsync(t.rows.get(), rows, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, s));
        if (int rc = launch(k_trial_gather_spec, copy_grid(F), dim3(kCopyThreads), 0, s,
                            reinterpret_cast<const uint8_t*>(t.codes.get()), t.rows.get(), (int32_t)F, (int32_t)k, K, t.B,
                            t.N, (int32_t)vec16(), reinterpret_cast<uint8_t*>(t.bcodes.get()), t.ctl.get()))
            return rc;
        return t.eng.decode_codes(t.bcodes.get(), table, LDPC_IN_LLR, B, max_iter, t.bhard.get(), nullptr,
                                  LDPC_POST_LLR, t.biters.get(), t.bvalid.get());
    }
    int decode(const int32_t* rows, int64_t B, const double* table, int32_t max_iter)
    {
        t.batch = rows != nullptr;
        if (!rows)
            return t.eng.decode_codes(t.codes.get(), table, LDPC_IN_LLR, B, max_iter, t.hard.get(), nullptr,
                                      LDPC_POST_LLR, t.iters.get(), t.valid.get());
        t.F = (int32_t)B;
        // (rows stays as it is until the stats call that follows has waited for the stream)
        LDPC_HIP(hipMemcpyAsync(t.rows.get(), rows, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, s));
        if (int rc = launch(k_trial_gather, copy_grid(B), dim3(kCopyThreads), 0, s,
                            reinterpret_cast<const uint8_t*>(t.codes.get()), t.rows.get(), t.B, t.N, (int32_t)vec16(),
                            reinterpret_cast<uint8_t*>(t.bcodes.get()), t.ctl.get()))
            return rc;
        return t.eng.decode_codes(t.bcodes.get(), table, LDPC_IN_LLR, B, max_iter, t.bhard.get(), nullptr,
                                  LDPC_POST_LLR, t.biters.get(), t.bvalid.get());
    }
    int stats(const int32_t* rows, int64_t B, int32_t* errors, uint8_t* valid, int32_t* re_decode)
    {
        LDPC_HIP(hipMemsetAsync(t.errors.get(), 0, sizeof(int32_t) * (size_t)B, s));
        if (re_decode) LDPC_HIP(hipMemsetAsync(t.re_decode.get(), 0, sizeof(int32_t) * (size_t)t.N, s));
        const dim3 grid((unsigned)(((int64_t)t.N + kStatThreads * kStatCols - 1) / (kStatThreads * kStatCols)),
                        (unsigned)((B + kStatRows - 1) / kStatRows));
        if (int rc = launch(k_trial_stats, grid, dim3(kStatThreads), 0, s, t.batch ? t.bhard.get() : t.hard.get(),
                            t.codes.get(), t.genie ? t.truth.get() : nullptr, rows ? t.rows.get() : nullptr, (int32_t)B,
                            t.B, t.N, t.errors.get(), re_decode ? t.re_decode.get() : nullptr, t.ctl.get()))
            return rc;
        LDPC_HIP(hipMemcpyAsync(errors, t.errors.get(), sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, s));
        LDPC_HIP(hipMemcpyAsync(valid, (t.batch ? t.bvalid : t.valid).get(), (size_t)B, hipMemcpyDeviceToHost, s));
        if (re_decode)
            LDPC_HIP(hipMemcpyAsync(re_decode, t.re_decode.get(), sizeof(int32_t) * (size_t)t.N,
                                    hipMemcpyDeviceToHost, s));
        return check_flag("k_trial_stats / k_trial_gather");  // (or k_trial_gather_spec)
    }
    int keep(const int32_t* rows, const int32_t* pos, int64_t n)
    {
        (void)rows;  // on the device since this decode's gather
        LDPC_HIP(hipMemcpyAsync(t.pos.get(), pos, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
        if (int rc = launch(k_trial_scatter, copy_grid(n), dim3(kCopyThreads), 0, s, t.bhard.get(), t.rows.get(),
                            t.pos.get(), t.F, t.B, t.N, (int32_t)vec16(), t.hard.get(), t.ctl.get()))
            return rc;
        return check_flag("k_trial_scatter");
    }
};

int trial_create(const ldpc_graph* g, int32_t device, int32_t algo, int32_t n_cw, const uint8_t* codewords,
                 const ldpc_schedule* schedule, std::unique_ptr<ldpc_trial>& out)
{
    if (!g) { set_error("ldpc_trial_create: null graph"); return LDPC_ERR_ARG; }
    if (algo != LDPC_ALGO_BP && algo != LDPC_ALGO_MSA) {
        set_error("ldpc_trial_create: algo must be LDPC_ALGO_BP or LDPC_ALGO_MSA");
        return LDPC_ERR_ARG;
    }
    const int64_t N = g->h.N;
    if (n_cw < 1 || N < 1 || (int64_t)n_cw > INT64_MAX / 8 / N) {
        set_error("ldpc_trial_create: n_cw must be >= 1 (and n_cw * N addressable)");
        return LDPC_ERR_ARG;
    }
    if (n_cw > 65535) {  // one grid row per codeword of a second decode
        set_error("ldpc_trial_create: more than 65535 codewords per trial are not supported");
        return LDPC_ERR_UNSUPPORTED;
    }
    auto t = std::make_unique<ldpc_trial>();
    t->g = &g->h;
    t->device = device;
    t->algo = algo;
    t->n_cw = n_cw;
    t->N = (int32_t)N;
    t->genie = codewords != nullptr;
    t->cap = n_cw;
    int rc;
    if ((rc = select_device("ldpc_trial_create", device))) return rc;
    const int64_t pool = n_cw <= kTrialPoolMax ? ((int64_t)n_cw + 63) / 64 * 64 : 0;
    if ((rc = t->eng.init(t->g, device, algo, pool, schedule))) return rc;
    const size_t n = (size_t)n_cw, mat = n * (size_t)N;
    if ((t->genie && (rc = upload(t->truth, codewords, mat))) || (rc = dev_alloc(t->codes, mat)) ||
        (rc = dev_alloc(t->bcodes, mat)) || (rc = dev_alloc(t->hard, mat)) || (rc = dev_alloc(t->bhard, mat)) ||
        (rc = dev_alloc(t->valid, n)) || (rc = dev_alloc(t->bvalid, n)) || (rc = dev_alloc(t->iters, n)) ||
        (rc = dev_alloc(t->biters, n)) || (rc = dev_alloc(t->errors, n)) || (rc = dev_alloc(t->re_decode, (size_t)N)) ||
        (rc = dev_alloc(t->rows, n)) || (rc = dev_alloc(t->pos, n)) || (rc = dev_alloc(t->ctl, 2)) ||
        (rc = make_event(t->planned)))
        return rc;
    out = std::move(t);
    return LDPC_OK;
}

// The control flow over the handle's code matrix (rows [0, B) are in place,
// enqueued on the engine's stream), and the outputs that stay on the device.
int trial_run(ldpc_trial& t, int32_t B, double eps, int32_t max_iter, int32_t faithful, ldpc_trial_result* out)
{
    t.B = B;
    t.counters = ldpc_trial_counters{};
    TrialDev be(t);
    if (int rc = trial::run_spec(be, B, t.N, eps, max_iter, faithful != 0, t.steps, out, &t.counters)) return rc;
    hipStream_t s = be.s;
    if (out->hard) LDPC_HIP(hipMemcpyAsync(out->hard, t.hard.get(), (size_t)B * (size_t)t.N, hipMemcpyDeviceToHost, s));
    if (out->iters) LDPC_HIP(hipMemcpyAsync(out->iters, t.iters.get(), sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, s));
    if (out->valid) LDPC_HIP(hipMemcpyAsync(out->valid, t.valid.get(), (size_t)B, hipMemcpyDeviceToHost, s));
    return t.eng.sync();
}

// With steps on for the first time: the batch buffers regrown to ceil64(n_cw)
// rows (a speculated batch fills the tiles its list occupies) and the word of
// k_trial_absmax.  The handle changes only when every allocation succeeded.
int trial_set_speculation(ldpc_trial* t, int32_t steps)
{
    if (!t || steps < -1) {
        set_error("ldpc_trial_set_speculation: null handle, or steps below -1");
        return LDPC_ERR_ARG;
    }
    if (steps != 0 && steps != 1 && !t->kmax) {
        LDPC_HIP(hipSetDevice(t->device));
        LDPC_HIP(hipStreamSynchronize(t->eng.stream.get()));
        const size_t cap = (size_t)trial::lanes64(t->n_cw), mat = cap * (size_t)t->N;
        dev_ptr<int8_t> bcodes;
        dev_ptr<uint8_t> bhard, bvalid;
        dev_ptr<int32_t> biters, errors, rows, pos, kmax;
        int rc;
        if ((rc = dev_alloc(bcodes, mat)) || (rc = dev_alloc(bhard, mat)) || (rc = dev_alloc(bvalid, cap)) ||
            (rc = dev_alloc(biters, cap)) || (rc = dev_alloc(errors, cap)) || (rc = dev_alloc(rows, cap)) ||
            (rc = dev_alloc(pos, cap)) || (rc = dev_alloc(kmax, 1)))
            return rc;
        t->bcodes = std::move(bcodes);
        t->bhard = std::move(bhard);
        t->bvalid = std::move(bvalid);
        t->biters = std::move(biters);
        t->errors = std::move(errors);
        t->rows = std::move(rows);
        t->pos = std::move(pos);
        t->kmax = std::move(kmax);
        t->cap = (int64_t)cap;
    }
    t->steps = steps;
    return LDPC_OK;
}

int trial_run_codes(ldpc_trial* t, const int8_t* codes, int64_t B, double eps, int32_t max_iter, int32_t faithful,
                    ldpc_trial_result* out)
{
    const std::string who = "ldpc_trial_run_codes: ";
    if (!t || !codes) { set_error(who + "null handle or codes"); return LDPC_ERR_ARG; }
    if (B < 1 || B > t->n_cw) { set_error(who + "B must be in 1 .. n_cw"); return LDPC_ERR_ARG; }
    const std::string err = trial::check_args(B, t->N, eps, max_iter, out);
    if (!err.empty()) { set_error(who + err); return LDPC_ERR_ARG; }
    LDPC_HIP(hipSetDevice(t->device));
    hipStream_t s = t->eng.stream.get();
    LDPC_HIP(hipMemsetAsync(t->ctl.get(), 0, 2 * sizeof(int32_t), s));
    LDPC_HIP(hipMemcpyAsync(t->codes.get(), codes, (size_t)B * (size_t)t->N, hipMemcpyHostToDevice, s));
    LDPC_HIP(hipStreamSynchronize(s));  // the caller's buffer is free whichever way the call ends
    out->codes_exact = 1;
    out->t_llr_s = 0.0;
    return trial_run(*t, (int32_t)B, eps, max_iter, faithful, out);
}

// The argument checks every reads-to-result call shares.
int trial_reads_args(const ldpc_trial* t, const std::string& who, const plan::Args& a, double eps, int32_t max_iter,
                     const ldpc_trial_result* out)
{
    if (!t) { set_error(who + ": null handle"); return LDPC_ERR_ARG; }
    const std::string err = trial::check_args(t->n_cw, t->N, eps, max_iter, out);
    if (!err.empty()) { set_error(who + ": " + err); return LDPC_ERR_ARG; }
    if (a.payload_nt < 1 || 2 * (int64_t)a.payload_nt != t->n_cw || a.n_strands != t->N) {
        set_error(who + ": needs 2 * payload_nt == n_cw and n_strands == N");
        return LDPC_ERR_ARG;
    }
    return LDPC_OK;
}

// Planner (reads from the host, or device-resident with `src`), code kernel
// into the handle's code matrix, trial.  t0: when the call's LLR stage began.
int trial_plan_run(ldpc_trial* t, const std::string& who, const plan::Args& a, const PlanSrc* src,
                   std::chrono::steady_clock::time_point t0, int64_t workspace_bytes, double eps, int32_t max_iter,
                   int32_t faithful, ldpc_trial_result* out)
{
    PlanDev pd;
    if (int rc = plan_device(who, a, false, t->device, workspace_bytes, &pd, src)) return rc;
    // the planner's kernels ran on the null stream: the engine's stream waits for them
    hipStream_t s = t->eng.stream.get();
    LDPC_HIP(hipEventRecord(t->planned.get(), nullptr));
    LDPC_HIP(hipStreamWaitEvent(s, t->planned.get(), 0));
    LDPC_HIP(hipMemsetAsync(t->ctl.get(), 0, 2 * sizeof(int32_t), s));
    const dim3 grid((unsigned)((a.n_strands + 255) / 256), (unsigned)a.payload_nt);
    if (int rc = launch(k_dna_codes, grid, dim3(256), 0, s, pd.kind.get(), pd.row_ptr.get(), pd.rows.get(),
                        pd.row_q.get(), a.n_strands, a.payload_nt, t->codes.get(), t->ctl.get() + 1))
        return rc;
    int32_t ov = 0;
    LDPC_HIP(hipMemcpyAsync(&ov, t->ctl.get() + 1, sizeof ov, hipMemcpyDeviceToHost, s));
    LDPC_HIP(hipStreamSynchronize(s));  // the plan is released below; ov is read
    out->codes_exact = ov ? 0 : 1;
    out->t_llr_s = trial::seconds_since(t0);
    if (ov) {
        set_error(who + ": a count difference is outside int8 (codes_exact = 0): the resident trial cannot "
                        "represent this input; use ldpc_dna_reads_llr and the fp64 decode");
        return LDPC_ERR_UNSUPPORTED;
    }
    return trial_run(*t, t->n_cw, eps, max_iter, faithful, out);
}

int trial_run_reads(ldpc_trial* t, const plan::Args& a, int64_t workspace_bytes, double eps, int32_t max_iter,
                    int32_t faithful, ldpc_trial_result* out)
{
    const std::string who = "ldpc_trial_run_reads";
    if (int rc = trial_reads_args(t, who, a, eps, max_iter, out)) return rc;
    return trial_plan_run(t, who, a, nullptr, std::chrono::steady_clock::now(), workspace_bytes, eps, max_iter,
                          faithful, out);
}

int trial_set_strands(ldpc_trial* t, const uint8_t* strands, int64_t n_strands, int32_t strand_nt)
{
    const std::string who = "ldpc_trial_set_strands: ";
    if (!t) { set_error(who + "null handle"); return LDPC_ERR_ARG; }
    if (n_strands != t->N || 2 * ((int64_t)strand_nt - rs::kPrefixNt) != t->n_cw) {
        set_error(who + "needs n_strands == N and 2 * (strand_nt - 16) == n_cw");
        return LDPC_ERR_ARG;
    }
    const std::string err = sim::check_strands(strands, n_strands, strand_nt);
    if (!err.empty()) { set_error(who + err); return LDPC_ERR_ARG; }
    LDPC_HIP(hipSetDevice(t->device));
    int rc;
    dev_ptr<uint8_t> d;
    if ((rc = upload(d, strands, (size_t)n_strands * (size_t)strand_nt))) return rc;
    if (!t->sim_qval && ((rc = dev_alloc(t->sim_qval, (size_t)sim::kMaxQuals)) ||
                         (rc = dev_alloc(t->sim_qlo, (size_t)sim::kMaxQuals)) || (rc = dev_alloc(t->sim_bad, 1))))
        return rc;
    t->strands = std::move(d);
    t->strand_nt = strand_nt;
    return LDPC_OK;
}

struct SimCall {
    uint64_t seed;
    int64_t r0, n_reads, t_sub, t_ins, t_del;
    const int32_t* q_val;
    const uint32_t* q_lo;
    int32_t nq;
};

// The channel's reads of [r0, r0 + n_reads) into the handle's buffers (null
// stream), then ldpc_trial_run_reads from the planner on with those as its source.
int trial_run_sim(ldpc_trial* t, const SimCall& c, const int32_t* strand_index_vals, int32_t align,
                  int64_t workspace_bytes, double eps, int32_t max_iter, int32_t faithful, ldpc_trial_result* out)
{
    const std::string who = "ldpc_trial_run_sim";
    if (!t) { set_error(who + ": null handle"); return LDPC_ERR_ARG; }
    if (t->strand_nt == 0) { set_error(who + ": no strands set (ldpc_trial_set_strands)"); return LDPC_ERR_ARG; }
    const plan::Args a{nullptr, nullptr, nullptr, nullptr, c.n_reads, nullptr, strand_index_vals, t->N,
                       t->strand_nt - rs::kPrefixNt, align, out ? out->kind : nullptr, nullptr, nullptr, nullptr,
                       out ? out->stats : nullptr};
    if (int rc = trial_reads_args(t, who, a, eps, max_iter, out)) return rc;
    const std::string err = sim::check_channel(t->strand_nt, c.r0, c.n_reads, c.t_sub, c.t_ins, c.t_del, c.q_val,
                                               c.q_lo, c.nq);
    if (!err.empty()) { set_error(who + ": " + err); return LDPC_ERR_ARG; }
    if (c.n_reads > INT32_MAX - 1024) {
        set_error(who + ": too many reads for one call");
        return LDPC_ERR_UNSUPPORTED;
    }
    const auto t0 = std::chrono::steady_clock::now();
    LDPC_HIP(hipSetDevice(t->device));
    const size_t n = (size_t)c.n_reads, bytes = n * (size_t)sim::stride(t->strand_nt);
    int rc;
    if (n > t->sim_cap_reads) {
        t->sim_cap_reads = 0;
        if ((rc = dev_alloc(t->sim_off, n)) || (rc = dev_alloc(t->sim_len, n)) || (rc = dev_alloc(t->sim_q, n)))
            return rc;
        t->sim_cap_reads = n;
    }
    if (bytes > t->sim_cap_bytes) {
        t->sim_cap_bytes = 0;
        if ((rc = dev_alloc(t->sim_reads, bytes))) return rc;
        t->sim_cap_bytes = bytes;
    }
    LDPC_HIP(hipMemcpy(t->sim_qval.get(), c.q_val, sizeof(int32_t) * (size_t)c.nq, hipMemcpyHostToDevice));
    LDPC_HIP(hipMemcpy(t->sim_qlo.get(), c.q_lo, sizeof(uint32_t) * (size_t)c.nq, hipMemcpyHostToDevice));
    LDPC_HIP(hipMemsetAsync(t->sim_bad.get(), 0, sizeof(int32_t), nullptr));
    if (n > 0 && (rc = launch_sim_reads(t->strands.get(), t->N, t->strand_nt, c.seed, c.r0, c.n_reads, c.t_sub,
                                        c.t_ins, c.t_del, t->sim_qval.get(), t->sim_qlo.get(), c.nq,
                                        t->sim_reads.get(), t->sim_off.get(), t->sim_len.get(), t->sim_q.get(),
                                        nullptr, t->sim_bad.get())))
        return rc;
    const PlanSrc src{t->sim_reads.get(), t->sim_off.get(), t->sim_len.get(), t->sim_q.get(), (int64_t)bytes,
                      t->sim_bad.get()};
    return trial_plan_run(t, who, a, &src, t0, workspace_bytes, eps, max_iter, faithful, out);
}

}  // namespace
}  // namespace ldpc

extern "C" {

int ldpc_dna_trial_host(const int8_t* codes, int32_t n_cw, int32_t N, const uint8_t* codewords,
                        ldpc_trial_decode_fn decode, void* user, double eps, int32_t max_iter, int32_t faithful,
                        ldpc_trial_result* out)
{
    return ldpc::dna_guard("ldpc_dna_trial_host", [&] {
        std::string err;
        const int rc = ldpc::trial::run_host(codes, n_cw, N, codewords, decode, user, eps, max_iter, faithful, out, &err);
        if (rc) set_error("ldpc_dna_trial_host: " + err);
        return rc;
    });
}

int ldpc_dna_trial_host_spec(const int8_t* codes, int32_t n_cw, int32_t N, const uint8_t* codewords,
                             ldpc_trial_decode_fn decode, void* user, double eps, int32_t max_iter, int32_t faithful,
                             ldpc_trial_result* out, int32_t steps, ldpc_trial_counters* counters)
{
    return ldpc::dna_guard("ldpc_dna_trial_host_spec", [&] {
        std::string err;
        const int rc = ldpc::trial::run_host_spec(codes, n_cw, N, codewords, decode, user, eps, max_iter, faithful,
                                                  steps, counters, out, &err);
        if (rc) set_error("ldpc_dna_trial_host_spec: " + err);
        return rc;
    });
}

ldpc_trial* ldpc_trial_create(const ldpc_graph* g, int32_t device, int32_t algo, int32_t n_cw,
                              const uint8_t* codewords, const ldpc_schedule* schedule, int* err)
{
    std::unique_ptr<ldpc_trial> t;
    const int rc = ldpc::dna_guard("ldpc_trial_create",
                                     [&] { return ldpc::trial_create(g, device, algo, n_cw, codewords, schedule, t); });
    if (err) *err = rc;
    return rc ? nullptr : t.release();
}

void ldpc_trial_free(ldpc_trial* t) { delete t; }

int ldpc_trial_run_reads(ldpc_trial* t, const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths,
                         const int32_t* quals, int64_t n_reads, const int32_t* index_vals, const int32_t* strands,
                         int32_t n_strands, int32_t payload_nt, int32_t align, int64_t workspace_bytes, double eps,
                         int32_t max_iter, int32_t faithful, ldpc_trial_result* out)
{
    return ldpc::dna_guard("ldpc_trial_run_reads", [&] {
        return ldpc::trial_run_reads(t, plan_args(seqs, offsets, lengths, quals, n_reads, index_vals, strands, n_strands,
                                                  payload_nt, align, out ? out->kind : nullptr, nullptr, nullptr,
                                                  nullptr, out ? out->stats : nullptr),
                                     workspace_bytes, eps, max_iter, faithful, out);
    });
}

int ldpc_trial_set_strands(ldpc_trial* t, const uint8_t* strands, int64_t n_strands, int32_t strand_nt)
{
    return ldpc::dna_guard("ldpc_trial_set_strands",
                             [&] { return ldpc::trial_set_strands(t, strands, n_strands, strand_nt); });
}

int ldpc_trial_run_sim(ldpc_trial* t, uint64_t seed, int64_t r0, int64_t n_reads, int64_t t_sub, int64_t t_ins,
                       int64_t t_del, const int32_t* q_val, const uint32_t* q_lo, int32_t nq,
                       const int32_t* strand_index_vals, int32_t align, int64_t workspace_bytes, double eps,
                       int32_t max_iter, int32_t faithful, ldpc_trial_result* out)
{
    return ldpc::dna_guard("ldpc_trial_run_sim", [&] {
        return ldpc::trial_run_sim(t, ldpc::SimCall{seed, r0, n_reads, t_sub, t_ins, t_del, q_val, q_lo, nq},
                                   strand_index_vals, align, workspace_bytes, eps, max_iter, faithful, out);
    });
}

int ldpc_trial_run_codes(ldpc_trial* t, const int8_t* codes, int64_t B, double eps, int32_t max_iter,
                         int32_t faithful, ldpc_trial_result* out)
{
    return ldpc::dna_guard("ldpc_trial_run_codes",
                             [&] { return ldpc::trial_run_codes(t, codes, B, eps, max_iter, faithful, out); });
}

int ldpc_trial_set_speculation(ldpc_trial* t, int32_t steps)
{
    return ldpc::dna_guard("ldpc_trial_set_speculation", [&] { return ldpc::trial_set_speculation(t, steps); });
}

int ldpc_trial_get_counters(const ldpc_trial* t, ldpc_trial_counters* out)
{
    if (!t || !out) {
        set_error("ldpc_trial_get_counters: null handle or counters");
        return LDPC_ERR_ARG;
    }
    *out = t->counters;
    return LDPC_OK;
}

int ldpc_trial_read_codes(ldpc_trial* t, int8_t* codes, int64_t B)
{
    if (!t || !codes || B < 0 || B > t->n_cw) {
        set_error("ldpc_trial_read_codes: bad arguments");
        return LDPC_ERR_ARG;
    }
    LDPC_HIP(hipSetDevice(t->device));
    hipStream_t s = t->eng.stream.get();
    LDPC_HIP(hipMemcpyAsync(codes, t->codes.get(), (size_t)B * (size_t)t->N, hipMemcpyDeviceToHost, s));
    LDPC_HIP(hipStreamSynchronize(s));
    return LDPC_OK;
}

}  // extern "C"
