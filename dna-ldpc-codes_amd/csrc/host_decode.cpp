// host_decode.cpp -- ldpc_decode / ldpc_decode_codes: host buffers in, host
// buffers out.
//
// Host side of the drop-in for ldpc.exe: a per-graph pool of device engines +
// pinned staging buffers (so repeated calls from decoder.py do not
// re-allocate), host-side exp() exactly as the reference (DNA_main.cpp:1344),
// and one host thread per GPU for multi-device calls -- contiguous codeword
// shards, no collective (the reference's dormant per-rank frame split,
// DNA_main.cpp:629-651, with its MPI_Reduce of counters, DNA_main.cpp:1187-1193,
// reduced to a host gather).
#include "host_decode.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>

#include "host_simd.hpp"

namespace ldpc {

constexpr int kMaxDevices = 64;       // opts.n_devices bound (one host thread per device)
constexpr int kMaxHostThreads = 256;  // opts.host_threads clamp
// shards up to this many codewords get a lane pool holding all of them
// (the 272-codeword DNA batch: 248k cw/s grouped vs 194k through the
// resident pool); larger ones use the engine's own pool
constexpr int64_t kExplicitPoolMax = 1024;
constexpr int64_t kXferChunk = 4096;  // codewords per PCIe chunk (at least); shards of <= kExplicitPoolMax
                                      // cross in one chunk (A/B on the DNA batch: chunks of 128 or 192
                                      // within noise of one, 64 slower)

// Persistent host workers (one set per device context): the host-side passes
// over a chunk (exp, LLR encoding, copies) split into `n` row ranges, run by
// the workers and the calling thread, with no thread creation per call.
class Workers {
  public:
    explicit Workers(int n) : n_(std::max(1, n))
    {
        for (int t = 1; t < n_; t++) th_.emplace_back([this, t] { loop(t); });
    }
    ~Workers()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    int size() const { return n_; }
    // f(t) for t = 0..n_-1, t = 0 on the calling thread; returns when all are
    // done.  Callers on different threads take turns.
    void run(const std::function<void(int)>& f)
    {
        if (n_ == 1) { f(0); return; }
        std::lock_guard<std::mutex> turn(run_mu_);
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &f;
            left_ = n_ - 1;
            gen_++;
        }
        cv_.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return left_ == 0; });
        job_ = nullptr;
    }

  private:
    void loop(int t)
    {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)>* f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                f = job_;
            }
            (*f)(t);
            std::lock_guard<std::mutex> lk(mu_);
            if (--left_ == 0) done_.notify_one();
        }
    }
    int n_;
    std::vector<std::thread> th_;
    std::mutex run_mu_, mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* job_ = nullptr;
    int left_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

namespace {

// Code table path (DNA batches): an LLR that is an exact multiple k * unit,
// |k| <= kCodeMax, crosses PCIe as the byte k and the engine decodes the codes
// (Engine::decode_codes) with table[k + 128] = k * unit: BP's LR is the host
// libm's exp of that value -- the same bits as exp(LLR), DNA_main.cpp:1344 --
// and min-sum reads the value itself.
constexpr int kCodeMax = 127;
constexpr int kTable = 256;

// the unit: the smallest nonzero |LLR| among the chunk's first rows (a guess;
// every value is checked against it)
double llr_unit(const double* src, int64_t rows, size_t N)
{
    double u = 0;
    const size_t n = (size_t)std::min<int64_t>(rows, 4) * N;
    for (size_t i = 0; i < n; i++) {
        const double a = std::fabs(src[i]);
        if (a > 0 && std::isfinite(a) && (u == 0 || a < u)) u = a;
    }
    return u;
}

// byte x -> 8 bytes, byte r = bit r of x (unpacking the device's packed hard bits)
struct BitBytes {
    uint64_t t[256];
    BitBytes()
    {
        for (int x = 0; x < 256; x++) {
            uint64_t v = 0;
            for (int r = 0; r < 8; r++) v |= (uint64_t)((x >> r) & 1) << (8 * r);
            t[x] = v;
        }
    }
};
const BitBytes kBitBytes;

// f(r0, r1) over n rows split across the slot's workers
template <typename F>
void parallel_rows(Workers& W, int64_t n, F&& f)
{
    const int T = W.size();
    if (T == 1 || n < 2) { f(0, n); return; }
    W.run([&](int t) {
        const int64_t r0 = n * t / T, r1 = n * (t + 1) / T;
        if (r1 > r0) f(r0, r1);
    });
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

int Stage::init(size_t rows_, size_t N_, bool codes)
{
    rows = rows_;
    N = N_;
    int rc;
    if ((rc = make_event(h2d)) || (rc = make_event(dec)) || (rc = make_event(d2h)) ||
        (rc = pinned_alloc(h_in, rows * N)) || (rc = pinned_alloc(h_hard, rows * N)) ||
        (rc = pinned_alloc(h_iters, rows)) || (rc = pinned_alloc(h_valid, rows)) ||
        (rc = dev_alloc(d_in, rows * N)) || (rc = dev_alloc(d_hard, rows * N)) || (rc = dev_alloc(d_iters, rows)) ||
        (rc = dev_alloc(d_valid, rows)))
        return rc;
    if (N % 8 == 0 && ((rc = pinned_alloc(h_hbits, rows * N / 8)) || (rc = dev_alloc(d_hbits, rows * N / 8)))) return rc;
    return codes ? want_codes() : LDPC_OK;
}

int Stage::want_codes()
{
    if (h_code) return LDPC_OK;
    int rc;
    if ((rc = pinned_alloc(h_code, rows * N)) || (rc = dev_alloc(d_code, rows * N))) return rc;
    table.assign(kTable, 0.0);
    return LDPC_OK;
}

int Stage::want_post()
{
    if (h_post) return LDPC_OK;
    int rc = pinned_alloc(h_post, rows * N);
    return rc ? rc : dev_alloc(d_post, rows * N);
}

Slot::Slot() = default;

Slot::~Slot()
{
    workers.reset();
    if (!eng) return;
    (void)hipSetDevice(device);
    if (copy) (void)hipStreamSynchronize(copy.get());
    if (copy_out) (void)hipStreamSynchronize(copy_out.get());
    if (eng->stream) (void)hipStreamSynchronize(eng->stream.get());
}

static int make_slot(const HostGraph* g, int device, int algo, int64_t pool, int64_t xfer, const ldpc_schedule& sched,
                     std::unique_ptr<Slot>& out)
{
    auto s = std::make_unique<Slot>();
    s->device = device;
    s->algo = algo;
    s->sched = sched;
    s->eng = std::make_unique<Engine>();
    int rc = s->eng->init(g, device, algo, pool, &sched, /*resolved=*/true);
    if (rc) return rc;
    s->pool = pool;
    s->xfer = xfer;
    if ((rc = make_stream(s->copy)) || (rc = make_stream(s->copy_out))) return rc;
    for (Stage& st : s->stage)
        if ((rc = st.init((size_t)xfer, (size_t)g->N, algo == LDPC_ALGO_BP || algo == LDPC_ALGO_MSA))) return rc;
    out = std::move(s);
    return LDPC_OK;
}

}  // namespace ldpc

std::unique_ptr<ldpc::Slot> ldpc_graph::take(int device, int algo, int64_t pool, int64_t xfer, bool small,
                                             const ldpc_schedule& sched)
{
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < free_slots.size(); i++) {
        auto& s = free_slots[i];
        const bool pool_ok = small ? (s->pool >= pool && s->pool <= ldpc::kExplicitPoolMax) : s->pool == pool;
        if (s->device == device && s->algo == algo && pool_ok && s->xfer >= xfer &&
            std::memcmp(&s->sched, &sched, sizeof(sched)) == 0) {
            auto r = std::move(s);
            free_slots.erase(free_slots.begin() + (long)i);
            return r;
        }
    }
    return nullptr;
}

void ldpc_graph::give(std::unique_ptr<ldpc::Slot> s)
{
    std::lock_guard<std::mutex> lk(mu);
    // keep at most a few idle slots per graph
    if (free_slots.size() >= 8) free_slots.erase(free_slots.begin());
    free_slots.push_back(std::move(s));
}

namespace ldpc {
namespace {

// The validated, resolved arguments of one call.
struct HostCall {
    ldpc_graph* g = nullptr;
    HostInput in;
    int64_t B = 0;
    int32_t max_iter = 0, algo = 0;
    uint8_t* hard_out = nullptr;
    double* post_out = nullptr;
    int32_t* iters_out = nullptr;
    uint8_t* valid_out = nullptr;
    ldpc_opts o{};            // the caller's, or the defaults
    int32_t q_prec = 6;       // quantized min-sum parameters: 0 selects the engine defaults (q 6, step 0.5)
    double q_step = 0.5;
    std::vector<int> devs;    // one shard per entry
    int host_threads = 1;     // per shard, for exp / packing
    ldpc_schedule sched{};    // resolved
    bool lr_table = false;
    bool timing = false;      // LDPC_API_TIMING: the only environment variable the library reads, a debug
                              // print of the host-leg split (never changes what is computed)
    bool codes_pinned = false;
    size_t N = 0;
};

// The argument checks, in this order: the first failing one decides the code
// and the message.  B == 0 returns LDPC_OK with nothing resolved.
int validate(const ldpc_graph* gc, const HostInput& in, int64_t B, int32_t max_iter, int32_t algo, uint8_t* hard_out,
             double* post_out, int32_t* iters_out, uint8_t* valid_out, const ldpc_opts* opts, HostCall& c)
{
    ldpc_graph* g = const_cast<ldpc_graph*>(gc);  // the slots are a cache behind g->mu
    if (!g) { set_error("null graph"); return LDPC_ERR_ARG; }
    if (B < 0 || max_iter < 0) { set_error("B and max_iter must be >= 0"); return LDPC_ERR_ARG; }
    if (B > 0 && ((!in.llr && !in.codes) || !hard_out)) { set_error("the channel input and hard_out are required"); return LDPC_ERR_ARG; }
    if (in.codes && !in.table) { set_error("ldpc_decode_codes: null table"); return LDPC_ERR_ARG; }
    if (in.codes && in.table_kind != LDPC_IN_LLR && !(in.table_kind == LDPC_IN_LR && algo == LDPC_ALGO_BP)) {
        set_error("table kind: LDPC_IN_LLR, or LDPC_IN_LR for BP");
        return LDPC_ERR_ARG;
    }
    if (algo < LDPC_ALGO_BP || algo > LDPC_ALGO_GALLAGER_B2) { set_error("unknown algorithm"); return LDPC_ERR_ARG; }
    ldpc_opts& o = c.o;
    o.exp_on_host = 1;
    if (opts) o = *opts;
    c.q_prec = o.msa_precision > 0 ? o.msa_precision : 6;
    c.q_step = o.msa_step > 0 ? o.msa_step : 0.5;
    if (algo == LDPC_ALGO_QMSA && (c.q_prec < 2 || c.q_prec > 16 || o.msa_offset < 0)) {
        set_error("quantized min-sum needs 2 <= msa_precision <= 16 and msa_offset >= 0");
        return LDPC_ERR_ARG;
    }
    if (algo != LDPC_ALGO_BP && post_out && o.post_kind == LDPC_POST_RATIO) {
        set_error("LDPC_POST_RATIO is BP-only");
        return LDPC_ERR_ARG;
    }
    // B [B][N] fp64 values must be addressable (the host code forms B * N * 8)
    if (B > (int64_t)(PTRDIFF_MAX / 8) / (int64_t)std::max<int32_t>(1, g->h.N)) {
        set_error("batch too large: B * N * 8 bytes overflow the address space");
        return LDPC_ERR_ARG;
    }
    if (o.n_devices > kMaxDevices) {
        set_error("opts.n_devices above " + std::to_string(kMaxDevices));
        return LDPC_ERR_ARG;
    }
    if (B == 0) return LDPC_OK;

    const int ndev = std::max(1, (int)o.n_devices);
    for (int i = 0; i < ndev; i++) {
        c.devs.push_back(o.devices ? o.devices[i] : i);
        if (c.devs.back() < 0) { set_error("negative device ordinal"); return LDPC_ERR_ARG; }
    }
    c.g = g;
    c.in = in;
    c.B = B;
    c.max_iter = max_iter;
    c.algo = algo;
    c.hard_out = hard_out;
    c.post_out = post_out;
    c.iters_out = iters_out;
    c.valid_out = valid_out;
    c.N = (size_t)g->h.N;
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    // host threads for exp / packing: the caller's count, clamped (each is an
    // OS thread of this call's worker pool)
    c.host_threads = o.host_threads > 0 ? std::min(o.host_threads, kMaxHostThreads)
                                        : std::min(16, std::max(1, hw / ndev));
    c.sched = resolve_schedule(o.schedule);
    c.lr_table = sched_flag(c.sched, LDPC_SCHED_LR_TABLE);
    const char* pev = std::getenv("LDPC_API_TIMING");
    c.timing = pev && *pev && std::atoi(pev) != 0;
    // codes in pinned host memory (ldpc_host_alloc / hipHostMalloc: mapped
    // for every device) cross PCIe straight from the caller's array; the
    // tested case is ldpc_host_alloc memory
    if (in.codes) {
        hipPointerAttribute_t a0{}, a1{};
        c.codes_pinned = hipPointerGetAttributes(&a0, in.codes) == hipSuccess && a0.type == hipMemoryTypeHost &&
                         hipPointerGetAttributes(&a1, in.codes + (size_t)B * c.N - 1) == hipSuccess &&
                         a1.type == hipMemoryTypeHost;
        (void)hipGetLastError();  // pageable memory: the attribute query's error is not sticky
    }
    return LDPC_OK;
}

// One device's share of a call: codewords [s0, s1) through one slot, in chunks
// of X codewords, chunk c through staging half c & 1.
//
// Order, per chunk c (st = its staging half):
//   prep(c)    host: wait st.h2d of chunk c - 2 (the pinned input is free again)
//              copy stream: wait st.dec of chunk c - 2 (the device input is free again),
//              the chunk's H2D copies (codes in pieces, each crossing while the
//              next is prepared; or fp64 after the exp / copy), record st.h2d
//   decode(c)  set_params (integer decoders), tie hash base = the chunk's offset in the call
//              engine stream: wait st.h2d, the decode, record st.dec, [pack_bits, record st.dec]
//              copy_out stream: wait st.dec (after each record), the D2H copies, record st.d2h
//   finish(c)  host: wait st.d2h, copy the outputs to the caller's arrays
// run() is prep(0), then for each c: prep(c + 1) on a helper thread while this
// thread does decode(c) and finish(c - 1); finish of the last chunk, the
// engine's sync, and the slot goes back to the graph only on success.  The
// helper thread touches only half (c + 1) & 1 and the copy stream; decode(c)
// and finish(c - 1) only the other state.
struct ShardRun {
    const HostCall& c;
    const size_t di;       // shard index
    const int dev;
    const int64_t s0, s1;  // the shard's codewords in the call
    Slot* S = nullptr;
    int64_t X = 0, nch = 0;  // codewords per chunk, chunks
    bool host_exp = false;
    int in_kind = LDPC_IN_LLR;

    ShardRun(const HostCall& call, size_t shard)
        : c(call), di(shard), dev(call.devs[shard]), s0(call.B * (int64_t)shard / (int64_t)call.devs.size()),
          s1(call.B * (int64_t)(shard + 1) / (int64_t)call.devs.size())
    {
    }

    int64_t c0(int64_t ch) const { return s0 + ch * X; }
    int64_t cn(int64_t ch) const { return std::min<int64_t>(X, s1 - c0(ch)); }
    double tick() const { return c.timing ? now_ms() : 0; }
    __attribute__((format(printf, 2, 3))) void note(const char* fmt, ...) const
    {
        if (!c.timing) return;
        va_list ap;
        va_start(ap, fmt);
        std::vfprintf(stderr, fmt, ap);
        va_end(ap);
    }

    // Rows [0, Bc) of st.h_code in up to four pieces: rows(p0, p1) fills a
    // piece (on the workers; false: the rows have no codes, stop), then its
    // H2D is enqueued and crosses PCIe while the next piece is filled.
    template <typename F>
    int send_code_pieces(Stage& st, int64_t Bc, bool* ok, F&& rows)
    {
        const size_t N = c.N;
        const int64_t pieces = std::min<int64_t>(4, Bc);
        *ok = false;
        for (int64_t pc = 0; pc < pieces; pc++) {
            const int64_t p0 = Bc * pc / pieces, p1 = Bc * (pc + 1) / pieces;
            std::atomic<bool> good{true};
            parallel_rows(*S->workers, p1 - p0, [&](int64_t r0, int64_t r1) {
                if (!rows(p0 + r0, p0 + r1)) good = false;
            });
            if (!good) return LDPC_OK;
            LDPC_HIP(hipMemcpyAsync(st.d_code.get() + (size_t)p0 * N, st.h_code.get() + (size_t)p0 * N,
                                    (size_t)(p1 - p0) * N, hipMemcpyHostToDevice, S->copy.get()));
        }
        *ok = true;
        return LDPC_OK;
    }

    // the caller's codes: straight from pinned memory, else through pinned staging
    int prep_codes(int64_t ch, Stage& st, const char** what)
    {
        const size_t N = c.N;
        const int64_t Bc = cn(ch);
        const int8_t* src = c.in.codes + (size_t)c0(ch) * N;
        *what = "codes copy";
        if (c.codes_pinned) {
            LDPC_HIP(hipMemcpyAsync(st.d_code.get(), src, (size_t)Bc * N, hipMemcpyHostToDevice, S->copy.get()));
        } else {
            bool ok;
            int rc = send_code_pieces(st, Bc, &ok, [&](int64_t r0, int64_t r1) {
                std::memcpy(st.h_code.get() + (size_t)r0 * N, src + (size_t)r0 * N, (size_t)(r1 - r0) * N);
                return true;
            });
            if (rc) return rc;
        }
        std::copy(c.in.table, c.in.table + kTable, st.table.begin());
        st.table_kind = c.in.table_kind;
        st.coded = true;
        return LDPC_OK;
    }

    // fp64 LLRs: as codes when all of the chunk's LLRs are exact multiples of
    // one unit (code table path); else exp (DNA_main.cpp:1344
    // g_received_LR[i] = exp(g_received_LLR[i])) or copy into st.h_in, also
    // when a later piece turns out to be off the lattice
    int prep_llr(int64_t ch, Stage& st, const char** what)
    {
        const size_t N = c.N;
        const int64_t Bc = cn(ch);
        const double* src = c.in.llr + (size_t)c0(ch) * N;
        const bool msa = c.algo == LDPC_ALGO_MSA;
        Workers& W = *S->workers;
        st.coded = false;
        const double unit = (host_exp || msa) && c.lr_table && st.h_code ? llr_unit(src, Bc, N) : 0;
        if (unit > 0) {
            int rc = send_code_pieces(st, Bc, &st.coded, [&](int64_t r0, int64_t r1) {
                return host_encode_lattice(src, st.h_code.get(), (size_t)r0 * N, (size_t)r1 * N, unit, kCodeMax,
                                           /*keep_neg_zero=*/msa);
            });
            if (rc) return rc;
        }
        *what = st.coded ? "encode" : "exp/copy";
        if (st.coded) {
            for (int q = -kCodeMax; q <= kCodeMax; q++) st.table[q + 128] = (double)q * unit;
            st.table_kind = LDPC_IN_LLR;
        } else if (host_exp) {
            parallel_rows(W, Bc, [&](int64_t r0, int64_t r1) {
                for (size_t i = (size_t)r0 * N; i < (size_t)r1 * N; i++) st.h_in[i] = std::exp(src[i]);
            });
        } else {
            parallel_rows(W, Bc, [&](int64_t r0, int64_t r1) {
                std::memcpy(st.h_in.get() + (size_t)r0 * N, src + (size_t)r0 * N, (size_t)(r1 - r0) * N * 8);
            });
        }
        return LDPC_OK;
    }

    // host side of chunk ch and its H2D on the copy stream
    int prep(int64_t ch)
    {
        Stage& st = S->stage[ch & 1];
        LDPC_HIP(hipSetDevice(dev));
        if (ch >= 2) {  // the half's last use was chunk ch - 2
            LDPC_HIP(hipEventSynchronize(st.h2d.get()));                       // pinned staging free again
            LDPC_HIP(hipStreamWaitEvent(S->copy.get(), st.dec.get(), 0));     // the decode that read the device buffers
        }
        const double t0 = tick();
        const char* what = "";
        int rc = c.in.codes ? prep_codes(ch, st, &what) : prep_llr(ch, st, &what);
        if (rc) return rc;
        const double t1 = tick();
        if (!st.coded)  // (codes are on their way already; their table goes with the decode)
            LDPC_HIP(hipMemcpyAsync(st.d_in.get(), st.h_in.get(), (size_t)cn(ch) * c.N * 8, hipMemcpyHostToDevice,
                                    S->copy.get()));
        LDPC_HIP(hipEventRecord(st.h2d.get(), S->copy.get()));
        if (c.timing) {
            LDPC_HIP(hipEventSynchronize(st.h2d.get()));
            note("api chunk %lld: %s %.3f ms, + H2D %.3f ms\n", (long long)ch, what, t1 - t0, now_ms() - t1);
        }
        return LDPC_OK;
    }

    int decode(int64_t ch)
    {
        Stage& st = S->stage[ch & 1];
        Engine& E = *S->eng;
        const size_t N = c.N;
        const int64_t Bc = cn(ch);
        const ldpc_opts& o = c.o;
        hipStream_t out = S->copy_out.get();
        LDPC_HIP(hipSetDevice(dev));
        if (c.algo == LDPC_ALGO_QMSA) {
            int r = E.set_params(c.q_prec, c.q_step, o.msa_offset, o.tie_seed);
            if (r) return r;
        }
        hipStream_t es = E.stream.get();
        LDPC_HIP(hipStreamWaitEvent(es, st.h2d.get(), 0));
        const double td0 = tick();
        double* d_post = c.post_out ? st.d_post.get() : nullptr;
        int r = st.coded ? E.decode_codes(st.d_code.get(), st.table.data(), st.table_kind, Bc, c.max_iter,
                                          st.d_hard.get(), d_post, o.post_kind, st.d_iters.get(), st.d_valid.get(),
                                          st.d_in.get(), c0(ch))
                         : E.decode(st.d_in.get(), in_kind, Bc, c.max_iter, st.d_hard.get(), d_post, o.post_kind,
                                    st.d_iters.get(), st.d_valid.get(), c0(ch));
        if (r) return r;
        note("api chunk %lld: decode enqueue + drain wait %.3f ms\n", (long long)ch, now_ms() - td0);
        LDPC_HIP(hipEventRecord(st.dec.get(), es));
        LDPC_HIP(hipStreamWaitEvent(out, st.dec.get(), 0));
        if (st.d_hbits) {  // 1/8 of the bytes across PCIe
            r = E.pack_bits(st.d_hard.get(), st.d_hbits.get(), Bc * (int64_t)N / 8);
            if (r) return r;
            LDPC_HIP(hipEventRecord(st.dec.get(), es));
            LDPC_HIP(hipStreamWaitEvent(out, st.dec.get(), 0));
            LDPC_HIP(hipMemcpyAsync(st.h_hbits.get(), st.d_hbits.get(), (size_t)Bc * N / 8, hipMemcpyDeviceToHost, out));
        } else {
            LDPC_HIP(hipMemcpyAsync(st.h_hard.get(), st.d_hard.get(), (size_t)Bc * N, hipMemcpyDeviceToHost, out));
        }
        if (c.post_out)
            LDPC_HIP(hipMemcpyAsync(st.h_post.get(), st.d_post.get(), (size_t)Bc * N * 8, hipMemcpyDeviceToHost, out));
        LDPC_HIP(hipMemcpyAsync(st.h_iters.get(), st.d_iters.get(), (size_t)Bc * 4, hipMemcpyDeviceToHost, out));
        LDPC_HIP(hipMemcpyAsync(st.h_valid.get(), st.d_valid.get(), (size_t)Bc, hipMemcpyDeviceToHost, out));
        LDPC_HIP(hipEventRecord(st.d2h.get(), out));
        return LDPC_OK;
    }

    // outputs of chunk ch, once its D2H copies are done
    int finish(int64_t ch)
    {
        Stage& st = S->stage[ch & 1];
        const size_t N = c.N;
        const int64_t b0 = c0(ch), Bc = cn(ch);
        const double tf0 = tick();
        LDPC_HIP(hipEventSynchronize(st.d2h.get()));
        const double tf1 = tick();
        parallel_rows(*S->workers, Bc, [&](int64_t r0, int64_t r1) {
            if (st.h_hbits) {  // packed: 8 hard bits per byte
                uint64_t* o = reinterpret_cast<uint64_t*>(c.hard_out + (size_t)(b0 + r0) * N);
                const uint8_t* in = st.h_hbits.get() + (size_t)r0 * N / 8;
                const size_t nb = (size_t)(r1 - r0) * N / 8;
                if (((uintptr_t)o & 7) == 0)
                    for (size_t q = 0; q < nb; q++) o[q] = kBitBytes.t[in[q]];
                else
                    for (size_t q = 0; q < nb; q++) std::memcpy((uint8_t*)o + 8 * q, &kBitBytes.t[in[q]], 8);
            } else {
                std::memcpy(c.hard_out + (size_t)(b0 + r0) * N, st.h_hard.get() + (size_t)r0 * N, (size_t)(r1 - r0) * N);
            }
            if (c.post_out)
                std::memcpy(c.post_out + (size_t)(b0 + r0) * N, st.h_post.get() + (size_t)r0 * N,
                            (size_t)(r1 - r0) * N * 8);
        });
        if (c.iters_out) std::memcpy(c.iters_out + b0, st.h_iters.get(), (size_t)Bc * 4);
        if (c.valid_out) std::memcpy(c.valid_out + b0, st.h_valid.get(), (size_t)Bc);
        note("api chunk %lld: wait decode + D2H %.3f ms, copy out %.3f ms\n", (long long)ch, tf1 - tf0, now_ms() - tf1);
        return LDPC_OK;
    }

    int run()
    {
        const int64_t shard = s1 - s0;
        if (shard <= 0) return LDPC_OK;
        // lane pool: the caller's chunk; else for small shards (the DNA batch)
        // one holding all of them (every codeword in flight at once), else the
        // engine's own (0: the resident pool for BP).  Codewords move through
        // PCIe in double-buffered chunks of `xfer`.
        const int64_t sh64 = (shard + 63) / 64 * 64;
        const int64_t pool = c.o.chunk > 0 ? c.o.chunk : (shard <= kExplicitPoolMax ? sh64 : 0);
        const int64_t xfer = std::min<int64_t>(sh64, std::max<int64_t>(kXferChunk, (pool + 63) / 64 * 64));
        std::unique_ptr<Slot> slot = c.g->take(dev, c.algo, pool, xfer, c.o.chunk <= 0 && pool > 0, c.sched);
        int rc = LDPC_OK;
        if (!slot) rc = make_slot(&c.g->h, dev, c.algo, pool, xfer, c.sched, slot);
        if (rc) return rc;
        LDPC_HIP(hipSetDevice(dev));  // (a slot from the pool: nothing has selected its device on this thread yet)
        for (Stage& st : slot->stage)
            if (c.post_out && (rc = st.want_post())) return rc;
        for (Stage& st : slot->stage)
            if (c.in.codes && (rc = st.want_codes())) return rc;
        if (!slot->workers || slot->workers->size() != c.host_threads)
            slot->workers = std::make_unique<Workers>(c.host_threads);
        S = slot.get();
        host_exp = c.algo == LDPC_ALGO_BP && c.o.exp_on_host;
        in_kind = host_exp ? LDPC_IN_LR : LDPC_IN_LLR;
        X = xfer;  // (the slot's staging holds >= xfer)
        nch = (shard + X - 1) / X;

        const double t_call = tick();
        rc = prep(0);
        for (int64_t ch = 0; ch < nch && rc == LDPC_OK; ch++) {
            // the next chunk's host work and H2D run on a helper thread while
            // this thread drives the decode of chunk ch
            int rc_next = LDPC_OK;
            std::string err_next;
            std::thread next;
            if (ch + 1 < nch)
                next = std::thread([&, ch] {
                    rc_next = prep(ch + 1);
                    if (rc_next) err_next = last_error();
                });
            rc = decode(ch);
            if (rc == LDPC_OK && ch >= 1) rc = finish(ch - 1);
            if (next.joinable()) next.join();
            if (rc == LDPC_OK && rc_next) { rc = rc_next; set_error(err_next); }
        }
        if (rc == LDPC_OK) rc = finish(nch - 1);
        note("api shard %zu: %.3f ms\n", di, now_ms() - t_call);
        if (rc == LDPC_OK) rc = S->eng->sync();  // surplus steps of the last decode; a device fault report
        if (rc) return rc;  // (the slot is dropped)
        c.g->give(std::move(slot));
        return LDPC_OK;
    }
};

}  // namespace

int host_decode(const ldpc_graph* g, const HostInput& in, int64_t B, int32_t max_iter, int32_t algo,
                uint8_t* hard_out, double* post_out, int32_t* iters_out, uint8_t* valid_out, const ldpc_opts* opts)
{
    HostCall call;
    int rc = validate(g, in, B, max_iter, algo, hard_out, post_out, iters_out, valid_out, opts, call);
    if (rc || B == 0) return rc;
    const size_t n = call.devs.size();
    std::vector<int> rcs(n, LDPC_OK);
    std::vector<std::string> msgs(n);
    auto work = [&](size_t di) {
        rcs[di] = ShardRun(call, di).run();
        if (rcs[di]) msgs[di] = last_error();
    };
    if (n == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (size_t i = 0; i < n; i++) th.emplace_back(work, i);
        for (auto& t : th) t.join();
    }
    for (size_t i = 0; i < n; i++)
        if (rcs[i]) { set_error("device " + std::to_string(call.devs[i]) + ": " + msgs[i]); return rcs[i]; }
    return LDPC_OK;
}

}  // namespace ldpc
