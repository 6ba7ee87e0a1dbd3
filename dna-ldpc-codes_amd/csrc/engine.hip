// engine.hip -- device engine: memory, launch sequence, profiling.
//
// One Engine = one device, one HIP stream, message buffers for `cap`
// resident codewords.  A decode is the reference's per-frame loop
// (Run_Belief_Propagation_Decoder dec.cpp:583-605 / Run_MSA_Decoder_INF
// dec.cpp:1216-1250) executed for many codewords at once:
//
//   init                                  (Init_*: dec.cpp:608 / 1300)
//   for n = 0..max_iter:
//       syndrome(n)  -> codewords with c == 0 or n == max_iter stop
//       if n == max_iter: break
//       check phase  (dec.cpp:646-662 / 1398-1433)
//       variable phase + hard decision (dec.cpp:667-693 / 1597-1678)
//   finalize (posterior, hard bits, iteration counts)
//
// Three schedules (include/ldpc_amd.h ldpc_schedule), all
// bit-exact; they differ only in which codewords share a launch:
//   * fixed passes (fixed_pass): passes of <= cap codewords, stopped codewords
//     masked out of every later kernel (the integer decoders, irregular
//     graphs, or LDPC_SCHED_CONTINUOUS off);
//   * continuous grouped (run_cont): a lane pool refilled as codewords
//     finish, check/variable launches per tile group so the group's c2v
//     stays in the Infinity Cache, a multi-block syndrome per step;
//   * resident pool (run_cont, `res`): a few tiles iterated in place, sized to
//     the 256 MB Infinity Cache, the syndrome fused into the check kernel.
// Which of them an engine runs, and how large its buffers are, is decided by
// plan_engine (engine_plan.hpp) before anything is allocated.  Every member
// that holds a HIP object owns it (hip_own.hpp); every kernel goes through
// Sampler::launch.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <utility>

#include "engine.hpp"
#include "kernels.hpp"
#include "kernels_int.hpp"
#include "encode_kernels.hpp"

namespace ldpc {

static_assert(kTile == dev::TILE && kMsaRecPlanes == dev::MSA_REC_PLANES && kMsaErShift == dev::MSA_ER_SHIFT,
              "engine_plan.hpp restates the kernels' layout constants");
constexpr int kProbes = 4;  // placement probe: candidate scratch allocations timed at init

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }

// ---------------------------------------------------------------------------
// Sampler: the one launch path
// ---------------------------------------------------------------------------
Event Sampler::get_event()
{
    if (!pool.empty()) { Event e = std::move(pool.back()); pool.pop_back(); return e; }
    // no system-scope fence: a default event record writes back and
    // invalidates the caches, which inflated the sampled launch by ~7 %
    // against the rocprofv3 kernel trace
    Event e;
    if (make_event(e, hipEventDisableSystemFence) != LDPC_OK) (void)hipGetLastError();
    return e;
}

// kernel arguments: an owning handle stands for its pointer
template <typename T>
static T* raw(const dev_ptr<T>& p) { return p.get(); }
template <typename T>
static const T& raw(const T& v) { return v; }

// A sampled launch's start / stop events ride on the kernel's own dispatch
// packet (hipExtLaunchKernelGGL), so they time the kernel as the profiler
// does -- separate marker packets around it added the dispatch latency (~4 us
// per 71 us launch against the rocprofv3 trace).  A sample whose launch
// failed returns its events to the pool and is not counted.
template <typename F, typename... A>
int Sampler::launch(int c, hipStream_t s, F kernel, dim3 grid, dim3 block, const A&... args)
{
    Event b, e;
    if (c >= 0) {
        const int64_t idx = launches[c]++;
        if (stride > 0 && idx % stride == 0) {
            b = get_event();
            e = get_event();
            if (!b || !e) {
                if (b) pool.push_back(std::move(b));
                if (e) pool.push_back(std::move(e));
                set_error("hipEventCreate failed");
                return LDPC_ERR_DEVICE;
            }
        }
    }
    if (b) hipExtLaunchKernelGGL(kernel, grid, block, 0, s, b.get(), e.get(), 0, raw(args)...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, s, raw(args)...);
    const hipError_t le = hipGetLastError();
    if (b && le == hipSuccess) {
        sampled[c]++;
        live[c].emplace_back(std::move(b), std::move(e));
    } else if (b) {
        pool.push_back(std::move(b));
        pool.push_back(std::move(e));
    }
    if (le != hipSuccess) {
        set_error(std::string("kernel launch: ") + hipGetErrorString(le));
        return LDPC_ERR_DEVICE;
    }
    return LDPC_OK;
}

int Sampler::collect()
{
    for (int c = 0; c < K_NCLASS; c++) {
        for (auto& p : live[c]) {
            float t = 0.f;
            LDPC_HIP(hipEventElapsedTime(&t, p.first.get(), p.second.get()));
            ms[c] += t;
            pool.push_back(std::move(p.first));
            pool.push_back(std::move(p.second));
        }
        live[c].clear();
    }
    return LDPC_OK;
}

void Sampler::reset(int new_stride)
{
    for (int c = 0; c < K_NCLASS; c++) { launches[c] = 0; ms[c] = 0; sampled[c] = 0; }
    stride = new_stride > 0 ? new_stride : 0;
}

void Sampler::snapshot(ldpc_kernel_stats* out) const
{
    std::memset(out, 0, sizeof(*out));
    for (int c = 0; c < K_NCLASS; c++) {
        out->launches[c] = launches[c];
        out->sampled[c] = sampled[c];
        out->ms[c] = ms[c];
    }
}

template <typename F, typename... A>
int Engine::launch(int c, F kernel, dim3 grid, dim3 block, const A&... args)
{
    return sampler.launch(c, stream.get(), kernel, grid, block, args...);
}

int Engine::collect_stats()
{
    LDPC_HIP(hipSetDevice(device));
    LDPC_HIP(hipStreamSynchronize(stream.get()));
    return sampler.collect();
}

int Engine::profile(int stride)
{
    if (int rc = collect_stats()) return rc;
    sampler.reset(stride);
    return LDPC_OK;
}

int Engine::stats(ldpc_kernel_stats* out)
{
    if (int rc = collect_stats()) return rc;
    sampler.snapshot(out);
    return LDPC_OK;
}

// ---------------------------------------------------------------------------
// the graph on the device
// ---------------------------------------------------------------------------
int DeviceGraph::build(const HostGraph& g, bool msa_c)
{
    int rc;
    if ((rc = upload(row_ptr, g.row_ptr)) || (rc = upload(col_idx, g.col_idx)) || (rc = upload(col_ptr, g.col_ptr)) ||
        (rc = upload(col_edge, g.col_edge)))
        return rc;
    if (msa_c) {  // (row << 18) | edge id per CSC position (k_var_msa_c); E < 2^18 (plan_engine), M < 2^14
        if (g.M >= (1 << (32 - dev::MSA_ER_SHIFT))) { set_error("MSA-C: too many rows"); return LDPC_ERR_UNSUPPORTED; }
        std::vector<uint32_t> er(g.col_edge.size());
        for (size_t q = 0; q < er.size(); q++)
            er[q] = ((uint32_t)g.edge_row[(size_t)g.col_edge[q]] << dev::MSA_ER_SHIFT) | (uint32_t)g.col_edge[q];
        if ((rc = upload(col_er, er))) return rc;
        // CSR edge -> its v2c position: the compressed min-sum keeps v2c in
        // column order (contiguous variable-phase stores, gathered check
        // reads), edge s of column j at j * DV + s -- or, row-block-major,
        // at s * N + j when edge s of every column lies in row block s
        // (array codes such as the DNA code's RS-LDPC H: M = DV blocks of
        // M / DV rows), so a row's gathers stay inside one N-segment region
        const int dv = g.dv_max;
        bool rb = g.M % dv == 0;  // (round 4 A/B: +1.1 %, profiles/r4/rb/)
        for (int32_t j = 0; rb && j < g.N; j++)
            for (int s2 = 0; rb && s2 < dv; s2++)
                rb = g.edge_row[(size_t)g.col_edge[(size_t)j * dv + s2]] / (g.M / dv) == s2;
        msa_pa = rb ? 1 : dv;
        msa_pb = rb ? g.N : 1;
        std::vector<int32_t> pos(g.col_edge.size());
        for (size_t q = 0; q < pos.size(); q++)
            pos[(size_t)g.col_edge[q]] = (int32_t)(q / dv) * msa_pa + (int32_t)(q % dv) * msa_pb;
        if ((rc = upload(row_pos, pos))) return rc;
    }
    if (g.regular_dc && g.dc_max > 0) {
        std::vector<int32_t> T((size_t)g.dc_max * g.M);
        for (int32_t i = 0; i < g.M; i++)
            for (int k = 0; k < g.dc_max; k++) T[(size_t)k * g.M + i] = g.col_idx[(size_t)i * g.dc_max + k];
        if ((rc = upload(col_idx_T, T))) return rc;
    }
    return LDPC_OK;
}

// ---------------------------------------------------------------------------
// the lane pool
// ---------------------------------------------------------------------------
// a pinned, device-mapped array of n zero words
static int mapped_words(pinned_ptr<unsigned long long>& h, unsigned long long** d, size_t n)
{
    if (int rc = pinned_alloc(h, n, hipHostMallocCoherent | hipHostMallocMapped)) return rc;
    std::memset(h.get(), 0, n * sizeof(unsigned long long));
    LDPC_HIP(hipHostGetDevicePointer((void**)d, h.get(), 0));
    return LDPC_OK;
}

int LanePool::build(const EnginePlan& p, int32_t N)
{
    const size_t tiles = (size_t)p.cap_tiles, cap = (size_t)p.cap;
    int rc;
    if ((rc = dev_alloc(fresh, tiles)) || (rc = dev_alloc(occ, tiles)) || (rc = dev_alloc(lane_b, cap)) ||
        (rc = dev_alloc(lane_n, cap)) || (rc = dev_alloc(ctr, (size_t)(1 + kRing))) ||
        (rc = mapped_words(h_poll, &d_poll, (size_t)kRing)) || (rc = mapped_words(h_fault, &d_fault, dev::kFaultWords)) ||
        (rc = dev_alloc(unsat, tiles)) || (rc = dev_alloc(done, tiles)) || (rc = dev_alloc(fin, tiles)) ||
        (rc = dev_alloc(fin_b, cap)) || (rc = dev_alloc(fin_n, cap)))
        return rc;
    if (p.handover &&
        ((rc = dev_alloc(ho, tiles * 3)) || (rc = dev_alloc(pend_b, cap)) || (rc = dev_alloc(hard_fin, tiles * (size_t)N))))
        return rc;
    return LDPC_OK;
}

void LanePool::poll_arm(dev::ContState& cs, uint64_t q) const
{
    cs.occ_count = ctr.get() + 1 + (q % kRing);
    cs.occ_clear = ctr.get() + 1 + ((q + 1) % kRing);
    cs.poll_host = d_poll + (q % kRing);
    cs.poll_tag = (q + 1) & ((1ull << (64 - dev::kOccTileShift)) - 1ull);  // never the initial 0
}

// Wait for poll q's device-written word.  The engine-wide sequence keeps tags
// unique across decodes (a previous decode's trailing steps may still write
// their slots).  The stream is queried while waiting: a device error, or a
// stream that finished without the word, is an error instead of a hang.
int LanePool::poll_wait(uint64_t q, unsigned long long* occ, hipStream_t stream)
{
    const unsigned long long want = (q + 1) & ((1ull << (64 - dev::kOccTileShift)) - 1ull);
    volatile unsigned long long* w = h_poll.get() + (q % kRing);
    for (uint64_t spin = 1;; spin++) {
        const unsigned long long v = *w;
        if ((v >> dev::kOccTileShift) == want) {
            *occ = v & dev::kOccMask;
            return check_fault();
        }
        if (spin % 64 == 0) {
            if (int rc = check_fault()) return rc;
            const hipError_t e = hipStreamQuery(stream);
            if (e == hipSuccess) {
                const unsigned long long v2 = *w;
                if ((v2 >> dev::kOccTileShift) == want) {
                    *occ = v2 & dev::kOccMask;
                    return LDPC_OK;
                }
                set_error("occupancy poll " + std::to_string(q) + ": the step finished without its device write");
                return LDPC_ERR_DEVICE;
            }
            if (e != hipErrorNotReady) {
                set_error(std::string("occupancy poll: ") + hipGetErrorString(e));
                return LDPC_ERR_DEVICE;
            }
            std::this_thread::yield();
        }
    }
}

int LanePool::check_fault()
{
    if (!h_fault) return LDPC_OK;
    volatile unsigned long long* w = h_fault.get();
    std::string msg;
    for (int k = 1; k < dev::kFaultWords; k++) {  // every word is read and cleared; the first set one is reported
        const unsigned long long v = w[k];
        if (!(v & dev::kFaultTag)) continue;
        w[k] = 0ull;
        if (!msg.empty()) continue;
        int64_t idx = (int64_t)(v & dev::kFaultIndex);
        if (idx & (int64_t)(1ull << 47)) idx -= (int64_t)(1ull << 48);  // sign of the 48-bit field
        if (k == dev::kFaultSchedule)
            msg = "device schedule fault: the code fill of tile " + std::to_string(-1 - idx) +
                  " found live or finished lanes";
        else if (k == dev::kFaultIters)
            msg = "device lane bookkeeping fault: codeword index " + std::to_string(idx) +
                  " out of range for the iteration count / valid flag access";
        else  // the variable kernels report the lane's pool slot (k_fill_codes the codeword index)
            msg = "device lane bookkeeping fault: pool slot or codeword index " + std::to_string(idx) +
                  " out of range for " + (k == dev::kFaultOutput ? "a finished codeword's hard bits / posterior" : "a refill's input row");
    }
    if (msg.empty()) return LDPC_OK;
    set_error(msg + " (skipped; the decode's outputs are incomplete)");
    return LDPC_ERR_DEVICE;
}

void LanePool::clear_faults()
{
    volatile unsigned long long* w = h_fault.get();
    for (int k = 1; w && k < dev::kFaultWords; k++) w[k] = 0ull;
}

// ---------------------------------------------------------------------------
// the engine
// ---------------------------------------------------------------------------
// The members release what they own, the stream last (engine.hpp).
Engine::~Engine()
{
    if (device >= 0) (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream.get());
}

static double* msa_rec(double* scratch) { return scratch; }
static uint16_t* msa_meta(double* scratch, int64_t tiles, int32_t M)
{
    return reinterpret_cast<uint16_t*>(scratch + (size_t)tiles * M * dev::MSA_REC_PLANES * dev::TILE);
}

// Run-time values to template arguments, the one mechanism of launch_check /
// launch_var.  with_bools: f(std::bool_constant<b>...).  dispatch: the
// member of the list equal to v first, f(std::integral_constant<int, v>,
// std::bool_constant<b>...); false, and f not called, when the list has no
// such member.  f is a generic lambda that names its kernel with D(), NT(), ...;
// combinations that are not to exist it leaves out with `if constexpr`, so
// they are not instantiated either.
template <typename F>
static void with_bools(F&& f)
{
    f();
}
template <typename F, typename... Bs>
static void with_bools(F&& f, bool b, Bs... rest)
{
    if (b) with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
template <int... Vs, typename F, typename... Bs>
static bool dispatch(int v, std::integer_sequence<int, Vs...>, F&& f, Bs... bs)
{
    return ((v == Vs && (with_bools([&](auto... cs) { f(std::integral_constant<int, Vs>{}, cs...); }, bs...), true)) || ...);
}

int Engine::init(const HostGraph* graph, int dev, int algorithm, int64_t chunk, const ldpc_schedule* schedule,
                 bool resolved)
{
    g = graph;
    device = dev;
    algo = algorithm;
    if (resolved && schedule && (schedule->flags_set & kResolved)) {
        sched = *schedule;  // the host API's slot: resolved once per call (host_decode.cpp)
        sched.pool_tiles = std::max(sched.pool_tiles, 0);
        sched.poll_every = std::max(sched.poll_every, 1);
        sched.syn_blocks = std::min(std::max(sched.syn_blocks, 1), 256);
    } else {
        sched = resolve_schedule(schedule);
    }
    if (algo < LDPC_ALGO_BP || algo > LDPC_ALGO_GALLAGER_B2) { set_error("unknown algorithm"); return LDPC_ERR_ARG; }
    int rc;
    if ((rc = select_device("engine", dev)) || (rc = make_stream(stream))) return rc;
    size_t fr = 0, tot = 0;
    if (chunk <= 0) LDPC_HIP(hipMemGetInfo(&fr, &tot));
    p = plan_engine(*g, algo, chunk, sched, fr);
    if (p.error) { set_error(p.error); return LDPC_ERR_ARG; }
    // k_var_bp_fused addresses a tile's messages through a buffer resource:
    // 32-bit byte offsets over E * 512 bytes
    if (g->E * (int64_t)(dev::TILE * sizeof(double)) > 0x7fffffff) p.fuse_block = -1;

    if ((rc = dg.build(*g, p.msa_c))) return rc;
    if (p.cont && (rc = lp.build(p, g->N))) return rc;
    const size_t E = (size_t)std::max<int64_t>(g->E, 1), cap = (size_t)p.cap, tiles = (size_t)p.cap_tiles, N = (size_t)g->N;
    if ((rc = dev_alloc(v2c, cap * E))) return rc;
    // (c2v_bytes: fp64 messages, or the compressed min-sum's records and meta words, a multiple of 8 too)
    if (!p.res && (rc = dev_alloc(c2v_buf, p.c2v_bytes / sizeof(double)))) return rc;
    if ((rc = dev_alloc(prior, cap * N)) || (p.msa_c && (rc = dev_alloc(d_sgn, cap * N))) ||
        (rc = dev_alloc(hard, tiles * N)) || (rc = dev_alloc(active, tiles)) || (rc = dev_alloc(iters, cap)) ||
        (rc = dev_alloc(valid, cap)))
        return rc;
    if (algo < LDPC_ALGO_QMSA && (p.res || p.group_tiles < p.cap_tiles)) return probe(kProbes);
    return LDPC_OK;
}

int32_t Engine::flags() const
{
    return (p.nt_d ? LDPC_SCHED_NONTEMPORAL : 0) | (p.cont ? LDPC_SCHED_CONTINUOUS : 0) |
           (p.msa_c ? LDPC_SCHED_MSA_COMPRESSED : 0) | (p.res ? LDPC_SCHED_RESIDENT : 0) |
           (p.syn_blocks > 0 ? LDPC_SCHED_SPLIT_SYNDROME : 0) | (p.first_fp ? LDPC_SCHED_FIRST_FROM_PRIOR : 0) |
           (p.handover ? LDPC_SCHED_HANDOVER : 0) | (p.fuse_block >= 0 ? LDPC_SCHED_FUSE_ROW_BLOCK : 0) |
           (sched.flags & (LDPC_SCHED_LR_TABLE | LDPC_SCHED_DEBUG_NO_DRAIN | LDPC_SCHED_DEBUG_BAD_LANE));
}

// Placement probe.  The resident pool (~226 MB at 3 tiles) and the grouped
// schedule's check->variable scratch (~226 MB at G = 3) are meant to stay in
// the 256 MB Infinity Cache, a memory-side cache whose slices belong to HBM
// channels: how well a given allocation fits depends on where its physical
// pages land, and identical engines were measured 3-4 % apart.  Allocate
// `probes` candidate buffers, time a few real check + variable steps on each
// (state zeroed, results discarded -- every decode re-initialises), keep the
// fastest.  The resident pool's candidates are timed with the plain check
// kernel on the same buffer (no syndrome bookkeeping; timing only).
int Engine::probe(int probes)
{
    // The engine's pool joins the candidates.  On every exit the best one --
    // the engine's own unless a faster one was timed -- is the engine's pool
    // again and the others are freed.
    dev_ptr<double>& pool = p.res ? v2c : c2v_buf;
    std::vector<dev_ptr<double>> cand;
    cand.push_back(std::move(pool));
    size_t best = 0;
    const int rc = time_candidates(probes, cand, &best);
    pool = std::move(cand[best]);
    return rc;
}

int Engine::time_candidates(int probes, std::vector<dev_ptr<double>>& cand, size_t* best)
{
    const size_t E = (size_t)std::max<int64_t>(g->E, 1);
    const size_t bytes = p.res ? (size_t)p.cap * E * sizeof(double) : p.c2v_bytes;
    const unsigned gt = (unsigned)(p.res ? p.cap_tiles : std::min<int64_t>(p.group_tiles, p.cap_tiles));
    hipStream_t s = stream.get();
    LDPC_HIP(hipMemsetAsync((p.res ? cand[0] : v2c).get(), 0, (size_t)gt * 64 * E * sizeof(double), s));
    LDPC_HIP(hipMemsetAsync(prior.get(), 0, (size_t)gt * 64 * g->N * sizeof(double), s));
    LDPC_HIP(hipMemsetAsync(active.get(), 0xff, (size_t)gt * sizeof(uint64_t), s));
    if (d_sgn) LDPC_HIP(hipMemsetAsync(d_sgn.get(), 0, (size_t)gt * 64 * g->N, s));
    for (int i = 1; i < probes; i++) {
        void* c = nullptr;
        if (hipMalloc(&c, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        cand.emplace_back(static_cast<double*>(c));
    }
    for (auto& c : cand) LDPC_HIP(hipMemsetAsync(c.get(), 0, bytes, s));
    Event e0, e1;
    int rc;
    if ((rc = make_event(e0, hipEventDefault)) || (rc = make_event(e1, hipEventDefault))) return rc;
    float best_ms = 1e30f;
    for (size_t c = 0; c < cand.size(); c++) {
        // a resident pool's candidate is timed as the engine's v2c, in place
        if (p.res) std::swap(v2c, cand[c]);
        float ms = 0;
        rc = time_steps((p.res ? v2c : cand[c]).get(), gt, e0.get(), e1.get(), &ms);
        if (p.res) std::swap(v2c, cand[c]);
        if (rc) return rc;
        if (ms < best_ms) { best_ms = ms; *best = c; }
    }
    return LDPC_OK;
}

// four timed check + variable steps on `pool` as the c2v of tiles 0 .. gt-1
int Engine::time_steps(double* pool, unsigned gt, hipEvent_t e0, hipEvent_t e1, float* ms)
{
    int rc;
    for (int rep = 0; rep < 5; rep++) {  // rep 0 warms up
        if (rep == 1) LDPC_HIP(hipEventRecord(e0, stream.get()));
        if ((rc = launch_check(pool, 0, gt, nullptr, true))) return rc;
        if ((rc = launch_var(pool, 0, gt, nullptr, dev::Refill{}, true))) return rc;
    }
    LDPC_HIP(hipEventRecord(e1, stream.get()));
    LDPC_HIP(hipEventSynchronize(e1));
    LDPC_HIP(hipEventElapsedTime(ms, e0, e1));
    return LDPC_OK;
}

// check phase of tiles t0 .. t0+gt-1 into `scratch` (that group's c2v); with
// rstep the resident pool's in-place check + fused syndrome step
int Engine::launch_check(double* scratch, int64_t t0, unsigned gt, const dev::ResStep* rstep, bool timing)
{
    using namespace dev;
    const int32_t M = g->M;
    const int64_t E = g->E;
    const bool reg72 = g->regular_dc && g->dc_max == 72;
    const dim3 grid((M + 3) / 4, gt), blk(256);
    const bool msa = algo == LDPC_ALGO_MSA;
    const int kc = timing ? K_UNCOUNTED : K_CHECK;
    int rc = LDPC_OK;
    if (rstep && !reg72) {
        const int cb = gen_bucket(g->dc_max, CheckBuckets{});
        if (!p.res || scratch != v2c.get() || t0 != 0 || !cb) { set_error("resident check: bad state"); return LDPC_ERR_ARG; }
        dispatch(cb, CheckBuckets{}, [&](auto D, auto MSA) {
            rc = launch(kc, (k_check_gr_res<MSA(), D()>), grid, blk, v2c, dg.row_ptr, M, E, *rstep);
        }, msa);
        return rc;
    }
    if (rstep) {
        if (!p.res || p.msa_c || scratch != v2c.get()) { set_error("resident check: bad state"); return LDPC_ERR_ARG; }
        if (msa) return launch(kc, (k_check_msa<72, false, true>), grid, blk, v2c, v2c, active, M, E, t0, *rstep);
        if (p.fuse_block >= 0) {  // the fused row block's messages belong to k_var_bp_fused (launch_var)
            if (t0 != 0) { set_error("resident check: bad state"); return LDPC_ERR_ARG; }
            const int32_t Q = M / 8;
            return launch(kc, (k_check_bp_skip<72>), grid, blk, v2c, v2c, M, E, p.fuse_block * Q, (p.fuse_block + 1) * Q,
                          *rstep);
        }
        return launch(kc, (k_check_bp<72, false, true>), grid, blk, v2c, v2c, active, M, E, t0, *rstep);
    }
    if (p.msa_c) {  // 1-D XCD-affine grid (k_check_msa_c)
        const dim3 g1((unsigned)((M + 3) / 4) * gt);
        with_bools([&](auto NT) {
            rc = launch(kc, (k_check_msa_c<72, NT()>), g1, blk, v2c, msa_rec(scratch), msa_meta(scratch, p.c2v_tiles, M),
                        active, dg.row_pos, M, E, t0, gt);
        }, p.nt_d);
        return rc;
    }
    if (reg72) {
        // scratch == v2c only in the resident pool's placement probe (timing)
        with_bools([&](auto NT) {
            if (msa) rc = launch(kc, (k_check_msa<72, NT(), false>), grid, blk, v2c, scratch, active, M, E, t0, ResStep{});
            else rc = launch(kc, (k_check_bp<72, NT(), false>), grid, blk, v2c, scratch, active, M, E, t0, ResStep{});
        }, p.nt_d);
        return rc;
    }
    // generic row degrees: registers up to the bucket of dc_max, else memory
    const bool bp = algo == LDPC_ALGO_BP;
    const bool in_regs = dispatch(gen_bucket(g->dc_max, CheckBuckets{}), CheckBuckets{}, [&](auto D, auto MSA) {
        rc = launch(kc, k_check_gr<MSA(), D()>, grid, blk, v2c, scratch, active, dg.row_ptr, M, E, t0);
    }, !bp);
    if (!in_regs && bp) rc = launch(kc, k_check_bp_gen, grid, blk, v2c, scratch, active, dg.row_ptr, M, E, t0);
    else if (!in_regs) rc = launch(kc, k_check_msa_gen, grid, blk, v2c, scratch, active, dg.row_ptr, M, E, t0);
    return rc;
}

// columns per variable-phase wave: the schedule's, or by default 2 for coded
// priors in the resident pool and the compressed min-sum, else 4 (same-box
// A/Bs, profiles/r3/coded/cpw_probe.txt)
int Engine::var_cpw_for(const dev::Refill& rf) const
{
    if (p.var_cpw > 0) return p.var_cpw;
    return (rf.fresh && rf.in_code && (p.res || p.msa_c)) ? kDefaultVarCpwCoded : kDefaultVarCpw;
}

// variable phase (+ hard decisions, optional posterior, continuous mode's
// refills and finished lanes' outputs) of tiles t0 .. t0+gt-1
int Engine::launch_var(double* scratch, int64_t t0, unsigned gt, double* pt, const dev::Refill& rf, bool timing)
{
    using namespace dev;
    const int32_t N = g->N, M = g->M;
    const int64_t E = g->E;
    const bool reg8 = g->regular_dv && g->dv_max == 8;
    const bool cnt = rf.fresh != nullptr;
    const bool pc = cnt && rf.in_code != nullptr;  // coded priors (continuous refills only)
    const bool inplace = scratch == v2c.get();     // the resident pool, or its placement probe
    const int kc = timing ? K_UNCOUNTED : K_VAR;
    int rc = LDPC_OK;
    bool ok = true;  // the columns per wave / the degree have a kernel
    if (p.msa_c) {  // N % 16 == 0 (plan_engine)
        int cpw = std::min(var_cpw_for(rf), 4);
        if (N % (4 * cpw) != 0) cpw = 1;  // (N % 16 == 0: every CPW but 3 divides)
        const unsigned nb = gt * (unsigned)(N / (4 * cpw));
        const double* rec = msa_rec(scratch);
        const uint16_t* meta = msa_meta(scratch, p.c2v_tiles, M);
        ok = dispatch(cpw, std::integer_sequence<int, 1, 2, 3, 4>{}, [&](auto CPW, auto CONT, auto NT, auto PC) {
            if constexpr (CONT() || !PC())
                rc = launch(kc, (k_var_msa_c<72, 8, CONT(), CPW(), NT(), PC()>), dim3(nb), dim3(256), rec, meta, v2c, prior,
                            hard, d_sgn, active, dg.col_er, pt, N, M, E, t0, (uint32_t)gt, dg.msa_pa, dg.msa_pb, rf);
        }, cnt, p.nt_d, pc);
    } else if (reg8 && p.fuse_block >= 0 && cnt && inplace) {
        // the resident pool's steps with a fused row block (plan_engine: BP,
        // (8, 72)-regular, default columns per wave): one workgroup per row of
        // the block, which also finishes that row's check (k_check_bp_skip)
        if (t0 != 0 || timing) { set_error("fused row block: bad state"); return LDPC_ERR_ARG; }
        const dim3 grid((unsigned)(M / 8), gt);
        with_bools([&](auto PC) {
            rc = launch(kc, (k_var_bp_fused<kFuseWaves, kFuseWindow, PC()>), grid, dim3(64 * kFuseWaves), v2c, prior, hard,
                        active, dg.col_edge, dg.col_idx, pt, N, E, p.fuse_block * (M / 8), rf);
        }, pc);
    } else if (reg8) {
        const int want = var_cpw_for(rf);
        const int cpw = (want != 3 && N % (4 * want) == 0) ? want : 1;
        const dim3 grid((unsigned)((N + 4 * cpw - 1) / (4 * cpw)), gt);
        // in place is never nontemporal
        ok = dispatch(cpw, std::integer_sequence<int, 1, 2, 4, 8>{},
                      [&](auto CPW, auto MSA, auto NT, auto CONT, auto IP, auto PC) {
            if constexpr (!(IP() && NT()) && (CONT() || !PC()))
                rc = launch(kc, (k_var_m<MSA(), 8, NT(), CONT(), CPW(), IP(), PC()>), grid, dim3(256), scratch, v2c, prior,
                            hard, active, dg.col_edge, pt, N, E, t0, rf);
        }, algo == LDPC_ALGO_MSA, p.nt_d && !inplace, cnt, inplace, pc);
    } else {
        const dim3 grid((N + 3) / 4, gt), blk(256);
        // generic column degrees: registers up to the bucket of dv_max, else memory
        const int vb = gen_bucket(g->dv_max, VarBuckets{});
        const bool bp = algo == LDPC_ALGO_BP;
        if (cnt) {
            if (!vb) { set_error("continuous mode needs column degrees <= 32"); return LDPC_ERR_ARG; }
            dispatch(vb, VarBuckets{}, [&](auto D, auto MSA, auto PC, auto IP) {
                rc = launch(kc, (k_var_gr_cont<MSA(), D(), PC(), IP()>), grid, blk, scratch, v2c, prior, hard, active,
                            dg.col_ptr, dg.col_edge, pt, N, E, t0, rf);
            }, algo == LDPC_ALGO_MSA, pc, inplace);
        } else {
            const bool in_regs = dispatch(vb, VarBuckets{}, [&](auto D, auto MSA) {
                rc = launch(kc, k_var_gr<MSA(), D()>, grid, blk, scratch, v2c, prior, hard, active, dg.col_ptr,
                            dg.col_edge, pt, N, E, t0);
            }, !bp);
            if (!in_regs && bp) rc = launch(kc, k_var_bp_gen, grid, blk, scratch, v2c, prior, hard, active, dg.col_ptr, dg.col_edge, pt, N, E, t0);
            else if (!in_regs) rc = launch(kc, k_var_msa_gen, grid, blk, scratch, v2c, prior, hard, active, dg.col_ptr, dg.col_edge, pt, N, E, t0);
        }
    }
    if (!ok) { set_error("variable phase: no kernel for these columns per wave"); return LDPC_ERR_ARG; }
    return rc;
}

// Fixed passes: every codeword of the pass is initialised at once and masked
// out of later kernels when it stops.  The sequence is stated here once; the
// fp64 decoders (run_chunk) and the integer ones (run_chunk_int) supply
// init(tiles), check(t0, gt), var(t0, gt, n, pt) and finalize(tiles).
template <typename Init, typename Check, typename Var, typename Final>
int Engine::fixed_pass(const DecodeCall& c, Init&& init, Check&& check, Var&& var, Final&& finalize)
{
    using namespace dev;
    const int32_t M = g->M, N = g->N;
    const int64_t Bc = c.B, tiles = (Bc + 63) / 64;
    const bool reg_rowT = g->regular_dc && dg.col_idx_T != nullptr;
    int rc;
    if (c.post && (rc = post_t.ensure((size_t)p.cap * N, stream.get()))) return rc;
    double* pt = c.post ? post_t.get() : nullptr;
    const dim3 blk(256);
    if ((rc = init(tiles))) return rc;
    for (int32_t n = 0;; n++) {
        if (reg_rowT && g->dc_max == 72)
            rc = launch(K_SYN, k_syndrome<72>, dim3((unsigned)tiles), dim3(1024), hard, active, iters, valid, dg.row_ptr,
                        dg.col_idx, dg.col_idx_T, M, N, n, c.max_iter);
        else
            rc = launch(K_SYN, k_syndrome<0>, dim3((unsigned)tiles), dim3(1024), hard, active, iters, valid, dg.row_ptr,
                        dg.col_idx, dg.col_idx_T, M, N, n, c.max_iter);
        if (rc) return rc;
        if (n >= c.max_iter) break;
        // groups of G tiles: check(group) then variable(group), the group's
        // c2v in the scratch
        for (int64_t t0 = 0; t0 < tiles; t0 += p.group_tiles) {
            const unsigned gt = (unsigned)std::min<int64_t>(p.group_tiles, tiles - t0);
            if ((rc = check(t0, gt)) || (rc = var(t0, gt, n, pt))) return rc;
        }
    }
    if (c.post && (rc = finalize(tiles))) return rc;
    if (c.hard) {
        const int64_t nblk = Bc * ((N + 255) / 256);
        const unsigned grid = (unsigned)std::min<int64_t>(nblk, 1 << 20);
        if ((rc = launch(K_FINAL, k_unpack_hard, dim3(grid), blk, hard, c.hard, Bc, N))) return rc;
    }
    hipStream_t s = stream.get();
    if (c.iters) LDPC_HIP(hipMemcpyAsync(c.iters, iters.get(), (size_t)Bc * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (c.valid) LDPC_HIP(hipMemcpyAsync(c.valid, valid.get(), (size_t)Bc, hipMemcpyDeviceToDevice, s));
    return LDPC_OK;
}

int Engine::run_chunk(const DecodeCall& c)
{
    using namespace dev;
    const int32_t N = g->N;
    const int64_t E = g->E;
    const int msa = algo == LDPC_ALGO_MSA;
    if (msa && c.in_kind == LDPC_IN_LR) { set_error("min-sum takes LLR input"); return LDPC_ERR_ARG; }
    if (msa && c.post_kind == LDPC_POST_RATIO) { set_error("LDPC_POST_RATIO is BP-only"); return LDPC_ERR_ARG; }
    const dim3 blk(256);
    return fixed_pass(
        c,
        [&](int64_t tiles) {
            return launch(K_INIT, k_init, dim3((N + 63) / 64, (unsigned)tiles), blk, c.in, c.in_kind == LDPC_IN_LLR ? 1 : 0,
                          msa, c.B, N, E, dg.col_ptr, dg.col_edge, prior, v2c, hard, active, iters, valid, d_sgn,
                          dg.msa_pa, dg.msa_pb);
        },
        [&](int64_t t0, unsigned gt) { return launch_check(c2v(), t0, gt, nullptr); },
        [&](int64_t t0, unsigned gt, int32_t, double* pt) { return launch_var(c2v(), t0, gt, pt, dev::Refill{}); },
        [&](int64_t tiles) {
            return launch(K_FINAL, k_finalize, dim3((N + 3) / 4, (unsigned)tiles), blk, post_t.p, prior, iters, c.post, msa,
                          c.post_kind == LDPC_POST_RATIO ? 1 : 0, c.B, N);
        });
}

int Engine::set_params(int32_t precision, double step, int32_t beta, uint64_t seed)
{
    if (precision < 2 || precision > 16 || !(step > 0) || beta < 0) {
        set_error("quantized min-sum needs 2 <= precision <= 16, step > 0, offset >= 0");
        return LDPC_ERR_ARG;
    }
    q_precision = precision;
    q_step = step;
    q_beta = beta;
    tie_seed = seed;
    return LDPC_OK;
}

// Integer-message decoders (kernels_int.hpp): the fixed passes on int32 views
// of the fp64 buffers; c.tie_base = global index of the pass's first codeword
// (tie hash).
int Engine::run_chunk_int(const DecodeCall& c)
{
    using namespace dev;
    const int32_t M = g->M, N = g->N;
    const int64_t E = g->E;
    IntParams ip{};
    ip.algo = algo;
    ip.max_value = (1 << (q_precision - 1)) - 1;  // Set_MSA dec.cpp:1688-1689
    ip.min_value = -ip.max_value;
    ip.beta = q_beta;
    ip.step = q_step;
    ip.seed = tie_seed;
    const int dv = g->dv_max;  // D_v (CheckRegular)
    if (algo == LDPC_ALGO_GALLAGER_A) { ip.b_var = dv - 1; ip.b_dec = dv; }
    else if (algo == LDPC_ALGO_GALLAGER_B1) { ip.b_var = dv - 2; ip.b_dec = dv - 1; }
    else { ip.b_var = dv / 2 + dv % 2; ip.b_dec = dv / 2 + 1; }
    int32_t* iv2c = reinterpret_cast<int32_t*>(v2c.get());
    int32_t* ic2v = reinterpret_cast<int32_t*>(c2v());
    int32_t* iprior = reinterpret_cast<int32_t*>(prior.get());
    const dim3 blk(256);
    return fixed_pass(
        c,
        [&](int64_t tiles) {
            return launch(K_INIT, k_init_int, dim3((N + 63) / 64, (unsigned)tiles), blk, c.in, c.B, c.tie_base, N, E,
                          dg.col_ptr, dg.col_edge, ip, iprior, iv2c, hard, active, iters, valid);
        },
        [&](int64_t t0, unsigned gt) {
            return launch(K_CHECK, k_check_int, dim3((M + 3) / 4, gt), blk, iv2c, ic2v, active, dg.row_ptr, M, E, t0, ip);
        },
        [&](int64_t t0, unsigned gt, int32_t n, double* pt) {
            return launch(K_VAR, k_var_int, dim3((N + 3) / 4, gt), blk, ic2v, iv2c, iprior, hard, active, dg.col_ptr,
                          dg.col_edge, pt, N, E, t0, c.tie_base, n, ip);
        },
        [&](int64_t tiles) {
            return launch(K_FINAL, k_finalize_int, dim3((N + 3) / 4, (unsigned)tiles), blk, post_t.p, iprior, iters, c.post,
                          c.B, N);
        });
}

// Coded input.  The continuous schedules keep every lane's prior as its code
// (1 byte per column and lane instead of 8; the kernels look the value up in
// the 256-entry table); the others decode fp64 input expanded from the codes
// one pass of <= cap codewords at a time.  Either way each codeword sees
// exactly the prior values the table gives its codes.
int Engine::decode_codes(const int8_t* d_codes, const double* h_table, int table_kind, int64_t B, int32_t max_iter,
                         uint8_t* d_hard, double* d_post, int post_kind, int32_t* d_iters, uint8_t* d_valid,
                         double* d_stage, int64_t tie_base)
{
    if (B < 0 || max_iter < 0) { set_error("B and max_iter must be >= 0"); return LDPC_ERR_ARG; }
    if (!h_table || (B > 0 && !d_codes)) { set_error("decode_codes: null codes or table"); return LDPC_ERR_ARG; }
    if (table_kind != LDPC_IN_LLR && table_kind != LDPC_IN_LR) { set_error("table kind: LDPC_IN_LLR or LDPC_IN_LR"); return LDPC_ERR_ARG; }
    const bool bp = algo == LDPC_ALGO_BP;
    if (!bp && table_kind != LDPC_IN_LLR) { set_error("min-sum and the integer decoders take an LLR table"); return LDPC_ERR_ARG; }
    if (B == 0) return LDPC_OK;
    LDPC_HIP(hipSetDevice(device));
    hipStream_t s = stream.get();
    constexpr int T = 256;
    // the prior of code k: BP's LR (the host libm exp of an LLR table, as
    // DNA_main.cpp:1344 computes LR), the LLR otherwise
    double tab[T];
    for (int i = 0; i < T; i++) tab[i] = (bp && table_kind == LDPC_IN_LLR) ? std::exp(h_table[i]) : h_table[i];
    int rc;
    if ((rc = d_ptab.ensure(T, s)) || (rc = h_ptab.ensure(T, s))) return rc;
    if (!ptab_valid || std::memcmp(tab, h_ptab.get(), sizeof tab) != 0) {
        // the previous upload (and every kernel that reads the table) done first
        LDPC_HIP(hipStreamSynchronize(s));
        std::memcpy(h_ptab.get(), tab, sizeof tab);
        LDPC_HIP(hipMemcpyAsync(d_ptab.get(), h_ptab.get(), sizeof tab, hipMemcpyHostToDevice, s));
        ptab_valid = true;
    }
    const DecodeCall all{nullptr, d_codes, bp ? LDPC_IN_LR : LDPC_IN_LLR, g->N, B, max_iter, d_hard, d_post, post_kind,
                         d_iters, d_valid, tie_base};
    if (p.cont && algo < LDPC_ALGO_QMSA) {
        if ((rc = pcode.ensure((size_t)p.cap * g->N, s))) return rc;
        return run_cont(all);
    }
    // fp64 staging of one pass: the caller's (the host API's d_in) or the
    // engine's own, sized to the largest pass seen
    const int64_t pass = std::min<int64_t>(p.cap, B);
    if (!d_stage && (rc = d_expand.ensure((size_t)pass * g->N, s))) return rc;
    double* stage = d_stage ? d_stage : d_expand.get();
    for (int64_t b0 = 0; b0 < B; b0 += p.cap) {
        DecodeCall c = all.slice(b0, std::min<int64_t>(p.cap, B - b0));
        if ((rc = expand_lr(c.codes, d_ptab.get(), stage, c.B * (int64_t)g->N, s))) return rc;
        c.codes = nullptr;
        c.in = stage;
        if ((rc = decode(c))) return rc;
    }
    return LDPC_OK;
}

int Engine::decode(const double* d_in, int in_kind, int64_t B, int32_t max_iter, uint8_t* d_hard, double* d_post,
                   int post_kind, int32_t* d_iters, uint8_t* d_valid, int64_t tie_base)
{
    return decode(DecodeCall{d_in, nullptr, in_kind, g->N, B, max_iter, d_hard, d_post, post_kind, d_iters, d_valid, tie_base});
}

int Engine::decode(const DecodeCall& c)
{
    if (c.B < 0 || c.max_iter < 0) { set_error("B and max_iter must be >= 0"); return LDPC_ERR_ARG; }
    if (c.B == 0) return LDPC_OK;
    LDPC_HIP(hipSetDevice(device));
    const bool int_algo = algo >= LDPC_ALGO_QMSA;
    if (int_algo) {
        if (c.in_kind != LDPC_IN_LLR) { set_error("integer decoders take LLR input"); return LDPC_ERR_ARG; }
        if (c.post_kind == LDPC_POST_RATIO && c.post) { set_error("LDPC_POST_RATIO is BP-only"); return LDPC_ERR_ARG; }
    } else if (p.cont) {
        return run_cont(c);
    }
    // passes of <= cap codewords; the fp64 decoders balance them (multiples of 64 except the tail)
    const int64_t npass = (c.B + p.cap - 1) / p.cap;
    const int64_t per = int_algo ? p.cap : std::min<int64_t>(p.cap, ((c.B + npass - 1) / npass + 63) / 64 * 64);
    for (int64_t b0 = 0; b0 < c.B; b0 += per) {
        const DecodeCall pass = c.slice(b0, std::min<int64_t>(per, c.B - b0));
        if (int rc = int_algo ? run_chunk_int(pass) : run_chunk(pass)) return rc;
    }
    return LDPC_OK;
}

int Engine::sync()
{
    LDPC_HIP(hipSetDevice(device));
    LDPC_HIP(hipStreamSynchronize(stream.get()));
    return lp.check_fault();
}

// Continuous batching over the whole batch: lanes are refilled as codewords
// finish (the last syndrome / check block of a tile runs the lane
// bookkeeping, res_arrive), so a 64-codeword tile never idles on its slowest
// member.  The host enqueues steps and stops kLag (1 for a single fill) polls
// after the device reports an empty pool (occupied lanes == 0 once the claim
// counter has passed B); the few surplus steps find no occupied lane.
// A decode that stops on an error (a device fault at a poll, a step overrun)
// leaves the steps it already enqueued running, and they can set the fault
// words again.  Wait for them and clear the words, so that the error belongs
// to this decode alone: the next sync or decode on the engine starts clean.
int Engine::run_cont(const DecodeCall& c)
{
    const int rc = run_cont_steps(c);
    if (rc != LDPC_OK && hipStreamSynchronize(stream.get()) == hipSuccess) lp.clear_faults();
    return rc;
}

int Engine::run_cont_steps(const DecodeCall& c)
{
    using namespace dev;
    constexpr int kRing = LanePool::kRing, kLag = LanePool::kLag;
    const int msa = algo == LDPC_ALGO_MSA;
    if (msa && c.in_kind == LDPC_IN_LR) { set_error("min-sum takes LLR input"); return LDPC_ERR_ARG; }
    if (msa && c.post_kind == LDPC_POST_RATIO) { set_error("LDPC_POST_RATIO is BP-only"); return LDPC_ERR_ARG; }
    if (!c.hard || !c.iters || !c.valid) { set_error("continuous mode needs hard, iters and valid outputs"); return LDPC_ERR_ARG; }
    const int32_t M = g->M, N = g->N;
    const int64_t B = c.B, cap_tiles = p.cap_tiles;
    const int64_t tiles = std::min<int64_t>(cap_tiles, (B + 63) / 64);
    int rc;
    if (c.post && (rc = post_t.ensure((size_t)p.cap * N, stream.get()))) return rc;
    double* pt = c.post ? post_t.get() : nullptr;
    // lane masks, claim counter + occupancy ring and the syndrome words in one launch
    static_assert(1 + kRing <= 256, "occupancy ring");
    if ((rc = launch(K_OTHER, k_cont_reset, dim3((unsigned)std::min<int64_t>((tiles + 255) / 256, 1024)), dim3(256), active,
                     lp.fresh, lp.occ, lp.ctr, 1 + kRing, lp.unsat, lp.done, tiles, lp.ho, cap_tiles)))
        return rc;
    ContState cs{active.get(), lp.fresh.get(), lp.occ.get(), lp.lane_b.get(), lp.lane_n.get(), lp.ctr.get(), nullptr, B};
    cs.ntiles = tiles;
    cs.fault = lp.d_fault;
    cs.debug_bad_lane = p.debug_bad_lane ? 1 : 0;
    const uint64_t q0 = lp.poll_seq;  // this decode's first poll
    ResStep rs{hard.get(), dg.col_idx.get(), lp.unsat.get(), lp.done.get(), lp.fin.get(), lp.fin_b.get(), lp.fin_n.get(),
               N, c.max_iter, cs, ContOut{c.iters, c.valid}, dg.row_ptr.get()};
    const bool syn72 = g->regular_dc && g->dc_max == 72;
    const int hard_vec = ((uintptr_t)c.hard % 8 == 0 && N % 8 == 0) ? 1 : 0;
    Refill rf{lp.fresh.get(), lp.lane_b.get(), c.in, c.in_kind == LDPC_IN_LLR ? 1 : 0, lp.fin.get(), lp.fin_b.get(),
              lp.fin_n.get(), c.hard, c.post, c.post_kind == LDPC_POST_RATIO ? 1 : 0, hard_vec};
    rf.nb = B;
    rf.fault = lp.d_fault;
    if (p.handover) {
        rs.last = lp.ho.get();
        rs.pend = lp.ho.get() + cap_tiles;
        rs.unsat_fin = reinterpret_cast<unsigned long long*>(lp.ho.get() + 2 * cap_tiles);
        rs.pend_b = lp.pend_b.get();
        rs.hard_fin = lp.hard_fin.get();
        rf.last = rs.last;
        rf.pend_b = lp.pend_b.get();
        rf.hard_fin = lp.hard_fin.get();
    }
    if (c.codes) {  // coded input (decode_codes): int8 priors
        rf.in = nullptr;
        rf.in_code = c.codes;
        rf.pcode = pcode.get();
        rf.ptab = d_ptab.get();
    }
    // A batch that fits the lane pool in one fill (the DNA batch) polls one
    // step behind instead of kLag in the resident pool, and in the grouped
    // schedule waits for the step's own poll (below): its steps take >= 30
    // us, time enough to enqueue the next, and the decode ends sooner.
    const bool single_fill = B <= tiles * 64;
    const int lag = single_fill ? 1 : kLag;
    // Host step bound.  A lane finishes its codeword at most max_iter + 2
    // steps after claiming it (refill step, max_iter iterations, the final
    // syndrome), so within every window of max_iter + 2 steps each lane either
    // finishes a codeword or has found the input drained; after
    // ceil(B / lanes) + 1 windows every lane is empty.  The host reads the
    // occupancy up to kLag polls late.  A decode still running past the bound
    // means broken device bookkeeping: stop enqueueing and report it instead
    // of spinning.  LDPC_SCHED_DEBUG_NO_DRAIN ignores the drained reading (tests).
    const int64_t lanes = tiles * 64;
    const int64_t windows = (B + lanes - 1) / lanes + 1;
    auto step_limit = [&](int64_t every) {
        return windows * ((int64_t)c.max_iter + 2) + (int64_t)(lag + 2) * every + 8;
    };
    auto drained = [&](unsigned long long occ) { return occ == 0 && !p.debug_no_drain; };
    auto overrun = [&](int64_t steps) {
        set_error("continuous decode of " + std::to_string(B) + " codewords did not drain within " +
                  std::to_string(steps) + " steps (device lane bookkeeping)");
        return LDPC_ERR_DEVICE;
    };
    if (p.res) {
        // resident pool: every step is check (+ the syndrome of the previous
        // step and the lane bookkeeping, ResStep) then variable (+ the
        // finished codewords' outputs) over the whole pool, messages in place;
        // the occupancy is read every res_poll steps, kLag polls behind.
        // Batches of a few pool fills (the DNA batch) poll every step: the
        // host stops at most kLag steps after the pool empties.
        const int every = B <= 8 * p.cap ? 1 : p.res_poll;
        const int64_t limit = step_limit(every);
        rc = LDPC_OK;
        for (int64_t s = 0; rc == LDPC_OK; s++) {
            if (s >= limit) { rc = overrun(s); break; }
            const bool poll = (s % every) == every - 1;
            const uint64_t q = poll ? lp.poll_seq++ : 0;
            if (poll) lp.poll_arm(rs.cs, q);
            else rs.cs.occ_count = rs.cs.occ_clear = rs.cs.poll_host = nullptr;
            if ((rc = launch_check(c2v(), 0, (unsigned)tiles, &rs))) break;
            if ((rc = launch_var(c2v(), 0, (unsigned)tiles, pt, rf))) break;
            if (poll && q >= q0 + (uint64_t)lag) {
                unsigned long long occ = 0;
                if ((rc = lp.poll_wait(q - lag, &occ, stream.get()))) break;
                if (drained(occ)) break;
            }
        }
        return rc;
    }
    // Grouped steps: the multi-block syndrome (+ lane bookkeeping) of every
    // tile, then check(group) + variable(group) per tile group so the group's
    // c2v stays in the Infinity Cache.  Once the input is drained and few lanes
    // remain, one check + one variable launch over all tiles per step (the
    // tail is launch-bound, and the c2v traffic is small); `low` lags the
    // device by kLag.
    bool low = false;
    // single fill: step 0's refill stores only the prior, step 1's check reads it
    const bool ffp = p.first_fp && single_fill;
    // single fill: wait for the step's own poll -- its syndrome (and with it
    // the poll word) comes first, so the answer arrives while the step's
    // check / variable launches still run, and no empty step follows the
    // drain; step 0 (claims and refills only) is not awaited
    const int glag = single_fill ? 0 : lag;
    Refill rf0 = rf;
    rf0.prior_only = ffp ? 1 : 0;
    const int64_t limit = step_limit(1);
    const dim3 g_syn((unsigned)(p.syn_blocks * tiles));
    for (int64_t s = 0;; s++) {
        if (s >= limit) return overrun(s);
        const uint64_t q = lp.poll_seq++;
        lp.poll_arm(rs.cs, q);
        if (syn72) rc = launch(K_SYN, k_syndrome_split<72>, g_syn, dim3(256), M, rs, (uint32_t)tiles);
        else rc = launch(K_SYN, k_syndrome_split_gen, g_syn, dim3(256), M, rs, (uint32_t)tiles);
        if (rc) return rc;
        const int64_t gstep = low ? std::max(p.group_tiles, p.c2v_tiles) : p.group_tiles;
        if (ffp && c.codes && s == 0 && N % 64 == 0) {
            // single fill on codes: step 0 is the transpose of the claimed
            // rows into the lane codes (+ Init's decision ballots).  It stands
            // in for that step's variable kernel because k_cont_reset left
            // every lane empty, so step 0 has no live lane (active) and no
            // finished one (fin) -- k_fill_codes checks both per tile and
            // reports a violation as a device fault.
            if ((rc = launch(K_INIT, k_fill_codes, dim3((unsigned)(N / 64), (unsigned)tiles), dim3(256), c.codes, lp.lane_b,
                             lp.fresh, pcode.p, d_ptab.p, hard, N, B, lp.d_fault, active, lp.fin)))
                return rc;
            continue;  // (the poll of step 0 is never awaited)
        }
        for (int64_t t0 = 0; t0 < tiles; t0 += gstep) {
            const unsigned gt = (unsigned)std::min<int64_t>(gstep, tiles - t0);
            const dim3 g_rows((M + 3) / 4, gt);
            if (ffp && s == 1) {
                if (c.codes)
                    rc = launch(K_CHECK, (k_check_bp_first<72, true>), g_rows, dim3(256), prior, pcode.p, d_ptab.p,
                                dg.col_idx, c2v_buf, active, M, N, (int64_t)g->E, t0);
                else
                    rc = launch(K_CHECK, (k_check_bp_first<72>), g_rows, dim3(256), prior, pcode.p, d_ptab.p, dg.col_idx,
                                c2v_buf, active, M, N, (int64_t)g->E, t0);
                if (rc) return rc;
            } else if (s == 0) {
                // step 0: the reset left every lane empty and the syndrome
                // launch above only claims codewords, so no lane is active
            } else if ((rc = launch_check(c2v_buf.get(), t0, gt, nullptr))) {
                return rc;
            }
            if ((rc = launch_var(c2v_buf.get(), t0, gt, pt, s == 0 ? rf0 : rf))) return rc;
        }
        if (q >= q0 + (uint64_t)glag && s > 0) {
            unsigned long long occ = 0;
            if ((rc = lp.poll_wait(q - glag, &occ, stream.get()))) return rc;
            if (drained(occ)) break;
            low = occ * 32 < (unsigned long long)(tiles * 64);
        }
    }
    return LDPC_OK;
}

int Engine::gen_bsc(double* d_out, int out_kind, int64_t b0, int64_t B, const uint8_t* d_cw, int32_t n_cw,
                    uint64_t seed, double p, double llr_mag)
{
    if (B <= 0) return LDPC_OK;
    if (n_cw <= 0 || !d_cw || !d_out) { set_error("gen_bsc: bad arguments"); return LDPC_ERR_ARG; }
    LDPC_HIP(hipSetDevice(device));
    double pos = llr_mag, neg = -llr_mag;
    if (out_kind == LDPC_IN_LR) {  // the reference's host exp (DNA_main.cpp:1344)
        pos = std::exp(llr_mag);
        neg = std::exp(-llr_mag);
    }
    const uint64_t seedmix = dev::splitmix64(seed);
    return launch(K_OTHER, dev::k_gen_bsc<double>, dim3(8192), dim3(256), d_out, out_kind == LDPC_IN_LR ? 1 : 0, b0, B,
                  d_cw, n_cw, g->N, seedmix, p, pos, neg);
}

int Engine::gen_bsc_codes(int8_t* d_out, int64_t b0, int64_t B, const uint8_t* d_cw, int32_t n_cw, uint64_t seed,
                          double p)
{
    if (B <= 0) return LDPC_OK;
    if (n_cw <= 0 || !d_cw || !d_out) { set_error("gen_bsc_codes: bad arguments"); return LDPC_ERR_ARG; }
    LDPC_HIP(hipSetDevice(device));
    const uint64_t seedmix = dev::splitmix64(seed);
    return launch(K_OTHER, dev::k_gen_bsc<int8_t>, dim3(8192), dim3(256), d_out, 0, b0, B, d_cw, n_cw, g->N, seedmix, p,
                  (int8_t)1, (int8_t)-1);
}

int Engine::expand_lr(const int8_t* d_code, const double* d_table, double* d_out, int64_t n, hipStream_t s)
{
    if (n <= 0) return LDPC_OK;
    LDPC_HIP(hipSetDevice(device));
    const int64_t blocks = std::min<int64_t>(4096, (n / 8 + 255) / 256 + 1);
    // the caller's codes may sit at any byte (ldpc_engine_decode_codes states no alignment): 8-byte loads only when aligned
    const int vec8 = reinterpret_cast<uintptr_t>(d_code) % 8 == 0 ? 1 : 0;
    return sampler.launch(K_UNCOUNTED, s, dev::k_lr_table, dim3((unsigned)blocks), dim3(256), d_code, d_table, d_out, n,
                          vec8);
}

int Engine::pack_bits(const uint8_t* d_in, uint8_t* d_out, int64_t nbytes)
{
    if (nbytes <= 0) return LDPC_OK;
    LDPC_HIP(hipSetDevice(device));
    const int64_t blocks = std::min<int64_t>(4096, (nbytes + 255) / 256);
    return launch(K_UNCOUNTED, dev::k_pack_bits, dim3((unsigned)blocks), dim3(256), (const uint64_t*)d_in, d_out, nbytes);
}

// Batched systematic encode (encode_kernels.hpp): per pass of <= ws_tiles
// tiles, clear the ballot words, pack the messages into the information
// positions, row parities (sparse step), T x s into the parity positions
// (dense step), unpack to one byte per bit.
int encode_launch(const EncoderDev& d, hipStream_t stream, const uint8_t* d_msg, int64_t B, uint8_t* d_cw, uint64_t* ws,
                  int64_t ws_tiles)
{
    using namespace dev;
    if (B <= 0) return LDPC_OK;
    if (!d_msg || !d_cw || !ws || ws_tiles < 1 || ws_tiles > kEncPassTiles) { set_error("encode: bad arguments"); return LDPC_ERR_ARG; }
    const size_t N = (size_t)d.N, K = (size_t)d.K;
    uint64_t* w = ws;
    uint64_t* s = ws + (size_t)ws_tiles * N;
    const size_t s_bytes = (size_t)d.Mw * TILE * sizeof(uint64_t);
    const bool in_lds = s_bytes <= ENC_DENSE_LDS_BYTES;
    for (int64_t b0 = 0; b0 < B; b0 += ws_tiles * TILE) {
        const int64_t Bc = std::min<int64_t>(ws_tiles * TILE, B - b0);
        const unsigned tiles = (unsigned)((Bc + TILE - 1) / TILE);
        const uint8_t* m = d_msg + (size_t)b0 * K;
        const int vec4 = ((reinterpret_cast<uintptr_t>(m) | K) & 3) == 0;
        const dim3 b256(256), dense((unsigned)((d.rank + ENC_DENSE_ROWS - 1) / ENC_DENSE_ROWS), tiles);
        const int64_t nblk = Bc * (((int64_t)N + 255) / 256);
        int rc;
        LDPC_HIP(hipMemsetAsync(w, 0, (size_t)tiles * N * sizeof(uint64_t), stream));
        if ((rc = launch(k_enc_pack, dim3((unsigned)((K + ENC_PACK_COLS - 1) / ENC_PACK_COLS), tiles), b256, 0, stream, m,
                         d.info_pos, w, Bc, d.K, d.N, vec4)) ||
            (d.M > 0 && (rc = launch(k_enc_rows, dim3((unsigned)((d.M + 3) / 4), tiles), b256, 0, stream, w, d.row_ptr,
                                     d.col_idx, s, d.M, d.N))) ||
            (d.rank > 0 && (rc = in_lds ? launch(k_enc_dense<true>, dense, b256, (uint32_t)s_bytes, stream, d.T, s,
                                                 d.par_pos, w, d.rank, d.M, d.Mw, d.N)
                                        : launch(k_enc_dense<false>, dense, b256, 0, stream, d.T, s, d.par_pos, w, d.rank,
                                                 d.M, d.Mw, d.N))) ||
            (rc = launch(k_unpack_hard, dim3((unsigned)std::min<int64_t>(nblk, 1 << 20)), b256, 0, stream, w,
                         d_cw + (size_t)b0 * N, Bc, d.N)))
            return rc;
    }
    return LDPC_OK;
}

}  // namespace ldpc

// --- the error-rate simulation (channel_sim.hpp, error_rate.hpp) ---
#include "channel_sim_kernels.hpp"
