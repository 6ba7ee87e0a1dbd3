// capi.cpp -- the extern "C" boundary declared in include/ldpc_amd.h: graph
// handles (immutable, shared), device engines, the systematic encoder and the
// small allocators.  ldpc_decode / ldpc_decode_codes run in host_decode.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ldpc_amd.h"
#include "engine.hpp"
#include "gf2.hpp"
#include "graph.hpp"
#include "hip_own.hpp"
#include "host_decode.hpp"

using ldpc::Engine;
using ldpc::HostGraph;
using ldpc::set_error;

struct ldpc_engine {
    std::unique_ptr<Engine> e;
};

namespace {

// Workspace of one encode call in flight (ballot words + row parities of a
// pass).  `ev` is recorded after the call's last kernel, and the next call to
// take the workspace makes its stream wait for it: calls on different streams
// may share workspaces without a host wait.  Move-only: it is with one call
// or in one context's idle list.
struct EncWork {
    ldpc::dev_ptr<uint64_t> buf;
    int64_t tiles = 0;
    ldpc::Event ev;
    bool recorded = false;
};

// An encoder's state on one device: T, the position lists and the CSR arrays
// (uploaded once), the library's own stream, idle workspaces.
struct EncCtx {
    int device = 0;
    ldpc::dev_ptr<int32_t> info_pos, par_pos, row_ptr, col_idx;
    ldpc::dev_ptr<uint64_t> T;
    ldpc::EncoderDev d;  // the kernels' view of the arrays above
    ldpc::Stream own;
    std::vector<EncWork> idle;

    // waits for the work in flight; then the members release themselves
    ~EncCtx()
    {
        (void)hipSetDevice(device);
        if (own) (void)hipStreamSynchronize(own.get());
        for (auto& wk : idle)
            if (wk.ev) (void)hipEventSynchronize(wk.ev.get());
    }
};

constexpr int64_t kEncXfer = 16384;  // ldpc_encode: codewords per pass through device memory

}  // namespace

struct ldpc_encoder {
    ldpc::HostEncoder h;
    std::mutex mu;  // ctx and every EncCtx::idle
    std::vector<std::unique_ptr<EncCtx>> ctx;

    // the device context, created (and the encoder uploaded) on first use
    int context(int device, EncCtx** out)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& c : ctx)
            if (c->device == device) { *out = c.get(); return LDPC_OK; }
        int rc = ldpc::select_device("encoder", device);
        if (rc) return rc;
        auto c = std::make_unique<EncCtx>();
        c->device = device;
        if ((rc = ldpc::upload(c->info_pos, h.info_pos)) || (rc = ldpc::upload(c->par_pos, h.par_pos)) ||
            (rc = ldpc::upload(c->row_ptr, h.row_ptr)) || (rc = ldpc::upload(c->col_idx, h.col_idx)) ||
            (rc = ldpc::upload(c->T, h.T)) || (rc = ldpc::make_stream(c->own)))
            return rc;
        c->d.M = h.M; c->d.N = h.N; c->d.K = h.K; c->d.rank = h.rank; c->d.Mw = h.Mw;
        c->d.info_pos = c->info_pos.get(); c->d.par_pos = c->par_pos.get(); c->d.row_ptr = c->row_ptr.get();
        c->d.col_idx = c->col_idx.get(); c->d.T = c->T.get();
        *out = c.get();
        ctx.push_back(std::move(c));
        return LDPC_OK;
    }
    int take(EncCtx& c, int64_t tiles, EncWork* out)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < c.idle.size(); i++)
                if (c.idle[i].tiles >= tiles) {
                    *out = std::move(c.idle[i]);
                    c.idle.erase(c.idle.begin() + (long)i);
                    return LDPC_OK;
                }
        }
        EncWork wk;
        wk.tiles = tiles;
        int rc;
        if ((rc = ldpc::dev_alloc(wk.buf, ldpc::encode_workspace_words(c.d, tiles))) || (rc = ldpc::make_event(wk.ev)))
            return rc;
        *out = std::move(wk);
        return LDPC_OK;
    }
    void give(EncCtx& c, EncWork wk)
    {
        std::lock_guard<std::mutex> lk(mu);
        c.idle.push_back(std::move(wk));
    }
};

static int fail(int rc, int* err)
{
    if (err) *err = rc;
    return rc;
}

extern "C" {

int ldpc_abi_version(void) { return LDPC_AMD_ABI_VERSION; }

const char* ldpc_last_error(void) { return ldpc::last_error(); }

int ldpc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

ldpc_graph* ldpc_graph_load(const char* pchk_path, int* err)
{
    if (!pchk_path) { set_error("null path"); fail(LDPC_ERR_ARG, err); return nullptr; }
    auto g = std::make_unique<ldpc_graph>();
    std::string msg;
    int rc = ldpc::load_pchk(pchk_path, g->h, &msg);
    if (rc) { set_error(msg); fail(rc, err); return nullptr; }
    if (err) *err = LDPC_OK;
    return g.release();
}

ldpc_graph* ldpc_graph_from_edges(int32_t M, int32_t N, const int32_t* rows, const int32_t* cols, int64_t n_edges,
                                  int* err)
{
    if ((!rows || !cols) && n_edges > 0) { set_error("null edge arrays"); fail(LDPC_ERR_ARG, err); return nullptr; }
    auto g = std::make_unique<ldpc_graph>();
    std::string msg;
    int rc = ldpc::build_graph(M, N, rows, cols, n_edges, g->h, &msg);
    if (rc) { set_error(msg); fail(rc, err); return nullptr; }
    if (err) *err = LDPC_OK;
    return g.release();
}

ldpc_graph* ldpc_graph_load_alist(const char* alist_path, int32_t transpose, int* err)
{
    if (!alist_path) { set_error("null path"); fail(LDPC_ERR_ARG, err); return nullptr; }
    auto g = std::make_unique<ldpc_graph>();
    std::string msg;
    int rc = ldpc::load_alist(alist_path, transpose != 0, g->h, &msg);
    if (rc) { set_error(msg); fail(rc, err); return nullptr; }
    if (err) *err = LDPC_OK;
    return g.release();
}

ldpc_graph* ldpc_graph_rs_ldpc(int32_t s, int32_t rho, int32_t gamma, int32_t* gen_poly, int32_t* coset,
                              int* err)
{
    auto g = std::make_unique<ldpc_graph>();
    std::string msg;
    std::vector<int> gp, cs;
    int rc = ldpc::build_rs_ldpc(s, rho, gamma, g->h, &gp, &cs, &msg);
    if (rc) { set_error(msg); fail(rc, err); return nullptr; }
    if (gen_poly) std::copy(gp.begin(), gp.end(), gen_poly);
    if (coset) std::copy(cs.begin(), cs.end(), coset);
    if (err) *err = LDPC_OK;
    return g.release();
}

int ldpc_graph_save_pchk(const ldpc_graph* g, const char* pchk_path)
{
    if (!g || !pchk_path) { set_error("null argument"); return LDPC_ERR_ARG; }
    std::string msg;
    int rc = ldpc::save_pchk(g->h, pchk_path, &msg);
    if (rc) set_error(msg);
    return rc;
}

int ldpc_graph_save_alist(const ldpc_graph* g, const char* alist_path)
{
    if (!g || !alist_path) { set_error("null argument"); return LDPC_ERR_ARG; }
    std::string msg;
    int rc = ldpc::save_alist(g->h, alist_path, &msg);
    if (rc) set_error(msg);
    return rc;
}

void ldpc_graph_free(ldpc_graph* g) { delete g; }

int ldpc_graph_info(const ldpc_graph* g, int32_t* M, int32_t* N, int64_t* E, int32_t* dv_max, int32_t* regular_dv,
                    int32_t* dc_max, int32_t* regular_dc)
{
    if (!g) { set_error("null graph"); return LDPC_ERR_ARG; }
    if (M) *M = g->h.M;
    if (N) *N = g->h.N;
    if (E) *E = g->h.E;
    if (dv_max) *dv_max = g->h.dv_max;
    if (regular_dv) *regular_dv = g->h.regular_dv;
    if (dc_max) *dc_max = g->h.dc_max;
    if (regular_dc) *regular_dc = g->h.regular_dc;
    return LDPC_OK;
}

int ldpc_graph_blocks(const ldpc_graph* g, int32_t* Q, int32_t* row_blocks, int32_t* col_blocks, int32_t* col_block)
{
    if (!g) { set_error("null graph"); return LDPC_ERR_ARG; }
    const ldpc::BlockLayout* L = ldpc::block_layout_of(g->h);
    if (Q) *Q = L ? L->Q : 0;
    if (row_blocks) *row_blocks = L ? L->GA : 0;
    if (col_blocks) *col_blocks = L ? L->RB : 0;
    if (L && col_block)
        for (size_t q = 0; q < L->col_orig.size(); q++) col_block[L->col_orig[q]] = (int32_t)(q / (size_t)L->Q);
    return LDPC_OK;
}

int ldpc_graph_edges(const ldpc_graph* g, int32_t* row_ptr, int32_t* col_idx, int32_t* col_ptr, int32_t* col_edge)
{
    if (!g) { set_error("null graph"); return LDPC_ERR_ARG; }
    const auto& h = g->h;
    if (row_ptr) std::memcpy(row_ptr, h.row_ptr.data(), h.row_ptr.size() * 4);
    if (col_idx) std::memcpy(col_idx, h.col_idx.data(), h.col_idx.size() * 4);
    if (col_ptr) std::memcpy(col_ptr, h.col_ptr.data(), h.col_ptr.size() * 4);
    if (col_edge) std::memcpy(col_edge, h.col_edge.data(), h.col_edge.size() * 4);
    return LDPC_OK;
}

int ldpc_graph_syndrome(const ldpc_graph* g, const uint8_t* dblk, uint8_t* pchk)
{
    if (!g || !dblk) { set_error("null argument"); return LDPC_ERR_ARG; }
    return ldpc::syndrome_host(g->h, dblk, pchk);
}

int ldpc_decode(const ldpc_graph* g, const double* llr, int64_t B, int32_t max_iter, int32_t algo, uint8_t* hard_out,
                double* post_out, int32_t* iters_out, uint8_t* valid_out, const ldpc_opts* opts)
{
    ldpc::HostInput in;
    in.llr = llr;
    return ldpc::host_decode(g, in, B, max_iter, algo, hard_out, post_out, iters_out, valid_out, opts);
}

int ldpc_decode_codes(const ldpc_graph* g, const int8_t* codes, const double* table, int32_t table_kind, int64_t B,
                      int32_t max_iter, int32_t algo, uint8_t* hard_out, double* post_out, int32_t* iters_out,
                      uint8_t* valid_out, const ldpc_opts* opts)
{
    ldpc::HostInput in;
    in.codes = codes;
    in.table = table;
    in.table_kind = table_kind;
    if (B > 0 && !codes) { set_error("null codes"); return LDPC_ERR_ARG; }
    return ldpc::host_decode(g, in, B, max_iter, algo, hard_out, post_out, iters_out, valid_out, opts);
}

int ldpc_engine_set_params(ldpc_engine* e, int32_t msa_precision, double msa_step, int32_t msa_offset,
                           uint64_t tie_seed)
{
    if (!e) { set_error("null engine"); return LDPC_ERR_ARG; }
    return e->e->set_params(msa_precision, msa_step, msa_offset, tie_seed);
}

ldpc_engine* ldpc_engine_create_ex(const ldpc_graph* g, int32_t device, int32_t algo, int64_t chunk,
                                   const ldpc_schedule* schedule, int* err)
{
    if (!g) { set_error("null graph"); fail(LDPC_ERR_ARG, err); return nullptr; }
    auto e = std::make_unique<ldpc_engine>();
    e->e = std::make_unique<Engine>();
    int rc = e->e->init(&g->h, device, algo, chunk, schedule);
    if (rc) { fail(rc, err); return nullptr; }
    if (err) *err = LDPC_OK;
    return e.release();
}

ldpc_engine* ldpc_engine_create(const ldpc_graph* g, int32_t device, int32_t algo, int64_t chunk, int* err)
{
    return ldpc_engine_create_ex(g, device, algo, chunk, nullptr, err);
}

int ldpc_engine_info(ldpc_engine* e, int64_t* cap, int64_t* group_tiles, int32_t* flags)
{
    if (!e) { set_error("null engine"); return LDPC_ERR_ARG; }
    if (cap) *cap = e->e->p.cap;
    if (group_tiles) *group_tiles = e->e->p.group_tiles;
    if (flags) *flags = e->e->flags();
    return LDPC_OK;
}

void ldpc_engine_free(ldpc_engine* e) { delete e; }

int ldpc_engine_decode(ldpc_engine* e, const double* d_in, int32_t in_kind, int64_t B, int32_t max_iter,
                       uint8_t* d_hard, double* d_post, int32_t post_kind, int32_t* d_iters, uint8_t* d_valid)
{
    if (!e) { set_error("null engine"); return LDPC_ERR_ARG; }
    if (B > 0 && !d_in) { set_error("null input"); return LDPC_ERR_ARG; }
    return e->e->decode(d_in, in_kind, B, max_iter, d_hard, d_post, post_kind, d_iters, d_valid);
}

int ldpc_engine_decode_codes(ldpc_engine* e, const int8_t* d_codes, const double* table, int32_t table_kind,
                             int64_t B, int32_t max_iter, uint8_t* d_hard, double* d_post, int32_t post_kind,
                             int32_t* d_iters, uint8_t* d_valid)
{
    if (!e) { set_error("null engine"); return LDPC_ERR_ARG; }
    return e->e->decode_codes(d_codes, table, table_kind, B, max_iter, d_hard, d_post, post_kind, d_iters, d_valid);
}

int ldpc_engine_sync(ldpc_engine* e)
{
    if (!e) { set_error("null engine"); return LDPC_ERR_ARG; }
    return e->e->sync();
}

void* ldpc_engine_stream(ldpc_engine* e) { return e ? (void*)e->e->stream.get() : nullptr; }

int ldpc_engine_gen_bsc(ldpc_engine* e, double* d_out, int32_t out_kind, int64_t b0, int64_t B,
                        const uint8_t* d_codewords, int32_t n_cw, uint64_t seed, double p, double llr_mag)
{
    if (!e) { set_error("null engine"); return LDPC_ERR_ARG; }
    return e->e->gen_bsc(d_out, out_kind, b0, B, d_codewords, n_cw, seed, p, llr_mag);
}

int ldpc_engine_gen_bsc_codes(ldpc_engine* e, int8_t* d_out, int64_t b0, int64_t B, const uint8_t* d_codewords,
                              int32_t n_cw, uint64_t seed, double p)
{
    if (!e) { set_error("null engine"); return LDPC_ERR_ARG; }
    return e->e->gen_bsc_codes(d_out, b0, B, d_codewords, n_cw, seed, p);
}

int ldpc_engine_profile(ldpc_engine* e, int32_t stride)
{
    if (!e) { set_error("null engine"); return LDPC_ERR_ARG; }
    return e->e->profile(stride);
}

int ldpc_engine_stats(ldpc_engine* e, ldpc_kernel_stats* out)
{
    if (!e || !out) { set_error("null argument"); return LDPC_ERR_ARG; }
    return e->e->stats(out);
}

// ---------------------------------------------------------------------------
// systematic encoding (gf2.hpp: definition, construction, host encoder;
// encode_kernels.hpp: the device path)
// ---------------------------------------------------------------------------
ldpc_encoder* ldpc_encoder_create(const ldpc_graph* g, int* err)
{
    if (!g) { set_error("null graph"); fail(LDPC_ERR_ARG, err); return nullptr; }
    auto e = std::make_unique<ldpc_encoder>();
    std::string msg;
    int rc = ldpc::build_encoder(g->h, e->h, &msg);
    if (rc) { set_error(msg); fail(rc, err); return nullptr; }
    if (err) *err = LDPC_OK;
    return e.release();
}

void ldpc_encoder_free(ldpc_encoder* e) { delete e; }

int ldpc_encoder_info(const ldpc_encoder* e, int32_t* N, int32_t* K, int32_t* rank, int32_t* info_pos, int32_t* par_pos)
{
    if (!e) { set_error("null encoder"); return LDPC_ERR_ARG; }
    if (N) *N = e->h.N;
    if (K) *K = e->h.K;
    if (rank) *rank = e->h.rank;
    if (info_pos) std::copy(e->h.info_pos.begin(), e->h.info_pos.end(), info_pos);
    if (par_pos) std::copy(e->h.par_pos.begin(), e->h.par_pos.end(), par_pos);
    return LDPC_OK;
}

static int encode_args(const ldpc_encoder* e, const void* msg, int64_t B, const void* cw)
{
    if (!e) { set_error("null encoder"); return LDPC_ERR_ARG; }
    if (B < 0) { set_error("B must be >= 0"); return LDPC_ERR_ARG; }
    if (B > 0 && (!msg || !cw)) { set_error("the messages and the codeword buffer are required"); return LDPC_ERR_ARG; }
    if (B > (int64_t)(PTRDIFF_MAX / 8) / (int64_t)std::max<int32_t>(1, e->h.N)) {
        set_error("batch too large: B * N bytes overflow the address space");
        return LDPC_ERR_ARG;
    }
    return LDPC_OK;
}

int ldpc_encode_host(const ldpc_encoder* e, const uint8_t* msg, int64_t B, uint8_t* cw_out)
{
    int rc = encode_args(e, msg, B, cw_out);
    if (rc || B == 0) return rc;
    std::string err;
    rc = ldpc::encode_host(e->h, msg, B, cw_out, &err);
    if (rc) set_error(err);
    return rc;
}

int ldpc_encoder_encode_device(const ldpc_encoder* ec, int32_t device, void* stream, const uint8_t* d_msg, int64_t B,
                               uint8_t* d_cw)
{
    int rc = encode_args(ec, d_msg, B, d_cw);
    if (rc || B == 0) return rc;
    ldpc_encoder* e = const_cast<ldpc_encoder*>(ec);  // the device contexts are a cache behind e->mu
    EncCtx* c = nullptr;
    if ((rc = e->context(device, &c))) return rc;
    LDPC_HIP(hipSetDevice(device));
    hipStream_t st = stream ? (hipStream_t)stream : c->own.get();
    EncWork wk;
    if ((rc = e->take(*c, std::min<int64_t>(ldpc::kEncPassTiles, (B + 63) / 64), &wk))) return rc;
    hipError_t he = wk.recorded ? hipStreamWaitEvent(st, wk.ev.get(), 0) : hipSuccess;
    if (he == hipSuccess) {
        rc = ldpc::encode_launch(c->d, st, d_msg, B, d_cw, wk.buf.get(), wk.tiles);
        he = hipEventRecord(wk.ev.get(), st);
        wk.recorded = he == hipSuccess;
    }
    e->give(*c, std::move(wk));
    if (he != hipSuccess) { set_error(std::string("encode: ") + hipGetErrorString(he)); return LDPC_ERR_DEVICE; }
    if (rc) return rc;
    // no stream of the caller's to wait on: the call itself waits
    if (!stream) LDPC_HIP(hipStreamSynchronize(c->own.get()));
    return LDPC_OK;
}

int ldpc_encode(const ldpc_encoder* e, const uint8_t* msg, int64_t B, uint8_t* cw_out, int32_t device)
{
    int rc = encode_args(e, msg, B, cw_out);
    if (rc || B == 0) return rc;
    const size_t K = (size_t)e->h.K, N = (size_t)e->h.N;
    size_t bad = 0;
    if (!ldpc::message_bytes_ok(msg, (size_t)B * K, &bad)) {
        set_error("message byte " + std::to_string(bad % K) + " of message " + std::to_string(bad / K) +
                  " is neither 0 nor 1");
        return LDPC_ERR_ARG;
    }
    if (ldpc_device_count() < 1) { set_error("no HIP device (ldpc_encode_host encodes on the CPU)"); return LDPC_ERR_DEVICE; }
    if ((rc = ldpc::select_device("ldpc_encode", device))) return rc;
    // any B: passes of kEncXfer codewords through device memory
    const size_t X = (size_t)std::min<int64_t>(B, kEncXfer);
    ldpc::dev_ptr<uint8_t> d_msg, d_cw;
    if ((rc = ldpc::dev_alloc(d_msg, X * K)) || (rc = ldpc::dev_alloc(d_cw, X * N))) return rc;
    for (int64_t b0 = 0; b0 < B; b0 += (int64_t)X) {
        const size_t Bc = (size_t)std::min<int64_t>((int64_t)X, B - b0);
        LDPC_HIP(hipMemcpy(d_msg.get(), msg + (size_t)b0 * K, Bc * K, hipMemcpyHostToDevice));
        if ((rc = ldpc_encoder_encode_device(e, device, nullptr, d_msg.get(), (int64_t)Bc, d_cw.get()))) return rc;  // waits
        LDPC_HIP(hipMemcpy(cw_out + (size_t)b0 * N, d_cw.get(), Bc * N, hipMemcpyDeviceToHost));
    }
    return LDPC_OK;
}

void* ldpc_host_alloc(size_t bytes)
{
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault);
    if (e != hipSuccess) { set_error(std::string("hipHostMalloc: ") + hipGetErrorString(e)); return nullptr; }
    return p;
}

int ldpc_host_free(void* p)
{
    if (p) LDPC_HIP(hipHostFree(p));
    return LDPC_OK;
}

void* ldpc_dev_malloc(int32_t device, size_t bytes)
{
    void* p = nullptr;
    if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
    hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 1));
    if (e != hipSuccess) { set_error(std::string("hipMalloc: ") + hipGetErrorString(e)); return nullptr; }
    return p;
}

int ldpc_dev_free(int32_t device, void* p)
{
    LDPC_HIP(hipSetDevice(device));
    LDPC_HIP(hipFree(p));
    return LDPC_OK;
}

int ldpc_dev_memcpy(int32_t device, void* dst, const void* src, size_t bytes, int32_t kind)
{
    hipMemcpyKind k = kind == LDPC_H2D ? hipMemcpyHostToDevice : kind == LDPC_D2H ? hipMemcpyDeviceToHost
                                                                                   : hipMemcpyDeviceToDevice;
    LDPC_HIP(hipSetDevice(device));
    LDPC_HIP(hipMemcpy(dst, src, bytes, k));
    return LDPC_OK;
}

}  // extern "C"
