// dna_trial.hpp -- the trial loop: the control flow of
// ex_decoder/decoder.py:541-664 that dna_pipeline.decode_trial mirrors in
// Python -- first decode, genie comparison, per-strand re_decode counts,
// erasure index, the eps2-rescaled second-decode loop.  Header-only host C++,
// no HIP: the body of ldpc_dna_trial_host and of the device handle
// (ldpc_trial_*, dna_trial_kernels.hpp), and what
// tests/dna_trial_san/trial_check.cpp includes.
//
// The decoder input is one int8 matrix codes [n_cw][N] of count differences:
// row i's LLRs are table[codes + 128].  The first decode uses
// table[k + 128] = k * unit, unit = log((1 - eps) / eps) (decoder.py:314).  The
// rescale of the second decode, x -> (x * num) / den with 0 kept
// (decoder.py:603-609), is an elementwise function of that double, so the
// rescaled input of a failed row is its same codes with the table
// rescale_table(): no fp64 matrix is rebuilt, and the doubles are those of
// dna_pipeline.rescale bit for bit on the same libm.
//
// A backend supplies the decoder and the statistics over whatever memory the
// matrix lives in (HostBackend below: host buffers and a caller's callback;
// dna_trial_kernels.hpp: the device):
//
//   int decode(const int32_t* rows, int64_t B, const double* table, int32_t max_iter)
//       decode B rows of the code matrix -- all of them in order when rows is
//       null (then B = n_cw and the result is the trial's `hard`), else rows
//       rows[0..B) (0-based) into the backend's batch
//   int stats(const int32_t* rows, int64_t B, int32_t* errors, uint8_t* valid, int32_t* re_decode)
//       of the last decode: errors[k] = number of hard != truth in batch row k
//       (0 without a truth), valid[k] its syndrome flag, re_decode[j] (may be
//       null) = rows with hard[k][j] != (code < 0)
//   int keep(const int32_t* rows, const int32_t* pos, int64_t n)
//       batch rows pos[0..n) of the last decode replace rows rows[pos[q]] of `hard`
//   bool has_truth()
// Each returns LDPC_OK or an error code that ends the trial.  The speculating
// form of the loop (run_spec, DESIGN.md sec. 8.10: several eps2 steps per
// decoder call, the control flow replayed over the results) asks for two more
// operations, described there.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ldpc_amd.h"

namespace ldpc {
namespace trial {

constexpr int32_t kErasureThreshold = 140;  // decoder.py:590 (re_index: re_decode > 140)
constexpr double kEpsStep = 0.0005;         // decoder.py:592, :611
constexpr double kEpsStop = 0.001;          // decoder.py:594 (while ... and eps2 > 0.001)
constexpr int32_t kNotRedecoded = -2;       // second_errors of a row the second decode never saw

// table[k + 128] = k * unit (dna_pipeline.code_table)
inline void code_table(double unit, double* table)
{
    for (int k = -128; k < 128; k++) table[k + 128] = (double)k * unit;
}

// dna_pipeline.rescale of code_table(log((1 - eps) / eps)): the same operations in the same order
inline void rescale_table(double eps, double eps2, double* table)
{
    const double num = std::log((1 - eps2 + kEpsStep) / (eps2 - kEpsStep));
    const double den = std::log((1 - eps) / eps);
    const double unit = std::log((1 - eps) / eps);
    for (int k = -128; k < 128; k++) {
        const double x = (double)k * unit;
        table[k + 128] = x == 0 ? x : (x * num) / den;
    }
}

// The argument errors of every form; empty: none.
inline std::string check_args(int64_t n_cw, int64_t N, double eps, int32_t max_iter, const ldpc_trial_result* out)
{
    if (!out) return "null result";
    if (n_cw < 1 || N < 1 || n_cw > INT32_MAX || N > INT32_MAX) return "n_cw and N must be in 1 .. 2^31 - 1";
    if (!(eps > 0.0015 && eps < 0.5)) return "eps must be inside (0.0015, 0.5)";
    if (max_iter < 0) return "max_iter must be >= 0";
    return std::string();
}

inline double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The eps2 values of the second decodes, by the loop's own subtraction chain
// (decoder.py:592-611), so the tables and the stop are the loop's.
inline std::vector<double> eps2_sequence(double eps)
{
    std::vector<double> seq;
    for (double eps2 = eps - kEpsStep; eps2 > kEpsStop; eps2 = eps2 - kEpsStep) seq.push_back(eps2);
    return seq;
}

inline int64_t lanes64(int64_t F) { return (F + 63) / 64 * 64; }

// Speculation.  The engine maps one wave to one (row,
// tile of 64 lanes), so a batch of F rows costs what lanes64(F) rows cost, and
// the decode of (row, eps2 step) depends on nothing else: the spare lanes hold
// the same rows under the next steps' tables, and the control flow is replayed
// over the results.  The codes are small, so several steps' tables fit side by
// side in the one 256-entry table: with K the largest |code|, W = 2K + 1 and
// P = 256 / W, step j of a batch has slice [j * W, j * W + W) and its copy of a
// row carries code + K + j * W - 128.
//
// Steps of one decoder call for a list of F rows with `rem` steps left; steps:
// the caller's setting (-1: as many as fit, n >= 2: at most n).
inline int64_t spec_steps(int64_t F, int64_t rem, int32_t P, int32_t steps)
{
    int64_t k = std::min<int64_t>(std::min<int64_t>(rem, P), lanes64(F) / F);
    if (steps >= 2) k = std::min<int64_t>(k, steps);
    return std::max<int64_t>(k, 1);
}

// T[j * W + (c + K)] = rescale_table(eps, eps2[j])[c + 128] for c in [-K, K], j < k; 0.0 elsewhere
inline void packed_table(double eps, const double* eps2, int64_t k, int32_t K, double* table)
{
    double one[256];
    const int32_t W = 2 * K + 1;
    std::fill(table, table + 256, 0.0);
    for (int64_t j = 0; j < k; j++) {
        rescale_table(eps, eps2[j], one);
        for (int32_t c = -K; c <= K; c++) table[j * W + (c + K)] = one[c + 128];
    }
}

// One trial over n_cw rows of N columns.  Fills every field of *out but hard,
// iters, valid (the backend's), kind, stats, codes_exact and t_llr_s (the
// caller's).  Returns LDPC_OK or the backend's error.  Spec: the form that may
// speculate (run_spec below); `steps` and the backend's absmax / decode_spec
// are used by it alone.  cnt (may be null) gets the counters.
template <bool Spec, class Backend>
int run_impl(Backend& be, int32_t n_cw, int32_t N, double eps, int32_t max_iter, bool faithful, int32_t steps,
             ldpc_trial_result* out, ldpc_trial_counters* cnt)
{
    const bool genie = be.has_truth();
    std::vector<int32_t> errors((size_t)n_cw), re_decode((size_t)N), second((size_t)n_cw, kNotRedecoded);
    std::vector<uint8_t> valid((size_t)n_cw);
    double table[256];
    int rc;
    ldpc_trial_counters c{};

    auto t0 = std::chrono::steady_clock::now();
    code_table(std::log((1 - eps) / eps), table);
    if ((rc = be.decode(nullptr, n_cw, table, max_iter))) return rc;
    if ((rc = be.stats(nullptr, n_cw, errors.data(), valid.data(), re_decode.data()))) return rc;
    out->t_first_s = seconds_since(t0);
    if (!genie)  // a codeword fails iff its syndrome at exit is not zero
        for (int32_t i = 0; i < n_cw; i++) errors[(size_t)i] = valid[(size_t)i] ? 0 : -1;
    std::vector<int32_t> fail;
    for (int32_t i = 0; i < n_cw; i++)
        if (errors[(size_t)i] != 0) fail.push_back(i + 1);
    int32_t n_erasure = 0;
    for (int32_t j = 0; j < N; j++)
        if (re_decode[(size_t)j] > kErasureThreshold) {
            if (out->erasure_index) out->erasure_index[n_erasure] = j;
            n_erasure++;
        }

    // The second decodes.  A decoder call covers steps [s, s + k) of the eps2
    // sequence for the current list (k = 1 unless it speculates): batch row
    // j * F + f is row fail2[f] under step s + j.  The replay walks the steps
    // in order; `cur` holds the list's positions f that are still failing.
    const std::vector<double> seq = eps2_sequence(eps);
    std::vector<int32_t> fail2(fail), rows, cur, next, keep, e2;
    std::vector<uint8_t> v2;
    int32_t iter_sec = 0;
    size_t s = 0;
    t0 = std::chrono::steady_clock::now();
    if constexpr (Spec) {
        if (steps != 0 && steps != 1 && !fail2.empty() && !seq.empty()) {
            rows.resize(fail2.size());
            for (size_t f = 0; f < fail2.size(); f++) rows[f] = fail2[f] - 1;
            if ((rc = be.absmax(rows.data(), (int64_t)rows.size(), &c.code_absmax))) return rc;
            c.steps_per_decode = 256 / (2 * c.code_absmax + 1);
        }
    }
    while (!fail2.empty() && s < seq.size()) {
        const int64_t F = (int64_t)fail2.size();
        int64_t k = 1;
        if constexpr (Spec)
            if (c.steps_per_decode >= 2) k = spec_steps(F, (int64_t)(seq.size() - s), c.steps_per_decode, steps);
        rows.resize((size_t)(k * F));
        e2.assign((size_t)(k * F), 0);
        v2.assign((size_t)(k * F), 0);
        for (int64_t q = 0; q < k * F; q++) rows[(size_t)q] = fail2[(size_t)(q % F)] - 1;
        if (k == 1) {
            rescale_table(eps, seq[s], table);
            if ((rc = be.decode(rows.data(), F, table, max_iter))) return rc;
        } else if constexpr (Spec) {
            packed_table(eps, seq.data() + s, k, c.code_absmax, table);
            if ((rc = be.decode_spec(rows.data(), F, k, c.code_absmax, table, max_iter))) return rc;
        }
        if ((rc = be.stats(rows.data(), k * F, e2.data(), v2.data(), nullptr))) return rc;
        c.second_decodes++;
        c.second_rows += k * F;
        keep.clear();
        cur.resize((size_t)F);
        for (int64_t f = 0; f < F; f++) cur[(size_t)f] = (int32_t)f;
        for (int64_t j = 0; j < k && !cur.empty(); j++) {
            iter_sec++;
            next.clear();
            for (const int32_t f : cur) {
                const int64_t q = j * F + f;
                const int32_t v = genie ? e2[(size_t)q] : (v2[(size_t)q] ? 0 : -1);
                second[(size_t)rows[(size_t)f]] = v;
                if (faithful) next.clear();  // decoder.py:659-661 resets the list per codeword
                if (v != 0) next.push_back(f);
                else keep.push_back((int32_t)q);  // (f leaves the list here: at most one keep per row)
                c.second_rows_used++;
            }
            cur.swap(next);
        }
        s += (size_t)k;
        if (!keep.empty() && (rc = be.keep(rows.data(), keep.data(), (int64_t)keep.size()))) return rc;
        next.clear();
        for (const int32_t f : cur) next.push_back(fail2[(size_t)f]);
        fail2.swap(next);
    }
    out->t_second_s = seconds_since(t0);
    if (cnt) *cnt = c;

    out->n = n_cw;
    out->first_success = n_cw - (int32_t)fail.size();
    out->second_success = n_cw - (int32_t)fail2.size();
    out->second_iterations = iter_sec;
    out->n_fail_first = (int32_t)fail.size();
    out->n_fail_second = (int32_t)fail2.size();
    out->n_erasure = n_erasure;
    if (out->fail_first) std::copy(fail.begin(), fail.end(), out->fail_first);  // (an empty list has no data())
    if (out->fail_second) std::copy(fail2.begin(), fail2.end(), out->fail_second);
    if (out->first_errors) std::copy(errors.begin(), errors.end(), out->first_errors);
    if (out->second_errors) std::copy(second.begin(), second.end(), out->second_errors);
    return LDPC_OK;
}

// One eps2 step per decoder call.
template <class Backend>
int run(Backend& be, int32_t n_cw, int32_t N, double eps, int32_t max_iter, bool faithful, ldpc_trial_result* out)
{
    return run_impl<false>(be, n_cw, N, eps, max_iter, faithful, 0, out, nullptr);
}

// run with up to `steps` eps2 steps per decoder call (0 or 1: off, the calls
// are run's; -1: as many as fit; the caller has refused anything below -1),
// and the counters.  Every field of *out is run's.  Besides run's operations
// the backend supplies
//   int absmax(const int32_t* rows, int64_t F, int32_t* K)
//       *K = the largest |code| over rows rows[0..F), as int32 (-128 gives 128)
//   int decode_spec(const int32_t* rows, int64_t F, int64_t k, int32_t K, const double* table, int32_t max_iter)
//       decode k * F batch rows: row j * F + f is row rows[f] with
//       K + j * (2K + 1) - 128 added to every code, under the packed table.
//       rows holds k * F entries, rows[j * F + f] = rows[f], what the stats
//       and keep calls that follow are handed too.
template <class Backend>
int run_spec(Backend& be, int32_t n_cw, int32_t N, double eps, int32_t max_iter, bool faithful, int32_t steps,
             ldpc_trial_result* out, ldpc_trial_counters* cnt)
{
    return run_impl<true>(be, n_cw, N, eps, max_iter, faithful, steps, out, cnt);
}

// The backend over host buffers: codes [n_cw][N], truth [n_cw][N] or null, and
// the caller's decoder.  `hard` and `valid` of the first decode stay here
// (hard with the second decode's replacements) for the caller to copy out.
struct HostBackend {
    const int8_t* codes;
    const uint8_t* truth;
    int32_t n_cw, N;
    ldpc_trial_decode_fn fn;
    void* user;
    std::vector<uint8_t> hard, valid, bhard, bvalid;
    std::vector<int8_t> bcodes;
    bool batch = false;  // the last decode went to bhard / bvalid

    HostBackend(const int8_t* c, const uint8_t* t, int32_t n, int32_t cols, ldpc_trial_decode_fn f, void* u)
        : codes(c), truth(t), n_cw(n), N(cols), fn(f), user(u), hard((size_t)n * (size_t)cols), valid((size_t)n)
    {
    }
    bool has_truth() const { return truth != nullptr; }
    int decode(const int32_t* rows, int64_t B, const double* table, int32_t max_iter)
    {
        const size_t n = (size_t)N;
        batch = rows != nullptr;
        if (!rows) return fn(user, codes, table, B, max_iter, hard.data(), valid.data());
        bcodes.resize((size_t)B * n);
        bhard.assign((size_t)B * n, 0);
        bvalid.assign((size_t)B, 0);
        for (int64_t k = 0; k < B; k++) std::memcpy(bcodes.data() + (size_t)k * n, codes + (size_t)rows[k] * n, n);
        return fn(user, bcodes.data(), table, B, max_iter, bhard.data(), bvalid.data());
    }
    int absmax(const int32_t* rows, int64_t F, int32_t* K)
    {
        int32_t m = 0;
        for (int64_t f = 0; f < F; f++) {
            const int8_t* r = codes + (size_t)rows[f] * (size_t)N;
            for (int32_t c = 0; c < N; c++) m = std::max<int32_t>(m, r[c] < 0 ? -(int32_t)r[c] : (int32_t)r[c]);
        }
        *K = m;
        return LDPC_OK;
    }
    int decode_spec(const int32_t* rows, int64_t F, int64_t k, int32_t K, const double* table, int32_t max_iter)
    {
        const size_t n = (size_t)N, B = (size_t)(k * F);
        batch = true;
        bcodes.resize(B * n);
        bhard.assign(B * n, 0);
        bvalid.assign(B, 0);
        for (int64_t j = 0; j < k; j++) {
            const int32_t shift = K + (int32_t)j * (2 * K + 1) - 128;
            for (int64_t f = 0; f < F; f++) {
                const int8_t* src = codes + (size_t)rows[f] * n;
                int8_t* dst = bcodes.data() + (size_t)(j * F + f) * n;
                for (size_t c = 0; c < n; c++) dst[c] = (int8_t)((int32_t)src[c] + shift);
            }
        }
        return fn(user, bcodes.data(), table, (int64_t)B, max_iter, bhard.data(), bvalid.data());
    }
    int stats(const int32_t* rows, int64_t B, int32_t* errors, uint8_t* v, int32_t* re_decode)
    {
        const size_t n = (size_t)N;
        const uint8_t* h = batch ? bhard.data() : hard.data();
        const uint8_t* vv = batch ? bvalid.data() : valid.data();
        if (re_decode) std::fill(re_decode, re_decode + N, 0);
        for (int64_t k = 0; k < B; k++) {
            const size_t i = rows ? (size_t)rows[k] : (size_t)k;
            const uint8_t* hk = h + (size_t)k * n;
            int32_t e = 0;
            if (truth)
                for (size_t j = 0; j < n; j++) e += hk[j] != truth[i * n + j];
            if (re_decode)
                for (size_t j = 0; j < n; j++) re_decode[j] += hk[j] != (uint8_t)(codes[i * n + j] < 0);
            errors[k] = e;
            v[k] = vv[k];
        }
        return LDPC_OK;
    }
    int keep(const int32_t* rows, const int32_t* pos, int64_t cnt)
    {
        const size_t n = (size_t)N;
        for (int64_t q = 0; q < cnt; q++)
            std::memcpy(hard.data() + (size_t)rows[pos[q]] * n, bhard.data() + (size_t)pos[q] * n, n);
        return LDPC_OK;
    }
};

// ldpc_dna_trial_host_spec without the error string: *err gets the message of
// an argument error.  iters of *out is not touched (the callback reports
// none); counters may be null.
inline int run_host_spec(const int8_t* codes, int32_t n_cw, int32_t N, const uint8_t* truth, ldpc_trial_decode_fn fn,
                         void* user, double eps, int32_t max_iter, int32_t faithful, int32_t steps,
                         ldpc_trial_counters* counters, ldpc_trial_result* out, std::string* err)
{
    *err = check_args(n_cw, N, eps, max_iter, out);
    if (err->empty() && (!codes || !fn)) *err = "null codes or decoder";
    if (err->empty() && steps < -1) *err = "steps must be >= -1";
    if (!err->empty()) return LDPC_ERR_ARG;
    HostBackend be(codes, truth, n_cw, N, fn, user);
    out->codes_exact = 1;
    out->t_llr_s = 0.0;
    if (int rc = run_spec(be, n_cw, N, eps, max_iter, faithful != 0, steps, out, counters)) {
        *err = "the decoder callback failed";
        return rc;
    }
    if (out->hard) std::memcpy(out->hard, be.hard.data(), be.hard.size());
    if (out->valid) std::memcpy(out->valid, be.valid.data(), be.valid.size());
    return LDPC_OK;
}

// ldpc_dna_trial_host: one eps2 step per decode.
inline int run_host(const int8_t* codes, int32_t n_cw, int32_t N, const uint8_t* truth, ldpc_trial_decode_fn fn,
                    void* user, double eps, int32_t max_iter, int32_t faithful, ldpc_trial_result* out,
                    std::string* err)
{
    return run_host_spec(codes, n_cw, N, truth, fn, user, eps, max_iter, faithful, 0, nullptr, out, err);
}

}  // namespace trial
}  // namespace ldpc
