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
// Each returns LDPC_OK or an error code that ends the trial.
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

// One trial over n_cw rows of N columns.  Fills every field of *out but hard,
// iters, valid (the backend's), kind, stats, codes_exact and t_llr_s (the
// caller's).  Returns LDPC_OK or the backend's error.
template <class Backend>
int run(Backend& be, int32_t n_cw, int32_t N, double eps, int32_t max_iter, bool faithful, ldpc_trial_result* out)
{
    const bool genie = be.has_truth();
    std::vector<int32_t> errors((size_t)n_cw), re_decode((size_t)N), second((size_t)n_cw, kNotRedecoded);
    std::vector<uint8_t> valid((size_t)n_cw);
    double table[256];
    int rc;

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

    std::vector<int32_t> fail2(fail), next, rows, keep, e2;
    std::vector<uint8_t> v2;
    int32_t iter_sec = 0;
    double eps2 = eps - kEpsStep;
    t0 = std::chrono::steady_clock::now();
    while (!fail2.empty() && eps2 > kEpsStop) {
        iter_sec++;
        rescale_table(eps, eps2, table);
        eps2 = eps2 - kEpsStep;
        const int64_t F = (int64_t)fail2.size();
        rows.resize((size_t)F);
        e2.assign((size_t)F, 0);
        v2.assign((size_t)F, 0);
        for (int64_t k = 0; k < F; k++) rows[(size_t)k] = fail2[(size_t)k] - 1;
        if ((rc = be.decode(rows.data(), F, table, max_iter))) return rc;
        if ((rc = be.stats(rows.data(), F, e2.data(), v2.data(), nullptr))) return rc;
        next.clear();
        keep.clear();
        for (int64_t k = 0; k < F; k++) {
            const int32_t v = genie ? e2[(size_t)k] : (v2[(size_t)k] ? 0 : -1);
            second[(size_t)rows[(size_t)k]] = v;
            if (faithful) next.clear();  // decoder.py:659-661 resets the list per codeword
            if (v != 0) next.push_back(fail2[(size_t)k]);
            else keep.push_back((int32_t)k);
        }
        if (!keep.empty() && (rc = be.keep(rows.data(), keep.data(), (int64_t)keep.size()))) return rc;
        fail2.swap(next);
    }
    out->t_second_s = seconds_since(t0);

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

// ldpc_dna_trial_host without the error string: *err gets the message of an
// argument error.  iters of *out is not touched (the callback reports none).
inline int run_host(const int8_t* codes, int32_t n_cw, int32_t N, const uint8_t* truth, ldpc_trial_decode_fn fn,
                    void* user, double eps, int32_t max_iter, int32_t faithful, ldpc_trial_result* out,
                    std::string* err)
{
    *err = check_args(n_cw, N, eps, max_iter, out);
    if (err->empty() && (!codes || !fn)) *err = "null codes or decoder";
    if (!err->empty()) return LDPC_ERR_ARG;
    HostBackend be(codes, truth, n_cw, N, fn, user);
    out->codes_exact = 1;
    out->t_llr_s = 0.0;
    if (int rc = run(be, n_cw, N, eps, max_iter, faithful != 0, out)) {
        *err = "the decoder callback failed";
        return rc;
    }
    if (out->hard) std::memcpy(out->hard, be.hard.data(), be.hard.size());
    if (out->valid) std::memcpy(out->valid, be.valid.data(), be.valid.size());
    return LDPC_OK;
}

}  // namespace trial
}  // namespace ldpc
