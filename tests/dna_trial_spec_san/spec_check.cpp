// spec_check.cpp -- TEST INFRASTRUCTURE: the speculating form of the trial loop
// (csrc/dna_trial.hpp) under ASan + UBSan, as a stand-alone
// host program (no HIP).  tests/test_dna_trial_spec_san.py compiles it with g++
// into a temporary directory and runs it:
//
//   spec_check
//
// The decoder is a stub whose verdict is a function of the LLRs alone, as a real
// decoder's is: hard = (LLR < 0), and a row decodes iff |LLR of column 0| > 5 K.
// Column 0 of row r holds +-a_r, so under the growing rescale of the eps2 steps
// rows with a large a_r recover one after the other (rows leave their list in
// the middle of a speculated batch) and rows with a small one never do.  All
// rows fail the first decode: F = n_cw.  The stub copies what it is handed into
// heap buffers of exactly B * N and B bytes and works on those, and every input
// and output of the trial is a heap buffer of exactly its size, so a packed
// batch that is short of its k * F rows, or a row list that is, is an ASan report.
//
// Cases: K = 0, 1, 42, 127, 128 (128: a -128 in a failing row); F = 1, 5, 64,
// 65; steps -1, 2, 64; faithful both ways.  Each is compared with a restatement
// of the flow over the stub's rule (every result field), and its counters with
// a restatement of the rule for the steps of a decoder call; the LLRs the stub
// sees are checked against the unpacked rescale of the row's own codes.
// Exit status 0 iff every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../dna-ldpc-codes_amd/csrc/dna_trial.hpp"

using namespace ldpc;

static int fails = 0, n_cases = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);          \
            fails++;                           \
        }                                      \
    } while (0)

constexpr double kEps = 0.02;

template <class T> static std::unique_ptr<T[]> heap(size_t n, T fill)
{
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; i++) p[i] = fill;
    return p;
}

static std::vector<double> eps2_steps()
{
    std::vector<double> s;
    for (double e = kEps - 0.0005; e > 0.001; e = e - 0.0005) s.push_back(e);
    return s;
}

// dna_pipeline.rescale of code c's first-decode LLR, restated
static double rescaled(int c, double eps2)
{
    const double unit = std::log((1 - kEps) / kEps), x = (double)c * unit;
    const double num = std::log((1 - eps2 + 0.0005) / (eps2 - 0.0005));
    return x == 0 ? x : (x * num) / unit;
}

struct Stub {
    int32_t N, K;
    int calls = 0;
    int64_t rows = 0;
    bool llr_ok = true;
    std::vector<double> seen;  // column 1's LLR of every row of every second decode, in order
};

static bool decodes(double llr0, int32_t K) { return std::fabs(llr0) > 5.0 * (double)K; }

static int stub_decode(void* user, const int8_t* codes, const double* table, int64_t B, int32_t max_iter,
                       uint8_t* hard, uint8_t* valid)
{
    Stub& s = *static_cast<Stub*>(user);
    (void)max_iter;
    const size_t n = (size_t)s.N, mat = (size_t)B * n;
    auto c = heap<int8_t>(mat, 0);
    auto t = heap<double>(256, 0.0);
    auto h = heap<uint8_t>(mat, 0);
    auto v = heap<uint8_t>((size_t)B, 0);
    std::memcpy(c.get(), codes, mat);
    std::memcpy(t.get(), table, 256 * sizeof(double));
    for (int64_t k = 0; k < B; k++) {
        for (size_t j = 0; j < n; j++) h[(size_t)k * n + j] = t[(size_t)(c[(size_t)k * n + j] + 128)] < 0;
        const bool ok = decodes(t[(size_t)(c[(size_t)k * n] + 128)], s.K);
        if (!ok) h[(size_t)k * n + n - 1] ^= 1;
        v[(size_t)k] = ok;
        if (s.calls > 0 && n > 1) s.seen.push_back(t[(size_t)(c[(size_t)k * n + 1] + 128)]);
    }
    std::memcpy(hard, h.get(), mat);
    std::memcpy(valid, v.get(), (size_t)B);
    if (s.calls++ > 0) s.rows += B;
    return LDPC_OK;
}

static int32_t amp(int32_t r, int32_t K) { return K == 0 ? 0 : std::max(1, std::min(K, 127) - (r % 7) * (K / 8)); }

// column 0: +-a_r; the others a pattern within [-K, K]; K = 128: row 0 has a -128
static std::vector<int8_t> make_codes(int32_t n_cw, int32_t N, int32_t K)
{
    std::vector<int8_t> c((size_t)n_cw * N);
    const int32_t M = std::min(K, 127);
    for (int32_t i = 0; i < n_cw; i++)
        for (int32_t j = 0; j < N; j++) {
            int v = M == 0 ? 0 : ((i * 7 + j * 3) % (2 * M + 1)) - M;
            if (j == 0) v = (i & 1) ? -amp(i, K) : amp(i, K);
            if (j == 2 && i == 0) v = K == 128 ? -128 : -M;  // the largest |code| is in a failing row
            c[(size_t)i * N + j] = (int8_t)v;
        }
    return c;
}

struct Want {
    std::vector<int32_t> fail_first, fail_second, second_errors;
    std::vector<uint8_t> hard;
    std::vector<size_t> list_sizes;  // F of every eps2 step that ran
    std::vector<double> seen;        // the LLRs of column 1 in batch order, per decoder call of the rule
    int32_t iterations = 0, decodes = 0, K = 0, P = 0;
    int64_t rows = 0, used = 0;
};

static Want expect(const std::vector<int8_t>& codes, bool genie, int32_t n_cw, int32_t N, int32_t K, bool faithful,
                   int32_t steps)
{
    Want w;
    const std::vector<double> seq = eps2_steps();
    const double unit = std::log((1 - kEps) / kEps);
    w.hard.resize((size_t)n_cw * N);
    w.second_errors.assign((size_t)n_cw, -2);
    for (int32_t i = 0; i < n_cw; i++) {
        for (int32_t j = 0; j < N; j++) w.hard[(size_t)i * N + j] = codes[(size_t)i * N + j] < 0;
        if (!decodes((double)codes[(size_t)i * N] * unit, K)) {
            w.hard[(size_t)i * N + N - 1] ^= 1;
            w.fail_first.push_back(i + 1);
        }
    }
    std::vector<int32_t> fail2 = w.fail_first;
    std::vector<std::vector<int32_t>> lists;
    for (size_t s = 0; s < seq.size() && !fail2.empty(); s++) {
        lists.push_back(fail2);
        w.iterations++;
        std::vector<int32_t> next;
        for (int32_t i : fail2) {
            const bool ok = decodes(rescaled(codes[(size_t)(i - 1) * N], seq[s]), K);
            w.second_errors[(size_t)(i - 1)] = ok ? 0 : (genie ? 1 : -1);
            w.used++;
            if (faithful) next.clear();
            if (!ok) next.push_back(i);
            else w.hard[(size_t)(i - 1) * N + N - 1] = codes[(size_t)(i - 1) * N + N - 1] < 0;
        }
        fail2 = next;
    }
    w.fail_second = fail2;
    // the rule, over the lists
    const bool on = steps != 0 && steps != 1 && !w.fail_first.empty();
    if (on) {
        for (int32_t i : w.fail_first)
            for (int32_t j = 0; j < N; j++) w.K = std::max(w.K, std::abs((int32_t)codes[(size_t)(i - 1) * N + j]));
        w.P = 256 / (2 * w.K + 1);
    }
    for (size_t s = 0; s < lists.size();) {
        const int64_t F = (int64_t)lists[s].size();
        int64_t k = 1;
        if (on) {
            k = std::min<int64_t>(std::min<int64_t>((int64_t)(seq.size() - s), w.P), (F + 63) / 64 * 64 / F);
            if (steps >= 2) k = std::min<int64_t>(k, steps);
            k = std::max<int64_t>(k, 1);
        }
        w.decodes++;
        w.rows += k * F;
        for (int64_t j = 0; j < k && N > 1; j++)
            for (int32_t i : lists[s]) w.seen.push_back(rescaled(codes[(size_t)(i - 1) * N + 1], seq[s + (size_t)j]));
        s += (size_t)k;
    }
    return w;
}

static void one(int32_t n_cw, int32_t N, int32_t K, bool genie, int32_t faithful, int32_t steps)
{
    n_cases++;
    char name[96];
    std::snprintf(name, sizeof name, "F %d N %d K %d genie %d faithful %d steps %d", n_cw, N, K, (int)genie, faithful,
                  steps);
    const std::vector<int8_t> codes = make_codes(n_cw, N, K);
    const size_t n = (size_t)n_cw, mat = n * (size_t)N;
    auto hc = heap<int8_t>(mat, 0);
    auto ht = heap<uint8_t>(mat, 0);
    std::memcpy(hc.get(), codes.data(), mat);
    for (size_t i = 0; i < mat; i++) ht[i] = codes[i] < 0;
    auto ff = heap<int32_t>(n, -9), fs = heap<int32_t>(n, -9), fe = heap<int32_t>(n, -9), se = heap<int32_t>(n, -9);
    auto er = heap<int32_t>((size_t)N, -9);
    auto hd = heap<uint8_t>(mat, 0xEE);
    auto vd = heap<uint8_t>(n, 0xEE);
    ldpc_trial_result r{};
    r.fail_first = ff.get(), r.fail_second = fs.get(), r.first_errors = fe.get(), r.second_errors = se.get();
    r.erasure_index = er.get(), r.hard = hd.get(), r.valid = vd.get();
    auto cnt = heap<ldpc_trial_counters>(1, ldpc_trial_counters{});
    Stub s{N, K};
    std::string err;
    const int rc = trial::run_host_spec(hc.get(), n_cw, N, genie ? ht.get() : nullptr, stub_decode, &s, kEps, 50,
                                        faithful, steps, cnt.get(), &r, &err);
    CHECK(rc == LDPC_OK, "%s: rc %d (%s)", name, rc, err.c_str());
    if (rc != LDPC_OK) return;
    const Want w = expect(codes, genie, n_cw, N, K, faithful != 0, steps);
    CHECK((int32_t)w.fail_first.size() == n_cw, "%s: the case is meant to fail every row first", name);
    CHECK(std::vector<int32_t>(ff.get(), ff.get() + r.n_fail_first) == w.fail_first, "%s: fail_first", name);
    CHECK(std::vector<int32_t>(fs.get(), fs.get() + r.n_fail_second) == w.fail_second, "%s: fail_second", name);
    CHECK(std::vector<int32_t>(se.get(), se.get() + n) == w.second_errors, "%s: second_errors", name);
    CHECK(std::vector<uint8_t>(hd.get(), hd.get() + mat) == w.hard, "%s: hard", name);
    CHECK(r.second_iterations == w.iterations, "%s: %d iterations, expected %d", name, r.second_iterations,
          w.iterations);
    CHECK(r.n == n_cw && r.first_success == 0 && r.second_success == n_cw - (int32_t)w.fail_second.size(),
          "%s: counts", name);
    for (size_t i = 0; i < n; i++) CHECK(fe[i] == (genie ? 1 : -1) && vd[i] == 0, "%s: first_errors / valid", name);
    const ldpc_trial_counters& c = cnt[0];
    CHECK(c.second_decodes == w.decodes && c.second_decodes == s.calls - 1, "%s: %d decodes (%d calls), expected %d",
          name, c.second_decodes, s.calls - 1, w.decodes);
    CHECK(c.second_rows == w.rows && c.second_rows == s.rows, "%s: %lld rows, expected %lld", name,
          (long long)c.second_rows, (long long)w.rows);
    CHECK(c.second_rows_used == w.used, "%s: %lld rows used, expected %lld", name, (long long)c.second_rows_used,
          (long long)w.used);
    CHECK(c.code_absmax == w.K && c.steps_per_decode == w.P, "%s: K %d P %d, expected %d %d", name, c.code_absmax,
          c.steps_per_decode, w.K, w.P);
    if (steps == 0)
        CHECK(c.second_decodes == r.second_iterations && c.second_rows == c.second_rows_used, "%s: off", name);
    CHECK(s.seen.size() == w.seen.size() &&
              (s.seen.empty() || std::memcmp(s.seen.data(), w.seen.data(), s.seen.size() * sizeof(double)) == 0),
          "%s: a decode was handed other LLRs than the rescale of its rows' codes", name);
}

int main()
{
    for (int32_t K : {0, 1, 42, 127, 128})
        for (int32_t F : {1, 5, 64, 65})
            for (int32_t steps : {0, -1, 2, 64})
                for (int32_t faithful = 0; faithful < 2; faithful++) one(F, 7, K, true, faithful, steps);
    one(5, 7, 42, false, 0, -1);  // genie-less
    one(5, 7, 42, false, 1, 3);
    one(5, 1, 1, true, 0, -1);    // N = 1
    {
        n_cases++;
        auto c = heap<int8_t>(6, 1);
        ldpc_trial_result r{};
        Stub s{3, 1};
        std::string err;
        CHECK(trial::run_host_spec(c.get(), 2, 3, nullptr, stub_decode, &s, kEps, 5, 1, -2, nullptr, &r, &err) ==
                      LDPC_ERR_ARG && s.calls == 0 && !err.empty(),
              "steps -2 is not an argument error");
        const int rc = trial::run_host_spec(c.get(), 2, 3, nullptr, stub_decode, &s, kEps, 5, 1, -1, nullptr, &r, &err);
        CHECK(rc == LDPC_OK, "null counters");
    }
    if (fails) {
        std::fprintf(stderr, "spec_check: %d checks failed\n", fails);
        return 1;
    }
    std::printf("spec_check ok: %d cases\n", n_cases);
    return 0;
}
