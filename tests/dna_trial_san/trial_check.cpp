// trial_check.cpp -- TEST INFRASTRUCTURE: the trial loop's host form
// (csrc/dna_trial.hpp) under ASan + UBSan, as a stand-alone host program (no
// HIP).  tests/test_dna_trial_san.py compiles it with g++ into a temporary
// directory and runs it:
//
//   trial_check
//
// The decoder is a stub: row r fails its first rounds[r] decodes (one wrong
// bit, valid 0) and then returns its true codeword.  It finds r in the codes
// themselves (column 0 holds the row number), so a wrong gather shows.  Every
// input and every output lives in a heap buffer of exactly its size (codes and
// truth [n_cw][N], the lists [n_cw], erasure_index [N], hard [n_cw][N]; the
// stub is handed exactly [B][N] / [B] by the code under test), so a read or
// write past an end is an ASan report.  The expected result comes from a plain
// restatement of dna_pipeline.decode_trial over the stub's rules.
// * B = 1 with and without a failure; no failures; rows that recover after 1, 2
//   and 3 rounds next to hopeless ones, faithful both ways;
// * all rows failing until eps2 runs out: the iteration count against the eps2
//   sequence computed here, and its closed form to within the rounding of the
//   last step;
// * genie-less (truth null): the fail lists from the valid flags, errors -1 / 0;
// * more than 140 disagreeing rows in a column: the erasure index;
// * every output pointer null; a failing callback; the argument errors.
// Exit status 0 iff every check held.
#include <climits>
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

struct Stub {
    int32_t n_cw, N;
    const uint8_t* truth;         // the stub's own copy: the trial may run without one
    std::vector<int32_t> rounds;  // decodes row r fails (INT_MAX: all)
    std::vector<int32_t> seen;    // decodes of row r so far
    double eps;
    int calls = 0, fail_at = -1;  // fail_at: the call that returns an error
    bool table_ok = true;
};

static int stub_decode(void* user, const int8_t* codes, const double* table, int64_t B, int32_t max_iter,
                       uint8_t* hard, uint8_t* valid)
{
    Stub& s = *static_cast<Stub*>(user);
    const int call = s.calls++;
    if (call == s.fail_at) return LDPC_ERR_DEVICE;
    (void)max_iter;
    // the table: k * unit first, then the rescale of the eps2 sequence
    double want[256];
    const double unit = std::log((1 - s.eps) / s.eps);
    if (call == 0) {
        for (int k = -128; k < 128; k++) want[k + 128] = (double)k * unit;
    } else {
        double eps2 = s.eps - 0.0005;
        for (int q = 1; q < call; q++) eps2 = eps2 - 0.0005;
        const double num = std::log((1 - eps2 + 0.0005) / (eps2 - 0.0005));
        for (int k = -128; k < 128; k++) want[k + 128] = k == 0 ? 0.0 : (((double)k * unit) * num) / unit;
    }
    if (std::memcmp(want, table, sizeof want) != 0) s.table_ok = false;
    for (int64_t k = 0; k < B; k++) {
        const int32_t r = (uint8_t)codes[(size_t)k * s.N];
        if (r >= s.n_cw) return LDPC_ERR_ARG;
        std::memcpy(hard + (size_t)k * s.N, s.truth + (size_t)r * s.N, (size_t)s.N);
        const bool bad = s.seen[(size_t)r]++ < s.rounds[(size_t)r];
        if (bad) hard[(size_t)k * s.N + (size_t)(s.N - 1)] ^= 1;
        valid[k] = !bad;
    }
    return LDPC_OK;
}

struct Res {
    int rc = 0;
    std::string err;
    ldpc_trial_result r{};
    std::vector<int32_t> fail_first, fail_second, first_errors, second_errors, erasure;
    std::vector<uint8_t> hard, valid;
};

template <class T> static std::unique_ptr<T[]> heap(size_t n, T fill)
{
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; i++) p[i] = fill;
    return p;
}

// codes: column 0 = the row number, the others a fixed pattern of signs
static std::vector<int8_t> make_codes(int32_t n_cw, int32_t N, bool col3_negative)
{
    std::vector<int8_t> c((size_t)n_cw * N);
    for (int32_t i = 0; i < n_cw; i++)
        for (int32_t j = 0; j < N; j++) {
            int v = ((i * 7 + j * 3) % 11) - 5;
            if (j == 0) v = (int8_t)(uint8_t)i;
            if (j == 3 && col3_negative) v = -4;
            c[(size_t)i * N + j] = (int8_t)v;
        }
    return c;
}

static std::vector<uint8_t> make_truth(int32_t n_cw, int32_t N)
{
    std::vector<uint8_t> t((size_t)n_cw * N);
    for (int32_t i = 0; i < n_cw; i++)
        for (int32_t j = 0; j < N; j++) t[(size_t)i * N + j] = (uint8_t)((i + j * j) & 1);
    for (int32_t i = 0; i < n_cw && N > 3; i++) t[(size_t)i * N + 3] = 0;
    return t;
}

static Res run_trial(const std::vector<int8_t>& codes, const std::vector<uint8_t>& truth, bool genie, int32_t n_cw,
                     int32_t N, const std::vector<int32_t>& rounds, double eps, int32_t faithful, bool outputs = true,
                     int fail_at = -1, bool* table_ok = nullptr)
{
    n_cases++;
    const size_t n = (size_t)n_cw, mat = n * (size_t)N;
    auto hc = heap<int8_t>(mat, 0);
    auto ht = heap<uint8_t>(mat, 0);
    std::memcpy(hc.get(), codes.data(), mat);
    std::memcpy(ht.get(), truth.data(), mat);
    Stub s{n_cw, N, ht.get(), rounds, std::vector<int32_t>(n, 0), eps};
    s.fail_at = fail_at;
    auto ff = heap<int32_t>(n, -9), fs = heap<int32_t>(n, -9), fe = heap<int32_t>(n, -9), se = heap<int32_t>(n, -9);
    auto er = heap<int32_t>((size_t)N, -9);
    auto hd = heap<uint8_t>(mat, 0xEE);
    auto vd = heap<uint8_t>(n, 0xEE);
    Res o;
    if (outputs) {
        o.r.fail_first = ff.get();
        o.r.fail_second = fs.get();
        o.r.first_errors = fe.get();
        o.r.second_errors = se.get();
        o.r.erasure_index = er.get();
        o.r.hard = hd.get();
        o.r.valid = vd.get();
    }
    o.rc = trial::run_host(hc.get(), n_cw, N, genie ? ht.get() : nullptr, stub_decode, &s, eps, 50, faithful, &o.r,
                           &o.err);
    if (table_ok) *table_ok = s.table_ok;
    if (o.rc == LDPC_OK && outputs) {
        o.fail_first.assign(ff.get(), ff.get() + o.r.n_fail_first);
        o.fail_second.assign(fs.get(), fs.get() + o.r.n_fail_second);
        o.first_errors.assign(fe.get(), fe.get() + n);
        o.second_errors.assign(se.get(), se.get() + n);
        o.erasure.assign(er.get(), er.get() + o.r.n_erasure);
        o.hard.assign(hd.get(), hd.get() + mat);
        o.valid.assign(vd.get(), vd.get() + n);
        for (size_t i = (size_t)o.r.n_fail_first; i < n; i++) CHECK(ff[i] == -9, "fail_first written past its count");
        for (size_t i = (size_t)o.r.n_fail_second; i < n; i++) CHECK(fs[i] == -9, "fail_second written past its count");
        for (size_t j = (size_t)o.r.n_erasure; j < (size_t)N; j++) CHECK(er[j] == -9, "erasure_index written past its count");
    }
    return o;
}

// dna_pipeline.decode_trial over the stub's rules, restated.
struct Want {
    std::vector<int32_t> fail_first, fail_second, first_errors, second_errors, erasure;
    std::vector<uint8_t> hard;
    int32_t iterations = 0;
};

static Want expect(const std::vector<int8_t>& codes, const std::vector<uint8_t>& truth, bool genie, int32_t n_cw,
                   int32_t N, const std::vector<int32_t>& rounds, double eps, bool faithful)
{
    Want w;
    std::vector<int32_t> seen((size_t)n_cw, 0);
    w.hard = truth;
    w.first_errors.assign((size_t)n_cw, 0);
    w.second_errors.assign((size_t)n_cw, -2);
    for (int32_t i = 0; i < n_cw; i++)
        if (seen[(size_t)i]++ < rounds[(size_t)i]) {
            w.hard[(size_t)i * N + (size_t)(N - 1)] ^= 1;
            w.first_errors[(size_t)i] = genie ? 1 : -1;
            w.fail_first.push_back(i + 1);
        }
    for (int32_t j = 0; j < N; j++) {
        int32_t c = 0;
        for (int32_t i = 0; i < n_cw; i++) c += w.hard[(size_t)i * N + j] != (uint8_t)(codes[(size_t)i * N + j] < 0);
        if (c > 140) w.erasure.push_back(j);
    }
    std::vector<int32_t> fail2 = w.fail_first;
    double eps2 = eps - 0.0005;
    while (!fail2.empty() && eps2 > 0.001) {
        w.iterations++;
        eps2 = eps2 - 0.0005;
        std::vector<int32_t> next;
        for (int32_t i : fail2) {
            const bool bad = seen[(size_t)(i - 1)]++ < rounds[(size_t)(i - 1)];
            w.second_errors[(size_t)(i - 1)] = bad ? (genie ? 1 : -1) : 0;
            if (faithful) next.clear();
            if (bad) next.push_back(i);
            else w.hard[(size_t)(i - 1) * N + (size_t)(N - 1)] = truth[(size_t)(i - 1) * N + (size_t)(N - 1)];
        }
        fail2 = next;
    }
    w.fail_second = fail2;
    return w;
}

static void compare(const char* name, const Res& o, const Want& w, int32_t n_cw)
{
    CHECK(o.rc == LDPC_OK, "%s: rc %d (%s)", name, o.rc, o.err.c_str());
    if (o.rc != LDPC_OK) return;
    CHECK(o.fail_first == w.fail_first, "%s: fail_first", name);
    CHECK(o.fail_second == w.fail_second, "%s: fail_second", name);
    CHECK(o.first_errors == w.first_errors, "%s: first_errors", name);
    CHECK(o.second_errors == w.second_errors, "%s: second_errors", name);
    CHECK(o.erasure == w.erasure, "%s: erasure_index", name);
    CHECK(o.hard == w.hard, "%s: hard", name);
    CHECK(o.r.second_iterations == w.iterations, "%s: %d iterations, expected %d", name, o.r.second_iterations,
          w.iterations);
    CHECK(o.r.n == n_cw && o.r.first_success == n_cw - (int32_t)w.fail_first.size() &&
              o.r.second_success == n_cw - (int32_t)w.fail_second.size(),
          "%s: counts", name);
    for (int32_t i = 0; i < n_cw; i++)
        CHECK(o.valid[(size_t)i] == (w.first_errors[(size_t)i] == 0), "%s: valid[%d]", name, i);
}

static void both(const char* name, int32_t n_cw, int32_t N, const std::vector<int32_t>& rounds, double eps, bool genie,
                 bool col3 = false)
{
    const std::vector<int8_t> codes = make_codes(n_cw, N, col3);
    const std::vector<uint8_t> truth = make_truth(n_cw, N);
    for (int faithful = 0; faithful < 2; faithful++) {
        bool table_ok = false;
        const Res o = run_trial(codes, truth, genie, n_cw, N, rounds, eps, faithful, true, -1, &table_ok);
        compare(name, o, expect(codes, truth, genie, n_cw, N, rounds, eps, faithful != 0), n_cw);
        CHECK(table_ok, "%s: a decode was handed the wrong table", name);
    }
}

int main()
{
    const int never = INT_MAX;
    both("B = 1", 1, 5, {0}, 0.02, true);
    both("B = 1, one retry", 1, 5, {1}, 0.02, true);
    both("B = 1, N = 1", 1, 1, {2}, 0.02, true);
    both("no failures", 6, 9, {0, 0, 0, 0, 0, 0}, 0.02, true);
    both("mixed", 7, 9, {0, 1, never, 2, 0, 3, never}, 0.02, true);
    both("mixed, last recovers", 7, 9, {never, 1, 0, 2, 0, 0, 1}, 0.02, true);
    both("genie-less", 7, 9, {0, 1, never, 2, 0, 3, never}, 0.02, false);
    both("genie-less, none fail", 3, 4, {0, 0, 0}, 0.05, false);
    both("erasure index", 150, 6, std::vector<int32_t>(150, 0), 0.02, true, true);
    {
        const Res o = run_trial(make_codes(150, 6, true), make_truth(150, 6), true, 150, 6,
                                std::vector<int32_t>(150, 0), 0.02, 1);
        CHECK(o.rc == LDPC_OK && !o.erasure.empty() && o.erasure.back() >= 3, "the erasure case has no erasure");
    }

    // all rows failing until eps2 runs out
    for (double eps : {0.02, 0.0016, 0.003, 0.1}) {
        int32_t want = 0;
        for (double e2 = eps - 0.0005; e2 > 0.001; e2 = e2 - 0.0005) want++;
        const double closed = std::ceil((eps - 0.0005 - 0.001) / 0.0005);  // terms of eps - 0.0005 m above 0.001
        CHECK(std::fabs((double)want - closed) <= 1.0, "eps %g: %d iterations, closed form %g", eps, want, closed);
        const std::vector<int8_t> codes = make_codes(4, 5, false);
        const std::vector<uint8_t> truth = make_truth(4, 5);
        for (int faithful = 0; faithful < 2; faithful++) {
            const Res o = run_trial(codes, truth, true, 4, 5, {never, never, never, never}, eps, faithful);
            CHECK(o.rc == LDPC_OK && o.r.second_iterations == want, "eps %g: %d iterations, expected %d", eps,
                  o.r.second_iterations, want);
            CHECK(o.fail_second == (faithful ? std::vector<int32_t>{4} : std::vector<int32_t>{1, 2, 3, 4}),
                  "eps %g faithful %d: fail_second", eps, faithful);
            compare("hopeless", o, expect(codes, truth, true, 4, 5, {never, never, never, never}, eps, faithful != 0), 4);
        }
        if (eps == 0.02) CHECK(want == 37 || want == 38, "eps 0.02 runs %d iterations", want);
    }

    // every output pointer null; a failing callback
    {
        const Res o = run_trial(make_codes(5, 4, false), make_truth(5, 4), true, 5, 4, {0, 1, never, 0, 2}, 0.02, 1,
                                false);
        CHECK(o.rc == LDPC_OK && o.r.n_fail_first == 3 && o.r.n_fail_second == 0 && o.r.n == 5,
              "null outputs: rc %d, %d / %d", o.rc, o.r.n_fail_first, o.r.n_fail_second);
        const Res f0 = run_trial(make_codes(5, 4, false), make_truth(5, 4), true, 5, 4, {0, 1, never, 0, 2}, 0.02, 1,
                                 true, 0);
        const Res f1 = run_trial(make_codes(5, 4, false), make_truth(5, 4), true, 5, 4, {0, 1, never, 0, 2}, 0.02, 1,
                                 true, 2);
        CHECK(f0.rc == LDPC_ERR_DEVICE && f1.rc == LDPC_ERR_DEVICE, "a failing callback: rc %d, %d", f0.rc, f1.rc);
    }

    // the argument errors
    {
        n_cases++;
        auto c = heap<int8_t>(6, 1);
        auto t = heap<uint8_t>(6, 0);
        Stub s{2, 3, t.get(), {0, 0}, {0, 0}, 0.02};
        ldpc_trial_result r{};
        std::string err;
        auto call = [&](const int8_t* codes, int32_t n_cw, int32_t N, ldpc_trial_decode_fn fn, double eps,
                        int32_t max_iter, ldpc_trial_result* out) {
            return trial::run_host(codes, n_cw, N, t.get(), fn, &s, eps, max_iter, 1, out, &err);
        };
        CHECK(call(nullptr, 2, 3, stub_decode, 0.02, 5, &r) == LDPC_ERR_ARG, "null codes");
        CHECK(call(c.get(), 2, 3, nullptr, 0.02, 5, &r) == LDPC_ERR_ARG, "null decoder");
        CHECK(call(c.get(), 2, 3, stub_decode, 0.02, 5, nullptr) == LDPC_ERR_ARG, "null result");
        CHECK(call(c.get(), 0, 3, stub_decode, 0.02, 5, &r) == LDPC_ERR_ARG, "n_cw 0");
        CHECK(call(c.get(), -1, 3, stub_decode, 0.02, 5, &r) == LDPC_ERR_ARG, "n_cw -1");
        CHECK(call(c.get(), 2, 0, stub_decode, 0.02, 5, &r) == LDPC_ERR_ARG, "N 0");
        CHECK(call(c.get(), 2, 3, stub_decode, 0.0015, 5, &r) == LDPC_ERR_ARG, "eps 0.0015");
        CHECK(call(c.get(), 2, 3, stub_decode, 0.5, 5, &r) == LDPC_ERR_ARG, "eps 0.5");
        CHECK(call(c.get(), 2, 3, stub_decode, -0.1, 5, &r) == LDPC_ERR_ARG, "eps < 0");
        CHECK(call(c.get(), 2, 3, stub_decode, std::nan(""), 5, &r) == LDPC_ERR_ARG, "eps NaN");
        CHECK(call(c.get(), 2, 3, stub_decode, 0.02, -1, &r) == LDPC_ERR_ARG, "max_iter -1");
        CHECK(s.calls == 0 && !err.empty(), "an argument error reached the decoder");
    }

    if (fails) {
        std::fprintf(stderr, "trial_check: %d checks failed\n", fails);
        return 1;
    }
    std::printf("trial_check ok: %d cases\n", n_cases);
    return 0;
}
