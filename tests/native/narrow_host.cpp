// BandEd score-only in two passes (launch_banded_narrow, launch_banded_probe) on the HOST, under sanitizers: the library's
// host layer built with g++ against the fake HIP runtime of tests/native/hip_stub, whose k_banded stand-in gives every task
// the score QE_STUB_BOUND / 2 and one block-column per pass; k_narrow is the host rendering in qe_stages.hip.  Checks the
// pool arithmetic of both launch sequences, the packed list, the counters and the policy's sequence through the C-ABI.
// Built and run by tests/test_host_narrow.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "quicked.h"
#include "quicked_batch.h"

extern "C" quicked_status_t quicked_debug_reload_env(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "narrow_host: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

struct Pairs { std::string pp, tp; std::vector<int64_t> po, to; std::vector<int32_t> pl, tl; int64_t n = 0; };
static Pairs make_pairs(int n, int len) {
    Pairs P;
    P.n = n;
    unsigned x = 12345;
    for (int i = 0; i < n; ++i) {
        P.po.push_back((int64_t)P.pp.size()); P.to.push_back((int64_t)P.tp.size());
        for (int k = 0; k < len; ++k) { x = x * 1664525u + 1013904223u; const char c = "ACGT"[x >> 30]; P.pp.push_back(c); P.tp.push_back(c); }
        P.pl.push_back(len); P.tl.push_back(len);
    }
    return P;
}
static void sw(const char* name, const char* v) { if (v) setenv(name, v, 1); else unsetenv(name); CHECK(quicked_debug_reload_env() >= 0); }

// -> counters[0], counters[7] of one run (sync, or queued + fetch)
static void run(quicked_batch_t* b, int64_t n, bool sync, int expect_score, int64_t& adv, int64_t& second) {
    quicked_params_t p = quicked_default_params();
    p.algo = BANDED; p.only_score = true; p.bandwidth = 15;
    CHECK(quicked_batch_run(b, &p, sync ? 1 : 0) >= 0);
    if (!sync) CHECK(quicked_batch_fetch(b) >= 0);
    std::vector<int32_t> sc((size_t)n), st((size_t)n);
    CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
    for (int64_t i = 0; i < n; ++i) CHECK(sc[(size_t)i] == expect_score);
    int64_t c[8];
    CHECK(quicked_batch_counters(b, c) >= 0);
    adv = c[0]; second = c[7];
}

int main() {
    int64_t adv = 0, second = 0;
    // forced, 2 000-base pairs (cutoff 300, first pass at 150): stub score 35 is accepted, 500 is not
    {
        const Pairs P = make_pairs(200, 2000);
        quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
        CHECK(b);
        sw("QE_SCORE_NARROW", "1");
        for (int sync = 0; sync < 2; ++sync) { run(b, P.n, sync, 35, adv, second); CHECK(adv == P.n && second == 0); }
        sw("QE_STUB_BOUND", "1000");
        for (int sync = 0; sync < 2; ++sync) { run(b, P.n, sync, 500, adv, second); CHECK(adv == 2 * P.n && second == P.n); }
        sw("QE_SCORE_NARROW", "0");
        run(b, P.n, true, 500, adv, second); CHECK(adv == P.n && second == 0);
        quicked_batch_destroy(b);
    }
    // the policy, on a list above the gate of the fake device (QE_STUB_CUS compute units): two passes, single passes, a probe
    {
        const char* cus = getenv("QE_STUB_CUS");
        const int groups = 4 * (cus ? atoi(cus) : 256) + 3;
        const Pairs P = make_pairs(64 * groups - 5, 900);               // cutoff 135 -> 67: four slots against three
        quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
        CHECK(b);
        sw("QE_SCORE_NARROW", nullptr);                                  // stub score 500: every task misses
        const int64_t sampled = 64 * (int64_t)((groups + 15) / 16) - ((groups - 1) % 16 == 0 ? 5 : 0);
        for (int k = 0; k < 18; ++k) {
            run(b, P.n, k % 2 == 0, 500, adv, second);
            if (k == 0) CHECK(adv == 2 * P.n && second == P.n);
            else if (k == 16) CHECK(adv == P.n + sampled && second == 0);
            else CHECK(adv == P.n && second == 0);
        }
        quicked_batch_destroy(b);
    }
    printf("narrow_host ok\n");
    return 0;
}
