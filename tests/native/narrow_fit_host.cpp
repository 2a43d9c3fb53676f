// The fitted first pass of BandEd score-only in two passes (QE_NARROW_FIT) on the HOST, under sanitizers: the library's host
// layer built with g++ against the fake HIP runtime of tests/native/hip_stub, as tests/native/narrow_host.cpp is.  The stub's
// k_banded gives every task the score QE_STUB_BOUND / 2 (read at every launch) and one block-column per pass; k_narrow is the
// host rendering in qe_stages.hip, the fit's group rule included.  Pairs of 2 000 bases: cutoff 300 (six slots), 150 at half
// (four slots, accepts up to 129: its band holds 64 diagonals below the main one), three slots for any fit, whose roomiest
// cutoff is 128.  So a score of 129 is accepted at half the cutoff and is a miss owed to the fit alone.
// Built and run by tests/test_host_narrow_fit.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "quicked.h"
#include "quicked_batch.h"

extern "C" quicked_status_t quicked_debug_reload_env(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "narrow_fit_host: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

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
    {   // forced: a ratio of 120 / 1024 asks for 36 of 300 -- three slots, cutoff 128
        const Pairs P = make_pairs(200, 2000);
        quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
        CHECK(b);
        sw("QE_SCORE_NARROW", "1");
        sw("QE_NARROW_FIT", "120");
        for (int sync = 0; sync < 2; ++sync) { run(b, P.n, sync, 35, adv, second); CHECK(adv == P.n && second == 0); }
        sw("QE_STUB_BOUND", "256");                                      // 128: the most the fitted band accepts
        for (int sync = 0; sync < 2; ++sync) { run(b, P.n, sync, 128, adv, second); CHECK(adv == P.n && second == 0); }
        sw("QE_STUB_BOUND", "258");                                      // 129: the fit's own miss
        for (int sync = 0; sync < 2; ++sync) { run(b, P.n, sync, 129, adv, second); CHECK(adv == 2 * P.n && second == P.n); }
        sw("QE_NARROW_FIT", "0");                                        // half the cutoff accepts it
        for (int sync = 0; sync < 2; ++sync) { run(b, P.n, sync, 129, adv, second); CHECK(adv == P.n && second == 0); }
        sw("QE_NARROW_FIT", nullptr);                                    // forced two passes alone: no policy, no fit
        run(b, P.n, true, 129, adv, second); CHECK(adv == P.n && second == 0);
        sw("QE_NARROW_FIT", "480");                                      // 141 of 300 needs the four slots half the cutoff has: kept
        run(b, P.n, true, 129, adv, second); CHECK(adv == P.n && second == 0);
        quicked_batch_destroy(b);
    }
    {   // learning, on a list above the gate of the fake device
        const char* cus = getenv("QE_STUB_CUS");
        const int groups = 4 * (cus ? atoi(cus) : 256) + 3;
        const Pairs P = make_pairs(64 * groups - 5, 2000);
        quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
        CHECK(b);
        sw("QE_NARROW_FIT", nullptr);
        sw("QE_SCORE_NARROW", nullptr);
        sw("QE_STUB_BOUND", "70");
        for (int k = 0; k < 3; ++k) { run(b, P.n, k % 2 == 0, 35, adv, second); CHECK(adv == P.n && second == 0); }      // half, then fitted to 35
        setenv("QE_STUB_BOUND", "258", 1);                               // (no reload: the library keeps what it has learnt)
        run(b, P.n, false, 129, adv, second); CHECK(adv == 2 * P.n && second == P.n);      // the stale fit misses every task ...
        for (int k = 0; k < 20; ++k) {                                   // ... the run after it is refitted, and the class never takes the
            run(b, P.n, k % 2 == 0, 129, adv, second);                   // single pass (no probe in 20 runs: a probe's sample would count)
            CHECK(adv == P.n && second == 0);
        }
        setenv("QE_STUB_BOUND", "1000", 1);                              // misses half the cutoff would have had too: does not pay
        run(b, P.n, true, 500, adv, second); CHECK(adv == 2 * P.n && second == P.n);
        run(b, P.n, true, 500, adv, second); CHECK(adv == P.n && second == 0);
        quicked_batch_destroy(b);
    }
    printf("narrow_fit_host ok\n");
    return 0;
}
