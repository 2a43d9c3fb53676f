// The pruning threshold of a fitted first pass (QE_NARROW_PRUNE) on the HOST, under sanitizers: the library's host layer built
// with g++ against the fake HIP runtime of tests/native/hip_stub, as tests/native/narrow_fit_host.cpp is.  The stub's k_banded
// gives every task the score QE_STUB_BOUND / 2 (read at every launch) and one block-column per pass; k_narrow is the host
// rendering in qe_stages.hip.  Pairs of 4 000 bases: cutoff 600 (eleven slots), six slots at half of it, which accepts up to 257;
// a fit for results of 130 .. 256 has five slots and the cutoff 256.  A score s is reported as the ratio ceil(1024 s / 600) and
// a ratio q stands for the result (600 q + 1023) >> 10:  150 -> 256 -> 150,  152 -> 260,  156 -> 267,  230 -> 393 -> 231,
// 240 -> 410 -> 241,  242 -> 414,  246 -> 420,  250 -> 427 -> 251,  256 -> 437 -> 257.
// Built and run by tests/test_host_narrow_prune.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "quicked.h"
#include "quicked_batch.h"

extern "C" quicked_status_t quicked_debug_reload_env(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "narrow_prune_host: %s failed at line %d (adv %lld second %lld)\n", #cond, __LINE__, (long long)adv, (long long)second); exit(1); } } while (0)

static int64_t adv = 0, second = 0;

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

static quicked_batch_t* g_b = nullptr;
static int64_t g_n = 0;
static int g_runs = 0;
// one run at the score `score` (no reload: the library keeps what it has learnt), sync and queued + fetch in turn
static void run(int score) {
    setenv("QE_STUB_BOUND", std::to_string(2 * score).c_str(), 1);
    const bool sync = (g_runs++ % 2) == 0;
    quicked_params_t p = quicked_default_params();
    p.algo = BANDED; p.only_score = true; p.bandwidth = 15;
    CHECK(quicked_batch_run(g_b, &p, sync ? 1 : 0) >= 0);
    if (!sync) CHECK(quicked_batch_fetch(g_b) >= 0);
    std::vector<int32_t> sc((size_t)g_n), st((size_t)g_n);
    CHECK(quicked_batch_scores(g_b, sc.data(), st.data()) >= 0);
    for (int64_t i = 0; i < g_n; ++i) CHECK(sc[(size_t)i] == score);
    int64_t c[8];
    CHECK(quicked_batch_counters(g_b, c) >= 0);
    adv = c[0]; second = c[7];
}
#define ACCEPTED(score) do { run(score); CHECK(adv == g_n && second == 0); } while (0)
#define MISSED(score) do { run(score); CHECK(adv == 2 * g_n && second == g_n); } while (0)

int main() {
    {   // forced switches
        const Pairs P = make_pairs(200, 4000);
        g_b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
        g_n = P.n;
        CHECK(g_b);
        sw("QE_SCORE_NARROW", "1");
        sw("QE_NARROW_FIT", "256");                  // a forced fit alone has no threshold: everything the fitted cutoff accepts
        ACCEPTED(151); ACCEPTED(256); ACCEPTED(256); MISSED(257);
        sw("QE_NARROW_PRUNE", "256");                // the threshold 150
        ACCEPTED(150); ACCEPTED(150); MISSED(151); MISSED(151); MISSED(256);
        sw("QE_NARROW_PRUNE", "1000");               // a threshold above the fitted cutoff is the fitted cutoff
        ACCEPTED(256); MISSED(257);
        sw("QE_NARROW_PRUNE", "0");
        ACCEPTED(151); ACCEPTED(256);
        sw("QE_NARROW_FIT", "0");                    // no fit, no threshold: half the cutoff accepts 257
        sw("QE_NARROW_PRUNE", "256");
        ACCEPTED(257); ACCEPTED(257);
        quicked_batch_destroy(g_b);
    }
    {   // a fitted band of three slots has no edge to move (first + 2 < last never holds): no threshold, whatever the ratio
        const Pairs P = make_pairs(200, 2000);       // cutoff 300: any fit has three slots and the cutoff 128
        g_b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
        g_n = P.n;
        CHECK(g_b);
        sw("QE_NARROW_FIT", "120");
        sw("QE_NARROW_PRUNE", "120");                // (would be 36)
        ACCEPTED(37); ACCEPTED(128); MISSED(129);
        quicked_batch_destroy(g_b);
    }
    {   // the policy, on a list above the gate of the fake device
        const char* cus = getenv("QE_STUB_CUS");
        const int groups = 4 * (cus ? atoi(cus) : 256) + 3;
        const Pairs P = make_pairs(64 * groups - 5, 4000);
        g_b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
        g_n = P.n;
        CHECK(g_b);
        sw("QE_NARROW_FIT", nullptr);
        sw("QE_SCORE_NARROW", nullptr);
        sw("QE_NARROW_PRUNE", nullptr);
        // one report: the fit (150 proved, cutoff 256), no threshold -- 152 is accepted and reported as 260
        ACCEPTED(150); ACCEPTED(152);
        // two reports, 256 and 260: q = 260, w = 4, the threshold of 264 is 155
        ACCEPTED(152);
        MISSED(156);                                 // between the threshold and the fitted cutoff: the second pass, and q rises to 267
        ACCEPTED(156);                               // (w = 11: the threshold of 278 is 163)
        // two EQUAL reports: the threshold is r^ itself, 150
        CHECK(quicked_debug_reload_env() >= 0);
        ACCEPTED(150); ACCEPTED(150); ACCEPTED(150);
        CHECK(quicked_debug_reload_env() >= 0);
        ACCEPTED(150); ACCEPTED(150); MISSED(151);
        // a shift: the reads now end at 230.  The run under the stale threshold misses and reports 393; with 256 still in the
        // ring w = 137 and the threshold of 530 is past the fitted cutoff: everything up to 256 is accepted
        CHECK(quicked_debug_reload_env() >= 0);
        ACCEPTED(150); ACCEPTED(150);
        MISSED(230);
        ACCEPTED(256);                               // (at r^ of 393, 231, it would have missed; reported as 437, whose r^ no fit holds:
        ACCEPTED(257);                               //  the lanes keep half the cutoff, which accepts 257, while it is in the ring)
        // ... and forgotten after 16 reports
        CHECK(quicked_debug_reload_env() >= 0);
        ACCEPTED(150); ACCEPTED(150);
        MISSED(230);
        for (int k = 0; k < 16; ++k) ACCEPTED(240);  // (reported as 410) ... 16 reports later the ring holds nothing else:
        MISSED(242);                                 // the threshold is that of 410, 241 -- the old entries are forgotten
        // such misses are the fit's own (stat[5]): the class keeps its two passes -- the next run misses again instead of
        // passing at the full band (ring 410 .. 414: the threshold of 418 is 245), and the one after it is refitted
        MISSED(246);
        for (int k = 0; k < 20; ++k) ACCEPTED(250);  // (ring .. 420: w = 10, the threshold of 430 is 252; no probe in 20 runs)
        // switched off: today's counts
        sw("QE_NARROW_PRUNE", "0");
        ACCEPTED(150); ACCEPTED(150); ACCEPTED(152); ACCEPTED(156); ACCEPTED(230);
        MISSED(257);
        quicked_batch_destroy(g_b);
    }
    printf("narrow_prune_host ok\n");
    return 0;
}
