// All-occurrences runs (quicked_batch_run_search_all) on the HOST, under sanitizers: the library's host layer built with g++
// against the fake HIP runtime of tests/native/hip_stub.  The stub's pack kernel leaves the planes zero -- every base reads as
// 'A' -- and the host stand-ins of k_search_hits / k_hits_expand / k_hits_finish (qe_stages.hip) run the real recurrence of
// qe_search.h over them, so the answers are known: row m of a pattern of m bases in a text of n falls to max(0, m - n) at
// column min(m, n) and never below, so a pair has exactly one occurrence {0, min(m, n), max(0, m - n)} when that score is within
// its bound, and none otherwise.  What is checked is the host side around the kernels: the argument rules, the
// QUICKED_UNIMPLEMENTED cases, the limits of max_hits, the flow (forward pass, offset scan, the total, expansion, the start pass
// per occurrence in both kernel forms and in slices, the read-back in the order of the pairs), empty pairs, the getters'
// rules after other runs, and a reload between runs.  One occurrence per pair is all these planes can give: a cap that
// overflows is the CPU and GPU suites' business (tests/test_search_hits_cpu.py, tests/test_gpu_search_hits.py); here the
// smallest and the largest cap have to give the same answers.  Built and run by tests/test_host_search_hits.py with
// -fsanitize=address,undefined.  A stand-alone program: nothing is loaded into Python.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "quicked.h"
#include "quicked_batch.h"

extern "C" quicked_status_t quicked_debug_reload_env(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "search_hits_host: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

struct Pairs { std::string pp, tp; std::vector<int64_t> po, to; std::vector<int32_t> pl, tl; int64_t n = 0; };
// pattern lengths through every list of the stage (1, 2, 3-4 and more blocks), texts longer and shorter than their patterns,
// empty sequences in the middle of a wave
static Pairs make_pairs(int n, unsigned seed, bool tiny = false) {
    static const int plen[] = {1, 40, 64, 65, 128, 150, 256, 257, 300, 1000}, tadd[] = {0, 1, 90, -20, 400, -1};
    Pairs P;
    P.n = n;
    unsigned x = seed;
    for (int i = 0; i < n; ++i) {
        int m = tiny ? 1 : plen[i % 10], t = tiny ? 1 : std::max(1, m + tadd[i % 6]);
        if (!tiny && i % 17 == 5) m = 0;
        if (!tiny && i % 19 == 7) t = 0;
        P.po.push_back((int64_t)P.pp.size()); P.to.push_back((int64_t)P.tp.size());
        for (int k = 0; k < m; ++k) { x = x * 1664525u + 1013904223u; P.pp.push_back("ACGT"[x >> 30]); }
        for (int k = 0; k < t; ++k) { x = x * 1664525u + 1013904223u; P.tp.push_back("ACGT"[x >> 30]); }
        P.pl.push_back(m); P.tl.push_back(t);
    }
    return P;
}
static quicked_batch_t* batch_of(const Pairs& P) {
    quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
    CHECK(b);
    return b;
}

static void set_form(const char* v) {
    if (v) setenv("QE_SEARCH_FORM", v, 1); else unsetenv("QE_SEARCH_FORM");
    CHECK(quicked_debug_reload_env() >= 0);
}

struct Got { std::vector<int32_t> sc, st, found, stored; std::vector<int64_t> off; std::vector<quicked_hit_t> hits; };
static Got read_results(quicked_batch_t* b, int64_t n) {
    Got g;
    g.sc.assign((size_t)n, 77); g.st.assign((size_t)n, 77); g.found.assign((size_t)n, 77); g.stored.assign((size_t)n, 77); g.off.assign((size_t)n + 1, 77);
    CHECK(quicked_batch_scores(b, g.sc.data(), g.st.data()) >= 0);
    CHECK(quicked_batch_hit_counts(b, g.found.data(), g.stored.data()) == QUICKED_OK);
    const int64_t total = quicked_batch_hit_total(b);
    CHECK(total >= 0);
    g.hits.assign((size_t)total + 1, quicked_hit_t{77, 77, 77});          // exactly the total, and a guard behind it
    CHECK(quicked_batch_hits(b, g.hits.data(), g.off.data()) == QUICKED_OK);
    CHECK(g.hits.back().text_start == 77 && g.hits.back().text_end == 77 && g.hits.back().score == 77);
    CHECK(g.off[0] == 0 && g.off[(size_t)n] == total);
    // either output may be NULL
    CHECK(quicked_batch_hit_counts(b, nullptr, nullptr) == QUICKED_OK && quicked_batch_hits(b, nullptr, nullptr) == QUICKED_OK);
    return g;
}
// what the all-'A' planes make of pair i with this bound
static void expect_pair(const Pairs& P, const Got& g, int64_t i, int32_t bound) {
    const int m = P.pl[(size_t)i], t = P.tl[(size_t)i];
    const size_t k = (size_t)i;
    const int64_t stored = g.off[k + 1] - g.off[k];
    CHECK(stored == g.stored[k] && stored >= 0);
    if (m == 0 || t == 0) { CHECK(g.st[k] == QUICKED_EMPTY_SEQUENCE && g.sc[k] == -1 && g.found[k] == 0 && stored == 0); return; }
    CHECK(g.st[k] == QUICKED_OK);
    const int d = t >= m ? 0 : m - t;
    if (d > bound) { CHECK(g.sc[k] == -1 && g.found[k] == 0 && stored == 0); return; }
    CHECK(g.sc[k] == d && g.found[k] == 1 && stored == 1);
    const quicked_hit_t h = g.hits[(size_t)g.off[k]];
    CHECK(h.text_start == 0 && h.text_end == std::min(m, t) && h.score == d);
}

static void scenario(int n, unsigned seed) {
    const Pairs P = make_pairs(n, seed);
    quicked_batch_t* b = batch_of(P);
    std::vector<int32_t> none((size_t)n), bounds((size_t)n);
    std::vector<int64_t> off((size_t)n + 1);
    for (int i = 0; i < n; ++i) bounds[(size_t)i] = (i % 3 == 0) ? 0 : ((i % 3 == 1) ? 19 : INT_MAX);
    auto refused = [&]() {
        return quicked_batch_hit_counts(b, none.data(), none.data()) == QUICKED_ERROR && quicked_batch_hit_total(b) == -1 &&
               quicked_batch_hits(b, nullptr, off.data()) == QUICKED_ERROR;
    };
    // ---- the getters before any run, and the argument rules: nothing is launched
    CHECK(refused());
    CHECK(quicked_batch_run_search_all(b, 0, nullptr, 3, 4, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, 3, nullptr, 3, 4, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, -1, 4, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, 3, 0, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, 3, -1, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, 3, 4097, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_PREFIX, nullptr, 3, 4097, 0) == QUICKED_ERROR);
    {
        std::vector<int32_t> neg = bounds;
        neg[(size_t)n / 2] = -4;
        CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_PREFIX, neg.data(), 0, 4, 1) == QUICKED_ERROR);
    }
    CHECK(refused());
    // ---- QUICKED_UNIMPLEMENTED: a queued run; any run with the in-run validator
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, 5, 4, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, 5, 4, 1) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_PREFIX, nullptr, 5, 4, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    CHECK(refused());
    // ---- the flow, both forms and the library's choice, both modes, per-pair bounds and one bound, the smallest and the
    // largest cap; the tags are ignored
    CHECK(quicked_batch_configure_tags(b, QUICKED_TAG_STATS) == QUICKED_OK);
    for (const char* form : {"0", "1", (const char*)nullptr}) {
        set_form(form);
        for (int mode : {(int)QUICKED_SEARCH_PREFIX, (int)QUICKED_SEARCH_INFIX}) {
            for (int cap : {1, 3, 4096}) {
                CHECK(quicked_batch_run_search_all(b, mode, bounds.data(), 0, cap, 1) == QUICKED_OK);
                Got g = read_results(b, n);
                for (int i = 0; i < n; ++i) expect_pair(P, g, i, bounds[(size_t)i]);
                int64_t cnt[8];
                CHECK(quicked_batch_counters(b, cnt) >= 0 && cnt[0] > 0);
                // no locations, no strings, no tag data
                CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
                std::vector<quicked_pair_stats_t> ps((size_t)n);
                CHECK(quicked_batch_pair_stats(b, ps.data()) == QUICKED_ERROR && quicked_batch_cigar_bytes(b) == 0);
            }
            CHECK(quicked_batch_run_search_all(b, mode, nullptr, INT_MAX, 2, 1) == QUICKED_OK);
            Got g = read_results(b, n);
            for (int i = 0; i < n; ++i) expect_pair(P, g, i, INT_MAX);
            CHECK(quicked_batch_run_search_all(b, mode, nullptr, 0, 2, 1) == QUICKED_OK);
            g = read_results(b, n);
            for (int i = 0; i < n; ++i) expect_pair(P, g, i, 0);
        }
    }
    set_form(nullptr);
    CHECK(quicked_batch_configure_tags(b, 0) == QUICKED_OK);
    // ---- the start pass in slices: a workspace of 64 KiB holds three groups of the tallest pattern (1 000 bases: 20 KiB each)
    setenv("QE_SEARCH_HITS_WS_KB", "64", 1);
    set_form("0");
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, bounds.data(), 0, 2, 1) == QUICKED_OK);
    { const Got g = read_results(b, n); for (int i = 0; i < n; ++i) expect_pair(P, g, i, bounds[(size_t)i]); }
    unsetenv("QE_SEARCH_HITS_WS_KB");
    set_form(nullptr);
    // ---- the getters after runs that are not all-occurrences runs, and the best search's getter after one that is
    quicked_params_t p = quicked_default_params();
    p.algo = BANDED; p.only_score = true;
    CHECK(quicked_batch_run(b, &p, 1) >= 0);
    CHECK(refused());
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_PREFIX, nullptr, INT_MAX, 8, 1) == QUICKED_OK);
    CHECK(quicked_batch_hit_total(b) > 0);
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, INT_MAX, 1, 1) == QUICKED_OK);
    CHECK(refused() && quicked_batch_locations(b, none.data(), none.data()) == QUICKED_OK);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, INT_MAX, 8, 1) == QUICKED_OK);
    CHECK(quicked_batch_run_bounded(b, nullptr, 1000, 1, 1) == QUICKED_OK);
    CHECK(refused());
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, INT_MAX, 8, 1) == QUICKED_OK);
    // a queued run and its fetch: the results of the all-occurrences run stand until the fetch, and are gone after it
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, 7, 1, 0) == QUICKED_OK);
    CHECK(quicked_batch_hit_total(b) > 0);
    CHECK(quicked_batch_fetch(b) == QUICKED_OK);
    CHECK(refused());
    // a refused call leaves the results of the last run alone
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, INT_MAX, 8, 1) == QUICKED_OK);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, INT_MAX, 0, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, INT_MAX, 8, 0) == QUICKED_UNIMPLEMENTED);
    { const Got g = read_results(b, n); for (int i = 0; i < n; ++i) expect_pair(P, g, i, INT_MAX); }
    // ---- a reload between runs: other pairs, another count
    const int n2 = n / 2 + 3;
    const Pairs Q = make_pairs(n2, seed + 1);
    CHECK(quicked_batch_reload(b, Q.n, Q.pp.data(), Q.po.data(), Q.pl.data(), Q.tp.data(), Q.to.data(), Q.tl.data()) >= 0);
    for (int mode : {(int)QUICKED_SEARCH_INFIX, (int)QUICKED_SEARCH_PREFIX}) {
        CHECK(quicked_batch_run_search_all(b, mode, nullptr, 25, 5, 1) == QUICKED_OK);
        const Got g = read_results(b, n2);
        for (int i = 0; i < n2; ++i) expect_pair(Q, g, i, 25);
    }
    quicked_batch_destroy(b);
}

// (pairs without an empty sequence) x max_hits above 2^26 is refused before anything is allocated or launched
static void product_limit() {
    const int n = (1 << 26) / 4096 + 1;           // 16 385 one-base pairs
    const Pairs P = make_pairs(n, 5, true);
    quicked_batch_t* b = batch_of(P);
    int64_t before[8], after[8];
    CHECK(quicked_pool_stats(before) >= 0);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, 1, 4096, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_PREFIX, nullptr, 1, 4096, 0) == QUICKED_ERROR);
    CHECK(quicked_pool_stats(after) >= 0 && after[0] == before[0] && after[5] == before[5]);      // the pools did not grow
    CHECK(quicked_batch_hit_total(b) == -1);
    quicked_batch_destroy(b);
    // empty pairs do not count: the same number of pairs, one of them empty, is at the limit and runs
    Pairs E = make_pairs(n, 6, true);
    E.pl[7] = 0;
    b = batch_of(E);
    CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX, nullptr, 1, 4096, 1) == QUICKED_OK);
    const Got h = read_results(b, n);
    for (int i = 0; i < n; ++i) expect_pair(E, h, i, 1);
    quicked_batch_destroy(b);
}

int main() {
    int32_t x = 0;
    int64_t o = 0;
    CHECK(quicked_batch_run_search_all(nullptr, QUICKED_SEARCH_INFIX, nullptr, 3, 4, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_hit_counts(nullptr, &x, &x) == QUICKED_ERROR && quicked_batch_hit_total(nullptr) == -1);
    CHECK(quicked_batch_hits(nullptr, nullptr, &o) == QUICKED_ERROR);
    scenario(7, 11);                // a few pairs: one partial wave per list
    scenario(700, 12);              // several waves per list
    product_limit();
    printf("search_hits_host ok\n");
    return 0;
}
