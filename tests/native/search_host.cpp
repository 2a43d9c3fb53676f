// Search runs (quicked_batch_run_search) on the HOST, under sanitizers: the library's host layer built with g++ against the
// fake HIP runtime of tests/native/hip_stub.  The stub's pack kernel leaves the planes zero -- every base reads as 'A' -- and
// the host stand-in of k_search (qe_stages.hip) runs the real recurrence of qe_search.h over them, so the answers are
// known: a pattern of m bases in a text of n >= m is found with d = 0 at [0, m), in a text of n < m with d = m - n at
// [0, n).  What is checked is the host side around the kernels: the argument rules, the QUICKED_UNIMPLEMENTED cases, the
// three-step flow (forward pass, start pass, CIGAR pass) in both kernel forms, the lists by block count, queued runs and
// their fetch, the getters' rules, and a reload between runs.  Built and run by tests/test_host_search.py with
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

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "search_host: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

struct Pairs { std::string pp, tp; std::vector<int64_t> po, to; std::vector<int32_t> pl, tl; int64_t n = 0; };
// pattern lengths through every list of the stage (1, 2, 3-4 and more blocks), texts longer and shorter than their patterns,
// empty sequences in the middle of a wave
static Pairs make_pairs(int n, unsigned seed) {
    static const int plen[] = {1, 40, 64, 65, 128, 150, 256, 257, 300, 1000}, tadd[] = {0, 1, 90, -20, 400, -1};
    Pairs P;
    P.n = n;
    unsigned x = seed;
    for (int i = 0; i < n; ++i) {
        int m = plen[i % 10], t = std::max(1, m + tadd[i % 6]);
        if (i % 17 == 5) m = 0;
        if (i % 19 == 7) t = 0;
        P.po.push_back((int64_t)P.pp.size()); P.to.push_back((int64_t)P.tp.size());
        for (int k = 0; k < m; ++k) { x = x * 1664525u + 1013904223u; P.pp.push_back("ACGT"[x >> 30]); }
        for (int k = 0; k < t; ++k) { x = x * 1664525u + 1013904223u; P.tp.push_back("ACGT"[x >> 30]); }
        P.pl.push_back(m); P.tl.push_back(t);
    }
    return P;
}

static void set_form(const char* v) {
    if (v) setenv("QE_SEARCH_FORM", v, 1); else unsetenv("QE_SEARCH_FORM");
    CHECK(quicked_debug_reload_env() >= 0);
}

struct Got { std::vector<int32_t> sc, st, ts, te; };
static Got read_results(quicked_batch_t* b, int64_t n) {
    Got g;
    g.sc.assign((size_t)n, 77); g.st.assign((size_t)n, 77); g.ts.assign((size_t)n, 77); g.te.assign((size_t)n, 77);
    CHECK(quicked_batch_scores(b, g.sc.data(), g.st.data()) >= 0);
    CHECK(quicked_batch_locations(b, g.ts.data(), g.te.data()) == QUICKED_OK);
    return g;
}
// what the all-'A' planes make of pair i with this bound
// (with_score = false: after a CIGAR run, whose scores are the edit counts of the stub's empty alignments)
static void expect_pair(const Pairs& P, const Got& g, int64_t i, int32_t bound, bool with_score = true) {
    const int m = P.pl[(size_t)i], t = P.tl[(size_t)i];
    const size_t k = (size_t)i;
    if (m == 0 || t == 0) { CHECK(g.st[k] == QUICKED_EMPTY_SEQUENCE && g.sc[k] == -1 && g.ts[k] == -1 && g.te[k] == -1); return; }
    CHECK(g.st[k] == QUICKED_OK);
    const int d = t >= m ? 0 : m - t;
    if (d > bound) { CHECK(g.sc[k] == -1 && g.ts[k] == -1 && g.te[k] == -1); return; }
    CHECK((!with_score || g.sc[k] == d) && g.sc[k] >= 0 && g.ts[k] == 0 && g.te[k] == std::min(m, t));
}

static void scenario(int n, unsigned seed) {
    const Pairs P = make_pairs(n, seed);
    quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
    CHECK(b);
    std::vector<int32_t> none((size_t)n), bounds((size_t)n);
    for (int i = 0; i < n; ++i) bounds[(size_t)i] = (i % 3 == 0) ? 0 : ((i % 3 == 1) ? 19 : INT_MAX);
    // ---- the getter before any run, and the argument rules: nothing is launched
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search(b, 0, nullptr, 3, 1, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search(b, 3, nullptr, 3, 1, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, -1, 1, 1) == QUICKED_ERROR);
    {
        std::vector<int32_t> neg = bounds;
        neg[(size_t)n / 2] = -4;
        CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_PREFIX, neg.data(), 0, 1, 0) == QUICKED_ERROR);
    }
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
    // ---- QUICKED_UNIMPLEMENTED: a queued CIGAR run; any search run with the in-run validator
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, 5, 0, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, 5, 1, 1) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, 5, 0, 1) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, 5, 1, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
    // ---- the flow, both forms and the library's choice, both modes: sync, queued + fetch, per-pair bounds and one bound
    for (const char* form : {"0", "1", (const char*)nullptr}) {
        set_form(form);
        for (int mode : {(int)QUICKED_SEARCH_PREFIX, (int)QUICKED_SEARCH_INFIX}) {
            CHECK(quicked_batch_run_search(b, mode, bounds.data(), 0, 1, 1) == QUICKED_OK);
            Got g = read_results(b, n);
            for (int i = 0; i < n; ++i) expect_pair(P, g, i, bounds[(size_t)i]);
            int64_t cnt[8];
            CHECK(quicked_batch_counters(b, cnt) >= 0 && cnt[0] > 0);
            CHECK(quicked_batch_run_search(b, mode, nullptr, INT_MAX, 1, 0) == QUICKED_OK);
            const Got before = read_results(b, n);                   // a queued run leaves the getters' data alone until the fetch
            CHECK(before.sc == g.sc && before.te == g.te);
            CHECK(quicked_batch_fetch(b) == QUICKED_OK);
            g = read_results(b, n);
            for (int i = 0; i < n; ++i) expect_pair(P, g, i, INT_MAX);
            // either output may be NULL
            std::vector<int32_t> te((size_t)n, 5);
            CHECK(quicked_batch_locations(b, nullptr, te.data()) == QUICKED_OK && te == g.te);
            CHECK(quicked_batch_locations(b, nullptr, nullptr) == QUICKED_OK);
        }
    }
    set_form(nullptr);
    // ---- the CIGAR pass: one string per pair within its bound (the stub's formatter: "1M"), none for the others
    for (int tags : {0, (int)QUICKED_TAG_STATS, (int)(QUICKED_TAG_STATS | QUICKED_TAG_NO_CIGAR)}) {
        CHECK(quicked_batch_configure_tags(b, tags) == QUICKED_OK);
        CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, bounds.data(), 0, 0, 1) == QUICKED_OK);
        const Got g = read_results(b, n);
        for (int i = 0; i < n; ++i) expect_pair(P, g, i, bounds[(size_t)i], false);
        std::vector<int64_t> coff((size_t)n);
        std::vector<char> pool((size_t)quicked_batch_cigar_bytes(b) + 1);
        CHECK(quicked_batch_cigars(b, pool.data(), coff.data()) >= 0);
        std::vector<quicked_pair_stats_t> ps((size_t)n);
        CHECK((quicked_batch_pair_stats(b, ps.data()) == QUICKED_OK) == ((tags & QUICKED_TAG_STATS) != 0));
        int64_t aligned = 0;
        for (int i = 0; i < n; ++i) {
            const bool within = g.sc[(size_t)i] >= 0;
            aligned += within;
            CHECK((coff[(size_t)i] >= 0) == (within && !(tags & QUICKED_TAG_NO_CIGAR)));
            if (tags & QUICKED_TAG_STATS) CHECK((ps[(size_t)i].columns >= 0) == within);
        }
        CHECK(aligned > 0 && aligned < n);
    }
    CHECK(quicked_batch_configure_tags(b, 0) == QUICKED_OK);
    // ---- the getter after runs that are not search runs
    quicked_params_t p = quicked_default_params();
    p.algo = BANDED; p.only_score = true;
    CHECK(quicked_batch_run(b, &p, 1) >= 0);
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_PREFIX, nullptr, INT_MAX, 1, 1) == QUICKED_OK);
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_OK);
    CHECK(quicked_batch_run_bounded(b, nullptr, 1000, 1, 1) == QUICKED_OK);
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_run(b, &p, 0) >= 0 && quicked_batch_fetch(b) >= 0);
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
    // ---- a reload between runs: other pairs, another count; a queued search run superseded by the reload
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, 7, 1, 0) == QUICKED_OK);
    const int n2 = n / 2 + 3;
    const Pairs Q = make_pairs(n2, seed + 1);
    CHECK(quicked_batch_reload(b, Q.n, Q.pp.data(), Q.po.data(), Q.pl.data(), Q.tp.data(), Q.to.data(), Q.tl.data()) >= 0);
    for (int mode : {(int)QUICKED_SEARCH_INFIX, (int)QUICKED_SEARCH_PREFIX}) {
        CHECK(quicked_batch_run_search(b, mode, nullptr, 25, 1, 1) == QUICKED_OK);
        const Got g = read_results(b, n2);
        for (int i = 0; i < n2; ++i) expect_pair(Q, g, i, 25);
    }
    quicked_batch_destroy(b);
}

int main() {
    int32_t x = 0;
    CHECK(quicked_batch_run_search(nullptr, QUICKED_SEARCH_INFIX, nullptr, 3, 1, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_locations(nullptr, &x, &x) == QUICKED_ERROR);
    scenario(7, 11);                // a few pairs: one partial wave per list
    scenario(700, 12);              // several waves per list
    printf("search_host ok\n");
    return 0;
}
