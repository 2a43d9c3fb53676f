// Flagged search runs (QUICKED_SEARCH_IUPAC, QUICKED_SEARCH_IUPAC_PATTERN) on the HOST, under sanitizers: the library's host
// layer built with g++ against the fake HIP runtime of tests/native/hip_stub.  The stand-ins of the two plane producers in
// qe_stages.hip are the scalar code of qe_iupac.h and the stand-in of k_search<NB, Eq> runs the real recurrence, so a flagged
// run of an ASCII batch gives TRUE answers here: they are compared with the expectations tests/test_host_search_iupac.py
// computed by brute force (file `cases` in the directory given).  An unflagged run reads the stub's zero planes -- every base
// 'A' -- as before, and so does a flagged run of a packed batch (its four planes are derived from those zeros).  Checked:
// the argument rules, the QUICKED_UNIMPLEMENTED cases, sync and queued flagged runs in both kernel forms, flagged and
// unflagged runs in turn on one batch object with a reload in between, a packed PLANES3 batch, quicked_batch_run_search_all
// with a cap of 1.  A stand-alone program: nothing is loaded into Python.
//
// cases: one line per pair -- pattern text, then for (flag 16, 32) x (PREFIX, INFIX) d start end, then for flag 16 / 32, INFIX,
// bound 2: found, and the first occurrence's start end score (-1 -1 -1: none).  "." is the empty sequence.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "quicked.h"
#include "quicked_batch.h"

extern "C" quicked_status_t quicked_debug_reload_env(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "search_iupac_host: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

struct Case { std::string p, t; int32_t best[2][2][3]; int32_t found[2], hit[2][3]; };
struct Pairs { std::string pp, tp; std::vector<int64_t> po, to; std::vector<int32_t> pl, tl; int64_t n = 0; };

static std::vector<Case> read_cases(const std::string& path) {
    std::vector<Case> out;
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream s(line);
        Case c;
        s >> c.p >> c.t;
        for (int fl = 0; fl < 2; ++fl) for (int md = 0; md < 2; ++md) for (int k = 0; k < 3; ++k) s >> c.best[fl][md][k];
        for (int fl = 0; fl < 2; ++fl) { s >> c.found[fl]; for (int k = 0; k < 3; ++k) s >> c.hit[fl][k]; }
        CHECK(!s.fail());
        if (c.p == ".") c.p.clear();
        if (c.t == ".") c.t.clear();
        out.push_back(c);
    }
    return out;
}
static Pairs pairs_of(const std::vector<Case>& cs, size_t from, size_t to) {
    Pairs P;
    for (size_t i = from; i < to; ++i) {
        P.po.push_back((int64_t)P.pp.size()); P.to.push_back((int64_t)P.tp.size());
        P.pp += cs[i].p; P.tp += cs[i].t;
        P.pl.push_back((int32_t)cs[i].p.size()); P.tl.push_back((int32_t)cs[i].t.size());
    }
    P.n = (int64_t)(to - from);
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
// a flagged run of an ASCII batch: the brute force's answer, cut at the bound
static void expect_true(const std::vector<Case>& cs, size_t from, const Got& g, int64_t n, int fl, int md, int32_t bound) {
    for (int64_t i = 0; i < n; ++i) {
        const Case& c = cs[from + (size_t)i];
        const size_t k = (size_t)i;
        if (c.p.empty() || c.t.empty()) { CHECK(g.st[k] == QUICKED_EMPTY_SEQUENCE && g.sc[k] == -1 && g.ts[k] == -1 && g.te[k] == -1); continue; }
        CHECK(g.st[k] == QUICKED_OK);
        const int32_t* e = c.best[fl][md];
        if (e[0] > std::min<int64_t>(bound, (int64_t)c.p.size())) { CHECK(g.sc[k] == -1 && g.ts[k] == -1 && g.te[k] == -1); continue; }
        if (!(g.sc[k] == e[0] && g.ts[k] == e[1] && g.te[k] == e[2]))
            fprintf(stderr, "pair %lld (m %zu, n %zu) flag %d mode %d: got %d [%d, %d), expected %d [%d, %d)\n", (long long)i, c.p.size(), c.t.size(), fl, md,
                    g.sc[k], g.ts[k], g.te[k], e[0], e[1], e[2]);
        CHECK(g.sc[k] == e[0] && g.ts[k] == e[1] && g.te[k] == e[2]);
    }
}
// the stub's zero planes: every base reads as 'A' (an unflagged run; a flagged run of a packed batch)
static void expect_all_a(const Pairs& P, const Got& g, int32_t bound) {
    for (int64_t i = 0; i < P.n; ++i) {
        const int m = P.pl[(size_t)i], t = P.tl[(size_t)i];
        const size_t k = (size_t)i;
        if (m == 0 || t == 0) { CHECK(g.st[k] == QUICKED_EMPTY_SEQUENCE && g.sc[k] == -1 && g.ts[k] == -1 && g.te[k] == -1); continue; }
        CHECK(g.st[k] == QUICKED_OK);
        const int d = t >= m ? 0 : m - t;
        if (d > bound) { CHECK(g.sc[k] == -1 && g.ts[k] == -1 && g.te[k] == -1); continue; }
        CHECK(g.sc[k] == d && g.ts[k] == 0 && g.te[k] == std::min(m, t));
    }
}

static const int FLAGS[2] = {QUICKED_SEARCH_IUPAC, QUICKED_SEARCH_IUPAC_PATTERN};
static const int MODES[2] = {QUICKED_SEARCH_PREFIX, QUICKED_SEARCH_INFIX};

int main(int argc, char** argv) {
    CHECK(argc == 2);
    const std::vector<Case> cs = read_cases(std::string(argv[1]) + "/cases");
    CHECK(cs.size() >= 20);
    const size_t half = cs.size() / 2;
    const Pairs P = pairs_of(cs, 0, half), Q = pairs_of(cs, half, cs.size());
    const int64_t n = P.n;
    quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
    CHECK(b);
    std::vector<int32_t> none((size_t)std::max(P.n, Q.n));
    // ---- the argument rules: nothing is launched
    for (int mode : {0, 3, 16, 16 | 3, 16 | 32 | 2, 64 | 2, 32, 4 | 16, 128 | 1, -1}) {
        CHECK(quicked_batch_run_search(b, mode, nullptr, 3, 1, 1) == QUICKED_ERROR);
        CHECK(quicked_batch_run_search(b, mode, nullptr, 3, 1, 0) == QUICKED_ERROR);
        CHECK(quicked_batch_run_search_all(b, mode, nullptr, 3, 4, 1) == QUICKED_ERROR);
    }
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX | QUICKED_SEARCH_IUPAC, nullptr, -1, 1, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search(nullptr, QUICKED_SEARCH_INFIX | QUICKED_SEARCH_IUPAC, nullptr, 3, 1, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
    // ---- QUICKED_UNIMPLEMENTED, nothing queued: a flagged CIGAR run; any search run with the in-run validator
    for (int fl : FLAGS) {
        CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX | fl, nullptr, 5, 0, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_PREFIX | fl, nullptr, 5, 0, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
        CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX | fl, nullptr, 5, 1, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX | fl, nullptr, 5, 1, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX | fl, nullptr, 5, 4, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    }
    CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_hit_total(b) == -1);
    // ---- an unflagged run first: what the getters returned before there were flags (the stub's all-'A' planes)
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, INT_MAX, 1, 1) == QUICKED_OK);
    const Got g0 = read_results(b, n);
    expect_all_a(P, g0, INT_MAX);
    int64_t cnt0[8], cnt1[8];
    CHECK(quicked_batch_counters(b, cnt0) >= 0 && cnt0[0] > 0);
    // ---- flagged runs, both forms and the library's choice, both flags and modes: sync, then queued + fetch with a bound
    for (const char* form : {"0", "1", (const char*)nullptr}) {
        set_form(form);
        for (int fl = 0; fl < 2; ++fl)
            for (int md = 0; md < 2; ++md) {
                const int mode = MODES[md] | FLAGS[fl];
                CHECK(quicked_batch_run_search(b, mode, nullptr, INT_MAX, 1, 1) == QUICKED_OK);
                Got g = read_results(b, n);
                expect_true(cs, 0, g, n, fl, md, INT_MAX);
                CHECK(quicked_batch_counters(b, cnt1) >= 0 && cnt1[0] > 0);
                std::vector<int32_t> bounds((size_t)n);
                for (int64_t i = 0; i < n; ++i) bounds[(size_t)i] = (i % 3 == 0) ? 0 : ((i % 3 == 1) ? 12 : INT_MAX);
                CHECK(quicked_batch_run_search(b, mode, bounds.data(), 0, 1, 0) == QUICKED_OK);
                const Got before = read_results(b, n);               // a queued run leaves the getters' data alone until the fetch
                CHECK(before.sc == g.sc && before.te == g.te);
                CHECK(quicked_batch_fetch(b) == QUICKED_OK);
                g = read_results(b, n);
                for (int64_t i = 0; i < n; ++i) {
                    Got one{{g.sc[(size_t)i]}, {g.st[(size_t)i]}, {g.ts[(size_t)i]}, {g.te[(size_t)i]}};
                    expect_true(cs, (size_t)i, one, 1, fl, md, bounds[(size_t)i]);
                }
            }
        // an unflagged run between flagged ones gives its old results and does its old work
        CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX, nullptr, INT_MAX, 1, 1) == QUICKED_OK);
        const Got g1 = read_results(b, n);
        CHECK(g1.sc == g0.sc && g1.st == g0.st && g1.ts == g0.ts && g1.te == g0.te);
        CHECK(quicked_batch_counters(b, cnt1) >= 0 && cnt1[0] == cnt0[0]);
    }
    set_form(nullptr);
    // ---- every occurrence, a cap of 1: found is exact, one occurrence stored, the first by text_end
    for (int fl = 0; fl < 2; ++fl) {
        CHECK(quicked_batch_run_search_all(b, QUICKED_SEARCH_INFIX | FLAGS[fl], nullptr, 2, 1, 1) == QUICKED_OK);
        std::vector<int32_t> found((size_t)n), stored((size_t)n);
        std::vector<int64_t> off((size_t)n + 1);
        CHECK(quicked_batch_hit_counts(b, found.data(), stored.data()) == QUICKED_OK);
        std::vector<quicked_hit_t> hits((size_t)std::max<int64_t>(1, quicked_batch_hit_total(b)));
        CHECK(quicked_batch_hits(b, hits.data(), off.data()) == QUICKED_OK);
        int64_t many = 0;
        for (int64_t i = 0; i < n; ++i) {
            const Case& c = cs[(size_t)i];
            if (c.p.empty() || c.t.empty()) { CHECK(found[(size_t)i] == 0 && stored[(size_t)i] == 0); continue; }
            CHECK(found[(size_t)i] == c.found[fl] && stored[(size_t)i] == std::min(1, c.found[fl]));
            many += c.found[fl] > 1;
            if (!stored[(size_t)i]) continue;
            const quicked_hit_t h = hits[(size_t)off[(size_t)i]];
            CHECK(h.text_start == c.hit[fl][0] && h.text_end == c.hit[fl][1] && h.score == c.hit[fl][2]);
        }
        CHECK(many > 0);
        CHECK(quicked_batch_locations(b, none.data(), none.data()) == QUICKED_ERROR);      // not a best-search run
    }
    // ---- a reload in between: other pairs, another count; a queued flagged run superseded by the reload
    CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_INFIX | QUICKED_SEARCH_IUPAC, nullptr, 7, 1, 0) == QUICKED_OK);
    CHECK(quicked_batch_reload(b, Q.n, Q.pp.data(), Q.po.data(), Q.pl.data(), Q.tp.data(), Q.to.data(), Q.tl.data()) >= 0);
    for (int round = 0; round < 2; ++round) {
        for (int fl = 0; fl < 2; ++fl)
            for (int md = 0; md < 2; ++md) {
                CHECK(quicked_batch_run_search(b, MODES[md] | FLAGS[fl], nullptr, 25, 1, 1) == QUICKED_OK);
                expect_true(cs, half, read_results(b, Q.n), Q.n, fl, md, 25);
            }
        CHECK(quicked_batch_run_search(b, QUICKED_SEARCH_PREFIX, nullptr, 25, 1, 1) == QUICKED_OK);
        expect_all_a(Q, read_results(b, Q.n), 25);
    }
    quicked_batch_destroy(b);
    // ---- a packed PLANES3 batch: the four planes are derived from the resident three (the stub's: zeros)
    {
        std::vector<uint64_t> pw, tw;
        std::vector<int64_t> pwo, two;
        for (int64_t i = 0; i < P.n; ++i) {
            pwo.push_back((int64_t)pw.size()); two.push_back((int64_t)tw.size());
            pw.resize(pw.size() + (size_t)quicked_wire_words(P.pl[(size_t)i], QUICKED_WIRE_PLANES3), 0);
            tw.resize(tw.size() + (size_t)quicked_wire_words(P.tl[(size_t)i], QUICKED_WIRE_PLANES3), 0);
        }
        pw.push_back(0); tw.push_back(0);
        quicked_batch_t* k = quicked_batch_create_packed(P.n, QUICKED_WIRE_PLANES3, pw.data(), pwo.data(), P.pl.data(), tw.data(), two.data(), P.tl.data());
        CHECK(k);
        for (const char* form : {"0", "1"}) {
            set_form(form);
            for (int fl : FLAGS)
                for (int md : MODES) {
                    CHECK(quicked_batch_run_search(k, md | fl, nullptr, 30, 1, 1) == QUICKED_OK);
                    expect_all_a(P, read_results(k, P.n), 30);
                    CHECK(quicked_batch_run_search(k, md | fl, nullptr, 30, 0, 1) == QUICKED_UNIMPLEMENTED);
                }
            CHECK(quicked_batch_run_search(k, QUICKED_SEARCH_INFIX, nullptr, 30, 1, 1) == QUICKED_OK);
            expect_all_a(P, read_results(k, P.n), 30);
            CHECK(quicked_batch_run_search_all(k, QUICKED_SEARCH_INFIX | QUICKED_SEARCH_IUPAC_PATTERN, nullptr, 0, 1, 1) == QUICKED_OK);
            CHECK(quicked_batch_hit_total(k) > 0);
        }
        set_form(nullptr);
        quicked_batch_destroy(k);
    }
    printf("search_iupac_host ok\n");
    return 0;
}
