// The 5' heads of the panel search (QUICKED_PANEL_HEADS) on the HOST, under sanitizers: the library's host layer built with g++
// against the fake HIP runtime of tests/native/hip_stub.  The stand-ins of k_panel_heads, k_panel_heads_merge,
// k_panel_head_planes and k_panel_heads_finish (hip_stub/qe_kernels_stub.h) are the device kernels' own source (qe_panel.h)
// run slot by slot, the end pass's stand-in runs the real recurrence and the stand-in of k_pack_iupac is the scalar packer of
// qe_iupac.h, so a run under an IUPAC flag of an ASCII batch gives true answers here: they are compared with the heads
// tests/test_panel_heads_cpu.py took from the fixture (file `cases` in the directory given; tests/panel_heads_lib.py's format).
//
// Checked: every argument rule with nothing launched (the bit on quicked_batch_run_panel, _run_panel_scan, _run_search and
// _run_search_all, with bits 128, 256, 1024, 4096 and 16384, PREFIX with the tails bit beside it, sync == 0, members over 256 bases,
// check != 0, quicked_batch_configure_panel_heads outside 1 .. 256); the getter's rules before any run, after runs without the
// bit, other kinds of run and a reload; true heads -- text_end from the end pass -- on every case under both flags with
// QE_PANEL_SLICES unset, 1 and 4096, in all eight combinations of QUICKED_PANEL_CIGARS, _TAILS and _HEADS in INFIX and with
// PREFIX, at min_overlap 1, 3 and 256; the results of the run without the bit -- records, counts, scores, statuses, counters
// [0] .. [3], the strings, the tails -- unchanged by the bit; counters [6] and [7] within the short sweep's bound; the tails'
// min_overlap left alone; a batch without a single full occurrence.
#define PANEL_HOST_NAME "panel_heads_host"
#include "panel_host_common.h"

struct Head { int32_t pattern, overlap, end, score; };
struct Conf { int flag, min_overlap; std::vector<Head> want; };
struct Group { std::vector<std::string> panel, texts; std::vector<int32_t> bound; std::vector<Conf> confs; };

struct Results {
    std::vector<int32_t> found, stored, sc, st;
    std::vector<int64_t> off;
    std::vector<quicked_panel_occ_t> occ;
    int64_t c[8];
    bool operator==(const Results& o) const {
        return found == o.found && stored == o.stored && sc == o.sc && st == o.st && off == o.off && !memcmp(c, o.c, 4 * sizeof(int64_t)) && occ.size() == o.occ.size() &&
               (occ.empty() || !memcmp(occ.data(), o.occ.data(), occ.size() * sizeof(quicked_panel_occ_t)));
    }
};
static Results results_of(quicked_batch_t* b, int64_t n) {
    Results R;
    R.found.resize((size_t)n); R.stored.resize((size_t)n); R.sc.resize((size_t)n); R.st.resize((size_t)n); R.off.resize((size_t)n + 1);
    CHECK(quicked_batch_panel_hit_counts(b, R.found.data(), R.stored.data()) == QUICKED_OK);
    const int64_t total = quicked_batch_panel_hit_total(b);
    CHECK(total >= 0);
    R.occ.assign((size_t)total + 1, quicked_panel_occ_t{-7, -7, -7, -7});
    CHECK(quicked_batch_panel_hits(b, R.occ.data(), R.off.data()) == QUICKED_OK);
    R.occ.resize((size_t)total);
    CHECK(quicked_batch_scores(b, R.sc.data(), R.st.data()) >= 0);
    CHECK(quicked_batch_counters(b, R.c) >= 0);
    return R;
}
static void heads_refused(quicked_batch_t* b) {
    quicked_panel_head_t t[4];
    CHECK(quicked_batch_panel_heads(b, t) == QUICKED_ERROR);
}
static void tails_refused(quicked_batch_t* b) {
    quicked_panel_tail_t t[4];
    CHECK(quicked_batch_panel_tails(b, t) == QUICKED_ERROR);
}
// the heads of the last run; the getter writes n records and no more
static std::vector<quicked_panel_head_t> heads_of(quicked_batch_t* b, int64_t n) {
    std::vector<quicked_panel_head_t> t((size_t)n + 1, quicked_panel_head_t{-7, -7, -7, -7});
    CHECK(quicked_batch_panel_heads(b, t.data()) == QUICKED_OK);
    CHECK(quicked_batch_panel_heads(b, nullptr) == QUICKED_ERROR);
    CHECK(t[(size_t)n].pattern == -7 && t[(size_t)n].score == -7);
    t.resize((size_t)n);
    return t;
}
static std::vector<quicked_panel_tail_t> tails_of(quicked_batch_t* b, int64_t n) {
    std::vector<quicked_panel_tail_t> t((size_t)n, quicked_panel_tail_t{-7, -7, -7, -7});
    CHECK(quicked_batch_panel_tails(b, t.data()) == QUICKED_OK);
    return t;
}

static long run_group(const Group& G, bool first) {
    const int K = (int)G.panel.size(), n = (int)G.texts.size();
    const Pool M = pool_of(G.panel), T = pool_of(G.texts);
    const std::vector<std::string> none_s((size_t)n);
    const Pool E = pool_of(none_s);
    quicked_batch_t* b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
    CHECK(b);
    const int INFIX = QUICKED_SEARCH_INFIX, PREFIX = QUICKED_SEARCH_PREFIX, IU = QUICKED_SEARCH_IUPAC, CG = QUICKED_PANEL_CIGARS, TL = QUICKED_PANEL_TAILS,
              HD = QUICKED_PANEL_HEADS;
    const int32_t* own = G.bound.data();
    auto all_run = [&](int mode, const int32_t* md, int32_t all, int32_t max_hits, int sync = 1) {
        return quicked_batch_run_panel_all(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, max_hits, sync);
    };
    auto scan = [&](int mode) { return quicked_batch_run_panel_scan(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), own, 0, 16, 64, 1); };
    auto best_run = [&](int mode) { return quicked_batch_run_panel(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), own, 0, 1); };
    // the short sweep's bound on counter [6], and the walk's on counter [7]
    int64_t step_bound = 0, row_bound = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t tn = (int64_t)G.texts[(size_t)i].size();
        if (!tn) continue;
        for (int p = 0; p < K; ++p) {
            const int64_t m = (int64_t)G.panel[(size_t)p].size(), k = std::min<int64_t>(G.bound[(size_t)p], m);
            step_bound += (m + 63) / 64 * std::min(tn, m + k);
            row_bound += m - 1;
        }
    }
    long checked = 0;
    int64_t c0[8], c1[8];
    if (first) {
        static_assert(sizeof(quicked_panel_head_t) == 16 && QUICKED_PANEL_HEADS == 8192, "the public surface");
        heads_refused(b);                                   // before any run
        CHECK(quicked_batch_panel_heads(nullptr, nullptr) == QUICKED_ERROR && quicked_batch_configure_panel_heads(nullptr, 3) == QUICKED_ERROR);
        // ---- a first flagged run, so that "nothing launched" has results, heads and counters to leave alone
        CHECK(all_run(INFIX | IU | HD, own, 0, 16) == QUICKED_OK);
        const Results first_r = results_of(b, n);
        const std::vector<quicked_panel_head_t> first_h = heads_of(b, n);
        CHECK(quicked_batch_counters(b, c0) >= 0 && c0[0] > 0 && c0[6] > 0 && c0[7] > 0 && c0[2] == 0);
        // ---- QUICKED_ERROR, nothing launched
        for (int fl : {0, IU, (int)QUICKED_SEARCH_IUPAC_PATTERN}) {
            CHECK(best_run(INFIX | fl | HD) == QUICKED_ERROR && best_run(INFIX | fl | HD | QUICKED_PANEL_MATRIX) == QUICKED_ERROR);
            CHECK(scan(INFIX | fl | HD) == QUICKED_ERROR && scan(INFIX | fl | HD | CG) == QUICKED_ERROR);
            CHECK(quicked_batch_run_search(b, INFIX | fl | HD, nullptr, 3, 1, 1) == QUICKED_ERROR);
            CHECK(quicked_batch_run_search_all(b, INFIX | fl | HD, nullptr, 3, 4, 1) == QUICKED_ERROR);
            CHECK(all_run(PREFIX | fl | HD | TL, nullptr, 3, 16) == QUICKED_ERROR && all_run(PREFIX | fl | HD | TL | CG, nullptr, 3, 16) == QUICKED_ERROR);
            CHECK(all_run(INFIX | fl | HD | 1024, nullptr, 3, 16) == QUICKED_ERROR && all_run(INFIX | fl | HD | QUICKED_PANEL_MATRIX, nullptr, 3, 16) == QUICKED_ERROR);
        }
        for (int other : {4, 8, 128, 256, 1024, 4096, 1 << 14}) CHECK(all_run(INFIX | HD | other, nullptr, 3, 16) == QUICKED_ERROR && all_run(INFIX | HD | TL | CG | other, nullptr, 3, 16) == QUICKED_ERROR);
        CHECK(all_run(HD, nullptr, 3, 16) == QUICKED_ERROR && all_run(INFIX | IU | QUICKED_SEARCH_IUPAC_PATTERN | HD, nullptr, 3, 16) == QUICKED_ERROR);
        CHECK(all_run(INFIX | HD, nullptr, -1, 16) == QUICKED_ERROR && all_run(INFIX | HD, nullptr, 3, 0) == QUICKED_ERROR);
        for (int32_t bad : {0, -1, QUICKED_PANEL_MAX_LEN + 1, INT_MAX, INT_MIN}) CHECK(quicked_batch_configure_panel_heads(b, bad) == QUICKED_ERROR);
        // ---- QUICKED_UNIMPLEMENTED, nothing queued: every refusal of the run stands
        CHECK(all_run(INFIX | HD, nullptr, 3, 16, 0) == QUICKED_UNIMPLEMENTED && all_run(PREFIX | HD, nullptr, 3, 16, 0) == QUICKED_UNIMPLEMENTED);
        {
            const std::string big((size_t)QUICKED_PANEL_MAX_LEN + 1, 'A');
            const int64_t o2[2] = {0, 0};
            int32_t len[2] = {4, QUICKED_PANEL_MAX_LEN + 1};
            CHECK(quicked_batch_run_panel_all(b, INFIX | HD, 2, big.data(), o2, len, nullptr, 3, 16, 1) == QUICKED_UNIMPLEMENTED);
            CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
            CHECK(all_run(INFIX | HD, nullptr, 3, 16) == QUICKED_UNIMPLEMENTED);
            CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
        }
        CHECK(quicked_batch_counters(b, c1) >= 0 && !memcmp(c0, c1, sizeof(c0)));
        CHECK(results_of(b, n) == first_r);
        const std::vector<quicked_panel_head_t> again = heads_of(b, n);
        CHECK(!memcmp(again.data(), first_h.data(), (size_t)n * sizeof(quicked_panel_head_t)));
        // ---- other kinds of run in turn: the heads are the last flagged run's only, and counters [6] and [7] with them
        CHECK(all_run(INFIX | IU, own, 0, 16) == QUICKED_OK);
        heads_refused(b);
        CHECK(quicked_batch_counters(b, c1) >= 0 && c1[6] == 0 && c1[7] == 0);
        CHECK(all_run(INFIX | IU | HD, own, 0, 16) == QUICKED_OK);
        (void)heads_of(b, n);
        tails_refused(b);
        CHECK(all_run(INFIX | IU | TL, own, 0, 16) == QUICKED_OK);
        heads_refused(b);
        CHECK(quicked_batch_counters(b, c1) >= 0 && c1[6] == 0 && c1[7] == 0);
        CHECK(best_run(INFIX | IU) == QUICKED_OK);
        heads_refused(b);
        CHECK(all_run(INFIX | IU | HD | CG, own, 0, 16) == QUICKED_OK);
        (void)heads_of(b, n);
        CHECK(scan(INFIX | IU | CG) == QUICKED_OK);
        heads_refused(b);
        CHECK(all_run(PREFIX | IU | HD, own, 0, 16) == QUICKED_OK);
        (void)heads_of(b, n);
        CHECK(quicked_batch_run_search_all(b, INFIX, nullptr, 3, 4, 1) >= QUICKED_EMPTY_SEQUENCE);
        heads_refused(b);
    }
    // ---- true heads: both flags, the slices forced, all eight combinations of the three bits, PREFIX, min_overlap 1, 3 and 256
    for (const char* slices : {(const char*)nullptr, "1", "4096"}) {
        set_env("QE_PANEL_SLICES", slices);
        for (const Conf& cf : G.confs) {
            if (cf.flag == 0) continue;
            // (the tails keep a min_overlap of their own: the other one of {1, 3})
            CHECK(quicked_batch_configure_panel_tails(b, 4 - cf.min_overlap) == QUICKED_OK);
            CHECK(quicked_batch_configure_panel_heads(b, cf.min_overlap) == QUICKED_OK);
            for (int base : {INFIX, PREFIX})
                for (int tl : {0, TL})
                    for (int cg : {0, CG})
                        for (int32_t cap : {1, 64}) {
                            if (cap == 1 && (cg || tl || slices)) continue;
                            if (base == PREFIX && (tl || (slices && cg))) continue;
                            CHECK(all_run(base | cf.flag | cg | tl, own, 0, cap) == QUICKED_OK);
                            const Results plain = results_of(b, n);
                            std::vector<std::string> plain_s;
                            std::vector<quicked_panel_tail_t> plain_t;
                            if (cg) plain_s = strings_of(b);
                            if (tl) plain_t = tails_of(b, n);
                            heads_refused(b);
                            CHECK(plain.c[6] == 0 && plain.c[7] == 0);
                            CHECK(all_run(base | cf.flag | cg | tl | HD, own, 0, cap) == QUICKED_OK);
                            const Results with = results_of(b, n);
                            CHECK(with == plain);                    // (counters [0] .. [3] among them)
                            if (cg) CHECK(strings_of(b) == plain_s);
                            else CHECK(quicked_batch_panel_hit_cigar_bytes(b) == -1);
                            if (tl) { const std::vector<quicked_panel_tail_t> t2 = tails_of(b, n); CHECK(!memcmp(t2.data(), plain_t.data(), (size_t)n * sizeof(quicked_panel_tail_t))); }
                            else tails_refused(b);
                            const std::vector<quicked_panel_head_t> got = heads_of(b, n);
                            for (int i = 0; i < n; ++i) {
                                const Head& w = cf.want[(size_t)i];
                                const quicked_panel_head_t& h = got[(size_t)i];
                                if (h.pattern != w.pattern || h.overlap != w.overlap || h.text_end != w.end || h.score != w.score)
                                    fprintf(stderr, "base %d flag %d min_overlap %d slices %s text %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n", base, cf.flag,
                                            cf.min_overlap, slices ? slices : "-", i, h.pattern, h.overlap, h.text_end, h.score, w.pattern, w.overlap, w.end, w.score);
                                CHECK(h.pattern == w.pattern && h.overlap == w.overlap && h.text_end == w.end && h.score == w.score);
                                ++checked;
                            }
                            CHECK(with.c[6] > 0 && with.c[6] <= step_bound);      // never more block steps than the short sweep has
                            CHECK(with.c[7] > 0 ? with.c[7] <= row_bound : row_bound == 0);
                        }
        }
        // min_overlap 256: no row of a member of at most 256 bases is that long
        CHECK(quicked_batch_configure_panel_heads(b, QUICKED_PANEL_MAX_LEN) == QUICKED_OK);
        CHECK(all_run(INFIX | IU | HD, own, 0, 16) == QUICKED_OK);
        for (const quicked_panel_head_t& h : heads_of(b, n)) CHECK(h.pattern == -1 && h.overlap == -1 && h.text_end == -1 && h.score == -1);
        CHECK(quicked_batch_configure_panel_heads(b, 3) == QUICKED_OK && quicked_batch_configure_panel_tails(b, 3) == QUICKED_OK);
    }
    set_env("QE_PANEL_SLICES", nullptr);
    if (first) {
        // ---- a reload clears the heads
        CHECK(all_run(INFIX | IU | HD, own, 0, 16) == QUICKED_OK);
        const std::vector<quicked_panel_head_t> before = heads_of(b, n);
        const int n2 = n / 2;
        std::vector<std::string> pats((size_t)n2), txts(G.texts.begin(), G.texts.begin() + n2);
        const Pool P2 = pool_of(pats), T2 = pool_of(txts);
        CHECK(quicked_batch_reload(b, n2, P2.bytes.data(), P2.off.data(), P2.len.data(), T2.bytes.data(), T2.off.data(), T2.len.data()) >= 0);
        heads_refused(b);
        CHECK(all_run(INFIX | IU | HD, own, 0, 16) == QUICKED_OK);
        const std::vector<quicked_panel_head_t> after = heads_of(b, n2);
        CHECK(!memcmp(after.data(), before.data(), (size_t)n2 * sizeof(quicked_panel_head_t)));
    }
    quicked_batch_destroy(b);
    return checked;
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream f(std::string(argv[1]) + "/cases");
    int ngroups = 0;
    f >> ngroups;
    CHECK(!f.fail() && ngroups >= 1);
    long checked = 0;
    for (int g = 0; g < ngroups; ++g) {
        int K = 0, n = 0, nconf = 0;
        f >> K >> n >> nconf;
        CHECK(!f.fail() && K >= 1 && n >= 1 && nconf >= 1);
        Group G;
        G.panel.resize((size_t)K); G.texts.resize((size_t)n); G.bound.resize((size_t)K);
        for (int p = 0; p < K; ++p) f >> G.panel[(size_t)p] >> G.bound[(size_t)p];
        for (int i = 0; i < n; ++i) { f >> G.texts[(size_t)i]; if (G.texts[(size_t)i] == ".") G.texts[(size_t)i].clear(); }
        G.confs.resize((size_t)nconf);
        for (Conf& cf : G.confs) {
            f >> cf.flag >> cf.min_overlap;
            cf.want.resize((size_t)n);
            for (Head& t : cf.want) f >> t.pattern >> t.overlap >> t.end >> t.score;
            CHECK(!f.fail());
        }
        checked += run_group(G, g == 0);
    }
    // ---- a batch without a single full occurrence still has its heads
    {
        const int64_t zero = 0;
        const int32_t none = 0, six = 6, thirteen = 13;
        quicked_batch_t* q = quicked_batch_create(1, "", &zero, &none, "GCCCCC", &zero, &six);
        CHECK(q);
        CHECK(quicked_batch_configure_panel_heads(q, 1) == QUICKED_OK);
        CHECK(quicked_batch_run_panel_all(q, QUICKED_SEARCH_INFIX | QUICKED_SEARCH_IUPAC | QUICKED_PANEL_HEADS, 1, "AGATCGGAAGAGC", &zero, &thirteen, nullptr, 0, 4, 1) == QUICKED_OK);
        quicked_panel_head_t t{-7, -7, -7, -7};
        CHECK(quicked_batch_panel_hit_total(q) == 0 && quicked_batch_panel_heads(q, &t) == QUICKED_OK);
        CHECK(t.pattern == 0 && t.overlap == 2 && t.text_end == 2 && t.score == 0);
        quicked_batch_destroy(q);
    }
    CHECK(checked > 1000);
    printf("panel_heads_host ok %ld\n", checked);
    return 0;
}
