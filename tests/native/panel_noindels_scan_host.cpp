// The windowed mismatch-only panel run (quicked_batch_run_panel_scan_no_indels) on the HOST, under sanitizers: the library's host
// layer built with g++ against the fake HIP runtime of tests/native/hip_stub.  The stand-ins of k_panel_ham_scan and
// k_panel_ham_scan_expand (hip_stub/qe_kernels_stub_noindels_scan.h) are the device kernels' own source (qe_panel_ham.h,
// qe_panel.h) run slot by slot, and the stand-in of k_pack_iupac is the scalar packer of qe_iupac.h, so a run under one of the
// IUPAC flags gives true answers here: they are compared with the lists and block steps tests/test_host_panel_noindels_scan.py
// handed over (file `cases` in the directory given; tests/panel_noindels_scan_lib.py's format) and with the flagged
// quicked_batch_run_panel_all on the same batch.  A run without an IUPAC flag reads planes the stub's k_pack never wrote: only its
// statuses and the shape of its results are checked.
// Checked: every QUICKED_ERROR and QUICKED_UNIMPLEMENTED rule with nothing launched, the getters' rules around other kinds of
// run, results cleared by a reload, QE_PANEL_SLICES unset, 1 and huge, windows of 64, 128, 192, 4096 and the library's, caps of
// 1, 2 and 4096, counters [0] .. [7] and kernel_times slot [0].
// A stand-alone program: nothing is loaded into Python.
#define PANEL_HOST_NAME "panel_noindels_scan_host"
#include "panel_host_common.h"

struct Occ { int32_t pattern, start, end, score; };
struct Conf { int flag; long long steps[4]; std::vector<std::vector<Occ>> want; };
struct Group { std::vector<std::string> panel, texts; std::vector<int32_t> bound; std::vector<Conf> confs; };
static const int32_t WINDOWS[4] = {64, 128, 192, 4096};
static const int NI = QUICKED_PANEL_NO_INDELS, INFIX = QUICKED_SEARCH_INFIX, PREFIX = QUICKED_SEARCH_PREFIX;

// everything the three getters and the scores give after a run of the kind
struct Results {
    std::vector<int32_t> found, stored, sc, st;
    std::vector<int64_t> off;
    std::vector<quicked_panel_occ_t> occ;
    bool operator==(const Results& o) const {
        return found == o.found && stored == o.stored && sc == o.sc && st == o.st && off == o.off && occ.size() == o.occ.size() &&
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
    CHECK(R.off[0] == 0 && R.off[(size_t)n] == total && R.occ[(size_t)total].pattern == -7);
    R.occ.resize((size_t)total);
    CHECK(quicked_batch_scores(b, R.sc.data(), R.st.data()) >= 0);
    return R;
}
// the counters of a flagged run: [0] -> returned, [1] .. [7] are 0; one timed launch in slot [0]
static int64_t counters_of(quicked_batch_t* b) {
    int64_t c[8];
    CHECK(quicked_batch_counters(b, c) >= 0);
    for (int j = 1; j < 8; ++j) CHECK(c[j] == 0);
    return c[0];
}

struct Batch {
    Pool M, T, E;
    quicked_batch_t* b;
    int K, n;
    explicit Batch(const Group& g) : M(pool_of(g.panel)), T(pool_of(g.texts)), E(pool_of(std::vector<std::string>(g.texts.size()))), K((int)g.panel.size()), n((int)g.texts.size()) {
        b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
        CHECK(b);
    }
    ~Batch() { quicked_batch_destroy(b); }
    quicked_status_t scan(int mode, const int32_t* md, int32_t all, int32_t mh, int32_t window, int sync = 1) const {
        return quicked_batch_run_panel_scan_no_indels(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, mh, window, sync);
    }
    quicked_status_t all_run(int mode, const int32_t* md, int32_t all, int32_t mh) const {
        return quicked_batch_run_panel_all(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, mh, 1);
    }
};

static void run_group(const Group& g, bool every_shape) {
    const Batch B(g);
    const int n = B.n;
    double ms_sum[4]; int64_t launches[4];
    for (const char* slices : {(const char*)nullptr, "1", "1000000000000"}) {
        if (slices && !every_shape) continue;
        set_env("QE_PANEL_SLICES", slices);
        for (const Conf& cf : g.confs) {
            if (!cf.flag) continue;
            for (int32_t cap : {1, 2, 4096}) {
                if (slices && cap == 2) continue;
                CHECK(B.all_run(INFIX | cf.flag | NI, g.bound.data(), 0, cap) == QUICKED_OK);
                const Results A = results_of(B.b, n);
                const int64_t steps_all = counters_of(B.b);
                for (int wi = 0; wi < 5; ++wi) {
                    const int32_t window = wi < 4 ? WINDOWS[wi] : 0;
                    if (!every_shape && (window == 192 || window == 4096)) continue;
                    CHECK(quicked_batch_kernel_times(B.b, ms_sum, launches) >= 0);
                    CHECK(B.scan(INFIX | cf.flag | (wi & 1 ? NI : 0), g.bound.data(), 0, cap, window) == QUICKED_OK);      // the bit means nothing more
                    const Results R = results_of(B.b, n);
                    CHECK(R == A);
                    const int64_t steps = counters_of(B.b);
                    if (wi < 4 && steps != cf.steps[wi]) fprintf(stderr, "flag %d cap %d window %d: %lld block steps, the model %lld\n", cf.flag, cap, window, (long long)steps, cf.steps[wi]);
                    CHECK(wi < 4 ? steps == cf.steps[wi] : steps >= steps_all);
                    CHECK(quicked_batch_kernel_times(B.b, ms_sum, launches) >= 0 && launches[0] == 1 && launches[1] == 0);
                    for (int i = 0; i < n; ++i) {
                        const std::vector<Occ>& w = cf.want[(size_t)i];
                        const int32_t keep = (int32_t)std::min<size_t>(w.size(), (size_t)cap);
                        int32_t best = -1;
                        for (const Occ& o : w) best = (best < 0 || o.score < best) ? o.score : best;
                        CHECK(R.found[(size_t)i] == (int32_t)w.size() && R.stored[(size_t)i] == keep && R.off[(size_t)i + 1] - R.off[(size_t)i] == keep);
                        CHECK(R.sc[(size_t)i] == best && R.st[(size_t)i] == (g.texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
                        for (int k = 0; k < keep; ++k) {
                            const quicked_panel_occ_t h = R.occ[(size_t)(R.off[(size_t)i] + k)];
                            const Occ& o = w[(size_t)k];
                            if (h.pattern != o.pattern || h.text_start != o.start || h.text_end != o.end || h.score != o.score)
                                fprintf(stderr, "flag %d cap %d window %d text %d occurrence %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n", cf.flag, cap, window, i, k,
                                        h.pattern, h.text_start, h.text_end, h.score, o.pattern, o.start, o.end, o.score);
                            CHECK(h.pattern == o.pattern && h.text_start == o.start && h.text_end == o.end && h.score == o.score);
                        }
                    }
                }
            }
        }
    }
    set_env("QE_PANEL_SLICES", nullptr);
}

// every refusal of the contract with nothing launched, the getters around other kinds of run, reload
static void rules(const Group& g) {
    const Batch B(g);
    const int K = B.K, n = B.n;
    const Pool& M = B.M;
    std::vector<int32_t> loc((size_t)n);
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<quicked_panel_hit_t> ph((size_t)n);
    auto getters_refuse = [&](quicked_batch_t* q) {
        CHECK(quicked_batch_panel_hit_counts(q, loc.data(), loc.data()) == QUICKED_ERROR);
        CHECK(quicked_batch_panel_hit_total(q) == -1);
        CHECK(quicked_batch_panel_hits(q, nullptr, off.data()) == QUICKED_ERROR);
    };
    getters_refuse(B.b);
    const int IU = QUICKED_SEARCH_IUPAC;
    // ---- a first run, so that "nothing launched" has counters and results to leave alone
    CHECK(B.scan(INFIX | IU, g.bound.data(), 0, 16, 64) == QUICKED_OK);
    const Results first = results_of(B.b, n);
    int64_t c0[8], c1[8];
    CHECK(quicked_batch_counters(B.b, c0) >= 0 && c0[0] > 0);
    const int64_t total0 = quicked_batch_panel_hit_total(B.b);
    CHECK(total0 > 0);
    // ---- QUICKED_ERROR, nothing launched: everything the scan answers so ...
    CHECK(quicked_batch_run_panel_scan_no_indels(nullptr, INFIX, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, 16, 64, 1) == QUICKED_ERROR);
    for (int mode : {0, NI, 3, 3 | NI, 4, 16, 16 | 32 | 2, 128 | 2, 256 | 1, 8 | 2, 1024 | 2, 4096 | 2, 16384 | 2, 65536 | 2, -1})
        for (int sync : {1, 0}) CHECK(B.scan(mode, nullptr, 2, 16, 64, sync) == QUICKED_ERROR);
    // ... QUICKED_PANEL_MATRIX, _TAILS and _HEADS: unknown bits of the scan, with and without the bit
    for (int bit : {(int)QUICKED_PANEL_MATRIX, (int)QUICKED_PANEL_TAILS, (int)QUICKED_PANEL_HEADS, (int)(QUICKED_PANEL_TAILS | QUICKED_PANEL_CIGARS)})
        for (int ni : {0, NI}) CHECK(B.scan(INFIX | bit | ni, nullptr, 2, 16, 64) == QUICKED_ERROR && B.scan(PREFIX | bit | ni | IU, nullptr, 2, 16, 0, 0) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel_scan_no_indels(B.b, INFIX, 0, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, 16, 64, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel_scan_no_indels(B.b, INFIX, QUICKED_PANEL_MAX_PATTERNS + 1, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, 16, 64, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel_scan_no_indels(B.b, INFIX, K, nullptr, M.off.data(), M.len.data(), nullptr, 2, 16, 64, 1) == QUICKED_ERROR);
    {
        std::vector<int32_t> len = M.len;
        len[0] = 0;                                               // an empty member -- even next to one that is too long
        CHECK(quicked_batch_run_panel_scan_no_indels(B.b, INFIX, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 2, 16, 64, 1) == QUICKED_ERROR);
        std::vector<int32_t> bad = g.bound;
        bad[(size_t)K - 1] = -1;                                  // a negative bound
        CHECK(B.scan(INFIX, bad.data(), 2, 16, 64) == QUICKED_ERROR && B.scan(INFIX, nullptr, -1, 16, 64) == QUICKED_ERROR);
    }
    for (int32_t mh : {0, -1, 4097, INT_MAX}) CHECK(B.scan(INFIX | NI, nullptr, 2, mh, 64) == QUICKED_ERROR);
    // ... and the window's, for PREFIX and with QUICKED_PANEL_CIGARS too: an error comes before "not built"
    for (int32_t w : {-64, -1, 1, 63, 65, 96, 100, 4095, INT_MAX, INT_MIN}) {
        CHECK(B.scan(INFIX, nullptr, 2, 16, w) == QUICKED_ERROR && B.scan(PREFIX | NI, nullptr, 2, 16, w) == QUICKED_ERROR);
        CHECK(B.scan(INFIX | QUICKED_PANEL_CIGARS, nullptr, 2, 16, w, 0) == QUICKED_ERROR);
    }
    // ---- the room for the stored occurrences: one text of 16 385 x 64 bases has one window slot too many at a forced window of
    // 64 and max_hits 4096; the rule comes before the QUICKED_UNIMPLEMENTED ones
    {
        const int64_t zero = 0;
        const int32_t one = 1, big_n = 16385 * 64, none = 0;
        const std::string big_text((size_t)big_n, 'A');
        quicked_batch_t* q = quicked_batch_create(1, "", &zero, &none, big_text.data(), &zero, &big_n);
        CHECK(q);
        auto one_scan = [&](int32_t mh, int32_t w, int sync) { return quicked_batch_run_panel_scan_no_indels(q, INFIX, 1, "C", &zero, &one, nullptr, 0, mh, w, sync); };
        CHECK(one_scan(4096, 64, 1) == QUICKED_ERROR && one_scan(4096, 64, 0) == QUICKED_ERROR);
        CHECK(one_scan(4095, 64, 0) == QUICKED_UNIMPLEMENTED && one_scan(4096, 128, 0) == QUICKED_UNIMPLEMENTED && one_scan(4096, 0, 0) == QUICKED_UNIMPLEMENTED);
        getters_refuse(q);
        quicked_batch_destroy(q);
        std::vector<int64_t> o((size_t)16385, 0);
        std::vector<int32_t> tl((size_t)16385, 1), pl((size_t)16385, 0);
        quicked_batch_t* over = quicked_batch_create(16385, "A", o.data(), pl.data(), "A", o.data(), tl.data());
        CHECK(over);
        for (int32_t w : {0, 64, 4096}) CHECK(quicked_batch_run_panel_scan_no_indels(over, INFIX, 1, "A", &zero, &one, nullptr, 0, 4096, w, 0) == QUICKED_ERROR);
        CHECK(quicked_batch_run_panel_scan_no_indels(over, INFIX, 1, "A", &zero, &one, nullptr, 0, 4095, 0, 0) == QUICKED_UNIMPLEMENTED);
        quicked_batch_destroy(over);
    }
    // ---- QUICKED_UNIMPLEMENTED, nothing launched
    for (int32_t w : {0, 64, 4096})
        for (int fl : {0, IU, (int)QUICKED_SEARCH_IUPAC_PATTERN})
            for (int ni : {0, NI}) CHECK(B.scan(PREFIX | fl | ni, nullptr, 2, 16, w) == QUICKED_UNIMPLEMENTED);
    for (int ni : {0, NI}) {
        CHECK(B.scan(INFIX | ni | QUICKED_PANEL_CIGARS, nullptr, 2, 16, 64) == QUICKED_UNIMPLEMENTED);
        CHECK(B.scan(INFIX | ni | QUICKED_PANEL_CIGARS | IU, g.bound.data(), 0, 16, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(B.scan(INFIX | ni, nullptr, 2, 16, 64, 0) == QUICKED_UNIMPLEMENTED);
    }
    // ... sync == 0 also on a batch object whose queue is switched on
    CHECK(quicked_batch_configure_panel_queue(B.b, 1 << 20) == QUICKED_OK);
    CHECK(B.scan(INFIX | NI, nullptr, 2, 16, 64, 0) == QUICKED_UNIMPLEMENTED && B.scan(INFIX | IU, nullptr, 2, 16, 0, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure_panel_queue(B.b, 0) == QUICKED_OK);
    {
        const std::string big((size_t)QUICKED_PANEL_MAX_LEN + 1, 'A');
        const int64_t o2[2] = {0, 0};
        int32_t len[2] = {4, QUICKED_PANEL_MAX_LEN + 1};
        CHECK(quicked_batch_run_panel_scan_no_indels(B.b, INFIX | NI, 2, big.data(), o2, len, nullptr, 2, 16, 64, 1) == QUICKED_UNIMPLEMENTED);
    }
    CHECK(quicked_batch_configure(B.b, 0, 1) == QUICKED_OK);                                        // check != 0
    CHECK(B.scan(INFIX | NI, nullptr, 2, 16, 64) == QUICKED_UNIMPLEMENTED && B.scan(INFIX | IU, nullptr, 2, 16, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure(B.b, 0, 0) == QUICKED_OK);
    // the bit on quicked_batch_run_panel_scan itself stays an unknown bit
    CHECK(quicked_batch_run_panel_scan(B.b, INFIX | NI, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, 16, 0, 1) == QUICKED_ERROR);
    // none of it ran: the results and the counters are the first run's
    CHECK(quicked_batch_counters(B.b, c1) >= 0 && !memcmp(c0, c1, sizeof(c0)) && results_of(B.b, n) == first);
    // ---- without an IUPAC flag the stub's k_pack writes no planes (whatever the pool held): statuses and shapes
    for (int32_t window : {64, 0}) {
        CHECK(B.scan(INFIX, nullptr, 2, 4, window) == QUICKED_OK);
        const Results R = results_of(B.b, n);
        counters_of(B.b);
        for (int i = 0; i < n; ++i) {
            CHECK(R.st[(size_t)i] == (g.texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
            CHECK(R.stored[(size_t)i] == std::min(R.found[(size_t)i], 4) && (R.found[(size_t)i] == 0) == (R.sc[(size_t)i] == -1));
            for (int64_t j = R.off[(size_t)i]; j < R.off[(size_t)i + 1]; ++j) {
                const quicked_panel_occ_t h = R.occ[(size_t)j];
                CHECK(h.pattern >= 0 && h.pattern < K && h.score >= 0 && h.score <= 2 && h.text_end <= (int32_t)g.texts[(size_t)i].size());
                CHECK(h.text_start == h.text_end - M.len[(size_t)h.pattern] && h.text_start >= 0);
            }
        }
    }
    // ---- other kinds of run in turn: each getter family reports its own run only, and this run is a run_panel_all's kind
    CHECK(quicked_batch_run_panel(B.b, INFIX | IU | NI, K, M.bytes.data(), M.off.data(), M.len.data(), g.bound.data(), 0, 1) == QUICKED_OK);
    getters_refuse(B.b);
    CHECK(quicked_batch_panel_results(B.b, ph.data()) == QUICKED_OK);
    CHECK(B.scan(INFIX | IU, g.bound.data(), 0, 16, 128) == QUICKED_OK && results_of(B.b, n) == first);
    CHECK(quicked_batch_panel_results(B.b, ph.data()) == QUICKED_ERROR && quicked_batch_panel_matrix(B.b, loc.data(), loc.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_locations(B.b, loc.data(), loc.data()) == QUICKED_ERROR && quicked_batch_hit_total(B.b) == -1);
    CHECK(quicked_batch_panel_hit_cigar_bytes(B.b) == -1 && quicked_batch_panel_queue_wanted(B.b) == -1 && quicked_batch_cigar_bytes(B.b) == 0);
    quicked_panel_tail_t tail; quicked_panel_head_t head;
    CHECK(quicked_batch_panel_tails(B.b, &tail) == QUICKED_ERROR && quicked_batch_panel_heads(B.b, &head) == QUICKED_ERROR);
    // the unflagged scan (edit distance) and back
    CHECK(quicked_batch_run_panel_scan(B.b, INFIX | IU, K, M.bytes.data(), M.off.data(), M.len.data(), g.bound.data(), 0, 16, 64, 1) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(B.b) >= 0);
    CHECK(B.scan(INFIX | IU | NI, g.bound.data(), 0, 16, 0) == QUICKED_OK && results_of(B.b, n) == first);
    CHECK(quicked_batch_run_search_all(B.b, INFIX, nullptr, 3, 4, 1) >= QUICKED_EMPTY_SEQUENCE);      // (the batch's patterns are all empty)
    getters_refuse(B.b);
    // ---- results cleared by a reload: fewer pairs, real patterns that play no part
    CHECK(B.scan(INFIX | IU, g.bound.data(), 0, 16, 64) == QUICKED_OK && results_of(B.b, n) == first);
    {
        const int n2 = n / 2;
        std::vector<std::string> pats((size_t)n2), txts(g.texts.begin(), g.texts.begin() + n2);
        for (int i = 0; i < n2; ++i) pats[(size_t)i] = g.panel[(size_t)(i % K)];
        const Pool P2 = pool_of(pats), T2 = pool_of(txts);
        CHECK(quicked_batch_reload(B.b, n2, P2.bytes.data(), P2.off.data(), P2.len.data(), T2.bytes.data(), T2.off.data(), T2.len.data()) >= 0);
        getters_refuse(B.b);
        const Conf* cf = nullptr;
        for (const Conf& c : g.confs) if (c.flag == IU) cf = &c;
        CHECK(cf);
        CHECK(B.scan(INFIX | IU, g.bound.data(), 0, 4096, 64) == QUICKED_OK);
        const Results R = results_of(B.b, n2);
        for (int i = 0; i < n2; ++i) {
            const std::vector<Occ>& w = cf->want[(size_t)i];
            CHECK(R.found[(size_t)i] == (int32_t)w.size() && R.stored[(size_t)i] == R.found[(size_t)i]);
            for (size_t k = 0; k < w.size(); ++k) {
                const quicked_panel_occ_t h = R.occ[(size_t)R.off[(size_t)i] + k];
                CHECK(h.pattern == w[k].pattern && h.text_start == w[k].start && h.text_end == w[k].end && h.score == w[k].score);
            }
        }
    }
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream f(std::string(argv[1]) + "/cases");
    int ngroups = 0;
    f >> ngroups;
    CHECK(!f.fail() && ngroups >= 1);
    std::vector<Group> groups((size_t)ngroups);
    for (Group& g : groups) {
        int K = 0, n = 0, nconf = 0;
        f >> K >> n >> nconf;
        CHECK(!f.fail() && K >= 1 && n >= 1 && nconf >= 1);
        g.panel.resize((size_t)K); g.bound.resize((size_t)K); g.texts.resize((size_t)n); g.confs.resize((size_t)nconf);
        for (int p = 0; p < K; ++p) f >> g.panel[(size_t)p] >> g.bound[(size_t)p];
        for (int i = 0; i < n; ++i) { f >> g.texts[(size_t)i]; if (g.texts[(size_t)i] == ".") g.texts[(size_t)i].clear(); }
        for (Conf& cf : g.confs) {
            f >> cf.flag >> cf.steps[0] >> cf.steps[1] >> cf.steps[2] >> cf.steps[3];
            cf.want.resize((size_t)n);
            for (int i = 0; i < n; ++i) {
                int found = 0;
                f >> found;
                CHECK(!f.fail() && found >= 0);
                cf.want[(size_t)i].resize((size_t)found);
                for (Occ& o : cf.want[(size_t)i]) f >> o.pattern >> o.start >> o.end >> o.score;
            }
            CHECK(!f.fail());
        }
    }
    rules(groups[0]);
    for (size_t i = 0; i < groups.size(); ++i) run_group(groups[i], i < 2);
    printf("panel_noindels_scan_host ok\n");
    return 0;
}
