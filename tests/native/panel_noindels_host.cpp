// Mismatch-only panel runs (QUICKED_PANEL_NO_INDELS on quicked_batch_run_panel / _run_panel_all) on the HOST, under sanitizers:
// the library's host layer built with g++ against the fake HIP runtime of tests/native/hip_stub.  The stand-ins of k_panel_ham /
// k_panel_ham_hits and the two finish steps (hip_stub/qe_kernels_stub.h) are the device kernels' own source
// (qe_panel_ham.h) run slot by slot, and the stand-in of k_pack_iupac is the scalar packer of qe_iupac.h, so a run under one of
// the IUPAC flags gives true answers here: they are compared with what tests/test_host_panel_noindels.py computed with
// tests/panel_noindels_lib.py (file `cases` in the directory given; the format of tests/native/panel_noindels_cpu.cpp).  A run
// without an IUPAC flag reads planes the stub's k_pack never wrote: only its statuses and the shape of its results are checked.
// Checked: every refusal of the contract with nothing launched, the fixture through both runs with QE_PANEL_SLICES unset, 1 and
// huge and caps of 1, 2 and the file's, and every getter the contract names -- results, matrix, counts, total, records, scores,
// statuses, counters [0] .. [7], kernel_times slot [0] -- with the other families' refusals.
// A stand-alone program: nothing is loaded into Python.
#define PANEL_HOST_NAME "panel_noindels_host"
#include "panel_host_common.h"

struct Occ { int32_t pattern, start, end, score; };
struct Conf { int mode, flag; std::vector<std::vector<int32_t>> d, e; std::vector<int32_t> found; std::vector<std::vector<Occ>> occ; };
struct Group { std::vector<std::string> panel, texts; std::vector<int32_t> bound; std::vector<Conf> confs; };

static const int NI = QUICKED_PANEL_NO_INDELS, INFIX = QUICKED_SEARCH_INFIX, PREFIX = QUICKED_SEARCH_PREFIX;

static int64_t block_steps(const Group& g, int mode) {
    int64_t total = 0;
    for (const std::string& t : g.texts)
        for (const std::string& q : g.panel) {
            const int64_t n = (int64_t)t.size(), m = (int64_t)q.size();
            total += (n < m ? 0 : (mode == PREFIX ? 1 : n - m + 1)) * ((m + 63) / 64);
        }
    return total;
}

static void run_group(const Group& g, int cap_file) {
    const int K = (int)g.panel.size(), n = (int)g.texts.size();
    const Pool M = pool_of(g.panel), T = pool_of(g.texts);
    const std::vector<std::string> none_s((size_t)n);
    const Pool E = pool_of(none_s);
    quicked_batch_t* b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
    CHECK(b);
    std::vector<quicked_panel_hit_t> ph((size_t)n);
    std::vector<int32_t> ms((size_t)n * (size_t)K), me((size_t)n * (size_t)K), found((size_t)n), stored((size_t)n), sc((size_t)n), st((size_t)n);
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<quicked_panel_occ_t> occ;
    int64_t c[8];
    double ms_sum[4]; int64_t launches[4];
    for (const char* slices : {(const char*)nullptr, "1", "1000000000000"}) {
        set_env("QE_PANEL_SLICES", slices);
        for (const Conf& cf : g.confs) {
            if (!cf.flag) continue;
            // ---- quicked_batch_run_panel, with and without the matrix
            for (int matrix : {0, (int)QUICKED_PANEL_MATRIX}) {
                CHECK(quicked_batch_kernel_times(b, ms_sum, launches) >= 0);
                CHECK(quicked_batch_run_panel(b, cf.mode | cf.flag | NI | matrix, K, M.bytes.data(), M.off.data(), M.len.data(), g.bound.data(), 0, 1) == QUICKED_OK);
                CHECK(quicked_batch_panel_results(b, ph.data()) == QUICKED_OK);
                CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
                CHECK(quicked_batch_counters(b, c) >= 0 && c[0] == block_steps(g, cf.mode));
                for (int j = 1; j < 8; ++j) CHECK(c[j] == 0);
                CHECK(quicked_batch_kernel_times(b, ms_sum, launches) >= 0 && launches[0] == 1 && launches[1] == 0);
                if (matrix) CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_OK);
                else CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_ERROR);
                for (int i = 0; i < n; ++i) {
                    const std::vector<int32_t>& wd = cf.d[(size_t)i];
                    const std::vector<int32_t>& we = cf.e[(size_t)i];
                    int32_t p1 = -1, s1 = -1, p2 = -1, s2 = -1;
                    for (int p = 0; p < K; ++p) {
                        if (wd[(size_t)p] < 0) continue;
                        if (p1 < 0 || wd[(size_t)p] < s1) { p2 = p1; s2 = s1; p1 = p; s1 = wd[(size_t)p]; }
                        else if (p2 < 0 || wd[(size_t)p] < s2) { p2 = p; s2 = wd[(size_t)p]; }
                    }
                    const quicked_panel_hit_t h = ph[(size_t)i];
                    const int32_t end = p1 < 0 ? -1 : we[(size_t)p1], start = p1 < 0 ? -1 : end - M.len[(size_t)p1];
                    if (h.pattern != p1 || h.score != s1 || h.text_start != start || h.text_end != end || h.second_pattern != p2 || h.second_score != s2)
                        fprintf(stderr, "mode %d flag %d text %d: got {%d, %d, %d, %d, %d, %d}, expected {%d, %d, %d, %d, %d, %d}\n", cf.mode, cf.flag, i, h.pattern, h.score,
                                h.text_start, h.text_end, h.second_pattern, h.second_score, p1, s1, start, end, p2, s2);
                    CHECK(h.pattern == p1 && h.score == s1 && h.text_start == start && h.text_end == end && h.second_pattern == p2 && h.second_score == s2);
                    CHECK(sc[(size_t)i] == s1 && st[(size_t)i] == (g.texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
                    if (matrix) for (int p = 0; p < K; ++p) CHECK(ms[(size_t)i * K + p] == wd[(size_t)p] && me[(size_t)i * K + p] == we[(size_t)p]);
                }
                CHECK(quicked_batch_panel_hit_total(b) == -1 && quicked_batch_panel_hits(b, nullptr, off.data()) == QUICKED_ERROR);
                CHECK(quicked_batch_locations(b, sc.data(), sc.data()) == QUICKED_ERROR && quicked_batch_hit_total(b) == -1);
                CHECK(quicked_batch_panel_queue_wanted(b) == -1);
            }
            // ---- quicked_batch_run_panel_all
            for (int32_t cap : {1, 2, cap_file}) {
                CHECK(quicked_batch_kernel_times(b, ms_sum, launches) >= 0);
                CHECK(quicked_batch_run_panel_all(b, cf.mode | cf.flag | NI, K, M.bytes.data(), M.off.data(), M.len.data(), g.bound.data(), 0, cap, 1) == QUICKED_OK);
                CHECK(quicked_batch_panel_hit_counts(b, found.data(), stored.data()) == QUICKED_OK);
                const int64_t total = quicked_batch_panel_hit_total(b);
                CHECK(total >= 0);
                occ.assign((size_t)total + 1, quicked_panel_occ_t{-7, -7, -7, -7});
                CHECK(quicked_batch_panel_hits(b, occ.data(), off.data()) == QUICKED_OK);
                CHECK(off[0] == 0 && off[(size_t)n] == total && occ[(size_t)total].pattern == -7);
                CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
                CHECK(quicked_batch_counters(b, c) >= 0 && c[0] == block_steps(g, cf.mode));
                for (int j = 1; j < 8; ++j) CHECK(c[j] == 0);
                CHECK(quicked_batch_kernel_times(b, ms_sum, launches) >= 0 && launches[0] == 1 && launches[1] == 0);
                for (int i = 0; i < n; ++i) {
                    const std::vector<Occ>& w = cf.occ[(size_t)i];
                    const int32_t keep = std::min(cf.found[(size_t)i], cap);
                    CHECK(found[(size_t)i] == cf.found[(size_t)i] && stored[(size_t)i] == keep && off[(size_t)i + 1] - off[(size_t)i] == keep);
                    int32_t best = -1;
                    for (int32_t d : cf.d[(size_t)i]) best = (d >= 0 && (best < 0 || d < best)) ? d : best;
                    CHECK(sc[(size_t)i] == best && st[(size_t)i] == (g.texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
                    for (int k = 0; k < keep; ++k) {
                        const quicked_panel_occ_t h = occ[(size_t)(off[(size_t)i] + k)];
                        const Occ& o = w[(size_t)k];
                        if (h.pattern != o.pattern || h.text_start != o.start || h.text_end != o.end || h.score != o.score)
                            fprintf(stderr, "mode %d flag %d cap %d text %d occurrence %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n", cf.mode, cf.flag, cap, i, k,
                                    h.pattern, h.text_start, h.text_end, h.score, o.pattern, o.start, o.end, o.score);
                        CHECK(h.pattern == o.pattern && h.text_start == o.start && h.text_end == o.end && h.score == o.score);
                    }
                }
                CHECK(quicked_batch_panel_results(b, ph.data()) == QUICKED_ERROR && quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_ERROR);
                CHECK(quicked_batch_panel_hit_cigar_bytes(b) == -1);
                quicked_panel_tail_t tail; quicked_panel_head_t head;
                CHECK(quicked_batch_panel_tails(b, &tail) == QUICKED_ERROR && quicked_batch_panel_heads(b, &head) == QUICKED_ERROR);
                CHECK(quicked_batch_panel_queue_wanted(b) == -1);
            }
        }
    }
    set_env("QE_PANEL_SLICES", nullptr);
    quicked_batch_destroy(b);
}

// every refusal of the contract, with nothing launched: the results and the counters stay those of the run before
static void refusals(const Group& g) {
    const int K = (int)g.panel.size(), n = (int)g.texts.size();
    const Pool M = pool_of(g.panel), T = pool_of(g.texts);
    const std::vector<std::string> none_s((size_t)n);
    const Pool E = pool_of(none_s);
    quicked_batch_t* b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
    CHECK(b);
    auto best = [&](int mode, int sync) { return quicked_batch_run_panel(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, sync); };
    auto all = [&](int mode, int32_t mh, int sync) { return quicked_batch_run_panel_all(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, mh, sync); };
    CHECK(all(INFIX | QUICKED_SEARCH_IUPAC | NI, 16, 1) == QUICKED_OK);
    const int64_t total0 = quicked_batch_panel_hit_total(b);
    int64_t c0[8], c1[8];
    CHECK(quicked_batch_counters(b, c0) >= 0 && c0[0] > 0 && total0 >= 0);
    // ---- the QUICKED_ERROR rules of the two runs come first, unchanged
    CHECK(quicked_batch_run_panel(nullptr, INFIX | NI, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel_all(nullptr, INFIX | NI, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, 16, 1) == QUICKED_ERROR);
    for (int bad : {NI + 0, 3 | NI, 4 | NI, INFIX | NI | 8, INFIX | NI | 128, INFIX | NI | 256, INFIX | NI | 1024, INFIX | NI | 4096, INFIX | NI | 16384, INFIX | NI | 65536,
                    INFIX | NI | QUICKED_SEARCH_IUPAC | QUICKED_SEARCH_IUPAC_PATTERN}) {
        CHECK(best(bad, 1) == QUICKED_ERROR && best(bad, 0) == QUICKED_ERROR);
        CHECK(all(bad, 16, 1) == QUICKED_ERROR && all(bad, 16, 0) == QUICKED_ERROR);
    }
    CHECK(all(INFIX | NI | QUICKED_PANEL_MATRIX, 16, 1) == QUICKED_ERROR);                         // the matrix is run_panel's
    CHECK(best(INFIX | NI | QUICKED_PANEL_CIGARS, 1) == QUICKED_ERROR && best(INFIX | NI | QUICKED_PANEL_TAILS, 1) == QUICKED_ERROR);
    CHECK(best(INFIX | NI | QUICKED_PANEL_HEADS, 1) == QUICKED_ERROR);
    CHECK(all(PREFIX | NI | QUICKED_PANEL_TAILS, 16, 1) == QUICKED_ERROR);                          // PREFIX with tails: an error before the bit is looked at
    for (int32_t mh : {0, -1, 4097}) CHECK(all(INFIX | NI, mh, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel(b, INFIX | NI, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, -1, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel(b, INFIX | NI, 0, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, 1) == QUICKED_ERROR);
    {
        std::vector<int32_t> len = M.len;
        len[0] = 0;
        CHECK(quicked_batch_run_panel(b, INFIX | NI, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 2, 0) == QUICKED_ERROR);
        CHECK(quicked_batch_run_panel_all(b, INFIX | NI, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 2, 16, 0) == QUICKED_ERROR);
    }
    // ---- the bit on the other runs: an unknown bit
    CHECK(quicked_batch_run_panel_scan(b, INFIX | NI, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 2, 16, 0, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search(b, INFIX | NI, nullptr, 2, 1, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search_all(b, INFIX | NI, nullptr, 2, 16, 1) == QUICKED_ERROR);
    // ---- QUICKED_UNIMPLEMENTED with the bit
    for (int mode : {INFIX, PREFIX}) {
        CHECK(all(mode | NI | QUICKED_PANEL_CIGARS, 16, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(all(mode | NI | QUICKED_PANEL_HEADS, 16, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(all(mode | NI | QUICKED_PANEL_HEADS | QUICKED_PANEL_CIGARS | QUICKED_SEARCH_IUPAC, 16, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(best(mode | NI, 0) == QUICKED_UNIMPLEMENTED && best(mode | NI | QUICKED_PANEL_MATRIX, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(all(mode | NI, 16, 0) == QUICKED_UNIMPLEMENTED);
    }
    CHECK(all(INFIX | NI | QUICKED_PANEL_TAILS, 16, 1) == QUICKED_UNIMPLEMENTED);
    CHECK(all(INFIX | NI | QUICKED_PANEL_TAILS | QUICKED_PANEL_HEADS, 16, 1) == QUICKED_UNIMPLEMENTED);
    // ... sync == 0 also on a batch object whose queue is switched on, where the unflagged runs are taken
    CHECK(quicked_batch_configure_panel_queue(b, 1 << 20) == QUICKED_OK);
    CHECK(best(INFIX | NI, 0) == QUICKED_UNIMPLEMENTED && all(INFIX | NI, 16, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(best(PREFIX | NI | QUICKED_SEARCH_IUPAC, 0) == QUICKED_UNIMPLEMENTED && all(PREFIX | NI | QUICKED_SEARCH_IUPAC_PATTERN, 16, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure_panel_queue(b, 0) == QUICKED_OK);
    {
        const std::string big((size_t)QUICKED_PANEL_MAX_LEN + 1, 'A');
        const int64_t o2[2] = {0, 0};
        int32_t len[2] = {4, QUICKED_PANEL_MAX_LEN + 1};
        CHECK(quicked_batch_run_panel(b, INFIX | NI, 2, big.data(), o2, len, nullptr, 2, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_panel_all(b, INFIX | NI, 2, big.data(), o2, len, nullptr, 2, 16, 1) == QUICKED_UNIMPLEMENTED);
    }
    CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);                                          // check != 0
    CHECK(best(INFIX | NI, 1) == QUICKED_UNIMPLEMENTED && all(INFIX | NI | QUICKED_SEARCH_IUPAC, 16, 1) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    // none of it ran
    CHECK(quicked_batch_counters(b, c1) >= 0 && !memcmp(c0, c1, sizeof(c0)) && quicked_batch_panel_hit_total(b) == total0);
    // ---- without an IUPAC flag the stub's k_pack writes no planes: statuses and shapes
    std::vector<quicked_panel_hit_t> ph((size_t)n);
    std::vector<int32_t> sc((size_t)n), st((size_t)n);
    for (int mode : {PREFIX, INFIX}) {
        CHECK(best(mode | NI, 1) == QUICKED_OK);
        CHECK(quicked_batch_panel_results(b, ph.data()) == QUICKED_OK && quicked_batch_scores(b, sc.data(), st.data()) >= 0);
        for (int i = 0; i < n; ++i) {
            const quicked_panel_hit_t h = ph[(size_t)i];
            CHECK(st[(size_t)i] == (g.texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
            CHECK(h.pattern < 0 ? (h.text_start == -1 && h.text_end == -1 && h.score == -1) : (h.text_start == h.text_end - M.len[(size_t)h.pattern] && h.text_start >= 0 && h.score <= 2));
            CHECK(mode != PREFIX || h.pattern < 0 || h.text_start == 0);
        }
        CHECK(all(mode | NI, 4, 1) == QUICKED_OK && quicked_batch_panel_hit_total(b) >= 0);
    }
    // ---- the unflagged runs beside it: each run's getters report that run
    CHECK(all(INFIX | QUICKED_SEARCH_IUPAC, 16, 1) == QUICKED_OK);
    CHECK(all(INFIX | QUICKED_SEARCH_IUPAC | NI, 16, 1) == QUICKED_OK && quicked_batch_panel_hit_total(b) == total0);
    quicked_batch_destroy(b);
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream f(std::string(argv[1]) + "/cases");
    int ngroups = 0, cap = 0;
    f >> ngroups >> cap;
    CHECK(!f.fail() && ngroups >= 1 && cap >= 3);
    std::vector<Group> groups((size_t)ngroups);
    for (Group& g : groups) {
        int K = 0, n = 0, nconf = 0;
        f >> K >> n >> nconf;
        CHECK(!f.fail() && K >= 1 && n >= 1 && nconf >= 1);
        g.panel.resize((size_t)K); g.bound.resize((size_t)K); g.texts.resize((size_t)n); g.confs.resize((size_t)nconf);
        for (int p = 0; p < K; ++p) f >> g.panel[(size_t)p] >> g.bound[(size_t)p];
        for (int i = 0; i < n; ++i) { f >> g.texts[(size_t)i]; if (g.texts[(size_t)i] == ".") g.texts[(size_t)i].clear(); }
        for (Conf& cf : g.confs) {
            f >> cf.mode >> cf.flag;
            cf.d.assign((size_t)n, std::vector<int32_t>((size_t)K)); cf.e = cf.d;
            cf.found.resize((size_t)n); cf.occ.resize((size_t)n);
            for (int i = 0; i < n; ++i) {
                for (int p = 0; p < K; ++p) f >> cf.d[(size_t)i][(size_t)p];
                for (int p = 0; p < K; ++p) f >> cf.e[(size_t)i][(size_t)p];
                f >> cf.found[(size_t)i];
                cf.occ[(size_t)i].resize((size_t)std::min(cf.found[(size_t)i], cap));
                for (Occ& o : cf.occ[(size_t)i]) f >> o.pattern >> o.start >> o.end >> o.score;
            }
            CHECK(!f.fail());
        }
    }
    refusals(groups[0]);
    for (const Group& g : groups) run_group(g, cap);
    printf("panel_noindels_host ok\n");
    return 0;
}
