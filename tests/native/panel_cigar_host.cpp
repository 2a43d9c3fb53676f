// Occurrence alignments (QUICKED_PANEL_CIGARS) on the HOST, under sanitizers: the library's host layer built with g++ against the
// fake HIP runtime of tests/native/hip_stub.  The stand-ins of k_panel_occ_align / k_panel_align_sizes
// (hip_stub/qe_kernels_stub.h) are the device kernels' own source (qe_panel_align.h) run occurrence by occurrence, the
// sweeps' stand-ins run the real recurrences and the stand-in of k_pack_iupac is the scalar packer of qe_iupac.h, so a run
// under an IUPAC flag of an ASCII batch gives true answers here: they are compared with the strings
// tests/test_host_panel_cigar.py took from the fixture (file `cases` in the directory given; tests/panel_cigar_lib.py's format).
//
// Checked: every argument rule with nothing launched (the bit on quicked_batch_run_panel, with QUICKED_PANEL_MATRIX, sync == 0,
// check != 0, PREFIX in the scan), the two getters' rules around runs without the bit, other kinds of run and a reload; true
// strings for quicked_batch_run_panel_all (PREFIX, INFIX) and quicked_batch_run_panel_scan (windows 64 and 0) in styles 0, 1, 2
// at caps 1, 2 and 64, with the history's budget unset and 1 KiB (one wave per launch: kernel_times slot [1] counts them); the
// results of the run without the bit -- records, scores, statuses, counter [0] -- unchanged by the bit; counters [1] and [3].
#define PANEL_HOST_NAME "panel_cigar_host"
#include "panel_host_common.h"

struct Occ { int32_t pattern, start, end, score; std::string want[3]; };
struct Conf { int mode, flag, uniform; std::vector<std::vector<Occ>> want; };

struct Results {
    std::vector<int32_t> found, stored, sc, st;
    std::vector<int64_t> off;
    std::vector<quicked_panel_occ_t> occ;
    int64_t steps = 0;
    bool operator==(const Results& o) const {
        return found == o.found && stored == o.stored && sc == o.sc && st == o.st && off == o.off && steps == o.steps && occ.size() == o.occ.size() &&
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
    int64_t c[8];
    CHECK(quicked_batch_counters(b, c) >= 0);
    R.steps = c[0];
    return R;
}
static void strings_refused(quicked_batch_t* b) {
    int64_t o[4];
    char p[4];
    CHECK(quicked_batch_panel_hit_cigar_bytes(b) == -1);
    CHECK(quicked_batch_panel_hit_cigars(b, p, o) == QUICKED_ERROR);
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream f(std::string(argv[1]) + "/cases");
    int K = 0, n = 0, nconf = 0;
    f >> K >> n >> nconf;
    CHECK(!f.fail() && K >= 2 && n >= 4 && nconf >= 1);
    std::vector<std::string> panel((size_t)K), texts((size_t)n);
    std::vector<int32_t> own((size_t)K);
    for (int p = 0; p < K; ++p) f >> panel[(size_t)p] >> own[(size_t)p];
    for (int i = 0; i < n; ++i) { f >> texts[(size_t)i]; if (texts[(size_t)i] == ".") texts[(size_t)i].clear(); }
    std::vector<Conf> confs((size_t)nconf);
    for (Conf& cf : confs) {
        f >> cf.mode >> cf.flag >> cf.uniform;
        cf.want.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            int found = 0;
            f >> found;
            cf.want[(size_t)i].resize((size_t)found);
            for (Occ& o : cf.want[(size_t)i]) f >> o.pattern >> o.start >> o.end >> o.score >> o.want[0] >> o.want[1] >> o.want[2];
        }
        CHECK(!f.fail() && cf.flag != 0);
    }
    const Pool M = pool_of(panel), T = pool_of(texts);
    const std::vector<std::string> none_s((size_t)n);
    const Pool E = pool_of(none_s);
    quicked_batch_t* b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
    CHECK(b);
    const int INFIX = QUICKED_SEARCH_INFIX, PREFIX = QUICKED_SEARCH_PREFIX, IU = QUICKED_SEARCH_IUPAC, CG = QUICKED_PANEL_CIGARS;
    auto scan = [&](int mode, const int32_t* md, int32_t all, int32_t max_hits, int32_t window, int sync = 1) {
        return quicked_batch_run_panel_scan(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, max_hits, window, sync);
    };
    auto all_run = [&](int mode, const int32_t* md, int32_t all, int32_t max_hits, int sync = 1) {
        return quicked_batch_run_panel_all(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, max_hits, sync);
    };
    auto best_run = [&](int mode) { return quicked_batch_run_panel(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), own.data(), 0, 1); };
    strings_refused(b);
    // ---- a first flagged run, so that "nothing launched" has results, strings and counters to leave alone
    CHECK(all_run(INFIX | IU | CG, own.data(), 0, 16) == QUICKED_OK);
    const Results first = results_of(b, n);
    const std::vector<std::string> first_s = strings_of(b);
    int64_t c0[8], c1[8];
    CHECK(quicked_batch_counters(b, c0) >= 0 && c0[0] > 0 && c0[1] > 0 && c0[3] > 0 && !first_s.empty());
    // ---- QUICKED_ERROR, nothing launched
    CHECK(best_run(INFIX | CG) == QUICKED_ERROR);
    CHECK(best_run(INFIX | IU | CG) == QUICKED_ERROR);
    CHECK(best_run(INFIX | QUICKED_PANEL_MATRIX | CG) == QUICKED_ERROR);
    for (int fl : {0, IU, (int)QUICKED_SEARCH_IUPAC_PATTERN}) {
        CHECK(all_run(INFIX | fl | CG | QUICKED_PANEL_MATRIX, nullptr, 3, 16) == QUICKED_ERROR);
        CHECK(scan(INFIX | fl | CG | QUICKED_PANEL_MATRIX, nullptr, 3, 16, 64) == QUICKED_ERROR);
    }
    for (int other : {4, 8, 128, 256, 1024}) { CHECK(all_run(INFIX | CG | other, nullptr, 3, 16) == QUICKED_ERROR); CHECK(scan(INFIX | CG | other, nullptr, 3, 16, 64) == QUICKED_ERROR); }
    CHECK(all_run(CG, nullptr, 3, 16) == QUICKED_ERROR && all_run(INFIX | IU | QUICKED_SEARCH_IUPAC_PATTERN | CG, nullptr, 3, 16) == QUICKED_ERROR);
    CHECK(all_run(INFIX | CG, nullptr, -1, 16) == QUICKED_ERROR && all_run(INFIX | CG, nullptr, 3, 0) == QUICKED_ERROR && scan(INFIX | CG, nullptr, 3, 16, 63) == QUICKED_ERROR);
    // ---- QUICKED_UNIMPLEMENTED, nothing queued: every refusal of the two runs stands
    CHECK(all_run(INFIX | CG, nullptr, 3, 16, 0) == QUICKED_UNIMPLEMENTED && scan(INFIX | CG, nullptr, 3, 16, 64, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(scan(PREFIX | CG, nullptr, 3, 16, 64) == QUICKED_UNIMPLEMENTED);
    {
        const std::string big((size_t)QUICKED_PANEL_MAX_LEN + 1, 'A');
        const int64_t o2[2] = {0, 0};
        int32_t len[2] = {4, QUICKED_PANEL_MAX_LEN + 1};
        CHECK(quicked_batch_run_panel_all(b, INFIX | CG, 2, big.data(), o2, len, nullptr, 3, 16, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
        CHECK(all_run(INFIX | CG, nullptr, 3, 16) == QUICKED_UNIMPLEMENTED && scan(INFIX | CG, nullptr, 3, 16, 64) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    }
    CHECK(quicked_batch_counters(b, c1) >= 0 && !memcmp(c0, c1, sizeof(c0)));
    CHECK(results_of(b, n) == first && strings_of(b) == first_s);
    // ---- true strings: both runs, both flags, every style and cap, the history's budget unset and one wave
    long checked = 0;
    for (const char* ws_kb : {(const char*)nullptr, "1"}) {
        set_env("QE_PANEL_ALIGN_WS_KB", ws_kb);
        for (const Conf& cf : confs)
            for (int style = 0; style < 3; ++style)
                for (int32_t cap : {1, 2, 64}) {
                    if (ws_kb && (style == 1 || cap == 2)) continue;
                    CHECK(quicked_batch_configure(b, style, 0) == QUICKED_OK);
                    const int32_t* md = cf.uniform < 0 ? own.data() : nullptr;
                    const int32_t all = cf.uniform < 0 ? 0 : cf.uniform;
                    for (int window : {-1, 64, 0}) {                  // -1: quicked_batch_run_panel_all
                        if (window >= 0 && (cf.mode != INFIX || (ws_kb && window == 0))) continue;
                        double ms[4]; int64_t launches[4];
                        CHECK(quicked_batch_kernel_times(b, ms, launches) >= 0);      // (since the last call)
                        // the run without the bit, then the run with it: everything the first leaves is left unchanged
                        CHECK((window < 0 ? all_run(cf.mode | cf.flag, md, all, cap) : scan(cf.mode | cf.flag, md, all, cap, window)) == QUICKED_OK);
                        const Results plain = results_of(b, n);
                        strings_refused(b);
                        CHECK(quicked_batch_counters(b, c1) >= 0 && c1[1] == 0 && c1[3] == 0);
                        CHECK(quicked_batch_kernel_times(b, ms, launches) >= 0 && launches[1] == 0);
                        CHECK(quicked_batch_configure_tags(b, QUICKED_TAG_STATS | QUICKED_TAG_MD) == QUICKED_OK);      // ignored
                        CHECK((window < 0 ? all_run(cf.mode | cf.flag | CG, md, all, cap) : scan(cf.mode | cf.flag | CG, md, all, cap, window)) == QUICKED_OK);
                        CHECK(quicked_batch_configure_tags(b, 0) == QUICKED_OK);
                        const Results R = results_of(b, n);
                        CHECK(R == plain);
                        const std::vector<std::string> got = strings_of(b);
                        CHECK((int64_t)got.size() == R.off[(size_t)n]);
                        int64_t ops = 0, steps = 0;
                        for (int i = 0; i < n; ++i) {
                            const std::vector<Occ>& w = cf.want[(size_t)i];
                            const int32_t keep = (int32_t)std::min<size_t>(w.size(), (size_t)cap);
                            CHECK(R.stored[(size_t)i] == keep);
                            for (int k = 0; k < keep; ++k) {
                                const quicked_panel_occ_t h = R.occ[(size_t)(R.off[(size_t)i] + k)];
                                const Occ& o = w[(size_t)k];
                                CHECK(h.pattern == o.pattern && h.text_start == o.start && h.text_end == o.end && h.score == o.score);
                                const std::string& s = got[(size_t)(R.off[(size_t)i] + k)];
                                if (s != o.want[style])
                                    fprintf(stderr, "mode %d flag %d uniform %d style %d cap %d window %d text %d occurrence %d: got %s, expected %s\n", cf.mode, cf.flag,
                                            cf.uniform, style, cap, window, i, k, s.c_str(), o.want[style].c_str());
                                CHECK(s == o.want[style]);
                                for (size_t q = 0, run = 0; q < o.want[0].size(); ++q) {
                                    const char ch = o.want[0][q];
                                    if (ch >= '0' && ch <= '9') run = 10 * run + (size_t)(ch - '0'); else { ops += (int64_t)run; run = 0; }
                                }
                                steps += (int64_t)((panel[(size_t)o.pattern].size() + 63) / 64) * (o.end - o.start);
                                ++checked;
                            }
                        }
                        CHECK(quicked_batch_counters(b, c1) >= 0 && c1[0] == plain.steps && c1[1] == steps && c1[3] == ops);
                        CHECK(quicked_batch_kernel_times(b, ms, launches) >= 0);
                        const int64_t total = R.off[(size_t)n];
                        CHECK(launches[1] == (total == 0 ? 0 : (ws_kb ? (total + 63) / 64 : 1)));
                        // the other getters: what they return after any run that produced none of their data
                        std::vector<int64_t> coff((size_t)n);
                        CHECK(quicked_batch_cigar_bytes(b) == 0 && quicked_batch_hit_total(b) == -1);
                        CHECK(quicked_batch_cigars(b, nullptr, coff.data()) >= 0);
                        for (int i = 0; i < n; ++i) CHECK(coff[(size_t)i] == -1);
                        quicked_pair_stats_t ps;
                        CHECK(quicked_batch_pair_stats(b, &ps) == QUICKED_ERROR);
                    }
                }
    }
    set_env("QE_PANEL_ALIGN_WS_KB", nullptr);
    CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    CHECK(checked > 1000);
    // ---- other kinds of run in turn, and a reload: the strings are the last flagged run's only
    CHECK(all_run(INFIX | IU | CG, own.data(), 0, 16) == QUICKED_OK && strings_of(b) == first_s);
    CHECK(best_run(INFIX | IU) == QUICKED_OK);
    strings_refused(b);
    CHECK(scan(INFIX | IU | CG, own.data(), 0, 16, 64) == QUICKED_OK && strings_of(b) == first_s);
    CHECK(quicked_batch_run_search_all(b, INFIX, nullptr, 3, 4, 1) >= QUICKED_EMPTY_SEQUENCE);
    strings_refused(b);
    CHECK(all_run(INFIX | IU | CG, own.data(), 0, 16) == QUICKED_OK && strings_of(b) == first_s);
    CHECK(all_run(INFIX | IU, own.data(), 0, 16) == QUICKED_OK);
    strings_refused(b);
    CHECK(all_run(INFIX | IU | CG, own.data(), 0, 16) == QUICKED_OK);
    {
        const int n2 = n / 2;
        std::vector<std::string> pats((size_t)n2), txts(texts.begin(), texts.begin() + n2);
        const Pool P2 = pool_of(pats), T2 = pool_of(txts);
        CHECK(quicked_batch_reload(b, n2, P2.bytes.data(), P2.off.data(), P2.len.data(), T2.bytes.data(), T2.off.data(), T2.len.data()) >= 0);
        strings_refused(b);
        CHECK(all_run(INFIX | IU | CG, own.data(), 0, 16) == QUICKED_OK);
        const std::vector<std::string> s2 = strings_of(b);
        CHECK(!s2.empty() && s2.size() <= first_s.size() && std::equal(s2.begin(), s2.end(), first_s.begin()));
    }
    // ---- a batch without a stored occurrence: the getters answer, with nothing
    {
        const int64_t zero = 0;
        const int32_t none = 0, four = 4, one = 1;
        quicked_batch_t* q = quicked_batch_create(1, "", &zero, &none, "CCCC", &zero, &four);
        CHECK(q);
        CHECK(quicked_batch_run_panel_all(q, INFIX | IU | CG, 1, "G", &zero, &one, nullptr, 0, 4, 1) == QUICKED_OK);
        CHECK(quicked_batch_panel_hit_total(q) == 0 && quicked_batch_panel_hit_cigar_bytes(q) == 0 && quicked_batch_panel_hit_cigars(q, nullptr, nullptr) == QUICKED_OK);
        quicked_batch_destroy(q);
    }
    quicked_batch_destroy(b);
    printf("panel_cigar_host ok %ld\n", checked);
    return 0;
}
