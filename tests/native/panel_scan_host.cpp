// Windowed panel runs (quicked_batch_run_panel_scan) on the HOST, under sanitizers: the library's host layer built with g++
// against the fake HIP runtime of tests/native/hip_stub.  The stand-ins of k_panel_scan / k_panel_scan_count /
// k_panel_scan_expand (hip_stub/qe_kernels_stub.h) are the device kernels' own source (qe_panel.h) run lane by lane, the
// stand-in of k_search<4, Eq> runs the real recurrence and the stand-in of k_pack_iupac is the scalar packer of qe_iupac.h, so
// a FLAGGED run of an ASCII batch gives true answers here: they are compared with the lists tests/test_host_panel_scan.py took
// from the fixture (file `cases` in the directory given; tests/panel_hits_lib.py's format) and with quicked_batch_run_panel_all
// on the same batch.  An unflagged run reads planes the stub's k_pack never wrote: only its statuses and shapes are checked.
// Checked: every QUICKED_ERROR and QUICKED_UNIMPLEMENTED rule with nothing launched -- the window's, PREFIX, the 2^26 rule with
// a forced window, and window == 0 accepted where a forced one is refused --, the getters' rules around other kinds of run,
// results cleared by a reload, QE_PANEL_SLICES = 1, 2 and a huge value, a 1 KiB QE_PANEL_HITS_RAW_KB, windows of 64, 128 and
// the library's.
// A stand-alone program: nothing is loaded into Python.
#define PANEL_HOST_NAME "panel_scan_host"
#include "panel_host_common.h"

struct Occ { int32_t pattern, start, end, score; };
struct Conf { int mode, flag, uniform; std::vector<std::vector<Occ>> want; };

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
    CHECK(quicked_batch_panel_hit_counts(b, nullptr, nullptr) == QUICKED_OK);
    const int64_t total = quicked_batch_panel_hit_total(b);
    CHECK(total >= 0);
    R.occ.assign((size_t)total + 1, quicked_panel_occ_t{-7, -7, -7, -7});
    CHECK(quicked_batch_panel_hits(b, R.occ.data(), R.off.data()) == QUICKED_OK);
    CHECK(R.off[0] == 0 && R.off[(size_t)n] == total && R.occ[(size_t)total].pattern == -7);
    R.occ.resize((size_t)total);
    CHECK(quicked_batch_scores(b, R.sc.data(), R.st.data()) >= 0);
    return R;
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
            for (Occ& o : cf.want[(size_t)i]) f >> o.pattern >> o.start >> o.end >> o.score;
        }
        CHECK(!f.fail() && cf.mode == QUICKED_SEARCH_INFIX);
    }
    const Pool M = pool_of(panel), T = pool_of(texts);
    const std::vector<std::string> none_s((size_t)n);              // the batch's own patterns: all empty
    const Pool E = pool_of(none_s);
    quicked_batch_t* b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
    CHECK(b);
    std::vector<int32_t> loc((size_t)n);
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<quicked_panel_hit_t> ph((size_t)n);
    const int INFIX = QUICKED_SEARCH_INFIX, PREFIX = QUICKED_SEARCH_PREFIX;
    auto scan = [&](int mode, const int32_t* md, int32_t all, int32_t max_hits, int32_t window) {
        return quicked_batch_run_panel_scan(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, max_hits, window, 1);
    };
    auto all_run = [&](int mode, const int32_t* md, int32_t all, int32_t max_hits) {
        return quicked_batch_run_panel_all(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, max_hits, 1);
    };
    auto getters_refuse = [&](quicked_batch_t* q) {
        CHECK(quicked_batch_panel_hit_counts(q, loc.data(), loc.data()) == QUICKED_ERROR);
        CHECK(quicked_batch_panel_hit_total(q) == -1);
        CHECK(quicked_batch_panel_hits(q, nullptr, off.data()) == QUICKED_ERROR);
    };
    getters_refuse(b);
    // ---- a first run, so that "nothing launched" has counters and results to leave alone
    CHECK(scan(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16, 64) == QUICKED_OK);
    const int64_t steps0 = steps_of(b), total0 = quicked_batch_panel_hit_total(b);
    CHECK(steps0 > 0 && total0 > 0);
    // ---- QUICKED_ERROR, nothing launched: run_panel_all's rules ...
    CHECK(quicked_batch_run_panel_scan(nullptr, INFIX, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 16, 64, 1) == QUICKED_ERROR);
    for (int mode : {0, 3, 4, 16, 64, 64 | 2, 64 | 16 | 2, 16 | 32 | 2, 128 | 2, 256 | 1, 8 | 2, -1}) CHECK(scan(mode, nullptr, 3, 16, 64) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel_scan(b, INFIX, 0, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 16, 64, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel_scan(b, INFIX, -5, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 16, 64, 1) == QUICKED_ERROR);
    {
        std::vector<int64_t> moff((size_t)QUICKED_PANEL_MAX_PATTERNS + 1, 0);
        std::vector<int32_t> mlen((size_t)QUICKED_PANEL_MAX_PATTERNS + 1, 1);
        CHECK(quicked_batch_run_panel_scan(b, INFIX, QUICKED_PANEL_MAX_PATTERNS + 1, M.bytes.data(), moff.data(), mlen.data(), nullptr, 3, 16, 64, 1) == QUICKED_ERROR);
        std::vector<int32_t> len = M.len;
        len[1] = 0;                                               // a member of length 0 -- even next to one that is too long
        CHECK(quicked_batch_run_panel_scan(b, INFIX, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 3, 16, 64, 1) == QUICKED_ERROR);
        len[0] = QUICKED_PANEL_MAX_LEN + 1;
        CHECK(quicked_batch_run_panel_scan(b, INFIX, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 3, 16, 64, 1) == QUICKED_ERROR);
        std::vector<int32_t> bad = own;
        bad[(size_t)K - 1] = -1;                                  // a negative bound
        CHECK(scan(INFIX, bad.data(), 3, 16, 64) == QUICKED_ERROR);
        CHECK(scan(INFIX, nullptr, -1, 16, 64) == QUICKED_ERROR);
    }
    for (int32_t mh : {0, -1, 4097, INT_MAX}) CHECK(scan(INFIX, nullptr, 3, mh, 64) == QUICKED_ERROR);
    // ... and the window's: a multiple of 64 that is at least 64, or 0 -- for PREFIX too: an error comes before "not built"
    for (int32_t w : {-64, -1, 1, 63, 65, 96, 100, 4095, INT_MAX, INT_MIN}) {
        CHECK(scan(INFIX, nullptr, 3, 16, w) == QUICKED_ERROR);
        CHECK(scan(PREFIX, nullptr, 3, 16, w) == QUICKED_ERROR);
    }
    // ---- the room for the stored occurrences.  One text of 16 385 x 64 bases: at a forced window of 64 it has 16 385 window
    // slots, one too many for max_hits 4096; at 128 it fits; the library's own window fits by construction.  The rule comes
    // before the QUICKED_UNIMPLEMENTED ones, so a queued run (sync == 0) tells which of the two refused, and nothing runs
    {
        const int64_t zero = 0;
        const int32_t one = 1, big_n = 16385 * 64;
        const std::string big_text((size_t)big_n, 'A');
        const int32_t none = 0;
        quicked_batch_t* q = quicked_batch_create(1, "", &zero, &none, big_text.data(), &zero, &big_n);
        CHECK(q);
        auto one_scan = [&](int32_t mh, int32_t w, int sync) { return quicked_batch_run_panel_scan(q, INFIX, 1, "C", &zero, &one, nullptr, 0, mh, w, sync); };
        int64_t c0[8], c1[8];
        CHECK(quicked_batch_counters(q, c0) >= 0);
        CHECK(one_scan(4096, 64, 1) == QUICKED_ERROR);
        CHECK(one_scan(4096, 64, 0) == QUICKED_ERROR);
        CHECK(one_scan(4095, 64, 0) == QUICKED_UNIMPLEMENTED);                              // within the room: not this rule
        CHECK(one_scan(4096, 128, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(one_scan(4096, 0, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_counters(q, c1) >= 0 && !memcmp(c0, c1, sizeof(c0)));
        getters_refuse(q);
        quicked_batch_destroy(q);
        // (non-empty texts) x max_hits above 2^26: no window helps, window == 0 included
        std::vector<int64_t> o((size_t)16385, 0);
        std::vector<int32_t> tl((size_t)16385, 1), pl((size_t)16385, 0);
        quicked_batch_t* over = quicked_batch_create(16385, "A", o.data(), pl.data(), "A", o.data(), tl.data());
        CHECK(over);
        for (int32_t w : {0, 64, 4096}) CHECK(quicked_batch_run_panel_scan(over, INFIX, 1, "A", &zero, &one, nullptr, 0, 4096, w, 0) == QUICKED_ERROR);
        CHECK(quicked_batch_run_panel_scan(over, INFIX, 1, "A", &zero, &one, nullptr, 0, 4095, 0, 0) == QUICKED_UNIMPLEMENTED);
        quicked_batch_destroy(over);
    }
    // ---- QUICKED_UNIMPLEMENTED, nothing queued
    {
        const std::string big((size_t)QUICKED_PANEL_MAX_LEN + 1, 'A');
        const int64_t o2[2] = {0, 0};
        int32_t len[2] = {4, QUICKED_PANEL_MAX_LEN + 1};
        CHECK(quicked_batch_run_panel_scan(b, INFIX, 2, big.data(), o2, len, nullptr, 3, 16, 64, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_panel_scan(b, INFIX, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 16, 64, 0) == QUICKED_UNIMPLEMENTED);
        for (int32_t w : {0, 64, 4096})
            for (int fl : {0, (int)QUICKED_SEARCH_IUPAC, (int)QUICKED_SEARCH_IUPAC_PATTERN}) CHECK(scan(PREFIX | fl, nullptr, 3, 16, w) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
        CHECK(scan(INFIX, nullptr, 3, 16, 64) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    }
    // none of it ran: the results and the counters are the first run's
    CHECK(steps_of(b) == steps0 && quicked_batch_panel_hit_total(b) == total0);
    // ---- true answers under the two flags: the fixture's lists and run_panel_all's results on the same batch, with the slices
    // forced and chosen, the raw buffer's budget 1 KiB (the slice count is lowered to one), windows of 64, 128 and the library's
    struct Shape { const char* slices; const char* raw_kb; };
    for (const Shape sh : {Shape{nullptr, nullptr}, Shape{"1", nullptr}, Shape{"2", nullptr}, Shape{"1000000000000", nullptr}, Shape{"1000000000000", "1"}, Shape{nullptr, "1"}}) {
        set_env("QE_PANEL_SLICES", sh.slices);
        set_env("QE_PANEL_HITS_RAW_KB", sh.raw_kb);
        for (const Conf& cf : confs) {
            if (!cf.flag) continue;
            for (int32_t cap : {1, 2, 64}) {
                if (sh.slices && cap == 2) continue;              // (every cap with the host's own choice, two of them under the forced ones)
                const int32_t* md = cf.uniform < 0 ? own.data() : nullptr;
                const int32_t all = cf.uniform < 0 ? 0 : cf.uniform;
                CHECK(all_run(cf.mode | cf.flag, md, all, cap) == QUICKED_OK);
                const Results A = results_of(b, n);
                const int64_t steps_all = steps_of(b);
                for (int32_t window : {64, 128, 0}) {
                    if (sh.slices && window == 128) continue;
                    CHECK(quicked_batch_configure_tags(b, QUICKED_TAG_STATS) == QUICKED_OK);      // ignored: no alignments
                    CHECK(scan(cf.mode | cf.flag, md, all, cap, window) == QUICKED_OK);
                    CHECK(quicked_batch_configure_tags(b, 0) == QUICKED_OK);
                    const Results R = results_of(b, n);
                    CHECK(R == A);
                    CHECK(steps_of(b) > 0 && (window != 64 || steps_of(b) > steps_all));          // warm-up columns are counted
                    for (int i = 0; i < n; ++i) {
                        const std::vector<Occ>& w = cf.want[(size_t)i];
                        const int32_t keep = (int32_t)std::min<size_t>(w.size(), (size_t)cap);
                        int32_t best = -1;
                        for (const Occ& o : w) best = (best < 0 || o.score < best) ? o.score : best;
                        if (R.found[(size_t)i] != (int32_t)w.size() || R.stored[(size_t)i] != keep)
                            fprintf(stderr, "flag %d uniform %d cap %d window %d text %d: found %d stored %d, expected %zu %d\n", cf.flag, cf.uniform, cap, window, i,
                                    R.found[(size_t)i], R.stored[(size_t)i], w.size(), keep);
                        CHECK(R.found[(size_t)i] == (int32_t)w.size() && R.stored[(size_t)i] == keep && R.off[(size_t)i + 1] - R.off[(size_t)i] == keep);
                        CHECK(R.sc[(size_t)i] == best);
                        CHECK(R.st[(size_t)i] == (texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
                        for (int k = 0; k < keep; ++k) {
                            const quicked_panel_occ_t h = R.occ[(size_t)(R.off[(size_t)i] + k)];
                            const Occ& o = w[(size_t)k];
                            if (h.pattern != o.pattern || h.text_start != o.start || h.text_end != o.end || h.score != o.score)
                                fprintf(stderr, "flag %d uniform %d cap %d window %d text %d occurrence %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n", cf.flag,
                                        cf.uniform, cap, window, i, k, h.pattern, h.text_start, h.text_end, h.score, o.pattern, o.start, o.end, o.score);
                            CHECK(h.pattern == o.pattern && h.text_start == o.start && h.text_end == o.end && h.score == o.score);
                        }
                    }
                    // the other getters: what they return after any run that produced none of their data
                    CHECK(quicked_batch_panel_results(b, ph.data()) == QUICKED_ERROR);
                    CHECK(quicked_batch_panel_matrix(b, loc.data(), loc.data()) == QUICKED_ERROR);
                    CHECK(quicked_batch_locations(b, loc.data(), loc.data()) == QUICKED_ERROR);
                    CHECK(quicked_batch_hit_total(b) == -1);
                    CHECK(quicked_batch_hit_counts(b, loc.data(), loc.data()) == QUICKED_ERROR);
                    CHECK(quicked_batch_hits(b, nullptr, off.data()) == QUICKED_ERROR);
                    CHECK(quicked_batch_cigar_bytes(b) == 0);
                    quicked_pair_stats_t ps;
                    CHECK(quicked_batch_pair_stats(b, &ps) == QUICKED_ERROR);
                }
            }
        }
    }
    set_env("QE_PANEL_SLICES", nullptr);
    set_env("QE_PANEL_HITS_RAW_KB", nullptr);
    // ---- an unflagged run: statuses and shapes (the stub's k_pack writes no planes)
    for (int32_t window : {64, 0}) {
        CHECK(scan(INFIX, nullptr, 3, 4, window) == QUICKED_OK);
        const Results R = results_of(b, n);
        for (int i = 0; i < n; ++i) {
            CHECK(R.st[(size_t)i] == (texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
            CHECK(R.stored[(size_t)i] == std::min(R.found[(size_t)i], 4) && R.off[(size_t)i + 1] - R.off[(size_t)i] == R.stored[(size_t)i]);
            CHECK((R.found[(size_t)i] == 0) == (R.sc[(size_t)i] == -1) && (!texts[(size_t)i].empty() || R.found[(size_t)i] == 0));
            for (int64_t j = R.off[(size_t)i]; j < R.off[(size_t)i + 1]; ++j) {
                const quicked_panel_occ_t h = R.occ[(size_t)j];
                CHECK(h.pattern >= 0 && h.pattern < K && h.score >= 0 && h.score <= 3 && h.text_end >= 1 && h.text_end <= (int32_t)texts[(size_t)i].size());
                CHECK(h.text_start >= -1 && h.text_start <= h.text_end);
                if (j > R.off[(size_t)i]) CHECK(R.occ[(size_t)j - 1].pattern < h.pattern || (R.occ[(size_t)j - 1].pattern == h.pattern && R.occ[(size_t)j - 1].text_end < h.text_end));
            }
        }
    }
    // ---- other kinds of run in turn: each getter family reports its own run only, and a scan run is a run_panel_all's kind
    CHECK(quicked_batch_run_panel(b, INFIX | QUICKED_SEARCH_IUPAC | QUICKED_PANEL_MATRIX, K, M.bytes.data(), M.off.data(), M.len.data(), own.data(), 0, 1) == QUICKED_OK);
    getters_refuse(b);
    CHECK(quicked_batch_panel_results(b, ph.data()) == QUICKED_OK);
    CHECK(scan(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16, 64) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(b) == total0);
    CHECK(quicked_batch_panel_results(b, ph.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search(b, INFIX, nullptr, 3, 1, 1) >= QUICKED_EMPTY_SEQUENCE);      // (the batch's patterns are all empty)
    getters_refuse(b);
    CHECK(all_run(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(b) == total0);
    CHECK(quicked_batch_run_search_all(b, INFIX, nullptr, 3, 4, 1) >= QUICKED_EMPTY_SEQUENCE);
    getters_refuse(b);
    CHECK(scan(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16, 0) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(b) == total0);
    {
        quicked_params_t p = quicked_default_params();
        p.algo = BANDED; p.only_score = true;
        (void)quicked_batch_run(b, &p, 1);
        getters_refuse(b);
    }
    // ---- results cleared by a reload: fewer pairs, real patterns that play no part
    CHECK(scan(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16, 128) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(b) == total0);
    {
        const int n2 = n / 2;
        std::vector<std::string> pats((size_t)n2), txts(texts.begin(), texts.begin() + n2);
        for (int i = 0; i < n2; ++i) pats[(size_t)i] = panel[(size_t)(i % K)];
        const Pool P2 = pool_of(pats), T2 = pool_of(txts);
        CHECK(quicked_batch_reload(b, n2, P2.bytes.data(), P2.off.data(), P2.len.data(), T2.bytes.data(), T2.off.data(), T2.len.data()) >= 0);
        getters_refuse(b);
        const Conf* cf = nullptr;
        for (const Conf& c : confs) if (c.flag == QUICKED_SEARCH_IUPAC && c.uniform < 0) cf = &c;
        CHECK(cf);
        CHECK(scan(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 4096, 64) == QUICKED_OK);
        const Results R = results_of(b, n2);
        for (int i = 0; i < n2; ++i) {
            const std::vector<Occ>& w = cf->want[(size_t)i];
            CHECK(R.found[(size_t)i] == (int32_t)w.size() && R.stored[(size_t)i] == R.found[(size_t)i]);
            for (size_t k = 0; k < w.size(); ++k) {
                const quicked_panel_occ_t h = R.occ[(size_t)R.off[(size_t)i] + k];
                CHECK(h.pattern == w[k].pattern && h.text_start == w[k].start && h.text_end == w[k].end && h.score == w[k].score);
            }
        }
    }
    quicked_batch_destroy(b);
    printf("panel_scan_host ok\n");
    return 0;
}
