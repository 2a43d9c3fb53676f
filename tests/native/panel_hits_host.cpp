// All-occurrences panel runs (quicked_batch_run_panel_all) on the HOST, under sanitizers: the library's host layer built with g++
// against the fake HIP runtime of tests/native/hip_stub.  The stand-ins of k_panel_hits / k_panel_hits_count /
// k_panel_hits_expand / k_panel_hits_finish (hip_stub/qe_kernels_stub.h) are the device kernels' own source (qe_panel.h) run slot by slot,
// the stand-in of k_search<4, Eq> runs the real recurrence and the stand-in of k_pack_iupac is the scalar packer of qe_iupac.h,
// so a FLAGGED run of an ASCII batch gives true answers here: they are compared with the lists tests/test_host_panel_hits.py
// computed with tests/panel_hits_lib.py (file `cases` in the directory given; the format of tests/native/panel_hits_cpu.cpp).
// An unflagged run reads planes the stub's k_pack never wrote: only its statuses and the shape of its results are checked.
// Checked: every QUICKED_ERROR and QUICKED_UNIMPLEMENTED rule with nothing launched, the getters' rules before and after each
// other kind of run, results cleared by a reload, QE_PANEL_SLICES = 1, 2 and a huge value, a tiny QE_PANEL_HITS_RAW_KB.
// A stand-alone program: nothing is loaded into Python.
#define PANEL_HOST_NAME "panel_hits_host"
#include "panel_host_common.h"

struct Occ { int32_t pattern, start, end, score; };
struct Conf { int mode, flag, uniform; std::vector<std::vector<Occ>> want; };

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
        CHECK(!f.fail());
    }
    const Pool M = pool_of(panel), T = pool_of(texts);
    const std::vector<std::string> none_s((size_t)n);              // the batch's own patterns: all empty
    const Pool E = pool_of(none_s);
    quicked_batch_t* b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
    CHECK(b);
    std::vector<int32_t> found((size_t)n), stored((size_t)n), sc((size_t)n), st((size_t)n), loc((size_t)n);
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<quicked_panel_occ_t> occ;
    std::vector<quicked_panel_hit_t> ph((size_t)n);
    const int INFIX = QUICKED_SEARCH_INFIX, PREFIX = QUICKED_SEARCH_PREFIX;
    auto run = [&](int mode, const int32_t* md, int32_t all, int32_t max_hits) {
        return quicked_batch_run_panel_all(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, max_hits, 1);
    };
    auto getters_refuse = [&](quicked_batch_t* q) {
        CHECK(quicked_batch_panel_hit_counts(q, found.data(), stored.data()) == QUICKED_ERROR);
        CHECK(quicked_batch_panel_hit_total(q) == -1);
        CHECK(quicked_batch_panel_hits(q, nullptr, off.data()) == QUICKED_ERROR);
    };
    // ---- before any run: the getters refuse
    getters_refuse(b);
    getters_refuse(nullptr);
    // ---- a first run, so that "nothing launched" has counters and results to leave alone
    CHECK(run(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16) == QUICKED_OK);
    const int64_t steps0 = steps_of(b), total0 = quicked_batch_panel_hit_total(b);
    CHECK(steps0 > 0 && total0 > 0);
    // ---- QUICKED_ERROR, nothing launched
    CHECK(quicked_batch_run_panel_all(nullptr, INFIX, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 16, 1) == QUICKED_ERROR);
    for (int mode : {0, 3, 4, 16, 64, 64 | 2, 64 | 16 | 2, 16 | 32 | 2, 128 | 2, 256 | 1, 8 | 2, -1}) CHECK(run(mode, nullptr, 3, 16) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel_all(b, INFIX, 0, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 16, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel_all(b, INFIX, -5, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 16, 1) == QUICKED_ERROR);
    {
        std::vector<int64_t> moff((size_t)QUICKED_PANEL_MAX_PATTERNS + 1, 0);
        std::vector<int32_t> mlen((size_t)QUICKED_PANEL_MAX_PATTERNS + 1, 1);
        CHECK(quicked_batch_run_panel_all(b, INFIX, QUICKED_PANEL_MAX_PATTERNS + 1, M.bytes.data(), moff.data(), mlen.data(), nullptr, 3, 16, 1) == QUICKED_ERROR);
    }
    {
        std::vector<int32_t> len = M.len;
        len[1] = 0;                                               // a member of length 0 -- even next to one that is too long
        CHECK(quicked_batch_run_panel_all(b, INFIX, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 3, 16, 1) == QUICKED_ERROR);
        len[0] = QUICKED_PANEL_MAX_LEN + 1;
        CHECK(quicked_batch_run_panel_all(b, INFIX, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 3, 16, 1) == QUICKED_ERROR);
        std::vector<int32_t> bad = own;
        bad[(size_t)K - 1] = -1;                                  // a negative bound
        CHECK(run(INFIX, bad.data(), 3, 16) == QUICKED_ERROR);
        CHECK(run(INFIX, nullptr, -1, 16) == QUICKED_ERROR);
    }
    for (int32_t mh : {0, -1, 4097, INT_MAX}) CHECK(run(INFIX, nullptr, 3, mh) == QUICKED_ERROR);
    // ---- (non-empty texts) x max_hits above 2^26: 16 385 texts x 4096; empty texts do not count.  The rule comes before the
    // QUICKED_UNIMPLEMENTED ones, so a queued run (sync == 0) tells which of the two refused, and nothing runs
    {
        auto batch_of_ones = [&](int64_t count, int64_t empty) {
            std::vector<int64_t> o((size_t)count, 0);
            std::vector<int32_t> tl((size_t)count, 1), pl((size_t)count, 0);
            for (int64_t i = count - empty; i < count; ++i) tl[(size_t)i] = 0;
            quicked_batch_t* q = quicked_batch_create(count, "A", o.data(), pl.data(), "A", o.data(), tl.data());
            CHECK(q);
            return q;
        };
        const int64_t zero = 0;
        const int32_t one = 1;
        auto all_run = [&](quicked_batch_t* q, int32_t mh, int sync) { return quicked_batch_run_panel_all(q, INFIX, 1, "A", &zero, &one, nullptr, 0, mh, sync); };
        quicked_batch_t* over = batch_of_ones(16385, 0);
        int64_t c0[8], c1[8];
        CHECK(quicked_batch_counters(over, c0) >= 0);
        CHECK(all_run(over, 4096, 1) == QUICKED_ERROR);
        CHECK(all_run(over, 4096, 0) == QUICKED_ERROR);
        CHECK(all_run(over, 4095, 0) == QUICKED_UNIMPLEMENTED);                             // within the room: not this rule
        CHECK(quicked_batch_counters(over, c1) >= 0 && !memcmp(c0, c1, sizeof(c0)));
        getters_refuse(over);
        quicked_batch_destroy(over);
        quicked_batch_t* holes = batch_of_ones(16385, 1);                                   // one of them empty: exactly 2^26
        CHECK(all_run(holes, 4096, 0) == QUICKED_UNIMPLEMENTED);
        quicked_batch_destroy(holes);
    }
    // ---- QUICKED_UNIMPLEMENTED, nothing queued
    {
        const std::string big((size_t)QUICKED_PANEL_MAX_LEN + 1, 'A');
        const int64_t o2[2] = {0, 0};
        int32_t len[2] = {4, QUICKED_PANEL_MAX_LEN + 1};
        CHECK(quicked_batch_run_panel_all(b, INFIX, 2, big.data(), o2, len, nullptr, 3, 16, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_panel_all(b, INFIX, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 16, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
        CHECK(run(INFIX, nullptr, 3, 16) == QUICKED_UNIMPLEMENTED);
        CHECK(run(PREFIX | QUICKED_SEARCH_IUPAC_PATTERN, nullptr, 3, 16) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    }
    // none of it ran: the results and the counters are the first run's
    CHECK(steps_of(b) == steps0 && quicked_batch_panel_hit_total(b) == total0);
    // ---- true answers under the two flags, every configuration and cap, with the slices forced and chosen and the raw
    // buffer's budget tiny (one slice's worth at the most: the count is lowered to one)
    struct Shape { const char* slices; const char* raw_kb; };
    for (const Shape sh : {Shape{nullptr, nullptr}, Shape{"1", nullptr}, Shape{"2", nullptr}, Shape{"1000000000000", nullptr}, Shape{"1000000000000", "1"}, Shape{nullptr, "1"}}) {
        set_env("QE_PANEL_SLICES", sh.slices);
        set_env("QE_PANEL_HITS_RAW_KB", sh.raw_kb);
        for (const Conf& cf : confs) {
            if (!cf.flag) continue;
            for (int32_t cap : {1, 2, 64}) {
                if (sh.slices && cap == 2) continue;              // (every cap with the host's own choice, two of them under the forced ones)
                CHECK(quicked_batch_configure_tags(b, QUICKED_TAG_STATS) == QUICKED_OK);      // ignored: no alignments
                CHECK(run(cf.mode | cf.flag, cf.uniform < 0 ? own.data() : nullptr, cf.uniform < 0 ? 0 : cf.uniform, cap) == QUICKED_OK);
                CHECK(quicked_batch_configure_tags(b, 0) == QUICKED_OK);
                CHECK(quicked_batch_panel_hit_counts(b, found.data(), stored.data()) == QUICKED_OK);
                CHECK(quicked_batch_panel_hit_counts(b, nullptr, nullptr) == QUICKED_OK);
                const int64_t total = quicked_batch_panel_hit_total(b);
                CHECK(total >= 0);
                occ.assign((size_t)total + 1, quicked_panel_occ_t{-7, -7, -7, -7});
                CHECK(quicked_batch_panel_hits(b, occ.data(), off.data()) == QUICKED_OK);
                CHECK(off[0] == 0 && off[(size_t)n] == total && occ[(size_t)total].pattern == -7);
                CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
                CHECK(steps_of(b) > 0);
                for (int i = 0; i < n; ++i) {
                    const std::vector<Occ>& w = cf.want[(size_t)i];
                    const int32_t keep = (int32_t)std::min<size_t>(w.size(), (size_t)cap);
                    int32_t best = -1;
                    for (const Occ& o : w) best = (best < 0 || o.score < best) ? o.score : best;
                    if (found[(size_t)i] != (int32_t)w.size() || stored[(size_t)i] != keep)
                        fprintf(stderr, "mode %d flag %d uniform %d cap %d text %d: found %d stored %d, expected %zu %d\n", cf.mode, cf.flag, cf.uniform, cap, i,
                                found[(size_t)i], stored[(size_t)i], w.size(), keep);
                    CHECK(found[(size_t)i] == (int32_t)w.size() && stored[(size_t)i] == keep && off[(size_t)i + 1] - off[(size_t)i] == keep);
                    CHECK(sc[(size_t)i] == best);
                    CHECK(st[(size_t)i] == (texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
                    for (int k = 0; k < keep; ++k) {
                        const quicked_panel_occ_t h = occ[(size_t)(off[(size_t)i] + k)];
                        const Occ& o = w[(size_t)k];
                        if (h.pattern != o.pattern || h.text_start != o.start || h.text_end != o.end || h.score != o.score)
                            fprintf(stderr, "mode %d flag %d uniform %d cap %d text %d occurrence %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n", cf.mode, cf.flag,
                                    cf.uniform, cap, i, k, h.pattern, h.text_start, h.text_end, h.score, o.pattern, o.start, o.end, o.score);
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
    set_env("QE_PANEL_SLICES", nullptr);
    set_env("QE_PANEL_HITS_RAW_KB", nullptr);
    // ---- an unflagged run: statuses and shapes (the stub's k_pack writes no planes)
    for (int mode : {PREFIX, INFIX}) {
        CHECK(run(mode, nullptr, 3, 4) == QUICKED_OK);
        CHECK(quicked_batch_panel_hit_counts(b, found.data(), stored.data()) == QUICKED_OK);
        const int64_t total = quicked_batch_panel_hit_total(b);
        occ.assign((size_t)total + 1, quicked_panel_occ_t{-7, -7, -7, -7});
        CHECK(quicked_batch_panel_hits(b, occ.data(), off.data()) == QUICKED_OK);
        CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
        for (int i = 0; i < n; ++i) {
            CHECK(st[(size_t)i] == (texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
            CHECK(stored[(size_t)i] == std::min(found[(size_t)i], 4) && off[(size_t)i + 1] - off[(size_t)i] == stored[(size_t)i]);
            CHECK((found[(size_t)i] == 0) == (sc[(size_t)i] == -1) && (!texts[(size_t)i].empty() || found[(size_t)i] == 0));
            for (int64_t j = off[(size_t)i]; j < off[(size_t)i + 1]; ++j) {
                const quicked_panel_occ_t h = occ[(size_t)j];
                CHECK(h.pattern >= 0 && h.pattern < K && h.score >= 0 && h.score <= 3 && h.text_end >= 1 && h.text_end <= (int32_t)texts[(size_t)i].size());
                CHECK(mode == PREFIX ? h.text_start == 0 : (h.text_start >= -1 && h.text_start <= h.text_end));
                if (j > off[(size_t)i]) CHECK(occ[(size_t)j - 1].pattern < h.pattern || (occ[(size_t)j - 1].pattern == h.pattern && occ[(size_t)j - 1].text_end < h.text_end));
            }
        }
    }
    // ---- other kinds of run in turn: each getter family reports its own run only
    CHECK(quicked_batch_run_panel(b, INFIX | QUICKED_SEARCH_IUPAC | QUICKED_PANEL_MATRIX, K, M.bytes.data(), M.off.data(), M.len.data(), own.data(), 0, 1) == QUICKED_OK);
    getters_refuse(b);
    CHECK(quicked_batch_panel_results(b, ph.data()) == QUICKED_OK);
    CHECK(run(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(b) == total0);
    CHECK(quicked_batch_panel_results(b, ph.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_run_search(b, INFIX, nullptr, 3, 1, 1) >= QUICKED_EMPTY_SEQUENCE);      // (the batch's patterns are all empty)
    getters_refuse(b);
    CHECK(run(PREFIX | QUICKED_SEARCH_IUPAC_PATTERN, nullptr, 3, 16) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(b) >= 0);
    CHECK(quicked_batch_run_search_all(b, INFIX, nullptr, 3, 4, 1) >= QUICKED_EMPTY_SEQUENCE);
    getters_refuse(b);
    CHECK(run(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16) == QUICKED_OK);
    {
        quicked_params_t p = quicked_default_params();
        p.algo = BANDED; p.only_score = true;
        (void)quicked_batch_run(b, &p, 1);
        getters_refuse(b);
        (void)quicked_batch_run_bounded(b, nullptr, 3, 1, 1);
        getters_refuse(b);
    }
    // ---- results cleared by a reload: fewer pairs, real patterns
    CHECK(run(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 16) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(b) == total0);
    {
        const int n2 = n / 2;
        std::vector<std::string> pats((size_t)n2), txts(texts.begin(), texts.begin() + n2);
        for (int i = 0; i < n2; ++i) pats[(size_t)i] = panel[(size_t)(i % K)];
        const Pool P2 = pool_of(pats), T2 = pool_of(txts);
        CHECK(quicked_batch_reload(b, n2, P2.bytes.data(), P2.off.data(), P2.len.data(), T2.bytes.data(), T2.off.data(), T2.len.data()) >= 0);
        getters_refuse(b);
        // ... and the batch's patterns play no part: the first n2 texts' answers
        const Conf* cf = nullptr;
        for (const Conf& c : confs) if (c.mode == INFIX && c.flag == QUICKED_SEARCH_IUPAC && c.uniform < 0) cf = &c;
        CHECK(cf);
        CHECK(run(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0, 4096) == QUICKED_OK);
        CHECK(quicked_batch_panel_hit_counts(b, found.data(), stored.data()) == QUICKED_OK);
        const int64_t total = quicked_batch_panel_hit_total(b);
        occ.assign((size_t)total + 1, quicked_panel_occ_t{-7, -7, -7, -7});
        CHECK(quicked_batch_panel_hits(b, occ.data(), off.data()) == QUICKED_OK);
        for (int i = 0; i < n2; ++i) {
            const std::vector<Occ>& w = cf->want[(size_t)i];
            CHECK(found[(size_t)i] == (int32_t)w.size() && stored[(size_t)i] == found[(size_t)i]);
            for (size_t k = 0; k < w.size(); ++k) {
                const quicked_panel_occ_t h = occ[(size_t)off[(size_t)i] + k];
                CHECK(h.pattern == w[k].pattern && h.text_start == w[k].start && h.text_end == w[k].end && h.score == w[k].score);
            }
        }
    }
    quicked_batch_destroy(b);
    printf("panel_hits_host ok\n");
    return 0;
}
