// Panel runs (quicked_batch_run_panel) on the HOST, under sanitizers: the library's host layer built with g++ against the fake
// HIP runtime of tests/native/hip_stub.  The stand-ins of k_search_panel / k_panel_reduce / k_panel_finish in qe_stages.hip are
// the device kernels' own source (qe_panel.h) run text by text, the stand-in of k_search<4, Eq> runs the real recurrence and
// the stand-in of k_pack_iupac is the scalar packer of qe_iupac.h, so a FLAGGED panel run of an ASCII batch gives true
// answers here: they are compared with the expectations tests/test_host_search_panel.py computed with tests/panel_lib.py (file
// `cases` in the directory given; the format of tests/native/search_panel_cpu.cpp).  An unflagged run reads planes the stub's
// k_pack never wrote: only its statuses and the shape of its results are checked.  Checked: every QUICKED_ERROR and
// QUICKED_UNIMPLEMENTED rule with nothing launched, the getters' rules before and after other kinds of run, results cleared by
// a reload, QE_PANEL_SLICES = 1, 2 and a huge value.  A stand-alone program: nothing is loaded into Python.
#define PANEL_HOST_NAME "search_panel_host"
#include "panel_host_common.h"

struct Conf { int mode, flag, uniform; std::vector<std::vector<int32_t>> want; };

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
        cf.want.assign((size_t)n, std::vector<int32_t>((size_t)(6 + 2 * K)));
        for (int i = 0; i < n; ++i) for (int k = 0; k < 6 + 2 * K; ++k) f >> cf.want[(size_t)i][(size_t)k];
        CHECK(!f.fail());
    }
    const Pool M = pool_of(panel), T = pool_of(texts);
    // the batch's own patterns: all empty
    const std::vector<std::string> none_s((size_t)n);
    const Pool E = pool_of(none_s);
    quicked_batch_t* b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
    CHECK(b);
    std::vector<quicked_panel_hit_t> hits((size_t)n);
    std::vector<int32_t> ms((size_t)n * (size_t)K), me((size_t)n * (size_t)K), sc((size_t)n), st((size_t)n), loc((size_t)n);
    const int INFIX = QUICKED_SEARCH_INFIX, PREFIX = QUICKED_SEARCH_PREFIX;
    auto run = [&](int mode, const int32_t* md, int32_t all) {
        return quicked_batch_run_panel(b, mode, K, M.bytes.data(), M.off.data(), M.len.data(), md, all, 1);
    };
    // ---- before any run: the panel getters refuse
    CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_ERROR);
    // ---- a first run, so that "nothing launched" has counters to leave alone
    CHECK(run(INFIX | QUICKED_SEARCH_IUPAC | QUICKED_PANEL_MATRIX, own.data(), 0) == QUICKED_OK);
    const int64_t steps0 = steps_of(b);
    CHECK(steps0 > 0);
    CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_OK);
    const std::vector<quicked_panel_hit_t> hits0 = hits;
    // ---- QUICKED_ERROR, nothing launched
    CHECK(quicked_batch_run_panel(nullptr, INFIX, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 1) == QUICKED_ERROR);
    for (int mode : {0, 3, 4, 16, 64, 16 | 32 | 2, 128 | 2, 256 | 1, 8 | 2, -1}) CHECK(run(mode, nullptr, 3) == QUICKED_ERROR);
    CHECK(run(INFIX | QUICKED_SEARCH_IUPAC | QUICKED_SEARCH_IUPAC_PATTERN | QUICKED_PANEL_MATRIX, nullptr, 3) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel(b, INFIX, 0, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 1) == QUICKED_ERROR);
    CHECK(quicked_batch_run_panel(b, INFIX, -5, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 1) == QUICKED_ERROR);
    {
        std::vector<int64_t> off((size_t)QUICKED_PANEL_MAX_PATTERNS + 1, 0);
        std::vector<int32_t> len((size_t)QUICKED_PANEL_MAX_PATTERNS + 1, 1);
        CHECK(quicked_batch_run_panel(b, INFIX, QUICKED_PANEL_MAX_PATTERNS + 1, M.bytes.data(), off.data(), len.data(), nullptr, 3, 1) == QUICKED_ERROR);
        CHECK(quicked_batch_run_panel(b, PREFIX, QUICKED_PANEL_MAX_PATTERNS, M.bytes.data(), off.data(), len.data(), nullptr, 0, 1) == QUICKED_OK);      // the limit itself
        CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_ERROR);      // ... without the flag
        CHECK(run(INFIX | QUICKED_SEARCH_IUPAC | QUICKED_PANEL_MATRIX, own.data(), 0) == QUICKED_OK);
        CHECK(steps_of(b) == steps0);
    }
    {
        std::vector<int32_t> len = M.len;
        len[1] = 0;                                               // a member of length 0 -- even next to one that is too long
        CHECK(quicked_batch_run_panel(b, INFIX, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 3, 1) == QUICKED_ERROR);
        len[0] = QUICKED_PANEL_MAX_LEN + 1;
        CHECK(quicked_batch_run_panel(b, INFIX, K, M.bytes.data(), M.off.data(), len.data(), nullptr, 3, 1) == QUICKED_ERROR);
        std::vector<int32_t> bad = own;
        bad[(size_t)K - 1] = -1;                                  // a negative bound
        CHECK(run(INFIX, bad.data(), 3) == QUICKED_ERROR);
        CHECK(run(INFIX, nullptr, -1) == QUICKED_ERROR);
    }
    // ---- with the matrix flag, (texts) x n_patterns above 2^28: 65 537 texts x 4096 members is one row too many.  The rule
    // comes before the QUICKED_UNIMPLEMENTED ones, so a queued run (sync == 0) tells which of the two refused, and nothing runs
    {
        const int32_t KM = QUICKED_PANEL_MAX_PATTERNS;
        const std::vector<int64_t> moff((size_t)KM, 0);
        const std::vector<int32_t> mlen((size_t)KM, 1);
        auto batch_of_ones = [&](int64_t count, int64_t empty) {      // `count` pairs: one-base texts, the last `empty` of them empty
            std::vector<int64_t> off((size_t)count, 0);
            std::vector<int32_t> tl((size_t)count, 1), pl((size_t)count, 0);
            for (int64_t i = count - empty; i < count; ++i) tl[(size_t)i] = 0;
            quicked_batch_t* q = quicked_batch_create(count, "A", off.data(), pl.data(), "A", off.data(), tl.data());
            CHECK(q);
            return q;
        };
        auto panel_run = [&](quicked_batch_t* q, int mode, int sync) { return quicked_batch_run_panel(q, mode, KM, "A", moff.data(), mlen.data(), nullptr, 0, sync); };
        quicked_batch_t* over = batch_of_ones(65537, 0);
        int64_t c0[8], c1[8];
        CHECK(quicked_batch_counters(over, c0) >= 0);
        CHECK(panel_run(over, INFIX | QUICKED_PANEL_MATRIX, 1) == QUICKED_ERROR);
        CHECK(panel_run(over, PREFIX | QUICKED_SEARCH_IUPAC | QUICKED_PANEL_MATRIX, 0) == QUICKED_ERROR);
        CHECK(panel_run(over, INFIX, 0) == QUICKED_UNIMPLEMENTED);                          // the same shape without the flag: not this rule
        CHECK(quicked_batch_counters(over, c1) >= 0 && !memcmp(c0, c1, sizeof(c0)));
        CHECK(quicked_batch_panel_results(over, nullptr) == QUICKED_ERROR);
        quicked_batch_destroy(over);
        quicked_batch_t* holes = batch_of_ones(65537, 40000);                               // empty texts have rows too
        CHECK(panel_run(holes, INFIX | QUICKED_PANEL_MATRIX, 1) == QUICKED_ERROR);
        quicked_batch_destroy(holes);
        quicked_batch_t* fits = batch_of_ones(65536, 0);                                    // one text fewer: exactly 2^28
        CHECK(panel_run(fits, INFIX | QUICKED_PANEL_MATRIX, 0) == QUICKED_UNIMPLEMENTED);
        quicked_batch_destroy(fits);
    }
    // ---- QUICKED_UNIMPLEMENTED, nothing queued
    {
        const std::string big((size_t)QUICKED_PANEL_MAX_LEN + 1, 'A'), fits((size_t)QUICKED_PANEL_MAX_LEN, 'A');
        const int64_t off[2] = {0, 0};
        int32_t len[2] = {4, QUICKED_PANEL_MAX_LEN + 1};
        CHECK(quicked_batch_run_panel(b, INFIX, 2, big.data(), off, len, nullptr, 3, 1) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_panel(b, INFIX, K, M.bytes.data(), M.off.data(), M.len.data(), nullptr, 3, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
        CHECK(run(INFIX, nullptr, 3) == QUICKED_UNIMPLEMENTED);
        CHECK(run(PREFIX | QUICKED_SEARCH_IUPAC_PATTERN, nullptr, 3) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
    }
    // none of it ran: the results and the counters are the first run's
    CHECK(steps_of(b) == steps0);
    CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_OK);
    CHECK(!memcmp(hits.data(), hits0.data(), hits.size() * sizeof(quicked_panel_hit_t)));
    // ---- true answers under the two flags, every configuration, with the slices forced and chosen
    for (const char* slices : {(const char*)nullptr, "1", "2", "1000000000000"}) {
        set_env("QE_PANEL_SLICES", slices);
        for (const Conf& cf : confs) {
            if (!cf.flag) continue;
            CHECK(quicked_batch_configure_tags(b, QUICKED_TAG_STATS) == QUICKED_OK);      // ignored: no alignments
            CHECK(run(cf.mode | cf.flag | QUICKED_PANEL_MATRIX, cf.uniform < 0 ? own.data() : nullptr, cf.uniform < 0 ? 0 : cf.uniform) == QUICKED_OK);
            CHECK(quicked_batch_configure_tags(b, 0) == QUICKED_OK);
            CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_OK);
            CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_OK);
            CHECK(quicked_batch_panel_matrix(b, nullptr, nullptr) == QUICKED_OK);
            CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
            CHECK(steps_of(b) > 0);
            for (int i = 0; i < n; ++i) {
                const std::vector<int32_t>& w = cf.want[(size_t)i];
                const quicked_panel_hit_t h = hits[(size_t)i];
                const int32_t have[6] = {h.pattern, h.score, h.text_start, h.text_end, h.second_pattern, h.second_score};
                for (int k = 0; k < 6; ++k) {
                    if (have[k] != w[(size_t)k]) fprintf(stderr, "mode %d flag %d uniform %d text %d field %d: got %d, expected %d\n", cf.mode, cf.flag, cf.uniform, i, k, have[k], w[(size_t)k]);
                    CHECK(have[k] == w[(size_t)k]);
                }
                for (int p = 0; p < K; ++p) CHECK(ms[(size_t)i * (size_t)K + (size_t)p] == w[(size_t)(6 + p)] && me[(size_t)i * (size_t)K + (size_t)p] == w[(size_t)(6 + K + p)]);
                CHECK(sc[(size_t)i] == w[1]);
                CHECK(st[(size_t)i] == (texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
            }
            // the other getters: what they return after any run that produced none of their data
            CHECK(quicked_batch_locations(b, loc.data(), loc.data()) == QUICKED_ERROR);
            CHECK(quicked_batch_hit_total(b) == -1);
            CHECK(quicked_batch_cigar_bytes(b) == 0);
            quicked_pair_stats_t ps;
            CHECK(quicked_batch_pair_stats(b, &ps) == QUICKED_ERROR);
        }
    }
    set_env("QE_PANEL_SLICES", nullptr);
    // ---- an unflagged run: statuses and shapes (the stub's k_pack writes no planes)
    CHECK(run(PREFIX, nullptr, 3) == QUICKED_OK);
    CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_OK);
    CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
    for (int i = 0; i < n; ++i) {
        const quicked_panel_hit_t h = hits[(size_t)i];
        CHECK(st[(size_t)i] == (texts[(size_t)i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
        CHECK(h.pattern >= -1 && h.pattern < K && h.second_pattern >= -1 && h.second_pattern < K && sc[(size_t)i] == h.score);
        if (texts[(size_t)i].empty() || h.pattern < 0) CHECK(h.pattern == -1 && h.score == -1 && h.text_start == -1 && h.text_end == -1 && h.second_pattern == -1 && h.second_score == -1);
        else CHECK(h.score >= 0 && h.score <= 3 && h.text_start == 0 && h.text_end >= 1 && h.text_end <= (int32_t)texts[(size_t)i].size());
    }
    // ---- other kinds of run in turn: each getter family reports its own run only
    CHECK(quicked_batch_run_search(b, INFIX, nullptr, 3, 1, 1) >= QUICKED_EMPTY_SEQUENCE);      // (the batch's patterns are all empty)
    CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_ERROR);
    CHECK(run(INFIX | QUICKED_SEARCH_IUPAC_PATTERN | QUICKED_PANEL_MATRIX, own.data(), 0) == QUICKED_OK);
    CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_OK);
    CHECK(quicked_batch_locations(b, loc.data(), loc.data()) == QUICKED_ERROR);
    {
        quicked_params_t p = quicked_default_params();
        p.algo = BANDED; p.only_score = true;
        (void)quicked_batch_run(b, &p, 1);
        CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_ERROR);
        CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_ERROR);
    }
    // ---- results cleared by a reload: fewer pairs, real patterns
    CHECK(run(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0) == QUICKED_OK);
    CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_OK);
    {
        const int n2 = n / 2;
        std::vector<std::string> pats((size_t)n2), txts(texts.begin(), texts.begin() + n2);
        for (int i = 0; i < n2; ++i) pats[(size_t)i] = panel[(size_t)(i % K)];
        const Pool P2 = pool_of(pats), T2 = pool_of(txts);
        CHECK(quicked_batch_reload(b, n2, P2.bytes.data(), P2.off.data(), P2.len.data(), T2.bytes.data(), T2.off.data(), T2.len.data()) >= 0);
        CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_ERROR);
        CHECK(quicked_batch_panel_matrix(b, ms.data(), me.data()) == QUICKED_ERROR);
        // ... and the batch's patterns play no part: the first n2 texts' answers
        const Conf* cf = nullptr;
        for (const Conf& c : confs) if (c.mode == INFIX && c.flag == QUICKED_SEARCH_IUPAC && c.uniform < 0) cf = &c;
        CHECK(cf);
        CHECK(run(INFIX | QUICKED_SEARCH_IUPAC, own.data(), 0) == QUICKED_OK);
        CHECK(quicked_batch_panel_results(b, hits.data()) == QUICKED_OK);
        for (int i = 0; i < n2; ++i) {
            const quicked_panel_hit_t h = hits[(size_t)i];
            const int32_t have[6] = {h.pattern, h.score, h.text_start, h.text_end, h.second_pattern, h.second_score};
            for (int k = 0; k < 6; ++k) CHECK(have[k] == cf->want[(size_t)i][(size_t)k]);
        }
    }
    quicked_batch_destroy(b);
    printf("search_panel_host ok\n");
    return 0;
}
