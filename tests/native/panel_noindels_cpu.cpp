// panel_noindels_cpu.cpp -- the mismatch-only panel runs (QUICKED_PANEL_NO_INDELS) compiled for the host: panel_ham_sweep,
// panel_ham_member, panel_ham_text, the scalar valley scan and panel_ham_text_hits, and the two finish bodies of
// quicked_amd/csrc/qe_panel_ham.h -- the very source k_panel_ham and k_panel_ham_hits run per lane.  A stand-alone program,
// built by tests/test_panel_noindels_cpu.py once plain and once with -fsanitize=address,undefined.
//
// panel_noindels_cpu cases <file>     the groups of the fixture, or of a seeded random set, against the values the Python side
//                                     computed with tests/panel_noindels_lib.py; prints "cases ok <entries> occ <records>"
//   file: ngroups cap / per group: K n nconf / K x {member bound} / n x text ("." = empty) / nconf x { mode flag,
//         n x { K x d, K x text_end, found, min(found, cap) x {pattern text_start text_end score} } }
// Per group and configuration, with the planes of every text in a vector of exactly the words that hold it (a read past the
// word of column n - 1 is a sanitizer error):
//   * every member against every text in every register form that holds it (NB = 1, 2, 4): {d, text_end} and the block steps;
//   * per slice count (1, 2, K): panel_ham_text over the slices, the keepers merged, against the best two keys of the matrix;
//   * panel_ham_text_hits over the slices with caps of 1, 2 and 4096: found, the smallest score, the stored records in
//     (pattern, text_end) order, text_start through the finish body.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

#include "qe_panel_ham.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "panel_noindels_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

static std::vector<uint64_t> planes3_of(const std::string& s) {
    const int len = (int)s.size();
    std::vector<uint64_t> pl((size_t)3 * (size_t)((len + 63) / 64), 0);
    for (int i = 0; i < len; ++i) {
        int code;
        switch (s[(size_t)i]) {
            case 'A': case 'a': code = 0; break;
            case 'C': case 'c': code = 1; break;
            case 'G': case 'g': code = 2; break;
            case 'T': case 't': code = 3; break;
            default: code = 4; break;
        }
        uint64_t* row = pl.data() + 3 * (size_t)(i >> 6);
        const uint64_t bit = (uint64_t)1 << (i & 63);
        if (code == 4) row[2] |= bit;
        else { if (code & 1) row[0] |= bit; if (code & 2) row[1] |= bit; }
    }
    return pl;
}
static std::vector<uint64_t> planes4_of(const std::string& s, bool acgt_only) {
    const int len = (int)s.size();
    std::vector<uint64_t> full((size_t)qe::iupac_words(len));
    qe::iupac_pack(reinterpret_cast<const uint8_t*>(s.data()), len, false, acgt_only, full.data());
    full.resize((size_t)4 * (size_t)((len + 63) / 64));
    return full;
}
template <class Eq> struct Planes;
template <> struct Planes<qe::SearchEq3> { static std::vector<uint64_t> of(const std::string& s, bool) { return planes3_of(s); } };
template <> struct Planes<qe::SearchEqIupac> { static std::vector<uint64_t> of(const std::string& s, bool acgt) { return planes4_of(s, acgt); } };

struct Occ { int32_t pattern, start, end, score; };
struct Conf { int mode, flag; std::vector<std::vector<int32_t>> d, e; std::vector<int32_t> found; std::vector<std::vector<Occ>> occ; };
struct Group { std::vector<std::string> panel, texts; std::vector<int32_t> bound; std::vector<Conf> confs; };

static long g_entries = 0, g_records = 0;

template <int NB, class Eq>
static void member_form(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int mode, int32_t d, int32_t e) {
    int32_t score = -7, end = -7;
    uint32_t steps = 0;
    qe::panel_ham_member<NB, Eq>(pp, m, bound, tp, n, mode, score, end, steps);
    if (score != d || end != e) fprintf(stderr, "NB %d m %d n %d bound %d mode %d: got {%d, %d}, expected {%d, %d}\n", NB, m, n, bound, mode, score, end, d, e);
    CHECK(score == d && end == e);
    const int starts = n < m ? 0 : (mode == qe::SEARCH_PREFIX ? 1 : n - m + 1);
    CHECK(steps == (uint32_t)starts * (uint32_t)((m + 63) / 64));
}

template <class Eq>
static void run_conf(const Group& g, const Conf& cf, int cap_file) {
    const int K = (int)g.panel.size(), n = (int)g.texts.size();
    const bool acgt = cf.flag == 32;
    // the panel: planes one member after another, two rows of zeros behind each (the library's layout)
    std::vector<uint64_t> pl;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    for (const std::string& q : g.panel) {
        const std::vector<uint64_t> f = Planes<Eq>::of(q, false);
        off.push_back((int64_t)(pl.size() / Eq::W) * 3);
        pl.insert(pl.end(), f.begin(), f.end());
        pl.insert(pl.end(), (size_t)2 * Eq::W, 0);
        len.push_back((int32_t)q.size());
    }
    qe::PanelView P;
    P.pl = pl.data(); P.off = off.data(); P.len = len.data(); P.bound = g.bound.data();
    for (int i = 0; i < n; ++i) {
        const std::string& text = g.texts[(size_t)i];
        const int tn = (int)text.size();
        const std::vector<uint64_t> tpl = Planes<Eq>::of(text, acgt);           // exactly the words of columns 0 .. n - 1
        const uint64_t* tp = tpl.data();
        const std::vector<int32_t>& wd = cf.d[(size_t)i];
        const std::vector<int32_t>& we = cf.e[(size_t)i];
        // ---- every register form that holds the member
        for (int p = 0; p < K; ++p) {
            const int m = len[(size_t)p], nb = qe::search_blocks(m);
            const uint64_t* pp = pl.data() + Eq::offset(off[(size_t)p]);
            if (nb <= 1) member_form<1, Eq>(pp, m, g.bound[(size_t)p], tp, tn, cf.mode, wd[(size_t)p], we[(size_t)p]);
            if (nb <= 2) member_form<2, Eq>(pp, m, g.bound[(size_t)p], tp, tn, cf.mode, wd[(size_t)p], we[(size_t)p]);
            member_form<4, Eq>(pp, m, g.bound[(size_t)p], tp, tn, cf.mode, wd[(size_t)p], we[(size_t)p]);
            ++g_entries;
        }
        // ---- the best two keys of the matrix row
        int32_t p1 = -1, s1 = -1, p2 = -1, s2 = -1;
        for (int p = 0; p < K; ++p) {
            if (wd[(size_t)p] < 0) continue;
            if (p1 < 0 || wd[(size_t)p] < s1) { p2 = p1; s2 = s1; p1 = p; s1 = wd[(size_t)p]; }
            else if (p2 < 0 || wd[(size_t)p] < s2) { p2 = p; s2 = wd[(size_t)p]; }
        }
        for (int nslices : {1, 2, K}) {
            const int per = (K + nslices - 1) / nslices;
            // ---- the keeper over the slices, merged in reverse order
            std::vector<int32_t> ms((size_t)K, -9), me((size_t)K, -9);
            std::vector<qe::PanelKeeper> parts;
            uint32_t steps = 0;
            for (int p0 = 0; p0 < K; p0 += per) {
                qe::PanelKeeper keep;
                keep.init();
                qe::panel_ham_text<Eq>(P, p0, std::min(K, p0 + per), tp, tn, cf.mode, keep, steps, ms.data(), me.data());
                parts.push_back(keep);
            }
            qe::PanelKeeper all;
            all.init();
            for (size_t s = parts.size(); s-- > 0;) all.merge(parts[s]);
            CHECK(ms == wd && me == we);
            CHECK(all.p1 == p1 && all.s1 == s1 && all.p2 == p2 && all.s2 == s2 && (p1 < 0 || all.e1 == we[(size_t)p1]));
            if (p1 >= 0) {
                int32_t hit[6] = {all.p1, all.s1, 0, all.e1, all.p2, all.s2};
                qe::panel_ham_finish_pair(0, len.data(), hit);
                CHECK(hit[2] == all.e1 - len[(size_t)p1] && hit[2] >= 0);
            }
            // ---- every occurrence over the slices: the lanes' stretches in slice order
            for (int cap : {1, 2, 4096}) {
                std::vector<qe::PanelRawHit> got;
                int32_t found = 0, best = -1;
                uint32_t hsteps = 0;
                for (int p0 = 0; p0 < K; p0 += per) {
                    std::vector<qe::PanelRawHit> raw((size_t)cap);
                    qe::PanelHamScan H;
                    qe::panel_hit_scan_init(H, raw.data(), cap);
                    qe::panel_ham_text_hits<Eq>(P, p0, std::min(K, p0 + per), tp, tn, cf.mode, H, hsteps);
                    CHECK(H.sink.count == std::min(H.found, cap));
                    found += H.found;
                    best = (H.best >= 0 && (best < 0 || H.best < best)) ? H.best : best;
                    for (int j = 0; j < H.sink.count && (int)got.size() < cap; ++j) got.push_back(raw[(size_t)j]);
                }
                CHECK(hsteps == steps);
                CHECK(found == cf.found[(size_t)i]);
                const std::vector<Occ>& w = cf.occ[(size_t)i];
                const size_t cmp = std::min<size_t>(std::min<size_t>((size_t)cap, (size_t)cap_file), w.size());
                CHECK(got.size() == (size_t)std::min(found, cap));
                int32_t wbest = -1;
                for (size_t j = 0; j < cmp; ++j) {
                    int32_t rec[4] = {got[j].pattern, 0, got[j].end, got[j].score};
                    qe::panel_ham_hits_finish_one(0, len.data(), rec);
                    if (rec[0] != w[j].pattern || rec[1] != w[j].start || rec[2] != w[j].end || rec[3] != w[j].score)
                        fprintf(stderr, "text %d mode %d flag %d occurrence %zu: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n", i, cf.mode, cf.flag, j,
                                rec[0], rec[1], rec[2], rec[3], w[j].pattern, w[j].start, w[j].end, w[j].score);
                    CHECK(rec[0] == w[j].pattern && rec[1] == w[j].start && rec[2] == w[j].end && rec[3] == w[j].score);
                    ++g_records;
                }
                // the text's score: the smallest over every found occurrence, which the matrix row has too
                for (int p = 0; p < K; ++p) if (wd[(size_t)p] >= 0 && (wbest < 0 || wd[(size_t)p] < wbest)) wbest = wd[(size_t)p];
                CHECK(best == wbest);
            }
        }
    }
}

int main(int argc, char** argv) {
    CHECK(argc == 3 && !strcmp(argv[1], "cases"));
    std::ifstream f(argv[2]);
    int ngroups = 0, cap = 0;
    f >> ngroups >> cap;
    CHECK(!f.fail() && ngroups >= 1 && cap >= 1);
    for (int gi = 0; gi < ngroups; ++gi) {
        int K = 0, n = 0, nconf = 0;
        f >> K >> n >> nconf;
        CHECK(!f.fail() && K >= 1 && n >= 1 && nconf >= 1);
        Group g;
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
        for (const Conf& cf : g.confs) {
            if (cf.flag) run_conf<qe::SearchEqIupac>(g, cf, cap);
            else run_conf<qe::SearchEq3>(g, cf, cap);
        }
    }
    printf("cases ok %ld occ %ld\n", g_entries, g_records);
    return 0;
}
