// panel_noindels_scan_cpu.cpp -- the windowed mismatch-only panel run compiled for the host: PanelHamScanOf with an owned range,
// panel_ham_window_hits (quicked_amd/csrc/qe_panel_ham.h) and the count / expand bodies of qe_panel.h -- the very source
// k_panel_ham_scan, k_panel_scan_sums, k_panel_scan_count, k_panel_ham_scan_expand and k_panel_ham_hits_finish run per lane --
// driven through the stage's steps.  A stand-alone program, built by tests/test_panel_noindels_scan_cpu.py once plain and once
// with -fsanitize=address,undefined.
//
// panel_noindels_scan_cpu cases <file>    the groups of tests/panel_noindels_scan_lib.py's cases_file against the lists and
//                                         block steps it holds; prints "cases ok <n checked>"
// Per group and flag, every text's planes in a vector of exactly the words that hold the text (a read past the word of column
// n - 1 is a sanitizer error):
//   * the unwindowed path once -- panel_ham_text_hits per text over one slice with cap 4096 --: its records are the list's;
//   * per window (64, 128, 192, 4096), cap (1, 2, 4096) and slice count (1, 2, K): the slot table as the stage builds it, the
//     forward pass over window slots x slices, the two count bodies, the offset scan, the expand body without tasks lane by
//     lane in DESCENDING lane order, the finish body: found, stored, the smallest score and every stored record against the
//     list's first `cap` and against the unwindowed path's; every hit slot written exactly once; the block steps the model's.
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

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "panel_noindels_scan_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

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
struct Conf { int flag; long long steps[4]; std::vector<std::vector<Occ>> want; };
struct Group { std::vector<std::string> panel, texts; std::vector<int32_t> bound; std::vector<Conf> confs; };
static const int WINDOWS[4] = {64, 128, 192, 4096};

template <class Eq>
static long run_conf(const Group& g, const Conf& cf) {
    const int K = (int)g.panel.size(), n = (int)g.texts.size();
    // the panel: planes one member after another, two rows of zeros behind each (the library's layout)
    std::vector<uint64_t> pl;
    std::vector<int64_t> m_off;
    std::vector<int32_t> m_len, t_len;
    for (const std::string& q : g.panel) {
        const std::vector<uint64_t> f = Planes<Eq>::of(q, false);
        m_off.push_back((int64_t)(pl.size() / Eq::W) * 3);
        pl.insert(pl.end(), f.begin(), f.end());
        pl.insert(pl.end(), (size_t)2 * Eq::W, 0);
        m_len.push_back((int32_t)q.size());
    }
    std::vector<std::vector<uint64_t>> tpl;                     // exactly the words of columns 0 .. n - 1, text by text
    for (const std::string& t : g.texts) { tpl.push_back(Planes<Eq>::of(t, cf.flag == 32)); t_len.push_back((int32_t)t.size()); }
    std::vector<int64_t> t_off((size_t)n, 0);                   // (the expand body without tasks never reads it)
    qe::PanelView P;
    P.pl = pl.data(); P.off = m_off.data(); P.len = m_len.data(); P.bound = g.bound.data();
    long checked = 0;
    std::vector<int32_t> text;
    for (int i = 0; i < n; ++i) if (!g.texts[(size_t)i].empty()) text.push_back(i);
    while (text.size() % 64) text.push_back(-1);
    const int ntext = (int)text.size();
    // ---- the unwindowed path: one slice, cap 4096
    std::vector<std::vector<qe::PanelRawHit>> whole((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (g.texts[(size_t)i].empty()) { CHECK(cf.want[(size_t)i].empty()); continue; }
        const int cap = 4096;
        std::vector<qe::PanelRawHit> raw((size_t)cap);
        qe::PanelHamScan H;
        qe::panel_hit_scan_init(H, raw.data(), cap);
        uint32_t steps = 0;
        qe::panel_ham_text_hits<Eq>(P, 0, K, tpl[(size_t)i].data(), t_len[(size_t)i], qe::SEARCH_INFIX, H, steps);
        CHECK(H.found == (int32_t)cf.want[(size_t)i].size() && H.found <= cap);
        whole[(size_t)i].assign(raw.begin(), raw.begin() + H.sink.count);
        for (int k = 0; k < H.sink.count; ++k) {
            const Occ& o = cf.want[(size_t)i][(size_t)k];
            CHECK(raw[(size_t)k].pattern == o.pattern && raw[(size_t)k].end == o.end && raw[(size_t)k].score == o.score);
        }
        ++checked;
    }
    // ---- the windowed stage's flow
    for (int wi = 0; wi < 4; ++wi) {
        const int window = WINDOWS[wi];
        std::vector<int32_t> w_pair, w_text, w_c0, w_c1, first_slot((size_t)n, 0), nwin((size_t)n, 0);
        for (int t = 0; t < ntext; ++t) {
            const int pair = text[(size_t)t];
            if (pair < 0) continue;
            first_slot[(size_t)pair] = (int32_t)w_pair.size();
            for (int c0 = 0; c0 < t_len[(size_t)pair]; c0 += window) {
                w_pair.push_back(pair); w_text.push_back(t); w_c0.push_back(c0); w_c1.push_back(std::min(t_len[(size_t)pair], c0 + window));
                ++nwin[(size_t)pair];
            }
        }
        while (w_pair.size() % 64) { w_pair.push_back(-1); w_text.push_back(-1); w_c0.push_back(0); w_c1.push_back(0); }
        const int nslots = (int)w_pair.size();
        for (int cap : {1, 2, 4096})
            for (int want_slices : {1, 2, K}) {
                const int per = (K + want_slices - 1) / want_slices, ns = (K + per - 1) / per;
                std::vector<int32_t> part((size_t)4 * (size_t)ns * (size_t)nslots, -7);
                std::vector<qe::PanelRawHit> raw((size_t)ns * (size_t)nslots * (size_t)cap);
                qe::PanelScanArgs A{};
                A.n_members = K; A.per_slice = per; A.nslots = nslots; A.max_hits = cap; A.part = part.data(); A.raw = raw.data();
                uint64_t walked = 0;
                for (int s = 0; s < ns; ++s)
                    for (int w = 0; w < nslots; ++w) {
                        const int pair = w_pair[(size_t)w];
                        if (pair < 0) continue;
                        qe::PanelHamWindowScan H;
                        qe::panel_ham_window_scan_init(H, raw.data() + ((size_t)s * (size_t)nslots + (size_t)w) * (size_t)cap, cap, w_c0[(size_t)w], w_c1[(size_t)w]);
                        uint32_t steps = 0;
                        qe::panel_ham_window_hits<Eq>(P, s * per, std::min(K, (s + 1) * per), tpl[(size_t)pair].data(), t_len[(size_t)pair],
                                                      w_c0[(size_t)w], w_c1[(size_t)w], H, steps);
                        CHECK(H.sink.count == std::min(H.found, cap));
                        walked += steps;
                        qe::panel_scan_store_part(A, ns, s, w, H, steps);
                    }
                if ((long long)walked != cf.steps[wi]) fprintf(stderr, "flag %d window %d cap %d slices %d: walked %llu, the model %lld\n", cf.flag, window, cap, ns, (unsigned long long)walked, cf.steps[wi]);
                CHECK((long long)walked == cf.steps[wi]);
                std::vector<int32_t> found((size_t)n, 0), best((size_t)n, -1), len((size_t)n, -1), base((size_t)ns * (size_t)ntext, -7);
                std::vector<uint32_t> adv((size_t)ntext, 0);
                qe::PanelScanCountArgs Cn{};
                Cn.ntext = ntext; Cn.nslots = nslots; Cn.nslices = ns; Cn.max_hits = cap;
                Cn.text = text.data(); Cn.first_slot = first_slot.data(); Cn.nwin = nwin.data(); Cn.part = part.data();
                std::vector<int32_t> sums((size_t)4 * (size_t)ns * (size_t)ntext, -7);
                Cn.sums = sums.data();
                Cn.found = found.data(); Cn.best = best.data(); Cn.len = len.data(); Cn.base = base.data(); Cn.o_adv = adv.data();
                for (int s = ns - 1; s >= 0; --s) for (int t = 0; t < ntext; ++t) qe::panel_scan_sums_slice(Cn, s, t);
                for (int t = 0; t < ntext; ++t) qe::panel_scan_count_text(Cn, t);
                uint64_t counted = 0;
                for (uint32_t a : adv) counted += a;
                CHECK(counted == walked);
                std::vector<int64_t> off((size_t)n + 1, 0);
                for (int i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + len[(size_t)i] + 1;      // k_scan_offsets
                const int64_t total = off[(size_t)n];
                std::vector<int32_t> hits((size_t)(4 * total + 4), -7);
                qe::PanelScanExpandArgs E{};                        // (every o_* stays null: the body without tasks touches none)
                E.ntext = ntext; E.nslots = nslots; E.nslices = ns; E.max_hits = cap;
                E.w_pair = w_pair.data(); E.w_text = w_text.data(); E.first_slot = first_slot.data(); E.nwin = nwin.data();
                E.part = part.data(); E.raw = raw.data(); E.base = base.data(); E.off = off.data();
                E.m_len = m_len.data(); E.m_off = m_off.data(); E.t_len = t_len.data(); E.t_off = t_off.data(); E.hits = hits.data();
                for (int s = ns - 1; s >= 0; --s) for (int w = nslots - 1; w >= 0; --w) qe::panel_scan_expand_lane_of<false>(E, s, w);
                for (int64_t j = 0; j < total; ++j) {
                    CHECK(hits[(size_t)(4 * j)] >= 0 && hits[(size_t)(4 * j + 1)] == 0);      // (-7: a slot no lane wrote)
                    qe::panel_ham_hits_finish_one(j, m_len.data(), hits.data());
                }
                CHECK(hits[(size_t)(4 * total)] == -7);
                for (int i = 0; i < n; ++i) {
                    const std::vector<Occ>& w = cf.want[(size_t)i];
                    const int32_t stored = (int32_t)std::min<size_t>(w.size(), (size_t)cap);
                    int32_t wbest = -1;
                    for (const Occ& o : w) wbest = (wbest < 0 || o.score < wbest) ? o.score : wbest;
                    if (found[(size_t)i] != (int32_t)w.size() || off[(size_t)i + 1] - off[(size_t)i] != stored || best[(size_t)i] != wbest)
                        fprintf(stderr, "flag %d window %d cap %d slices %d text %d: found %d stored %lld best %d, expected %zu %d %d\n", cf.flag,
                                window, cap, ns, i, found[(size_t)i], (long long)(off[(size_t)i + 1] - off[(size_t)i]), best[(size_t)i], w.size(), stored, wbest);
                    CHECK(found[(size_t)i] == (int32_t)w.size() && off[(size_t)i + 1] - off[(size_t)i] == stored && best[(size_t)i] == wbest);
                    for (int k = 0; k < stored; ++k) {
                        const int32_t* h = hits.data() + 4 * (off[(size_t)i] + k);
                        const Occ& o = w[(size_t)k];
                        const qe::PanelRawHit& u = whole[(size_t)i][(size_t)k];
                        if (h[0] != o.pattern || h[1] != o.start || h[2] != o.end || h[3] != o.score)
                            fprintf(stderr, "flag %d window %d cap %d slices %d text %d occurrence %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n",
                                    cf.flag, window, cap, ns, i, k, h[0], h[1], h[2], h[3], o.pattern, o.start, o.end, o.score);
                        CHECK(h[0] == o.pattern && h[1] == o.start && h[2] == o.end && h[3] == o.score);
                        CHECK(h[0] == u.pattern && h[2] == u.end && h[3] == u.score);
                        ++checked;
                    }
                    ++checked;
                }
            }
    }
    return checked;
}

static int cases(const char* path) {
    std::ifstream f(path);
    int ngroups = 0;
    f >> ngroups;
    CHECK(!f.fail() && ngroups >= 1);
    long checked = 0;
    for (int gi = 0; gi < ngroups; ++gi) {
        int K = 0, n = 0, nconf = 0;
        f >> K >> n >> nconf;
        CHECK(!f.fail() && K >= 1 && n >= 1 && nconf >= 1);
        Group g;
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
            checked += cf.flag ? run_conf<qe::SearchEqIupac>(g, cf) : run_conf<qe::SearchEq3>(g, cf);
        }
    }
    printf("cases ok %ld\n", checked);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "cases")) return cases(argv[2]);
    fprintf(stderr, "usage: panel_noindels_scan_cpu cases <file>\n");
    return 2;
}
