// panel_scan_cpu.cpp -- the windowed panel search compiled for the host: SearchHitScanOf with an owned range,
// panel_window_hits and the count / expand bodies of quicked_amd/csrc/qe_panel.h -- the very source k_panel_scan,
// k_panel_scan_sums, k_panel_scan_count and k_panel_scan_expand run per lane -- driven through the stage's steps.  A
// stand-alone program, built by tests/test_panel_scan_cpu.py once plain and once with -fsanitize=address,undefined.
//
// panel_scan_cpu cases <file>      the cases of tests/test_panel_scan_cpu.py against the lists it took from the fixtures
//                                  (tests/panel_hits_lib.py's format: see cases_file there); prints "cases ok <n checked>"
// Per configuration (INFIX; flag; the members' own bounds or the uniform one):
//   * the unwindowed path once -- panel_text_hits per text over one slice with cap 4096, the count and expand bodies --: its
//     records are the list's;
//   * per window (64, 128, 192, 4096), cap (1, 2, 4096) and slice count (1, 2, K): the slot table as the stage builds it,
//     the forward pass over window slots x slices (panel_window_hits, panel_scan_store_part), the two count bodies, the
//     offset scan, the expand body lane by lane -- in DESCENDING lane order: a record's place must not depend on who wrote before -- and
//     the start pass with k_search's stand-in arithmetic, then the finish body: found, stored, the smallest score and every
//     stored record against the list's first `cap` and against the unwindowed path's; every hit slot is written exactly once.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

#include "qe_panel.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "panel_scan_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

static std::vector<uint64_t> planes3_of(const std::string& s, bool reverse) {
    const int len = (int)s.size();
    std::vector<uint64_t> pl((size_t)3 * (size_t)((len + 63) / 64), 0);
    for (int i = 0; i < len; ++i) {
        int code;
        switch (s[(size_t)(reverse ? len - 1 - i : i)]) {
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
static std::vector<uint64_t> planes4_of(const std::string& s, bool reverse, bool acgt_only) {
    const int len = (int)s.size();
    std::vector<uint64_t> full((size_t)qe::iupac_words(len));
    qe::iupac_pack(reinterpret_cast<const uint8_t*>(s.data()), len, reverse, acgt_only, full.data());
    full.resize((size_t)4 * (size_t)((len + 63) / 64));
    return full;
}
template <class Eq> struct Planes;
template <> struct Planes<qe::SearchEq3> { static std::vector<uint64_t> of(const std::string& s, bool rev, bool) { return planes3_of(s, rev); } };
template <> struct Planes<qe::SearchEqIupac> { static std::vector<uint64_t> of(const std::string& s, bool rev, bool acgt) { return planes4_of(s, rev, acgt); } };

// sequences' planes one after another without padding rows; off: three-plane word offsets (Eq::offset maps them)
template <class Eq>
struct Pool {
    std::vector<uint64_t> fwd, rev;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    void add(const std::string& s, bool acgt) {
        const std::vector<uint64_t> f = Planes<Eq>::of(s, false, acgt), r = Planes<Eq>::of(s, true, acgt);
        off.push_back((int64_t)(fwd.size() / Eq::W) * 3);
        fwd.insert(fwd.end(), f.begin(), f.end()); rev.insert(rev.end(), r.begin(), r.end());
        len.push_back((int32_t)s.size());
    }
};

struct Occ { int32_t pattern, start, end, score; };
struct Conf { int mode, flag, uniform; std::vector<std::vector<Occ>> want; };

template <class Eq>
static long run_conf(const Conf& cf, const std::vector<std::string>& panel, const std::vector<int32_t>& own, const std::vector<std::string>& texts) {
    const int K = (int)panel.size(), n = (int)texts.size();
    CHECK(cf.mode == qe::SEARCH_INFIX);
    Pool<Eq> M, T;
    std::vector<int32_t> bound((size_t)K);
    for (int p = 0; p < K; ++p) { M.add(panel[(size_t)p], false); bound[(size_t)p] = cf.uniform >= 0 ? cf.uniform : own[(size_t)p]; }
    for (int i = 0; i < n; ++i) T.add(texts[(size_t)i], cf.flag == 32);
    M.fwd.push_back(0); M.rev.push_back(0); T.fwd.push_back(0); T.rev.push_back(0);      // (data() of an all-empty pool)
    qe::PanelView P;
    P.pl = M.fwd.data(); P.off = M.off.data(); P.len = M.len.data(); P.bound = bound.data();
    long checked = 0;
    std::vector<int32_t> text;
    for (int i = 0; i < n; ++i) if (!texts[(size_t)i].empty()) text.push_back(i);
    while (text.size() % 64) text.push_back(-1);
    const int ntext = (int)text.size();
    // ---- the unwindowed path: one slice, cap 4096
    std::vector<std::vector<qe::PanelRawHit>> whole((size_t)n);
    {
        const int cap = 4096;
        std::vector<int32_t> part((size_t)4 * (size_t)ntext, -7);
        std::vector<qe::PanelRawHit> raw((size_t)ntext * (size_t)cap);
        qe::PanelHitsArgs A{};
        A.n_members = K; A.per_slice = K; A.nslots = ntext; A.text = text.data(); A.mode = cf.mode; A.max_hits = cap; A.part = part.data(); A.raw = raw.data();
        for (int t = 0; t < ntext; ++t) {
            const int pair = text[(size_t)t];
            if (pair < 0) continue;
            qe::PanelHitScan H;
            qe::panel_hit_scan_init(H, raw.data() + (size_t)t * (size_t)cap, cap);
            uint32_t steps = 0;
            qe::panel_text_hits<Eq>(P, 0, K, T.fwd.data() + Eq::offset(T.off[(size_t)pair]), T.len[(size_t)pair], cf.mode, H, steps);
            qe::panel_hits_store_part(A, 1, 0, t, H, steps);
            CHECK(H.found == (int32_t)cf.want[(size_t)pair].size() && H.found <= cap);
            whole[(size_t)pair].assign(raw.begin() + (ptrdiff_t)((size_t)t * (size_t)cap), raw.begin() + (ptrdiff_t)((size_t)t * (size_t)cap + (size_t)H.sink.count));
            for (int k = 0; k < H.sink.count; ++k) {
                const qe::PanelRawHit& h = whole[(size_t)pair][(size_t)k];
                const Occ& o = cf.want[(size_t)pair][(size_t)k];
                CHECK(h.pattern == o.pattern && h.end == o.end && h.score == o.score);
            }
            ++checked;
        }
    }
    // ---- the windowed stage's flow
    for (int window : {64, 128, 192, 4096}) {
        std::vector<int32_t> w_pair, w_text, w_c0, w_c1, first_slot((size_t)n, 0), nwin((size_t)n, 0);
        for (int t = 0; t < ntext; ++t) {
            const int pair = text[(size_t)t];
            if (pair < 0) continue;
            first_slot[(size_t)pair] = (int32_t)w_pair.size();
            for (int c0 = 0; c0 < T.len[(size_t)pair]; c0 += window) {
                w_pair.push_back(pair); w_text.push_back(t); w_c0.push_back(c0); w_c1.push_back(std::min(T.len[(size_t)pair], c0 + window));
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
                A.pl_m = M.fwd.data(); A.m_off = M.off.data(); A.m_len = M.len.data(); A.m_bound = bound.data();
                A.n_members = K; A.per_slice = per;
                A.pl_t = T.fwd.data(); A.pl_t_off = T.off.data(); A.t_len = T.len.data();
                A.nslots = nslots; A.text = w_pair.data(); A.w_c0 = w_c0.data(); A.w_c1 = w_c1.data(); A.max_hits = cap; A.part = part.data(); A.raw = raw.data();
                uint64_t walked = 0, owned = 0;
                for (int s = 0; s < ns; ++s)
                    for (int w = 0; w < nslots; ++w) {
                        const int pair = w_pair[(size_t)w];
                        if (pair < 0) continue;
                        qe::PanelWindowScan H;
                        qe::panel_window_scan_init(H, raw.data() + ((size_t)s * (size_t)nslots + (size_t)w) * (size_t)cap, cap, w_c0[(size_t)w], w_c1[(size_t)w]);
                        uint32_t steps = 0;
                        qe::panel_window_hits<Eq>(P, s * per, std::min(K, (s + 1) * per), A.pl_t + Eq::offset(A.pl_t_off[pair]), A.t_len[pair],
                                                  w_c0[(size_t)w], w_c1[(size_t)w], H, steps);
                        CHECK(steps > 0);
                        walked += steps; owned += (uint64_t)(w_c1[(size_t)w] - w_c0[(size_t)w]) * (uint64_t)(std::min(K, (s + 1) * per) - s * per);
                        qe::panel_scan_store_part(A, ns, s, w, H, steps);
                    }
                CHECK(walked >= owned);                          // (every owned column is walked by at least the top block)
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
                std::vector<int32_t> hits((size_t)(4 * total + 4), -7), o_pair((size_t)total + 1, -7), o_m((size_t)total + 1), o_n((size_t)total + 1),
                    o_score((size_t)total + 1), o_end((size_t)total + 1), o_start((size_t)total + 1, -1);
                std::vector<int64_t> o_plp((size_t)total + 1), o_plt((size_t)total + 1);
                qe::PanelScanExpandArgs E{};
                E.ntext = ntext; E.nslots = nslots; E.nslices = ns; E.max_hits = cap;
                E.w_pair = w_pair.data(); E.w_text = w_text.data(); E.first_slot = first_slot.data(); E.nwin = nwin.data();
                E.part = part.data(); E.raw = raw.data(); E.base = base.data(); E.off = off.data();
                E.m_len = M.len.data(); E.m_off = M.off.data(); E.t_len = T.len.data(); E.t_off = T.off.data(); E.hits = hits.data();
                E.o_pair = o_pair.data(); E.o_m = o_m.data(); E.o_n = o_n.data(); E.o_score = o_score.data(); E.o_end = o_end.data();
                E.o_plp_off = o_plp.data(); E.o_plt_off = o_plt.data();
                for (int s = ns - 1; s >= 0; --s) for (int w = nslots - 1; w >= 0; --w) qe::panel_scan_expand_lane(E, s, w);
                for (int64_t j = 0; j < total; ++j) {               // k_search<4, Eq>'s start-pass form, task j with pair = j
                    CHECK(o_pair[(size_t)j] == (int32_t)j);         // (-7: a slot no lane wrote)
                    const int m = o_m[(size_t)j], tn = o_n[(size_t)j], sc = o_score[(size_t)j], in_end = o_end[(size_t)j];
                    CHECK(sc >= 0 && in_end >= 1 && in_end <= tn);
                    qe::SearchLane L;
                    qe::search_lane_init(L, m, in_end, qe::SEARCH_PREFIX, sc, qe::SEARCH_LARGEST_END);
                    qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS, Eq> R;
                    for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { R.pv[b] = R.mv[b] = 0; R.s[b] = 0; }
                    R.load(M.rev.data() + Eq::offset(o_plp[(size_t)j]), m);
                    qe::search_run<qe::QE_SEARCH_REG_BLOCKS>(R, L, T.rev.data() + Eq::offset(o_plt[(size_t)j]), (int64_t)tn - in_end);
                    int32_t score, end;
                    qe::search_answer(L, score, end);
                    o_start[(size_t)j] = score == sc ? in_end - end : -1;
                }
                for (int64_t j = 0; j < total; ++j) qe::panel_hits_finish_one(j, o_start.data(), hits.data());
                CHECK(hits[(size_t)(4 * total)] == -7);
                for (int i = 0; i < n; ++i) {
                    const std::vector<Occ>& w = cf.want[(size_t)i];
                    const int32_t stored = (int32_t)std::min<size_t>(w.size(), (size_t)cap);
                    int32_t wbest = -1;
                    for (const Occ& o : w) wbest = (wbest < 0 || o.score < wbest) ? o.score : wbest;
                    if (found[(size_t)i] != (int32_t)w.size() || off[(size_t)i + 1] - off[(size_t)i] != stored || best[(size_t)i] != wbest)
                        fprintf(stderr, "flag %d uniform %d window %d cap %d slices %d text %d: found %d stored %lld best %d, expected %zu %d %d\n", cf.flag,
                                cf.uniform, window, cap, ns, i, found[(size_t)i], (long long)(off[(size_t)i + 1] - off[(size_t)i]), best[(size_t)i], w.size(), stored, wbest);
                    CHECK(found[(size_t)i] == (int32_t)w.size() && off[(size_t)i + 1] - off[(size_t)i] == stored && best[(size_t)i] == wbest);
                    for (int k = 0; k < stored; ++k) {
                        const int32_t* h = hits.data() + 4 * (off[(size_t)i] + k);
                        const Occ& o = w[(size_t)k];
                        const qe::PanelRawHit& u = whole[(size_t)i][(size_t)k];
                        if (h[0] != o.pattern || h[1] != o.start || h[2] != o.end || h[3] != o.score)
                            fprintf(stderr, "flag %d uniform %d window %d cap %d slices %d text %d occurrence %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n",
                                    cf.flag, cf.uniform, window, cap, ns, i, k, h[0], h[1], h[2], h[3], o.pattern, o.start, o.end, o.score);
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
    int K = 0, n = 0, nconf = 0;
    f >> K >> n >> nconf;
    CHECK(!f.fail() && K >= 1 && n >= 1 && nconf >= 1);
    std::vector<std::string> panel((size_t)K), texts((size_t)n);
    std::vector<int32_t> own((size_t)K);
    for (int p = 0; p < K; ++p) f >> panel[(size_t)p] >> own[(size_t)p];
    for (int i = 0; i < n; ++i) { f >> texts[(size_t)i]; if (texts[(size_t)i] == ".") texts[(size_t)i].clear(); }
    long checked = 0;
    for (int c = 0; c < nconf; ++c) {
        Conf cf;
        f >> cf.mode >> cf.flag >> cf.uniform;
        cf.want.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            int found = 0;
            f >> found;
            cf.want[(size_t)i].resize((size_t)found);
            for (Occ& o : cf.want[(size_t)i]) f >> o.pattern >> o.start >> o.end >> o.score;
        }
        CHECK(!f.fail());
        checked += cf.flag ? run_conf<qe::SearchEqIupac>(cf, panel, own, texts) : run_conf<qe::SearchEq3>(cf, panel, own, texts);
    }
    printf("cases ok %ld\n", checked);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "cases")) return cases(argv[2]);
    fprintf(stderr, "usage: panel_scan_cpu cases <file>\n");
    return 2;
}
