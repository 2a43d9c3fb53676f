// panel_hits_cpu.cpp -- the all-occurrences panel search compiled for the host: SearchHitScanOf, panel_text_hits and the
// per-slot bodies of quicked_amd/csrc/qe_panel.h / qe_search.h -- the very source k_panel_hits, k_panel_hits_count,
// k_panel_hits_expand and k_panel_hits_finish run per lane -- driven through the stage's steps.  A stand-alone program, built by
// tests/test_panel_hits_cpu.py once plain and once with -fsanitize=address,undefined.
//
// panel_hits_cpu cases <file>      the cases of tests/test_panel_hits_cpu.py against the lists it computed with
//                                  tests/panel_hits_lib.py; prints "cases ok <n checked>"
//   file: K n nconf / K x {member bound} / n x text ("." = empty) / nconf x { mode flag uniform(-1: the members' own bounds),
//         n x {found, found x {pattern text_start text_end score}} }
// Per configuration:
//   * per (text, member) the generalised scan with its default {end, score} sink, as k_search_hits runs it, against the
//     member's part of the list (the answers tests/native/search_hits_cpu.cpp checks the same way);
//   * per cap (1, 2, 4096) and slice count (1, 2, K): the forward pass over slots x slices (panel_text_hits,
//     panel_hits_store_part), the count body, the offset scan, the expand body and -- INFIX -- the start pass with k_search's
//     stand-in arithmetic over the register store of four blocks with task j's pair = j, then the finish body: found, stored,
//     the smallest score and every stored record against the list's first `cap`.
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

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "panel_hits_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

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
    const bool infix = cf.mode == qe::SEARCH_INFIX;
    Pool<Eq> M, T;
    std::vector<int32_t> bound((size_t)K);
    for (int p = 0; p < K; ++p) { M.add(panel[(size_t)p], false); bound[(size_t)p] = cf.uniform >= 0 ? cf.uniform : own[(size_t)p]; }
    for (int i = 0; i < n; ++i) T.add(texts[(size_t)i], cf.flag == 32);
    M.fwd.push_back(0); M.rev.push_back(0); T.fwd.push_back(0); T.rev.push_back(0);      // (data() of an all-empty pool)
    long checked = 0;
    // ---- the generalised scan with its default sink, pair by pair
    for (int i = 0; i < n; ++i)
        for (int p = 0; p < K && !texts[(size_t)i].empty(); ++p) {
            const int m = M.len[(size_t)p];
            std::vector<qe::SearchHit> out(64);
            qe::SearchLane L;
            qe::search_lane_init(L, m, T.len[(size_t)i], cf.mode, bound[(size_t)p], 0);
            qe::SearchHitScan H;
            H.init(L, out.data(), 1, (int32_t)out.size());
            qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS, Eq> R;
            for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { R.pv[b] = R.mv[b] = 0; R.s[b] = 0; }
            R.load(M.fwd.data() + Eq::offset(M.off[(size_t)p]), m);
            qe::search_run_hits<qe::QE_SEARCH_REG_BLOCKS>(R, L, H, T.fwd.data() + Eq::offset(T.off[(size_t)i]), 0);
            std::vector<Occ> mine;
            for (const Occ& o : cf.want[(size_t)i]) if (o.pattern == p) mine.push_back(o);
            CHECK(H.found == (int32_t)mine.size() && H.sink.count == std::min<int32_t>(H.found, 64));
            int32_t best = -1;
            for (const Occ& o : mine) best = (best < 0 || o.score < best) ? o.score : best;
            CHECK(H.best == best);
            for (int k = 0; k < H.sink.count; ++k) CHECK(out[(size_t)k].end == mine[(size_t)k].end && out[(size_t)k].score == mine[(size_t)k].score);
            ++checked;
        }
    // ---- the stage's flow
    std::vector<int32_t> text;
    for (int i = 0; i < n; ++i) if (!texts[(size_t)i].empty()) text.push_back(i);
    while (text.size() % 64) text.push_back(-1);
    const int nslots = (int)text.size();
    for (int cap : {1, 2, 4096})
        for (int want_slices : {1, 2, K}) {
            const int per = (K + want_slices - 1) / want_slices, ns = (K + per - 1) / per;
            std::vector<int32_t> part((size_t)4 * (size_t)ns * (size_t)nslots, -7);
            std::vector<qe::PanelRawHit> raw((size_t)ns * (size_t)nslots * (size_t)cap);
            qe::PanelHitsArgs A{};
            A.pl_m = M.fwd.data(); A.m_off = M.off.data(); A.m_len = M.len.data(); A.m_bound = bound.data();
            A.n_members = K; A.per_slice = per;
            A.pl_t = T.fwd.data(); A.pl_t_off = T.off.data(); A.t_len = T.len.data();
            A.nslots = nslots; A.text = text.data(); A.mode = cf.mode; A.max_hits = cap; A.part = part.data(); A.raw = raw.data();
            qe::PanelView P;
            P.pl = A.pl_m; P.off = A.m_off; P.len = A.m_len; P.bound = A.m_bound;
            for (int s = 0; s < ns; ++s)
                for (int t = 0; t < nslots; ++t) {
                    const int pair = text[(size_t)t];
                    if (pair < 0) continue;
                    qe::PanelHitScan H;
                    qe::panel_hit_scan_init(H, raw.data() + ((size_t)s * (size_t)nslots + (size_t)t) * (size_t)cap, cap);
                    uint32_t steps = 0;
                    qe::panel_text_hits<Eq>(P, s * per, std::min(K, (s + 1) * per), A.pl_t + Eq::offset(A.pl_t_off[pair]), A.t_len[pair], cf.mode, H, steps);
                    CHECK(steps > 0);
                    qe::panel_hits_store_part(A, ns, s, t, H, steps);
                }
            std::vector<int32_t> found((size_t)n, 0), best((size_t)n, -1), len((size_t)n, -1);
            std::vector<uint32_t> adv((size_t)nslots, 0);
            qe::PanelHitsCountArgs Cn{};
            Cn.nslots = nslots; Cn.nslices = ns; Cn.max_hits = cap; Cn.text = text.data(); Cn.part = part.data();
            Cn.found = found.data(); Cn.best = best.data(); Cn.len = len.data(); Cn.o_adv = adv.data();
            for (int t = 0; t < nslots; ++t) qe::panel_hits_count_slot(Cn, t);
            std::vector<int64_t> off((size_t)n + 1, 0);
            for (int i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + len[(size_t)i] + 1;      // k_scan_offsets
            const int64_t total = off[(size_t)n];
            std::vector<int32_t> hits((size_t)(4 * total + 4), -7), o_pair((size_t)total + 1, -7), o_m((size_t)total + 1), o_n((size_t)total + 1),
                o_score((size_t)total + 1), o_end((size_t)total + 1), o_start((size_t)total + 1, -1);
            std::vector<int64_t> o_plp((size_t)total + 1), o_plt((size_t)total + 1);
            qe::PanelHitsExpandArgs E{};
            E.nslots = nslots; E.nslices = ns; E.max_hits = cap; E.infix = infix ? 1 : 0;
            E.text = text.data(); E.part = part.data(); E.raw = raw.data(); E.off = off.data();
            E.m_len = M.len.data(); E.m_off = M.off.data(); E.t_len = T.len.data(); E.t_off = T.off.data(); E.hits = hits.data();
            if (infix) { E.o_pair = o_pair.data(); E.o_m = o_m.data(); E.o_n = o_n.data(); E.o_score = o_score.data(); E.o_end = o_end.data(); E.o_plp_off = o_plp.data(); E.o_plt_off = o_plt.data(); }
            for (int t = 0; t < nslots; ++t) qe::panel_hits_expand_slot(E, t);
            if (infix) {
                for (int64_t j = 0; j < total; ++j) {               // k_search<4, Eq>'s start-pass form, task j with pair = j
                    CHECK(o_pair[(size_t)j] == (int32_t)j);
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
            }
            for (int i = 0; i < n; ++i) {
                const std::vector<Occ>& w = cf.want[(size_t)i];
                const int32_t stored = (int32_t)std::min<size_t>(w.size(), (size_t)cap);
                int32_t wbest = -1;
                for (const Occ& o : w) wbest = (wbest < 0 || o.score < wbest) ? o.score : wbest;
                if (found[(size_t)i] != (int32_t)w.size() || off[(size_t)i + 1] - off[(size_t)i] != stored || best[(size_t)i] != wbest)
                    fprintf(stderr, "mode %d flag %d uniform %d cap %d slices %d text %d: found %d stored %lld best %d, expected %zu %d %d\n", cf.mode, cf.flag,
                            cf.uniform, cap, ns, i, found[(size_t)i], (long long)(off[(size_t)i + 1] - off[(size_t)i]), best[(size_t)i], w.size(), stored, wbest);
                CHECK(found[(size_t)i] == (int32_t)w.size() && off[(size_t)i + 1] - off[(size_t)i] == stored && best[(size_t)i] == wbest);
                for (int k = 0; k < stored; ++k) {
                    const int32_t* h = hits.data() + 4 * (off[(size_t)i] + k);
                    const Occ& o = w[(size_t)k];
                    if (h[0] != o.pattern || h[1] != o.start || h[2] != o.end || h[3] != o.score)
                        fprintf(stderr, "mode %d flag %d uniform %d cap %d slices %d text %d occurrence %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n", cf.mode,
                                cf.flag, cf.uniform, cap, ns, i, k, h[0], h[1], h[2], h[3], o.pattern, o.start, o.end, o.score);
                    CHECK(h[0] == o.pattern && h[1] == o.start && h[2] == o.end && h[3] == o.score);
                    ++checked;
                }
                ++checked;
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
    fprintf(stderr, "usage: panel_hits_cpu cases <file>\n");
    return 2;
}
