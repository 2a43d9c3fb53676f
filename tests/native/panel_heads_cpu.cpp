// panel_heads_cpu.cpp -- the 5' heads of the panel search (QUICKED_PANEL_HEADS) compiled for the host: panel_head_chunk,
// panel_member_heads, panel_text_heads, the tails' walk and keeper behind them and the per-slot bodies of
// quicked_amd/csrc/qe_panel.h -- the very source k_panel_heads, k_panel_heads_merge, k_panel_head_planes and
// k_panel_heads_finish run per lane -- driven through the stage's steps.  A stand-alone program, built by
// tests/test_panel_heads_cpu.py once plain and once with -fsanitize=address,undefined.
//
// panel_heads_cpu cases <file>     the groups of tests/test_panel_heads_cpu.py against the heads it computed with
//                                  tests/panel_heads_lib.py; prints "cases ok <n checked> short <n> cut <n>"
//   file: ngroups / per group: K n nconf / K x {member bound} / n x text ("." = empty) / nconf x { flag min_overlap,
//         n x {pattern overlap text_end score} }
// Per group and configuration:
//   * the backward chunk reader against the reversed text's own planes, at every column count of every text's start;
//   * per text the sweep, walk and keeper over every member in the register store of NB = 1, 2 and 4 blocks (every member that
//     fits the form; the rest in four), against the text's {pattern, overlap, score}, with the block steps within the short
//     sweep's bound blocks(m) min(n, m + k); `short` counts the walks that found a head while the lane's live blocks stopped
//     short of the member's last block, `cut` the sweeps that stopped before the text did;
//   * per slice count (1, 2, K): the sweep over slots x slices (panel_text_heads, the store_part body), the merge body, the
//     planes body, the end pass with k_search's stand-in arithmetic over the register store of four blocks, then the finish
//     body: all four fields of every text.
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

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "panel_heads_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

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

struct Head { int32_t pattern, overlap, end, score; };
struct Conf { int flag, min_overlap; std::vector<Head> want; };
struct Group { std::vector<std::string> panel, texts; std::vector<int32_t> bound; std::vector<Conf> confs; };

static long g_short = 0, g_cut = 0;

// the backward reader: sweep columns [col0, col0 + ncols) over text[0:c0) are columns [col0, ..) of the planes of that start
// reversed, whatever the split into chunks
template <class Eq>
static void reader_by_hand(const std::string& text, bool acgt, const uint64_t* tp) {
    const int n = (int)text.size();
    for (int c0 = 1; c0 <= n; c0 = c0 < 200 ? c0 + 1 : c0 + 61) {
        const std::vector<uint64_t> ref = Planes<Eq>::of(text.substr(0, (size_t)c0), true, acgt);
        for (int col0 = 0; col0 < c0;) {
            const int ncols = col0 ? 64 : ((c0 - 1) & 63) + 1;
            uint64_t t[Eq::W], want[Eq::W];
            qe::panel_head_chunk<Eq>(tp, c0, col0, ncols, t);
            qe::search_text_words<Eq::W>(ref.data(), col0, ncols, want);
            for (int k = 0; k < Eq::W; ++k) CHECK(t[k] == (ncols < 64 ? want[k] & (((uint64_t)1 << ncols) - 1) : want[k]));
            col0 += ncols;
        }
        // ... and at an offset that is no word boundary
        if (c0 > 70) {
            uint64_t t[Eq::W], want[Eq::W];
            qe::panel_head_chunk<Eq>(tp, c0, 5, 37, t);
            qe::search_text_words<Eq::W>(ref.data(), 5, 37, want);
            for (int k = 0; k < Eq::W; ++k) CHECK(t[k] == (want[k] & (((uint64_t)1 << 37) - 1)));
        }
    }
}

// one member (pp: its reversed planes) against the start of one text in the register store of NB blocks
template <int NB, class Eq>
static void member_by_hand(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int min_overlap, int p, qe::PanelTailKeeper& keep, uint32_t& rows) {
    qe::PanelTailKeeper mine;
    mine.init();
    uint32_t steps = 0;
    qe::panel_member_heads<NB, Eq>(pp, m, bound, tp, n, min_overlap, p, mine, steps, rows);
    const int reach = m + qe::search_effective(bound, m);
    CHECK(steps <= (uint32_t)(qe::search_blocks(m) * std::min(n, reach)) && (n == 0 || steps >= (uint32_t)std::min(n, reach)));
    if (reach < n) ++g_cut;
    if (mine.p >= 0 && steps < (uint32_t)(qe::search_blocks(m) * std::min(n, reach))) ++g_short;
    keep.merge(mine);
}

template <class Eq>
static long run_conf(const Group& G, const Conf& cf) {
    const int K = (int)G.panel.size(), n = (int)G.texts.size();
    Pool<Eq> M, T;
    for (int p = 0; p < K; ++p) M.add(G.panel[(size_t)p], false);
    for (int i = 0; i < n; ++i) T.add(G.texts[(size_t)i], cf.flag == 32);
    M.fwd.push_back(0); M.rev.push_back(0); T.fwd.push_back(0); T.rev.push_back(0);      // (data() of an all-empty pool)
    long checked = 0;
    int tallest = 1;
    for (int p = 0; p < K; ++p) tallest = std::max(tallest, qe::search_blocks(M.len[(size_t)p]));
    // ---- the reader (once per equality and text set: the first min_overlap of the file)
    if (cf.min_overlap == 1)
        for (int i = 0; i < n; ++i) reader_by_hand<Eq>(G.texts[(size_t)i], cf.flag == 32, T.fwd.data() + Eq::offset(T.off[(size_t)i]));
    // ---- the sweep, the walk and the keeper by hand, every register form
    for (int form : {1, 2, 4})
        for (int i = 0; i < n; ++i) {
            qe::PanelTailKeeper keep;
            keep.init();
            uint32_t rows = 0;
            const uint64_t* tp = T.fwd.data() + Eq::offset(T.off[(size_t)i]);
            for (int p = 0; p < K; ++p) {
                const int m = M.len[(size_t)p], nb = qe::search_blocks(m);
                const uint64_t* pp = M.rev.data() + Eq::offset(M.off[(size_t)p]);
                if (form == 1 && nb <= 1) member_by_hand<1, Eq>(pp, m, G.bound[(size_t)p], tp, T.len[(size_t)i], cf.min_overlap, p, keep, rows);
                else if (form <= 2 && nb <= 2) member_by_hand<2, Eq>(pp, m, G.bound[(size_t)p], tp, T.len[(size_t)i], cf.min_overlap, p, keep, rows);
                else member_by_hand<4, Eq>(pp, m, G.bound[(size_t)p], tp, T.len[(size_t)i], cf.min_overlap, p, keep, rows);
            }
            const Head& w = cf.want[(size_t)i];
            if (keep.p != w.pattern || keep.r != w.overlap || keep.d != w.score)
                fprintf(stderr, "flag %d min_overlap %d form %d text %d: got {%d, %d, %d}, expected {%d, %d, %d}\n", cf.flag, cf.min_overlap, form, i, keep.p, keep.r, keep.d,
                        w.pattern, w.overlap, w.score);
            CHECK(keep.p == w.pattern && keep.r == w.overlap && keep.d == w.score);
            CHECK(G.texts[(size_t)i].empty() ? rows == 0 : true);
            ++checked;
        }
    // ---- the stage's flow
    std::vector<int32_t> text;
    for (int i = 0; i < n; ++i) if (!G.texts[(size_t)i].empty()) text.push_back(i);
    while (text.size() % 64) text.push_back(-1);
    const int nslots = (int)text.size();
    for (int want_slices : {1, 2, K}) {
        const int per = (K + want_slices - 1) / want_slices, ns = (K + per - 1) / per;
        std::vector<int32_t> hpart((size_t)5 * (size_t)ns * (size_t)nslots, -7);
        qe::PanelHeadsArgs A{};
        A.pl_m = M.rev.data(); A.m_off = M.off.data(); A.m_len = M.len.data(); A.m_bound = G.bound.data();
        A.n_members = K; A.per_slice = per;
        A.pl_t = T.fwd.data(); A.pl_t_off = T.off.data(); A.t_len = T.len.data();
        A.nslots = nslots; A.text = text.data(); A.min_overlap = cf.min_overlap; A.hpart = hpart.data();
        qe::PanelView P;
        P.pl = A.pl_m; P.off = A.m_off; P.len = A.m_len; P.bound = A.m_bound;
        uint64_t all_steps = 0, all_rows = 0;
        for (int s = 0; s < ns; ++s)
            for (int t = 0; t < nslots; ++t) {
                const int pair = text[(size_t)t];
                if (pair < 0) continue;
                const uint64_t* tp = A.pl_t + Eq::offset(A.pl_t_off[pair]);
                qe::PanelTailKeeper keep;
                keep.init();
                uint32_t steps = 0, rows = 0;
                qe::panel_text_heads<Eq>(P, s * per, std::min(K, (s + 1) * per), tp, A.t_len[pair], cf.min_overlap, keep, steps, rows);
                CHECK(steps > 0);
                all_steps += steps; all_rows += rows;
                qe::panel_heads_store_part(A, ns, s, t, keep, rows, steps);
            }
        std::vector<int32_t> heads((size_t)4 * (size_t)n, -1), o_pair((size_t)nslots, -7), o_m((size_t)nslots), o_n((size_t)nslots), o_score((size_t)nslots),
            o_end((size_t)nslots), o_start((size_t)nslots, -1);
        std::vector<uint32_t> o_rows((size_t)nslots, 0), o_steps((size_t)nslots, 0);
        std::vector<int64_t> o_plp((size_t)n, 0);
        qe::PanelHeadsMergeArgs Mg{};
        Mg.nslots = nslots; Mg.nslices = ns; Mg.text = text.data(); Mg.hpart = hpart.data(); Mg.t_len = T.len.data();
        Mg.plane_stride = 3 * (int64_t)(tallest + 2);
        Mg.heads = heads.data(); Mg.o_rows = o_rows.data(); Mg.o_steps = o_steps.data();
        Mg.o_pair = o_pair.data(); Mg.o_m = o_m.data(); Mg.o_n = o_n.data(); Mg.o_score = o_score.data(); Mg.o_end = o_end.data(); Mg.o_plp_off = o_plp.data();
        for (int t = 0; t < nslots; ++t) qe::panel_heads_merge_slot(Mg, t);
        uint64_t got_steps = 0, got_rows = 0;
        for (int t = 0; t < nslots; ++t) { got_steps += o_steps[(size_t)t]; got_rows += o_rows[(size_t)t]; }
        CHECK(got_steps == all_steps && got_rows == all_rows);
        std::vector<uint64_t> pool((size_t)Eq::offset(Mg.plane_stride) * (size_t)nslots + 1, 0xA5A5A5A5A5A5A5A5ull);      // (stale words, as a scratch pool has)
        qe::PanelHeadPlanesArgs W{};
        W.nslots = nslots; W.o_pair = o_pair.data(); W.heads = heads.data();
        W.pl_m = M.fwd.data(); W.m_off = M.off.data(); W.m_len = M.len.data(); W.o_plp_off = o_plp.data(); W.pool = pool.data();
        for (int t = 0; t < nslots; ++t) qe::panel_head_planes_slot<Eq>(W, t);
        CHECK(pool.back() == 0xA5A5A5A5A5A5A5A5ull);
        for (int t = 0; t < nslots; ++t) {                 // k_search<4, Eq>'s start-pass form over the slots
            const int pair = o_pair[(size_t)t];
            CHECK(pair == -1 || pair == text[(size_t)t]);
            if (pair < 0) continue;
            const int m = o_m[(size_t)t], tn = o_n[(size_t)t], sc = o_score[(size_t)t], in_end = o_end[(size_t)t];
            CHECK(m >= 1 && sc >= 0 && in_end >= 1 && in_end == tn && tn <= T.len[(size_t)pair]);
            // the planes are the packer's of the member's last m bases, zeros behind
            const std::string& q = G.panel[(size_t)heads[4 * (size_t)pair]];
            const std::vector<uint64_t> ref = Planes<Eq>::of(q.substr(q.size() - (size_t)m), false, false);
            const uint64_t* got = pool.data() + Eq::offset(o_plp[(size_t)pair]);
            for (size_t k = 0; k < ref.size(); ++k) CHECK(got[k] == ref[k]);
            for (size_t k = ref.size(); k < ref.size() + 2 * (size_t)Eq::W; ++k) CHECK(got[k] == 0);
            qe::SearchLane L;
            qe::search_lane_init(L, m, in_end, qe::SEARCH_PREFIX, sc, qe::SEARCH_LARGEST_END);
            qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS, Eq> R;
            for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { R.pv[b] = R.mv[b] = 0; R.s[b] = 0; }
            R.load(got, m);
            qe::search_run<qe::QE_SEARCH_REG_BLOCKS>(R, L, T.fwd.data() + Eq::offset(T.off[(size_t)pair]), (int64_t)tn - in_end);
            int32_t score, end;
            qe::search_answer(L, score, end);
            o_start[(size_t)t] = score == sc ? in_end - end : -1;
        }
        for (int t = 0; t < nslots; ++t) qe::panel_heads_finish_slot(t, o_pair.data(), o_start.data(), heads.data());
        for (int i = 0; i < n; ++i) {
            const int32_t* h = heads.data() + 4 * (size_t)i;
            const Head& w = cf.want[(size_t)i];
            if (h[0] != w.pattern || h[1] != w.overlap || h[2] != w.end || h[3] != w.score)
                fprintf(stderr, "flag %d min_overlap %d slices %d text %d: got {%d, %d, %d, %d}, expected {%d, %d, %d, %d}\n", cf.flag, cf.min_overlap, ns, i, h[0], h[1],
                        h[2], h[3], w.pattern, w.overlap, w.end, w.score);
            CHECK(h[0] == w.pattern && h[1] == w.overlap && h[2] == w.end && h[3] == w.score);
            ++checked;
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
    for (int g = 0; g < ngroups; ++g) {
        int K = 0, n = 0, nconf = 0;
        f >> K >> n >> nconf;
        CHECK(!f.fail() && K >= 1 && n >= 1 && nconf >= 1);
        Group G;
        G.panel.resize((size_t)K); G.texts.resize((size_t)n); G.bound.resize((size_t)K);
        for (int p = 0; p < K; ++p) f >> G.panel[(size_t)p] >> G.bound[(size_t)p];
        for (int i = 0; i < n; ++i) { f >> G.texts[(size_t)i]; if (G.texts[(size_t)i] == ".") G.texts[(size_t)i].clear(); }
        for (int c = 0; c < nconf; ++c) {
            Conf cf;
            f >> cf.flag >> cf.min_overlap;
            cf.want.resize((size_t)n);
            for (Head& t : cf.want) f >> t.pattern >> t.overlap >> t.end >> t.score;
            CHECK(!f.fail());
            checked += cf.flag ? run_conf<qe::SearchEqIupac>(G, cf) : run_conf<qe::SearchEq3>(G, cf);
        }
    }
    printf("cases ok %ld short %ld cut %ld\n", checked, g_short, g_cut);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "cases")) return cases(argv[2]);
    fprintf(stderr, "usage: panel_heads_cpu cases <file>\n");
    return 2;
}
