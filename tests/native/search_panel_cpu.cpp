// search_panel_cpu.cpp -- panel search compiled for the host: the keeper, panel_text and panel_start_task of
// quicked_amd/csrc/qe_panel.h -- the very source k_search_panel and k_panel_reduce run per lane -- driven text by text through
// the stage's steps.  A stand-alone program, built by tests/test_search_panel_cpu.py once plain and once with
// -fsanitize=address,undefined.
//
// search_panel_cpu keeper             take() against a sort, merge() associative, commutative and equal to one pass, over random
//                                     key lists with ties; prints "keeper ok"
// search_panel_cpu blocks             the register store of four blocks holds zero planes for the blocks a member of 1, 64, 65 or
//                                     256 bases does not have, under both equalities (what the start pass relies on); "blocks ok"
// search_panel_cpu cases <file>       the cases of tests/test_search_panel_cpu.py against the expectations it computed with
//                                     tests/panel_lib.py; prints "cases ok <n checked>"
//   file: K n nconf / K x {member bound} / n x text ("." = empty) / nconf x { mode flag uniform(-1: the members' own bounds),
//         n x {6 hit fields, K scores, K ends} }
// Per configuration and text: panel_text over the member range cut into 1, 2 and K slices, the slices' keepers merged in
// two groupings; the matrix panel_text leaves; for INFIX panel_start_task and the start pass with k_search's stand-in
// arithmetic over the register store of four blocks, whatever the member's length.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "qe_panel.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "search_panel_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

using qe::PanelKeeper;

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
    return std::vector<uint64_t>(full.begin(), full.end());      // a tight allocation: exactly the rows of the sequence
}
template <class Eq> struct Planes;
template <> struct Planes<qe::SearchEq3> { static std::vector<uint64_t> of(const std::string& s, bool rev, bool) { return planes3_of(s, rev); } };
template <> struct Planes<qe::SearchEqIupac> { static std::vector<uint64_t> of(const std::string& s, bool rev, bool acgt) { return planes4_of(s, rev, acgt); } };

// ---- the keeper
static bool same(const PanelKeeper& a, const PanelKeeper& b) {
    return a.p1 == b.p1 && a.s1 == b.s1 && a.p2 == b.p2 && a.s2 == b.s2 && (a.p1 < 0 || a.e1 == b.e1);
}
static int keeper() {
    std::mt19937 rng(12345);
    for (int round = 0; round < 4000; ++round) {
        const int len = (int)(rng() % 9);
        std::vector<int> member((size_t)len), score((size_t)len);
        std::vector<int> ids(40);
        for (int i = 0; i < 40; ++i) ids[(size_t)i] = i;
        std::shuffle(ids.begin(), ids.end(), rng);
        for (int i = 0; i < len; ++i) { member[(size_t)i] = ids[(size_t)i]; score[(size_t)i] = (int)(rng() % 3); }      // many ties
        // one pass, in this (arbitrary) order
        PanelKeeper one;
        one.init();
        for (int i = 0; i < len; ++i) one.take(member[(size_t)i], score[(size_t)i], 1000 + member[(size_t)i]);
        one.take(-1, 0, 0);                                       // "nothing" changes nothing
        std::vector<std::pair<int, int>> keys;
        for (int i = 0; i < len; ++i) keys.push_back({score[(size_t)i], member[(size_t)i]});
        std::sort(keys.begin(), keys.end());
        CHECK(one.p1 == (len > 0 ? keys[0].second : -1) && one.s1 == (len > 0 ? keys[0].first : -1));
        CHECK(one.p2 == (len > 1 ? keys[1].second : -1) && one.s2 == (len > 1 ? keys[1].first : -1));
        CHECK(len == 0 || one.e1 == 1000 + one.p1);
        // three slices at random cuts, merged in both groupings and in reverse
        const int c1 = len ? (int)(rng() % (unsigned)(len + 1)) : 0, c2 = c1 + (len - c1 ? (int)(rng() % (unsigned)(len - c1 + 1)) : 0);
        PanelKeeper a, b, c;
        a.init(); b.init(); c.init();
        for (int i = 0; i < c1; ++i) a.take(member[(size_t)i], score[(size_t)i], 1000 + member[(size_t)i]);
        for (int i = c1; i < c2; ++i) b.take(member[(size_t)i], score[(size_t)i], 1000 + member[(size_t)i]);
        for (int i = c2; i < len; ++i) c.take(member[(size_t)i], score[(size_t)i], 1000 + member[(size_t)i]);
        PanelKeeper ab = a; ab.merge(b); ab.merge(c);             // (a + b) + c
        PanelKeeper bc = b; bc.merge(c);
        PanelKeeper a_bc = a; a_bc.merge(bc);                     // a + (b + c)
        PanelKeeper rev = c; rev.merge(b); rev.merge(a);          // c + b + a
        CHECK(same(ab, one) && same(a_bc, one) && same(rev, one));
    }
    printf("keeper ok\n");
    return 0;
}

// ---- absent blocks of the four-block register store
template <class Eq>
static void blocks_of() {
    for (int m : {1, 64, 65, 256}) {
        const std::string s((size_t)m, 'G');
        const std::vector<uint64_t> pp = Planes<Eq>::of(s, false, false);      // tight: reading a block the member lacks is out of bounds
        qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS, Eq> R;
        R.load(pp.data(), m);
        for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) {
            uint64_t any = 0;
            for (int k = 0; k < Eq::W; ++k) any |= R.pl[b][k];
            CHECK((b < (m + 63) / 64) == (any != 0));
        }
    }
}

// ---- the cases
struct Conf { int mode, flag, uniform; std::vector<std::vector<int32_t>> want; };

template <class Eq>
static long run_conf(const Conf& cf, const std::vector<std::string>& panel, const std::vector<int32_t>& own, const std::vector<std::string>& texts) {
    const int K = (int)panel.size();
    const bool text_acgt = cf.flag == 32;
    // the panel's planes, forward and reversed, member after member without padding rows
    std::vector<uint64_t> fwd, rev;
    std::vector<int64_t> off((size_t)K);
    std::vector<int32_t> len((size_t)K), bound((size_t)K);
    for (int p = 0; p < K; ++p) {
        const std::vector<uint64_t> f = Planes<Eq>::of(panel[(size_t)p], false, false), r = Planes<Eq>::of(panel[(size_t)p], true, false);
        off[(size_t)p] = (int64_t)(fwd.size() / Eq::W) * 3;             // three-plane offsets: Eq::offset maps them
        fwd.insert(fwd.end(), f.begin(), f.end()); rev.insert(rev.end(), r.begin(), r.end());
        len[(size_t)p] = (int32_t)panel[(size_t)p].size();
        bound[(size_t)p] = cf.uniform >= 0 ? cf.uniform : own[(size_t)p];
    }
    qe::PanelView P;
    P.pl = fwd.data(); P.off = off.data(); P.len = len.data(); P.bound = bound.data();
    long checked = 0;
    for (size_t i = 0; i < texts.size(); ++i) {
        const std::string& t = texts[i];
        const int n = (int)t.size();
        const std::vector<int32_t>& want = cf.want[i];
        const std::vector<uint64_t> tp = Planes<Eq>::of(t, false, text_acgt);
        PanelKeeper got;
        got.init();
        for (int nslices : {1, 2, K}) {
            const int per = (K + nslices - 1) / nslices, ns = (K + per - 1) / per;
            std::vector<PanelKeeper> part((size_t)ns);
            std::vector<int32_t> ms((size_t)K, -7), me((size_t)K, -7);
            uint32_t steps = 0;
            for (int s = 0; s < ns; ++s) {
                part[(size_t)s].init();
                qe::panel_text<Eq>(P, s * per, std::min(K, (s + 1) * per), tp.data(), n, cf.mode, part[(size_t)s], steps, ms.data(), me.data());
            }
            PanelKeeper left, right;                             // merged from the left, and from the right
            left.init(); right.init();
            for (int s = 0; s < ns; ++s) left.merge(part[(size_t)s]);
            for (int s = ns - 1; s >= 0; --s) right.merge(part[(size_t)s]);
            CHECK(same(left, right));
            if (nslices > 1) CHECK(same(left, got));
            got = left;
            CHECK(n == 0 || steps > 0);
            for (int p = 0; p < K; ++p) {                        // the matrix
                if (ms[(size_t)p] != want[(size_t)(6 + p)] || me[(size_t)p] != want[(size_t)(6 + K + p)])
                    fprintf(stderr, "mode %d flag %d text %zu member %d: got {%d, %d}, expected {%d, %d}\n", cf.mode, cf.flag, i, p, ms[(size_t)p], me[(size_t)p],
                            want[(size_t)(6 + p)], want[(size_t)(6 + K + p)]);
                CHECK(ms[(size_t)p] == want[(size_t)(6 + p)] && me[(size_t)p] == want[(size_t)(6 + K + p)]);
                ++checked;
            }
        }
        // text_start: PREFIX 0; INFIX the start pass of the best member, as k_search's stand-in runs a task with in_score
        int32_t start = got.p1 >= 0 ? 0 : -1;
        if (got.p1 >= 0 && cf.mode == qe::SEARCH_INFIX) {
            const int m = len[(size_t)got.p1];
            int32_t task_n, in_end, base;
            qe::panel_start_task(m, n, got.e1, got.s1, task_n, in_end, base);
            CHECK(in_end >= 1 && in_end <= task_n && task_n <= n);
            const std::vector<uint64_t> tr = Planes<Eq>::of(t, true, text_acgt);
            qe::SearchLane L;
            qe::search_lane_init(L, m, in_end, qe::SEARCH_PREFIX, got.s1, qe::SEARCH_LARGEST_END);
            qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS, Eq> R;
            for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { R.pv[b] = R.mv[b] = 0; R.s[b] = 0; }
            R.load(rev.data() + Eq::offset(off[(size_t)got.p1]), m);
            qe::search_run<qe::QE_SEARCH_REG_BLOCKS>(R, L, tr.data(), (int64_t)task_n - in_end);
            int32_t score, end;
            qe::search_answer(L, score, end);
            start = score == got.s1 ? base + (in_end - end) : -99;
        }
        const int32_t have[6] = {got.p1, got.s1, start, got.e1, got.p2, got.s2};
        for (int f = 0; f < 6; ++f) {
            if (have[f] != want[(size_t)f])
                fprintf(stderr, "mode %d flag %d uniform %d text %zu field %d: got %d, expected %d\n", cf.mode, cf.flag, cf.uniform, i, f, have[f], want[(size_t)f]);
            CHECK(have[f] == want[(size_t)f]);
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
        cf.want.assign((size_t)n, std::vector<int32_t>((size_t)(6 + 2 * K)));
        for (int i = 0; i < n; ++i) for (int k = 0; k < 6 + 2 * K; ++k) f >> cf.want[(size_t)i][(size_t)k];
        CHECK(!f.fail());
        checked += cf.flag ? run_conf<qe::SearchEqIupac>(cf, panel, own, texts) : run_conf<qe::SearchEq3>(cf, panel, own, texts);
    }
    printf("cases ok %ld\n", checked);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "keeper")) return keeper();
    if (argc == 2 && !strcmp(argv[1], "blocks")) { blocks_of<qe::SearchEq3>(); blocks_of<qe::SearchEqIupac>(); printf("blocks ok\n"); return 0; }
    if (argc == 3 && !strcmp(argv[1], "cases")) return cases(argv[2]);
    fprintf(stderr, "usage: search_panel_cpu keeper | blocks | cases <file>\n");
    return 2;
}
