// panel_cigar_cpu.cpp -- the occurrence aligner compiled for the host: panel_align_occ / panel_align_lane of
// quicked_amd/csrc/qe_panel_align.h -- the very source k_panel_occ_align<Eq> runs per lane -- driven through the stage's steps
// (the slot sizes, the offset scan, the launches over sub-batches that share one history).  A stand-alone program, built by
// tests/test_panel_cigar_cpu.py once plain and once with -fsanitize=address,undefined.
//
// panel_cigar_cpu cases <file>     the cases of tests/test_panel_cigar_cpu.py against the strings it took from the definition
//                                  (tests/panel_cigar_lib.py's cases_file format); prints "cases ok <n checked>"
// Per configuration (mode; flag; the members' own bounds or the uniform one) the recorded occurrences are the tasks -- what the
// sweeps of the run leave in `hits`.  Per style (0, 1, 2) and history budget (every wave at once; ONE wave, so that every
// launch but the last reuses the same cells):
//   * every string is the definition's in that style, NUL-terminated inside its own slot, nothing written outside the slots
//     (guard bytes around the pool and between checks), o_ops the operations of the style-0 string, o_steps the block steps;
//   * the checked failure path: the same tasks with every score off by one (both ways) report -1 and write inside their slots
//     only; tasks outside the history (text_start -1, an empty stretch, a history one column or one block short) report -1.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

#include "qe_panel_align.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "panel_cigar_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

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

// sequences' planes one after another, two rows of zeros behind each (as the library packs them); off: three-plane word offsets
template <class Eq>
struct Pool {
    std::vector<uint64_t> fwd;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    void add(const std::string& s, bool acgt) {
        const std::vector<uint64_t> f = Planes<Eq>::of(s, acgt);
        off.push_back((int64_t)(fwd.size() / Eq::W) * 3);
        fwd.insert(fwd.end(), f.begin(), f.end());
        fwd.insert(fwd.end(), (size_t)2 * Eq::W, 0);
        len.push_back((int32_t)s.size());
    }
};

struct Occ { int32_t pattern, start, end, score; std::string want[3]; };
struct Conf { int mode, flag, uniform; std::vector<std::vector<Occ>> occ; };

static int ops_of(const std::string& rle) {
    int total = 0, run = 0;
    for (char c : rle) { if (c >= '0' && c <= '9') run = 10 * run + (c - '0'); else { total += run; run = 0; } }
    return total;
}

enum Twist { TRUE_TASKS, SCORE_UP, SCORE_DOWN, START_NEGATIVE, EMPTY_STRETCH, COLUMN_SHORT, BLOCK_SHORT };

template <class Eq>
static long run_conf(const Conf& cf, const std::vector<std::string>& panel, const std::vector<std::string>& texts) {
    const int K = (int)panel.size(), n = (int)texts.size();
    Pool<Eq> M, T;
    for (int p = 0; p < K; ++p) M.add(panel[(size_t)p], false);
    for (int i = 0; i < n; ++i) T.add(texts[(size_t)i], cf.flag == 32);
    std::vector<int64_t> occ_off((size_t)n + 1, 0);
    std::vector<const Occ*> flat;
    for (int i = 0; i < n; ++i) {
        for (const Occ& o : cf.occ[(size_t)i]) flat.push_back(&o);
        occ_off[(size_t)i + 1] = (int64_t)flat.size();
    }
    const int64_t total = (int64_t)flat.size();
    if (total == 0) return 0;
    int cols = 1, blocks = 1;
    for (const Occ* o : flat) { cols = std::max(cols, o->end - o->start); blocks = std::max(blocks, qe::search_blocks(M.len[(size_t)o->pattern])); }
    long checked = 0;
    for (int twist : {TRUE_TASKS, SCORE_UP, SCORE_DOWN, START_NEGATIVE, EMPTY_STRETCH, COLUMN_SHORT, BLOCK_SHORT})
        for (int style = 0; style < 3; ++style)
            for (int one_wave = 0; one_wave < 2; ++one_wave) {
                if (twist != TRUE_TASKS && (style != 0 || one_wave)) continue;
                std::vector<int32_t> hits((size_t)(4 * total));
                for (int64_t j = 0; j < total; ++j) {
                    const Occ& o = *flat[(size_t)j];
                    int32_t* h = hits.data() + 4 * j;
                    h[0] = o.pattern; h[1] = o.start; h[2] = o.end; h[3] = o.score;
                    if (twist == SCORE_UP) h[3] = o.score + 1;
                    if (twist == SCORE_DOWN) h[3] = o.score - 1;
                    if (twist == START_NEGATIVE) h[1] = -1;
                    if (twist == EMPTY_STRETCH) h[1] = h[2];
                }
                const int hc = twist == COLUMN_SHORT ? cols - 1 : cols, hb = twist == BLOCK_SHORT ? blocks - 1 : blocks;
                // ---- the slot sizes and their offsets (k_panel_align_sizes, k_scan_offsets)
                std::vector<int32_t> len((size_t)total);
                std::vector<int64_t> str_off((size_t)total + 1, 0);
                for (int64_t j = 0; j < total; ++j) qe::panel_align_size_one(j, hits.data(), len.data());
                for (int64_t j = 0; j < total; ++j) str_off[(size_t)j + 1] = str_off[(size_t)j] + len[(size_t)j] + 1;
                const int64_t bytes = str_off[(size_t)total];
                const char GUARD = (char)0x7E;
                std::vector<char> pool((size_t)bytes + 32, GUARD);
                const int64_t waves = (total + 63) / 64, per = one_wave ? 1 : waves;
                const size_t wave_cells = (size_t)std::max(hc, 0) * (size_t)std::max(hb, 0) * 64;
                std::vector<qe::AlignCell> hist((size_t)per * wave_cells + 1);
                std::vector<int64_t> o_off((size_t)total, -7);
                std::vector<uint32_t> o_steps((size_t)total, 7), o_ops((size_t)total, 7);
                qe::PanelAlignArgs A{};
                A.pl_m = M.fwd.data(); A.m_off = M.off.data(); A.m_len = M.len.data(); A.n_members = K;
                A.pl_t = T.fwd.data(); A.t_off = T.off.data(); A.t_len = T.len.data();
                A.occ_off = occ_off.data(); A.npairs = n;
                A.hits = hits.data(); A.total = total;
                A.hist = hist.data(); A.hist_cols = hc; A.hist_blocks = hb; A.style = style;
                A.str_off = str_off.data(); A.pool = pool.data() + 16;
                A.o_off = o_off.data(); A.o_steps = o_steps.data(); A.o_ops = o_ops.data();
                for (int64_t w0 = 0; w0 < waves; w0 += per) {
                    A.first = 64 * w0; A.count = std::min<int64_t>(total - A.first, 64 * per);
                    // (descending: a lane's result must not depend on who ran before it; one lane past the count does nothing)
                    for (int64_t k = 64 * per; k >= 0; --k) qe::panel_align_occ<Eq>(A, k);
                }
                for (int g = 0; g < 16; ++g) CHECK(pool[(size_t)g] == GUARD && pool[(size_t)bytes + 16 + (size_t)g] == GUARD);
                for (int64_t j = 0; j < total; ++j) {
                    const Occ& o = *flat[(size_t)j];
                    const int blocks_j = qe::search_blocks(M.len[(size_t)o.pattern]);
                    bool fails = twist != TRUE_TASKS;
                    if (twist == COLUMN_SHORT) fails = o.end - o.start > hc;
                    if (twist == BLOCK_SHORT) fails = blocks_j > hb;
                    if (fails) { CHECK(o_off[(size_t)j] == -1); ++checked; continue; }
                    const int64_t at = o_off[(size_t)j];
                    if (at < str_off[(size_t)j] || at >= str_off[(size_t)j + 1])
                        fprintf(stderr, "mode %d flag %d uniform %d style %d occurrence %lld {%d %d %d %d}: offset %lld outside [%lld, %lld)\n", cf.mode, cf.flag, cf.uniform,
                                style, (long long)j, o.pattern, o.start, o.end, o.score, (long long)at, (long long)str_off[(size_t)j], (long long)str_off[(size_t)j + 1]);
                    CHECK(at >= str_off[(size_t)j] && at < str_off[(size_t)j + 1]);
                    CHECK(pool[(size_t)(16 + str_off[(size_t)j + 1] - 1)] == '\0');
                    const std::string got(pool.data() + 16 + at);
                    if (got != o.want[style])
                        fprintf(stderr, "mode %d flag %d uniform %d style %d occurrence %lld {%d %d %d %d}: got %s, expected %s\n", cf.mode, cf.flag, cf.uniform, style,
                                (long long)j, o.pattern, o.start, o.end, o.score, got.c_str(), o.want[style].c_str());
                    CHECK(got == o.want[style]);
                    CHECK(at + (int64_t)got.size() + 1 == str_off[(size_t)j + 1]);
                    CHECK((int)o_ops[(size_t)j] == ops_of(o.want[0]));
                    CHECK((int64_t)o_steps[(size_t)j] == (int64_t)blocks_j * (o.end - o.start));
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
    for (int p = 0; p < K; ++p) { int bound = 0; f >> panel[(size_t)p] >> bound; }
    for (int i = 0; i < n; ++i) { f >> texts[(size_t)i]; if (texts[(size_t)i] == ".") texts[(size_t)i].clear(); }
    long checked = 0;
    for (int c = 0; c < nconf; ++c) {
        Conf cf;
        f >> cf.mode >> cf.flag >> cf.uniform;
        cf.occ.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            int stored = 0;
            f >> stored;
            cf.occ[(size_t)i].resize((size_t)stored);
            for (Occ& o : cf.occ[(size_t)i]) f >> o.pattern >> o.start >> o.end >> o.score >> o.want[0] >> o.want[1] >> o.want[2];
        }
        CHECK(!f.fail());
        checked += cf.flag ? run_conf<qe::SearchEqIupac>(cf, panel, texts) : run_conf<qe::SearchEq3>(cf, panel, texts);
    }
    printf("cases ok %ld\n", checked);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "cases")) return cases(argv[2]);
    fprintf(stderr, "usage: panel_cigar_cpu cases <file>\n");
    return 2;
}
