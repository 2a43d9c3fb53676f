// qe_panel_ham.h -- panel search by mismatches only (QUICKED_PANEL_NO_INDELS on quicked_batch_run_panel / _run_panel_all;
// DESIGN.md 4.14.7).  Plain C++ with no HIP dependency, like qe_panel.h: k_panel_ham / k_panel_ham_hits (qe_kernels.hip) run
// it one lane per text, the host stand-ins of the stub build run it text by text, and the CPU suite compiles the very same
// source with g++ (tests/native/panel_noindels_cpu.cpp) and checks it against plain loops over bytes (tests/panel_noindels_lib.py).
//
// The definition.  Member p (m bases, effective bound k = min(bound, m)) against a text of n bases: for a start s in
// [0, n - m], H[s] = the positions r in [0, m) where member[r] and text[s + r] are NOT equal under the run's equality, and
// R[e] = H[e - m] for the ends e in E -- INFIX {m .. n}, PREFIX {m}, none when n < m.  Every column outside E counts as higher
// than every value.  qe_panel.h's contracts then hold with D[m][e] read as R[e]: the best run takes d = min R and the smallest
// e that has it, the all-occurrences run the valleys of R (the library's rule, a plateau counted once).  text_start = e - m.
//
// The sweep.  Chunks of 64 start positions; start s puts block b of the member (rows 64 b ..) on text positions s + 64 b ..,
// which lie in two words of each text plane.  The lane holds the words c .. c + NB of the chunk that starts at position 64 c
// as one chain per plane and shifts the chain right by one position per start: block b reads word b of the chain.  After 64
// starts the chain has moved down by one word, so a chunk loads one new word per plane.  Per block and start: the
// position-wise equality (Eq::eq_pos), masked to the block's rows, and a population count of the zeros.  Everything about
// the member -- planes, length, row masks, bound -- is the same for every lane (scalar registers on the device).
// Text words past the one that holds column n - 1 are never read; every loop is bounded by n, m and the block count.
#pragma once
#include <stdint.h>

#include "qe_panel.h"

namespace qe {

// word `idx` of every plane of a text whose last column lies in word `last`; past it: zeros, never read
template <class Eq>
QE_S_HD void panel_ham_word(const uint64_t* tp, int idx, int last, uint64_t (&t)[Eq::W]) {
    for (int k = 0; k < Eq::W; ++k) t[k] = idx <= last ? tp[Eq::W * (int64_t)idx + k] : 0;
}

// One member of NB blocks at the most (planes pp, m bases) against one text (planes tp, n columns): out.put(e, R[e]) for every
// e of E in ascending order.  steps: block steps -- the starts x the member's blocks --, added to
template <int NB, class Eq, class Out>
QE_S_HD void panel_ham_sweep(const uint64_t* pp, int m, const uint64_t* tp, int n, int mode, Out& out, uint32_t& steps) {
    const int nb = search_blocks(m);
    const int nstarts = n < m ? 0 : (mode == SEARCH_PREFIX ? 1 : n - m + 1);
    if (nstarts <= 0) return;
    uint64_t p[NB][Eq::W], mask[NB];
    QE_S_UNROLL
    for (int b = 0; b < NB; ++b) {
        Eq::pattern_rows(pp, m, b, p[b]);
        const int rows = search_rows(b, m);
        mask[b] = rows >= 64 ? ~(uint64_t)0 : (rows > 0 ? ((uint64_t)1 << rows) - 1 : 0);
    }
    const int last = (n - 1) >> 6;
    uint64_t t[NB + 1][Eq::W];
    QE_S_UNROLL
    for (int i = 0; i < NB; ++i) panel_ham_word<Eq>(tp, i, last, t[i]);
    for (int s0 = 0; s0 < nstarts; s0 += 64) {
        panel_ham_word<Eq>(tp, (s0 >> 6) + NB, last, t[NB]);
        const int cnt = nstarts - s0 < 64 ? nstarts - s0 : 64;
        for (int j = 0; j < cnt; ++j) {
            int32_t v = 0;
            QE_S_UNROLL
            for (int b = 0; b < NB; ++b)
                if (b < nb) v += search_popc(~Eq::eq_pos(p[b], t[b]) & mask[b]);
            out.put(s0 + j + m, v);
            QE_S_UNROLL
            for (int i = 0; i < NB; ++i)
                for (int k = 0; k < Eq::W; ++k) t[i][k] = (t[i][k] >> 1) | (t[i + 1][k] << 63);
            for (int k = 0; k < Eq::W; ++k) t[NB][k] >>= 1;
        }
    }
    steps += (uint32_t)nstarts * (uint32_t)nb;
}

// ---- the best member per text (quicked_batch_run_panel): min R and the smallest end that has it
struct PanelHamBest {
    int32_t best, end;                                // best > k: nothing within the bound
    QE_S_HD void init(int k) { best = k + 1; end = -1; }
    QE_S_HD void put(int32_t e, int32_t v) { const bool lower = v < best; best = lower ? v : best; end = lower ? e : end; }
};
template <int NB, class Eq>
QE_S_HD void panel_ham_member(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int mode, int32_t& score, int32_t& end, uint32_t& steps) {
    const int k = search_effective(bound, m);
    PanelHamBest B;
    B.init(k);
    panel_ham_sweep<NB, Eq>(pp, m, tp, n, mode, B, steps);
    score = B.best <= k ? B.best : -1; end = B.best <= k ? B.end : -1;
}
// One text against the members [p0, p1): panel_text's arguments and results under this file's definition
template <class Eq>
QE_S_HD void panel_ham_text(const PanelView& P, int p0, int p1, const uint64_t* tp, int n, int mode, PanelKeeper& keep, uint32_t& steps,
                            int32_t* m_score, int32_t* m_end) {
    panel_each_member<Eq>(P, p0, p1, [&](auto NB, int p, const uint64_t* pp, int m, int bound) {
        int32_t score = -1, end = -1;
        panel_ham_member<NB, Eq>(pp, m, bound, tp, n, mode, score, end, steps);
        if (m_score) { m_score[p] = score; m_end[p] = end; }
        keep.take(score >= 0 ? p : -1, score, end);
    });
}

// ---- every occurrence (quicked_batch_run_panel_all): the valley rule over scalar values.  qe_search.h's scan reads row m as
// +-1 delta words, which R is not; this one takes R[e] itself.  It is the lane's PanelHitScan -- the previous value, the
// pending plateau's first end and its score; the sink, found and best run on over the members -- with the member's bound
// beside it.  It walks w = min(R, k + 1) as that scan does: a value above k is no occurrence, ends a plateau as a rise
// whatever it is, and is a column every value <= k lies below.  A pending plateau is emitted when w rises or E ends
// (finish) and dropped when w falls.
struct PanelHamScan : PanelHitScan {
    int32_t k;
    QE_S_HD void member(int bound) { k = bound; prev = k + 1; pend_end = -1; pend_val = 0; }      // column m - 1: higher than every value
    QE_S_HD void put(int32_t e, int32_t v) {
        const int32_t w = v <= k ? v : k + 1;
        if (w < prev) { pend_end = e; pend_val = w; }
        else if (w > prev) emit();
        prev = w;
    }
};
template <int NB, class Eq>
QE_S_HD void panel_ham_member_hits(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int mode, PanelHamScan& H, uint32_t& steps) {
    H.member(search_effective(bound, m));
    panel_ham_sweep<NB, Eq>(pp, m, tp, n, mode, H, steps);
    H.finish();
}
// One text against the members [p0, p1): panel_text_hits' arguments and results under this file's definition
template <class Eq>
QE_S_HD void panel_ham_text_hits(const PanelView& P, int p0, int p1, const uint64_t* tp, int n, int mode, PanelHamScan& H, uint32_t& steps) {
    panel_each_member<Eq>(P, p0, p1, [&](auto NB, int p, const uint64_t* pp, int m, int bound) {
        H.sink.member = p;
        panel_ham_member_hits<NB, Eq>(pp, m, bound, tp, n, mode, H, steps);
    });
}

// ---- text_start = text_end - m, behind the unchanged k_panel_reduce / k_panel_hits_expand in their PREFIX form (no start
// pass): k_panel_ham_finish's pair i of the texts' quicked_panel_hit_t, k_panel_ham_hits_finish's stored occurrence j
QE_S_HD void panel_ham_finish_pair(int64_t i, const int32_t* m_len, int32_t* hits) {
    int32_t* h = hits + 6 * i;
    if (h[0] >= 0) h[2] = h[3] - m_len[h[0]];
}
QE_S_HD void panel_ham_hits_finish_one(int64_t j, const int32_t* m_len, int32_t* hits) {
    int32_t* o = hits + 4 * j;
    o[1] = o[2] - m_len[o[0]];
}

}  // namespace qe
