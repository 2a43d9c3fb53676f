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
//
// The end of the file is the same run with long texts split across lanes (quicked_batch_run_panel_scan_no_indels; DESIGN.md
// 4.14.8): k_panel_ham_scan, a window slot per lane.
#pragma once
#include <stdint.h>

#include "qe_panel.h"

namespace qe {

// word `idx` of every plane of a text whose last column lies in word `last`; past it: zeros, never read
template <class Eq>
QE_S_HD void panel_ham_word(const uint64_t* tp, int idx, int last, uint64_t (&t)[Eq::W]) {
    for (int k = 0; k < Eq::W; ++k) t[k] = idx <= last ? tp[Eq::W * (int64_t)idx + k] : 0;
}

// What a sweep holds per member and lane: the member's rows and row masks (the same for every lane) and the chain of NB + 1
// words per text plane.  value(): H of the start the chain stands at; shift(): the chain down by one position.  The windowed
// sweep at the end of the file is written over it.  panel_ham_sweep below keeps the same steps written out: over this struct
// k_panel_ham / k_panel_ham_hits came out with another instruction stream, and in the one run that measured it
// k_panel_ham_hits was 5 % behind (profiles/panel_noindels_scan.md, "The fold that was not kept"); as it stands their
// assembly is the parent commit's line for line.
template <int NB, class Eq>
struct PanelHamChain {
    uint64_t p[NB][Eq::W], mask[NB], t[NB + 1][Eq::W];
    int nb;
    QE_S_HD void member(const uint64_t* pp, int m) {
        nb = search_blocks(m);
        QE_S_UNROLL
        for (int b = 0; b < NB; ++b) {
            Eq::pattern_rows(pp, m, b, p[b]);
            const int rows = search_rows(b, m);
            mask[b] = rows >= 64 ? ~(uint64_t)0 : (rows > 0 ? ((uint64_t)1 << rows) - 1 : 0);
        }
    }
    QE_S_HD int32_t value() const {
        int32_t v = 0;
        QE_S_UNROLL
        for (int b = 0; b < NB; ++b)
            if (b < nb) v += search_popc(~Eq::eq_pos(p[b], t[b]) & mask[b]);
        return v;
    }
    QE_S_HD void shift() {
        QE_S_UNROLL
        for (int i = 0; i < NB; ++i)
            for (int k = 0; k < Eq::W; ++k) t[i][k] = (t[i][k] >> 1) | (t[i + 1][k] << 63);
        for (int k = 0; k < Eq::W; ++k) t[NB][k] >>= 1;
    }
};

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
template <class Range>
struct PanelHamScanOf : SearchHitScanOf<PanelHitSink, Range> {
    int32_t k;
    QE_S_HD void member(int bound) { k = bound; this->prev = k + 1; this->pend_end = -1; this->pend_val = 0; }      // column m - 1: higher than every value
    QE_S_HD void put(int32_t e, int32_t v) {
        const int32_t w = v <= k ? v : k + 1;
        if (w < this->prev) { this->pend_end = Range::owns(e) ? e : -1; this->pend_val = w; }      // (a window's lane: a descent outside (c0, c1] clears)
        else if (w > this->prev) this->emit();
        this->prev = w;
    }
};
typedef PanelHamScanOf<SearchAllColumns> PanelHamScan;
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

// ---- every occurrence, long texts split across lanes (quicked_batch_run_panel_scan_no_indels)
// A lane is a window slot {pair, c0, c1} of qe_panel.h's windowed run and owns the ends e in (c0, c1].  R[e] = H[e - m] reads
// text[e - m, e) only, so there is no warm-up in that run's sense: the lane's row is the text's row wherever it computes it.
// Per member of m bases it walks the starts s0 = max(0, c0 - m) upwards:
//   lead-in   c0 >= m: the one start c0 - m, whose value R[c0] is the scan's `prev` for the first owned end.  The scan takes it
//             as a column it does not own.  c0 < m: no such column exists -- the scan starts at "higher than every value", and
//             the first owned end is m.  c1 < m (the window lies wholly below m, or n < m): nothing is owned, nothing walked.
//   owned     the starts up to c1 - m: a descent of min(R, k + 1) makes a candidate.
//   run-out   the starts after c1 - m, one by one while the candidate is pending: a rise or the text's end emits it, a descent
//             clears it (PanelHamScanOf<SearchOwnedColumns>: that valley's first end is a later window's).  A plateau that
//             enters from the left is w == prev at the first owned end: no candidate.
// The chain starts at s0, which lies on no word boundary: it is loaded at the word that holds s0 and shifted down by s0 & 63
// once -- the same shift for every lane of a wave with c0 >= m, m being the wave's and c0 a multiple of 64 --, and takes its
// next word whenever a start crosses into a new word.  A member longer than the window reaches back over several earlier
// windows' words.  Words past the one that holds column n - 1 are never read; every loop is bounded by n, m and the block count.
// steps: (the starts walked, s0 to the last one of the run-out) x the member's blocks.
typedef PanelHamScanOf<SearchOwnedColumns> PanelHamWindowScan;
QE_S_HD void panel_ham_window_scan_init(PanelHamWindowScan& H, PanelRawHit* out, int32_t cap, int32_t c0, int32_t c1) {
    panel_window_scan_init(H, out, cap, c0, c1);
    H.k = 0;
}
// the first start a lane walks and the end of its owned stretch (exclusive); first >= own_end: the lane walks nothing
QE_S_HD void panel_ham_window_starts(int m, int c0, int c1, int& first, int& own_end) {
    first = c0 > m ? c0 - m : 0;
    own_end = c1 >= m ? c1 - m + 1 : 0;
}
template <int NB, class Eq>
QE_S_HD void panel_ham_member_window(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int c0, int c1, PanelHamWindowScan& H, uint32_t& steps) {
    H.member(search_effective(bound, m));
    int s, own_end;
    panel_ham_window_starts(m, c0, c1, s, own_end);
    if (s >= own_end) return;                                   // (c1 <= n, so n >= m from here on)
    const int nstarts = n - m + 1, first = s;
    PanelHamChain<NB, Eq> C;
    C.member(pp, m);
    const int last = (n - 1) >> 6;
    QE_S_UNROLL
    for (int i = 0; i <= NB; ++i) panel_ham_word<Eq>(tp, (s >> 6) + i, last, C.t[i]);
    // (per lane: lanes with c0 < m shift by 0 beside lanes that shift by (c0 - m) & 63, so the amount is no scalar)
    const int sh = s & 63;
    if (sh) {
        QE_S_UNROLL
        for (int i = 0; i < NB; ++i)
            for (int k = 0; k < Eq::W; ++k) C.t[i][k] = (C.t[i][k] >> sh) | (C.t[i + 1][k] << (64 - sh));
        for (int k = 0; k < Eq::W; ++k) C.t[NB][k] >>= sh;
    }
    // one start: its value to the scan, the chain down by one position; the next word when the next start opens one
    auto step = [&]() { H.put(s + m, C.value()); C.shift(); ++s; };
    auto next_word = [&]() { if (!(s & 63)) panel_ham_word<Eq>(tp, (s >> 6) + NB, last, C.t[NB]); };
    while (s < own_end) {                                       // the lead-in start and the owned ones, word by word
        const int left = own_end - s, cnt = left < 64 - (s & 63) ? left : 64 - (s & 63);
        for (int j = 0; j < cnt; ++j) step();
        next_word();
    }
    while (s < nstarts && H.pend_end >= 0) { step(); next_word(); }      // the run-out
    H.finish();                                                 // still pending: the walk reached the text's end, where a plateau counts
    steps += (uint32_t)(s - first) * (uint32_t)C.nb;
}
// The window (c0, c1] of one text against the members [p0, p1): panel_window_hits' arguments and results under this file's definition
template <class Eq>
QE_S_HD void panel_ham_window_hits(const PanelView& P, int p0, int p1, const uint64_t* tp, int n, int c0, int c1, PanelHamWindowScan& H, uint32_t& steps) {
    panel_each_member<Eq>(P, p0, p1, [&](auto NB, int p, const uint64_t* pp, int m, int bound) {
        H.sink.member = p;
        panel_ham_member_window<NB, Eq>(pp, m, bound, tp, n, c0, c1, H, steps);
    });
}

}  // namespace qe
