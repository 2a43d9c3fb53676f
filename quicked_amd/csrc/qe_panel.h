// qe_panel.h -- panel search: every text of a batch against one shared set of patterns (quicked_batch_run_panel; DESIGN.md
// 4.14).  Plain C++ with no HIP dependency, like qe_search.h: k_search_panel (qe_kernels.hip) runs it one lane per text, the
// host stand-ins of the stub build run it text by text, and the CPU suite compiles the very same source with g++
// (tests/native/search_panel_cpu.cpp) and checks it against the per-pair brute force (tests/panel_lib.py).
//
// The definition.  Per text and panel member p, {d, text_end} is what qe_search.h defines for that pattern against that text
// (mode, equality, the bound clamped to m); d > bound: p is beyond for this text.  The members within their bound are ordered
// by the key (score, panel index), ascending: the smallest is the text's best, the smallest of the others its runner-up.
//
// The keeper holds the two smallest keys seen.  take() compares keys, never arrival order, and merge() takes the two smallest
// of the union of two keepers -- the runner-up of a keeper can never be the best of a union that holds that keeper's best --
// so merging is associative and commutative: a panel may be cut into slices that are searched in any order and merged in any
// grouping.
//
// Why one lane per text.  Everything about a member is the same for every text (panel_slice below says why that puts it in
// scalar registers on the device).  A lane keeps the text side only: the chunk's words, {Pv, Mv, S} of up to four blocks,
// the SearchLane and the keeper.
//
// The second half of the file is the all-occurrences run (quicked_batch_run_panel_all): the same lanes and
// slices with qe_search.h's valley scan in the keeper's place; behind it the 3' tails (QUICKED_PANEL_TAILS):
// the walk down the column that run ends in; the 5' heads (QUICKED_PANEL_HEADS): a short sweep of the
// reversed member over the text's start, and the same walk; and the windowed run (quicked_batch_run_panel_scan).
#pragma once
#include <stdint.h>
#include <type_traits>

#include "qe_search.h"

namespace qe {

enum : int { PANEL_MAX_PATTERNS = 4096, PANEL_MAX_LEN = 256 };                   // QUICKED_PANEL_MAX_PATTERNS / _MAX_LEN

struct PanelKeeper {
    int32_t p1, s1, e1;      // the smallest key (score s1, member p1) and that member's text_end; p1 < 0: none
    int32_t p2, s2;          // the smallest key among the others; p2 < 0: none
    QE_S_HD void init() { p1 = -1; s1 = -1; e1 = -1; p2 = -1; s2 = -1; }
    static QE_S_HD bool less(int32_t sa, int32_t pa, int32_t sb, int32_t pb) { return sa < sb || (sa == sb && pa < pb); }
    // member p is within its bound at distance `score`, ending at `end` (p < 0: nothing)
    QE_S_HD void take(int32_t p, int32_t score, int32_t end) {
        // (selects, not branches around stores: the five fields stay five registers on the device)
        const bool first = p >= 0 && (p1 < 0 || less(score, p, s1, p1));
        const bool second = p >= 0 && !first && (p2 < 0 || less(score, p, s2, p2));
        p2 = first ? p1 : (second ? p : p2); s2 = first ? s1 : (second ? score : s2);
        p1 = first ? p : p1; s1 = first ? score : s1; e1 = first ? end : e1;
    }
    QE_S_HD void merge(const PanelKeeper& o) { take(o.p1, o.s1, o.e1); take(o.p2, o.s2, -1); }
};

// The panel as a pass reads it: member p has len[p] bases, the caller's bound bound[p] (>= 0; clamped to len[p] by
// search_lane_init) and its planes -- Eq::W words per 64 bases, two rows of zeros behind -- at word Eq::offset(off[p]) of pl
// (off: three-plane word offsets, as a batch's)
struct PanelView {
    const uint64_t* pl;
    const int64_t* off;
    const int32_t* len;
    const int32_t* bound;
};
// The member loop of every sweep: f(NB, p, pp, m, bound) for the members [p0, p1) in ascending order -- NB a
// std::integral_constant, the register form that holds the member's blocks (1, 2 or QE_SEARCH_REG_BLOCKS); pp its planes
template <class Eq, class F>
QE_S_HD void panel_each_member(const PanelView& P, int p0, int p1, F&& f) {
    for (int p = p0; p < p1; ++p) {
        const int m = P.len[p], bound = P.bound[p], nb = search_blocks(m);
        const uint64_t* pp = P.pl + Eq::offset(P.off[p]);
        if (nb <= 1) f(std::integral_constant<int, 1>{}, p, pp, m, bound);
        else if (nb == 2) f(std::integral_constant<int, 2>{}, p, pp, m, bound);
        else if (nb <= QE_SEARCH_REG_BLOCKS) f(std::integral_constant<int, QE_SEARCH_REG_BLOCKS>{}, p, pp, m, bound);
    }
}

// one member of NB blocks at the most against one text (n columns from the start of its planes tp): the register form
template <int NB, class Eq>
QE_S_HD void panel_member(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int mode, int32_t& score, int32_t& end, uint32_t& steps) {
    SearchLane L;
    search_lane_init(L, m, n, mode, bound, 0);
    SearchRegStore<NB, Eq> R;
    R.clear();
    R.load(pp, m);
    search_run<NB>(R, L, tp, 0);
    search_answer(L, score, end);
    steps += L.steps;
}

// One text (planes tp, n >= 0 columns) against the members [p0, p1): the keeper takes every member within its bound;
// m_score / m_end (null: not kept) get every member's {d or -1, text_end or -1} at index p; steps: block steps, added to
template <class Eq>
QE_S_HD void panel_text(const PanelView& P, int p0, int p1, const uint64_t* tp, int n, int mode, PanelKeeper& keep, uint32_t& steps,
                        int32_t* m_score, int32_t* m_end) {
    panel_each_member<Eq>(P, p0, p1, [&](auto NB, int p, const uint64_t* pp, int m, int bound) {
        int32_t score = -1, end = -1;
        panel_member<NB, Eq>(pp, m, bound, tp, n, mode, score, end, steps);
        keep.take(score >= 0 ? p : -1, score, end);               // (before the stores: profiles/panel_shells.md)
        if (m_score) { m_score[p] = score; m_end[p] = end; }
    });
}

// The start-pass task of a text's best member (INFIX): member of m bases found at distance `score` ending at `end` in a text
// of n bases.  The pass -- k_search<4, Eq> in PREFIX mode with SEARCH_LARGEST_END over the member's reversed planes and the
// text's reversed planes, SearchArgs::in_score = score, in_end -- walks the window of min(end, m + score) columns that ends
// at text_end and leaves o_start relative to it: text_start = base + o_start
QE_S_HD void panel_start_task(int m, int n, int end, int score, int32_t& task_n, int32_t& in_end, int32_t& base) {
    search_hit_task(m, n, end, score, task_n, in_end, base);
}

// ---- the kernels' argument blocks, and what the kernels and their host stand-ins do per text slot
// Panel search (k_search_panel<Eq>, qe_panel.h; quicked_batch_run_panel): one lane per text, grid = text groups x panel slices.
// Text slot t (nslots of them, a multiple of 64) is pair text[t] of the batch (-1: an empty slot); slice s searches the members
// [s per_slice, min(n_members, (s + 1) per_slice)).  The panel: member p has m_len[p] bases, bound m_bound[p] and its planes at
// word Eq::offset(m_off[p]) of pl_m (three-plane offsets, as a batch's).  Per (slice, slot) one partial keeper and the lane's
// block steps: field f of {p1, s1, e1, p2, s2, steps} at part[(f nslices + s) nslots + t].  m_score / m_end (null: not kept):
// every member's {d or -1, text_end or -1} at [pair n_members + p].
//
// PanelSweepArgs is what every per-text sweep kernel reads first, and the leading block of each one's arguments.  k_panel_heads
// has the members' REVERSED planes in pl_m; k_panel_scan has window slots for text slots, so its `text` is the window slots'
// pairs.  Those two blocks' own names for the two fields, pl_m_rev and w_pair, stay valid beside the shared ones.
struct PanelSweepArgs {
    union { const uint64_t* pl_m;  const uint64_t* pl_m_rev; };
    const int64_t* m_off;  const int32_t* m_len;  const int32_t* m_bound;
    int32_t n_members, per_slice;
    const uint64_t* pl_t;  const int64_t* pl_t_off;  const int32_t* t_len;
    int32_t nslots;
    union { const int32_t* text;  const int32_t* w_pair; };
};
// The opener of every sweep, in two halves.  The slice half is computed from kernel arguments and the slice index
// (blockIdx.y on the device) alone, and the member loop (panel_each_member) adds a loop counter: so everything about a member
// -- its index, length, bound, block count, row bit, plane words -- is wave-uniform, read through uniform addresses into
// scalar registers, and the dispatch on the block count is a uniform branch.  The text half is the lane's own.  They stay two
// structs returned by value, and a kernel's early exits stay in the kernel: one struct filled through a reference, exits
// inside, moved the member data out of the scalar registers (profiles/panel_shells.md).
struct PanelSlice { int slice, nslices, p0, p1; PanelView P; };      // the members [p0, p1); nslices = gridDim.y
struct PanelLane { int slot, pair, n; const uint64_t* tp; };          // pair < 0: an empty slot, n = 0 and no store
QE_S_HD PanelSlice panel_slice(const PanelSweepArgs& A, int slice) {
    PanelSlice S;
    S.slice = slice; S.nslices = (A.n_members + A.per_slice - 1) / A.per_slice;
    S.p0 = slice * A.per_slice; S.p1 = A.n_members < S.p0 + A.per_slice ? A.n_members : S.p0 + A.per_slice;
    S.P.pl = A.pl_m; S.P.off = A.m_off; S.P.len = A.m_len; S.P.bound = A.m_bound;
    return S;
}
template <class Eq>
QE_S_HD PanelLane panel_lane(const PanelSweepArgs& A, int slot) {
    PanelLane T;
    T.slot = slot; T.pair = A.text[slot]; T.n = 0; T.tp = A.pl_t;       // (nslots is a multiple of 64)
    if (T.pair >= 0) { T.n = A.t_len[T.pair]; T.tp = A.pl_t + Eq::offset(A.pl_t_off[T.pair]); }
    return T;
}
struct PanelArgs : PanelSweepArgs {
    int32_t mode;                            // SEARCH_PREFIX / SEARCH_INFIX
    int32_t* part;
    int32_t* m_score;  int32_t* m_end;
};
// One thread per text slot (k_panel_reduce): the slices' keepers merged into hits[pair] = quicked_panel_hit_t as {pattern,
// score, text_start, text_end, second_pattern, second_score} and o_adv[t] = the slot's block steps.  text_start: PREFIX 0;
// INFIX the base of the start pass's window, and the slot's task of that pass (panel_start_task) goes to o_pair / o_m / o_n /
// o_score / o_end [t] (o_pair -1: no member within its bound) with the offset of the best member's planes at o_plp_off[pair];
// k_panel_finish then adds the pass's o_start (or leaves -1).
struct PanelReduceArgs {
    int32_t nslots, nslices, infix;
    const int32_t* text;  const int32_t* part;
    const int32_t* m_len;  const int64_t* m_off;  const int32_t* t_len;
    int32_t* hits;  uint32_t* o_adv;
    int32_t* o_pair;  int32_t* o_m;  int32_t* o_n;  int32_t* o_score;  int32_t* o_end;  int64_t* o_plp_off;
};

// a lane's partial keeper and block steps to their places: field f at part[(f nslices + slice) nslots + slot]
QE_S_HD void panel_store_part(const PanelArgs& A, int nslices, int slice, int slot, const PanelKeeper& keep, uint32_t steps) {
    const int64_t stride = (int64_t)nslices * A.nslots;
    int32_t* q = A.part + (int64_t)slice * A.nslots + slot;
    q[0] = keep.p1; q[stride] = keep.s1; q[2 * stride] = keep.e1; q[3 * stride] = keep.p2; q[4 * stride] = keep.s2;
    q[5 * stride] = (int32_t)steps;
}
// k_panel_reduce's slot t: the slices' keepers merged (any grouping gives the same two keys), the text's quicked_panel_hit_t
// and -- INFIX -- its task of the start pass
QE_S_HD void panel_reduce_slot(const PanelReduceArgs& A, int t) {
    const int pair = A.text[t];
    if (A.infix) A.o_pair[t] = -1;
    if (pair < 0) return;
    const int64_t stride = (int64_t)A.nslices * A.nslots;
    PanelKeeper keep;
    keep.init();
    uint32_t steps = 0;
    for (int s = 0; s < A.nslices; ++s) {
        const int32_t* q = A.part + (int64_t)s * A.nslots + t;
        PanelKeeper o;
        o.p1 = q[0]; o.s1 = q[stride]; o.e1 = q[2 * stride]; o.p2 = q[3 * stride]; o.s2 = q[4 * stride];
        keep.merge(o);
        steps += (uint32_t)q[5 * stride];
    }
    int32_t* h = A.hits + 6 * (int64_t)pair;
    int32_t start = keep.p1 >= 0 ? 0 : -1;
    if (A.infix && keep.p1 >= 0) {
        const int m = A.m_len[keep.p1];
        int32_t task_n, in_end, base;
        panel_start_task(m, A.t_len[pair], keep.e1, keep.s1, task_n, in_end, base);
        start = base;
        A.o_pair[t] = pair; A.o_m[t] = m; A.o_n[t] = task_n; A.o_score[t] = keep.s1; A.o_end[t] = in_end;
        A.o_plp_off[pair] = A.m_off[keep.p1];
    }
    h[0] = keep.p1; h[1] = keep.s1; h[2] = start; h[3] = keep.e1; h[4] = keep.p2; h[5] = keep.s2;
    A.o_adv[t] = steps;
}
// k_panel_finish's slot t: the start pass's o_start is relative to the best member's window
QE_S_HD void panel_finish_slot(int t, const int32_t* text, const int32_t* o_pair, const int32_t* o_start, int32_t* hits) {
    const int pair = text[t];
    if (pair < 0 || o_pair[t] < 0) return;
    int32_t* h = hits + 6 * (int64_t)pair;
    h[2] = o_start[t] < 0 ? -1 : h[2] + o_start[t];
}

// ---- every occurrence of every member (quicked_batch_run_panel_all)
// Per text and member p the occurrences are what qe_search.h defines for that pattern against that text with that bound
// (SearchHitScanOf: the valley rule, decided there and nowhere else); a text's occurrences are ordered by (member, text_end).
// A lane keeps ONE scan across the members of its slice: found, the smallest score and the sink run on, begin() starts a
// member at column 0 with no candidate.  The sink records the member beside {end, score}: the lane's stretch then holds its
// slice's occurrences in (member, text_end) order already, and the first `cap` of them.
struct PanelRawHit { int32_t pattern, end, score; };
struct PanelHitSink {
    PanelRawHit* out; int32_t cap, count, member;
    QE_S_HD void put(int32_t end, int32_t score) {
        if (count < cap) { out[count] = PanelRawHit{member, end, score}; ++count; }
    }
};
typedef SearchHitScanOf<PanelHitSink> PanelHitScan;
QE_S_HD void panel_hit_scan_init(PanelHitScan& H, PanelRawHit* out, int32_t cap) {
    H.prev = 0; H.pend_end = -1; H.pend_val = 0; H.found = 0; H.best = -1;
    H.sink.out = out; H.sink.cap = cap; H.sink.count = 0; H.sink.member = -1;
}

// one member of NB blocks at the most against one text: the register form, the bound kept for the whole text, no early exit
template <int NB, class Eq>
QE_S_HD void panel_member_hits(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int mode, PanelHitScan& H, uint32_t& steps) {
    SearchLane L;
    search_lane_init(L, m, n, mode, bound, 0);
    SearchRegStore<NB, Eq> R;
    R.clear();
    R.load(pp, m);
    H.begin(L);
    search_run_hits<NB>(R, L, H, tp, 0);
    steps += L.steps;
}

// One text (planes tp, n >= 0 columns) against the members [p0, p1): every occurrence goes to H's sink, H.found / H.best run
// on over the members; steps: block steps, added to
template <class Eq>
QE_S_HD void panel_text_hits(const PanelView& P, int p0, int p1, const uint64_t* tp, int n, int mode, PanelHitScan& H, uint32_t& steps) {
    panel_each_member<Eq>(P, p0, p1, [&](auto NB, int p, const uint64_t* pp, int m, int bound) {
        H.sink.member = p;
        panel_member_hits<NB, Eq>(pp, m, bound, tp, n, mode, H, steps);
    });
}

// k_panel_hits<Eq>: k_search_panel's grid and slots (PanelArgs above), the members' occurrences instead of the two best keys.
// Per (slice s, slot t): field f of {found, stored, best, steps} at part[(f nslices + s) nslots + t], and the stored
// occurrences -- at most max_hits, the slice's first in (member, text_end) order -- as PanelRawHit number i at
// raw[(s nslots + t) max_hits + i].  A slot without a text writes nothing.
struct PanelHitsArgs : PanelSweepArgs {
    int32_t mode, max_hits;
    int32_t* part;
    PanelRawHit* raw;
};
// the stretch of a lane's raw records (here and in PanelScanArgs), null for an empty slot, whose room is 0
template <class A>
QE_S_HD PanelRawHit* panel_lane_raw(const A& a, const PanelSlice& S, const PanelLane& T) {
    return T.pair >= 0 ? a.raw + ((int64_t)S.slice * a.nslots + T.slot) * a.max_hits : nullptr;
}
// One thread per text slot (k_panel_hits_count): the slices' counts merged into found[pair], best[pair] (the smallest score
// among all found occurrences, -1: none) and len[pair] = stored - 1, stored = min(found, max_hits) -- what k_scan_offsets adds
// 1 to --, and o_adv[t] = the slot's block steps.  Every slice stores its first min(found_s, max_hits), so the first
// `stored` of the slices' stretches in slice order are all there.
struct PanelHitsCountArgs {
    int32_t nslots, nslices, max_hits;
    const int32_t* text;  const int32_t* part;
    int32_t* found;  int32_t* best;  int32_t* len;  uint32_t* o_adv;
};
// One thread per text slot (k_panel_hits_expand): the slot's stored occurrences to hits[off[pair] + i] = quicked_panel_occ_t as
// {pattern, text_start, text_end, score}, in slice order and in stored order within a slice -- slices are ascending member
// ranges, so that is (pattern, text_end) order.  text_start: PREFIX 0; INFIX the base of the start pass's window, and
// occurrence j's task of that pass (search_hit_task) goes to o_pair / o_m / o_n / o_score / o_end [j] with o_pair[j] = j:
// the pass reads a task's pair only to index its two plane offsets, which are o_plp_off[j] (the member's, into the reversed
// panel planes) and o_plt_off[j] (the text's).  k_panel_hits_finish then adds the pass's o_start (or leaves -1).
struct PanelHitsExpandArgs {
    int32_t nslots, nslices, max_hits, infix;
    const int32_t* text;  const int32_t* part;  const PanelRawHit* raw;
    const int64_t* off;
    const int32_t* m_len;  const int64_t* m_off;  const int32_t* t_len;  const int64_t* t_off;
    int32_t* hits;
    int32_t* o_pair;  int32_t* o_m;  int32_t* o_n;  int32_t* o_score;  int32_t* o_end;  int64_t* o_plp_off;  int64_t* o_plt_off;
};

QE_S_HD void panel_hits_store_part(const PanelHitsArgs& A, int nslices, int slice, int slot, const PanelHitScan& H, uint32_t steps) {
    const int64_t stride = (int64_t)nslices * A.nslots;
    int32_t* q = A.part + (int64_t)slice * A.nslots + slot;
    q[0] = H.found; q[stride] = H.sink.count; q[2 * stride] = H.best; q[3 * stride] = (int32_t)steps;
}
QE_S_HD void panel_hits_count_slot(const PanelHitsCountArgs& A, int t) {
    const int pair = A.text[t];
    if (pair < 0) return;
    const int64_t stride = (int64_t)A.nslices * A.nslots;
    int32_t found = 0, stored = 0, best = -1;
    uint32_t steps = 0;
    for (int s = 0; s < A.nslices; ++s) {
        const int32_t* q = A.part + (int64_t)s * A.nslots + t;
        const int32_t b = q[2 * stride];
        found += q[0];
        stored = stored + q[stride] < A.max_hits ? stored + q[stride] : A.max_hits;
        best = (b >= 0 && (best < 0 || b < best)) ? b : best;
        steps += (uint32_t)q[3 * stride];
    }
    A.found[pair] = found; A.best[pair] = best; A.len[pair] = stored - 1;
    A.o_adv[t] = steps;
}
// CAPPED (a queued run, panel_queue_expand_slot below): nothing is written at an index >= cap
template <bool CAPPED>
QE_S_HD void panel_hits_expand_slot_of(const PanelHitsExpandArgs& A, int t, int64_t cap) {
    const int pair = A.text[t];
    if (pair < 0) return;
    const int64_t stride = (int64_t)A.nslices * A.nslots;
    const int n = A.t_len[pair];
    int64_t j = A.off[pair];
    int left = A.max_hits;
    for (int s = 0; s < A.nslices && left > 0; ++s) {
        const int32_t have = A.part[(int64_t)s * A.nslots + t + stride];
        const PanelRawHit* raw = A.raw + ((int64_t)s * A.nslots + t) * A.max_hits;
        for (int i = 0; i < have && left > 0; ++i, ++j, --left) {
            if (CAPPED && j >= cap) return;
            const PanelRawHit h = raw[i];
            int32_t* o = A.hits + 4 * j;
            int32_t start = 0;
            if (A.infix) {
                const int m = A.m_len[h.pattern];
                int32_t task_n, in_end, base;
                search_hit_task(m, n, h.end, h.score, task_n, in_end, base);
                start = base;
                A.o_pair[j] = (int32_t)j; A.o_m[j] = m; A.o_n[j] = task_n; A.o_score[j] = h.score; A.o_end[j] = in_end;
                A.o_plp_off[j] = A.m_off[h.pattern]; A.o_plt_off[j] = A.t_off[pair];
            }
            o[0] = h.pattern; o[1] = start; o[2] = h.end; o[3] = h.score;
        }
    }
}
QE_S_HD void panel_hits_expand_slot(const PanelHitsExpandArgs& A, int t) { panel_hits_expand_slot_of<false>(A, t, 0); }
// k_panel_hits_finish's occurrence j: the start pass's o_start is relative to the occurrence's window
QE_S_HD void panel_hits_finish_one(int64_t j, const int32_t* o_start, int32_t* hits) {
    hits[4 * j + 1] = o_start[j] < 0 ? -1 : hits[4 * j + 1] + o_start[j];
}

// ---- the same run queued (quicked_batch_configure_panel_queue): no host read between the passes, so the
// arrays the total W = off[n] sizes in the sync run are taken at cap = min(max_total, texts x max_hits) instead, and every step
// behind the offset scan keeps below cap on its own.  The records are in the order of the pairs, so what fits is the first
// min(W, cap) of the sync run's array whatever the slots' order is.
// k_panel_queue_expand's slot: panel_hits_expand_slot, writing records and start-pass tasks at indices < cap only.  The pass
// then runs over cap task slots whose o_pair was preset to -1: a lane that was never written does nothing.
QE_S_HD void panel_queue_expand_slot(const PanelHitsExpandArgs& A, int t, int64_t cap) { panel_hits_expand_slot_of<true>(A, t, cap); }
// k_panel_queue_finish's occurrence j of cap: panel_hits_finish_one below min(*total, cap), the total read on the device
QE_S_HD void panel_queue_finish_one(int64_t j, const int64_t* total, int64_t cap, const int32_t* o_start, int32_t* hits) {
    const int64_t stored = *total < cap ? *total : cap;
    if (j < stored) panel_hits_finish_one(j, o_start, hits);
}
// k_panel_queue_clamp's element i of 0 .. n: off[i] = min(off[i], cap) -- stored'[i] = off'[i + 1] - off'[i] follows --, and
// element n keeps what the fetch wants beside it: q[0] = W, q[1] / q[2] = the bytes of the stored records / of their step
// counts, for the copies to their real length (k_copy_total)
QE_S_HD void panel_queue_clamp_one(int64_t i, int64_t n, int64_t cap, int64_t* off, int64_t* q) {
    const int64_t v = off[i], c = v < cap ? v : cap;
    if (i == n) { q[0] = v; q[1] = c * 16; q[2] = c * 4; }
    off[i] = c;
}

// ---- a member cut off by the text's end: 3' tails (QUICKED_PANEL_TAILS on quicked_batch_run_panel_all)
// The definition.  D is the INFIX matrix of member p (m bases, effective bound k = min(bound, m)) against the text (n >= 1
// columns).  Row r is a tail of p when min_overlap <= r <= m - 1 and D[r][n] <= floor(r k / m): the member's first r bases end
// where the text ends, at the member's own error rate.  The key of a tail is (matched length r - D[r][n] descending, D[r][n]
// ascending, member index ascending); within one member the first two fix r.  A text's tail is the smallest key over its members.
//
// Where D[.][n] comes from.  After search_run_hits the lane's store holds column n: Pv / Mv of block b are the vertical deltas
// of rows 64 b + 1 .. 64 b + 64 and S(b - 1) is the value of row 64 b (row 0: 0), so a running sum down the live blocks gives
// D[i][n].  Every allowance is at most k, the live-block rule keeps every cell <= k exact and every other cell above k, and a
// block that is not live holds no cell <= k (qe_search.h, "Why that loses no answer"): the walk over the live blocks decides
// every row as the full matrix does.  What a tail is is decided here and nowhere else.
struct PanelTailKeeper {
    int32_t p, r, d;         // the smallest key: member p, overlap r, score d; p < 0: none
    QE_S_HD void init() { p = -1; r = -1; d = -1; }
    static QE_S_HD bool before(int32_t ra, int32_t da, int32_t pa, int32_t rb, int32_t db, int32_t pb) {
        const int32_t ma = ra - da, mb = rb - db;
        return ma > mb || (ma == mb && (da < db || (da == db && pa < pb)));
    }
    // row rr of member pp is a tail at distance dd (pp < 0: nothing); selects, as PanelKeeper::take
    QE_S_HD void take(int32_t pp, int32_t rr, int32_t dd) {
        const bool t = pp >= 0 && (p < 0 || before(rr, dd, pp, r, d, p));
        p = t ? pp : p; r = t ? rr : r; d = t ? dd : d;
    }
    QE_S_HD void merge(const PanelTailKeeper& o) { take(o.p, o.r, o.d); }
};

// The walk: column n of the lane's store after the member's search_run_hits.  m, k, min_overlap and every loop bound are the
// member's (wave-uniform on the device); L.live and the words are the lane's.  The allowance floor(i k / m) runs along with
// the row: k <= m, so it rises by at most one per row.  rows: the row steps, added to
template <int NB, class Store>
QE_S_HD void panel_tail_walk(Store& st, const SearchLane& L, int min_overlap, int32_t p, PanelTailKeeper& keep, uint32_t& rows) {
    if (L.n < 1) return;                                      // an empty text has no tail
    const int m = L.m, k = search_effective(L.k, m);          // (an all-occurrences lane keeps its bound: L.k is the member's)
    QE_S_UNROLL
    for (int b = 0; b < NB; ++b) {
        const int left = m - 1 - 64 * b, nrows = left < 64 ? left : 64;      // rows 64 b + 1 .. m - 1 of this block
        if (nrows <= 0 || b >= L.live) continue;
        int32_t allow = b ? (64 * b * k) / m : 0, acc = b ? (64 * b * k) % m : 0;
        int32_t v = b ? st.S(b - 1) : 0;
        const uint64_t P = st.P(b), M = st.M(b);
        for (int r = 0; r < nrows; ++r) {
            v += (int32_t)((P >> r) & 1) - (int32_t)((M >> r) & 1);
            acc += k;
            if (acc >= m) { acc -= m; ++allow; }
            const int i = 64 * b + r + 1;
            keep.take((i >= min_overlap && v <= allow) ? p : -1, i, v);
        }
        rows += (uint32_t)nrows;
    }
}

// one member of NB blocks at the most against one text: panel_member_hits, and the walk over the column it ends in
template <int NB, class Eq>
QE_S_HD void panel_member_tails(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int mode, int min_overlap, int32_t p,
                                PanelHitScan& H, PanelTailKeeper& keep, uint32_t& steps, uint32_t& rows) {
    SearchLane L;
    search_lane_init(L, m, n, mode, bound, 0);
    SearchRegStore<NB, Eq> R;
    QE_S_UNROLL
    for (int b = 0; b < NB; ++b) { R.pv[b] = R.mv[b] = 0; R.s[b] = 0; }      // (not R.clear(): profiles/panel_shells.md)
    R.load(pp, m);
    H.begin(L);
    search_run_hits<NB>(R, L, H, tp, 0);
    steps += L.steps;
    panel_tail_walk<NB>(R, L, min_overlap, p, keep, rows);
}
// One text against the members [p0, p1): panel_text_hits, with the text's best tail among them in `keep`
template <class Eq>
QE_S_HD void panel_text_tails(const PanelView& P, int p0, int p1, const uint64_t* tp, int n, int mode, int min_overlap,
                              PanelHitScan& H, PanelTailKeeper& keep, uint32_t& steps, uint32_t& rows) {
    panel_each_member<Eq>(P, p0, p1, [&](auto NB, int p, const uint64_t* pp, int m, int bound) {
        H.sink.member = p;
        panel_member_tails<NB, Eq>(pp, m, bound, tp, n, mode, min_overlap, p, H, keep, steps, rows);
    });
}

// k_panel_tails<Eq>: k_panel_hits with the walk.  H is k_panel_hits' argument block and everything it names is written as that
// kernel writes it; besides, per (slice s, slot t), field f of {pattern, overlap, score, row steps} of the slice's best tail at
// tpart[(f nslices + s) nslots + t].
struct PanelTailsArgs {
    PanelHitsArgs H;
    int32_t min_overlap;
    int32_t* tpart;
};
// One thread per text slot (k_panel_tails_merge): the slices' keepers merged by the key into tails[pair] =
// quicked_panel_tail_t as {pattern, overlap, text_start, score} (tails: -1 everywhere before) and o_rows[t] = the slot's row
// steps.  text_start: the base of the start pass's window, and the slot's task of that pass -- search_hit_task for the
// overlap's rows ending at column n -- goes to o_pair / o_m / o_n / o_score / o_end [t] (o_pair -1: no tail); the task's pattern
// is the reversed prefix, which k_panel_tail_planes lays out at three-plane word t plane_stride of a scratch pool
// (o_plp_off[pair]).  k_panel_tails_finish then adds the pass's o_start (or leaves -1).
struct PanelTailsMergeArgs {
    int32_t nslots, nslices;
    const int32_t* text;  const int32_t* tpart;  const int32_t* t_len;
    int64_t plane_stride;
    int32_t* tails;  uint32_t* o_rows;
    int32_t* o_pair;  int32_t* o_m;  int32_t* o_n;  int32_t* o_score;  int32_t* o_end;  int64_t* o_plp_off;
};
// One thread per text slot (k_panel_tail_planes<Eq>): the first `overlap` bases of the tail's member, reversed, from the
// member's forward planes (Eq::W words per row, at Eq::offset(m_off[pattern]) of pl_m) to Eq::offset(o_plp_off[pair]) of pool,
// two rows of zeros behind
struct PanelTailPlanesArgs {
    int32_t nslots;
    const int32_t* o_pair;  const int32_t* tails;
    const uint64_t* pl_m;  const int64_t* m_off;  const int64_t* o_plp_off;
    uint64_t* pool;
};

QE_S_HD void panel_tails_store_part(const PanelTailsArgs& A, int nslices, int slice, int slot, const PanelTailKeeper& keep, uint32_t rows) {
    const int64_t stride = (int64_t)nslices * A.H.nslots;
    int32_t* q = A.tpart + (int64_t)slice * A.H.nslots + slot;
    q[0] = keep.p; q[stride] = keep.r; q[2 * stride] = keep.d; q[3 * stride] = (int32_t)rows;
}
// slot t's keepers of the slices merged by the key (any order gives the same one); -> the sum of the slices' fourth field
QE_S_HD uint32_t panel_tail_parts_merge(const int32_t* tpart, int nslices, int nslots, int t, PanelTailKeeper& keep) {
    const int64_t stride = (int64_t)nslices * nslots;
    keep.init();
    uint32_t rows = 0;
    for (int s = 0; s < nslices; ++s) {
        const int32_t* q = tpart + (int64_t)s * nslots + t;
        PanelTailKeeper o;
        o.p = q[0]; o.r = q[stride]; o.d = q[2 * stride];
        keep.merge(o);
        rows += (uint32_t)q[3 * stride];
    }
    return rows;
}
QE_S_HD void panel_tails_merge_slot(const PanelTailsMergeArgs& A, int t) {
    const int pair = A.text[t];
    A.o_pair[t] = -1;
    if (pair < 0) return;
    PanelTailKeeper keep;
    A.o_rows[t] = panel_tail_parts_merge(A.tpart, A.nslices, A.nslots, t, keep);
    if (keep.p < 0) return;
    const int n = A.t_len[pair];
    int32_t task_n, in_end, base;
    search_hit_task(keep.r, n, n, keep.d, task_n, in_end, base);
    A.o_pair[t] = pair; A.o_m[t] = keep.r; A.o_n[t] = task_n; A.o_score[t] = keep.d; A.o_end[t] = in_end;
    A.o_plp_off[pair] = (int64_t)t * A.plane_stride;
    int32_t* o = A.tails + 4 * (int64_t)pair;
    o[0] = keep.p; o[1] = keep.r; o[2] = base; o[3] = keep.d;
}
QE_S_HD uint64_t panel_reverse_bits(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brevll(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
#endif
}
// the reversed prefix of `len` bases: reversed positions [64 row, 64 row + 64) are the forward positions e - 1 down to e - 64,
// e = len - 64 row (k_reverse_planes' formula, for any plane count); rows past the prefix are zeros
template <class Eq>
QE_S_HD void panel_tail_planes_slot(const PanelTailPlanesArgs& A, int t) {
    const int pair = A.o_pair[t];
    if (pair < 0) return;
    const int len = A.tails[4 * (int64_t)pair + 1], nw = (len + 63) >> 6;
    const uint64_t* src = A.pl_m + Eq::offset(A.m_off[A.tails[4 * (int64_t)pair]]);
    uint64_t* dst = A.pool + Eq::offset(A.o_plp_off[pair]);
    for (int row = 0; row < nw + 2; ++row) {
        uint64_t x[Eq::W];
        for (int k = 0; k < Eq::W; ++k) x[k] = 0;
        if (row < nw) {
            const int s = len - 64 * row - 64;
            if (s >= 0) search_text_words<Eq::W>(src, s, 64, x);
            else for (int k = 0; k < Eq::W; ++k) x[k] = src[k] << (-s);
            for (int k = 0; k < Eq::W; ++k) x[k] = panel_reverse_bits(x[k]);
        }
        for (int k = 0; k < Eq::W; ++k) dst[Eq::W * (int64_t)row + k] = x[k];
    }
}
// k_panel_tails_finish's slot t: the start pass's o_start is relative to the tail's window
QE_S_HD void panel_tails_finish_slot(int t, const int32_t* o_pair, const int32_t* o_start, int32_t* tails) {
    const int pair = o_pair[t];
    if (pair < 0) return;
    int32_t* o = tails + 4 * (int64_t)pair;
    o[2] = o_start[t] < 0 ? -1 : o[2] + o_start[t];
}

// ---- a member cut off by the text's start: 5' heads (QUICKED_PANEL_HEADS on quicked_batch_run_panel_all)
// The definition.  D^R is the INFIX matrix of rev(member p) (m bases, effective bound k) against rev(text) (n >= 1 columns),
// rev() plain reversal.  Row r is a head of p when min_overlap <= r <= m - 1 and D^R[r][n] <= floor(r k / m): the member's last
// r bases fit a stretch text[0:e) at the member's own error rate.  That is the tails' rule on the reversed sequences, so the
// walk, the key and the keeper are the tails' own (panel_tail_walk, PanelTailKeeper): what a head is and which one wins is
// decided there and nowhere else.
//
// Where D^R[.][n] comes from.  Nothing computes that matrix for the occurrences, so the lane sweeps it itself -- but only its
// last c0 = min(n, m + k) columns, which are the text's FIRST c0 columns taken backwards: a head row within its allowance has
// d <= floor(r k / m) <= k and its stretch at most r + d <= m - 1 + k text bases, so a fresh INFIX sweep of rev(member) over
// rev(text[0:c0)) -- the stretches inside text[0:c0) only -- gives values >= the full matrix's and equal ones wherever the full
// value is within the allowance (4.14.2's warm-up argument).  The sweep is search_chunk under the live-block rule with no scan
// of row m; the store then holds the column the walk wants.
struct PanelNoScan {
    QE_S_HD void row(SearchLane&, int32_t, uint64_t, uint64_t, int, int) {}
    QE_S_HD void no_row(SearchLane&) {}
};
// sweep columns [col0, col0 + ncols) of the backward walk over text[0:c0): the forward columns c0 - 1 - col0 down to
// c0 - col0 - ncols, read forwards from the text's planes at that bit offset and reversed in registers; bits >= ncols are zero
template <class Eq>
QE_S_HD void panel_head_chunk(const uint64_t* tp, int c0, int col0, int ncols, uint64_t (&t)[Eq::W]) {
    Eq::text_chunk(tp, c0 - col0 - ncols, ncols, t);
    for (int k = 0; k < Eq::W; ++k) t[k] = panel_reverse_bits(t[k]) >> (64 - ncols);
}
// one member of NB blocks at the most (pp: its REVERSED planes) against the start of one text (tp: its forward planes, n
// columns).  The partial chunk comes first, so every later chunk is a whole word of the text's planes.  steps: block steps of
// the sweep, rows: row steps of the walk, both added to
template <int NB, class Eq>
QE_S_HD void panel_member_heads(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int min_overlap, int32_t p,
                                PanelTailKeeper& keep, uint32_t& steps, uint32_t& rows) {
    const int reach = m + search_effective(bound, m), c0 = n < reach ? n : reach;
    SearchLane L;
    search_lane_init(L, m, c0, SEARCH_INFIX, bound, 0);
    SearchRegStore<NB, Eq> R;
    QE_S_UNROLL
    for (int b = 0; b < NB; ++b) { R.pv[b] = R.mv[b] = 0; R.s[b] = 0; }      // (not R.clear(): profiles/panel_shells.md)
    R.load(pp, m);
    search_store_init<NB>(R, L);
    PanelNoScan none;
    for (int col0 = 0; col0 < c0;) {
        const int ncols = col0 ? 64 : ((c0 - 1) & 63) + 1;
        uint64_t t[Eq::W];
        panel_head_chunk<Eq>(tp, c0, col0, ncols, t);
        search_chunk<NB>(R, L, t, col0, ncols, none);
        col0 += ncols;
    }
    steps += L.steps;
    panel_tail_walk<NB>(R, L, min_overlap, p, keep, rows);      // (c0 = 0: an empty text has no head)
}
// One text against the members [p0, p1) of P, whose planes are the members' REVERSED ones: the text's best head among them
template <class Eq>
QE_S_HD void panel_text_heads(const PanelView& P, int p0, int p1, const uint64_t* tp, int n, int min_overlap,
                              PanelTailKeeper& keep, uint32_t& steps, uint32_t& rows) {
    panel_each_member<Eq>(P, p0, p1, [&](auto NB, int p, const uint64_t* pp, int m, int bound) {
        panel_member_heads<NB, Eq>(pp, m, bound, tp, n, min_overlap, p, keep, steps, rows);
    });
}

// k_panel_heads<Eq>: k_panel_hits' grid, slots and slices over the members' reversed planes (in pl_m; offsets, lengths and
// bounds the panel's) and the texts' forward planes.  Per (slice s, slot t): field f of {pattern, overlap, score, row steps,
// block steps} of the slice's best head at hpart[(f nslices + s) nslots + t].  A slot without a text writes nothing.
struct PanelHeadsArgs : PanelSweepArgs {
    int32_t min_overlap;
    int32_t* hpart;
};
// One thread per text slot (k_panel_heads_merge): the slices' keepers merged by the key into heads[pair] =
// quicked_panel_head_t as {pattern, overlap, text_end, score} (heads: -1 everywhere before), o_rows[t] / o_steps[t] = the slot's
// row and block steps.  text_end: the columns of the end pass's window, and the slot's task of that pass -- the member's last
// `overlap` bases against the text's first min(n, overlap + score) columns, both forwards -- goes to o_pair / o_m / o_n / o_score
// / o_end [t] (o_pair -1: no head); the task's pattern is laid out by k_panel_head_planes at three-plane word t plane_stride
// of a scratch pool (o_plp_off[pair]).  k_panel_heads_finish then subtracts the pass's o_start (or leaves -1).
struct PanelHeadsMergeArgs {
    int32_t nslots, nslices;
    const int32_t* text;  const int32_t* hpart;  const int32_t* t_len;
    int64_t plane_stride;
    int32_t* heads;  uint32_t* o_rows;  uint32_t* o_steps;
    int32_t* o_pair;  int32_t* o_m;  int32_t* o_n;  int32_t* o_score;  int32_t* o_end;  int64_t* o_plp_off;
};
// One thread per text slot (k_panel_head_planes<Eq>): the last `overlap` bases of the head's member -- bits [m - overlap, m) of
// the member's FORWARD planes (Eq::W words per row, at Eq::offset(m_off[pattern]) of pl_m) -- word-aligned to
// Eq::offset(o_plp_off[pair]) of pool, two rows of zeros behind
struct PanelHeadPlanesArgs {
    int32_t nslots;
    const int32_t* o_pair;  const int32_t* heads;
    const uint64_t* pl_m;  const int64_t* m_off;  const int32_t* m_len;  const int64_t* o_plp_off;
    uint64_t* pool;
};

QE_S_HD void panel_heads_store_part(const PanelHeadsArgs& A, int nslices, int slice, int slot, const PanelTailKeeper& keep, uint32_t rows, uint32_t steps) {
    const int64_t stride = (int64_t)nslices * A.nslots;
    int32_t* q = A.hpart + (int64_t)slice * A.nslots + slot;
    q[0] = keep.p; q[stride] = keep.r; q[2 * stride] = keep.d; q[3 * stride] = (int32_t)rows; q[4 * stride] = (int32_t)steps;
}
QE_S_HD void panel_heads_merge_slot(const PanelHeadsMergeArgs& A, int t) {
    const int pair = A.text[t];
    A.o_pair[t] = -1;
    if (pair < 0) return;
    PanelTailKeeper keep;
    A.o_rows[t] = panel_tail_parts_merge(A.hpart, A.nslices, A.nslots, t, keep);
    uint32_t steps = 0;
    for (int s = 0; s < A.nslices; ++s) steps += (uint32_t)A.hpart[((int64_t)4 * A.nslices + s) * A.nslots + t];
    A.o_steps[t] = steps;
    if (keep.p < 0) return;
    // the best search's start-pass form walks the in_end columns that end at column task_n: both the window, from column 0
    const int n = A.t_len[pair], w = search_hit_window(keep.r, n, keep.d);
    A.o_pair[t] = pair; A.o_m[t] = keep.r; A.o_n[t] = w; A.o_score[t] = keep.d; A.o_end[t] = w;
    A.o_plp_off[pair] = (int64_t)t * A.plane_stride;
    int32_t* o = A.heads + 4 * (int64_t)pair;
    o[0] = keep.p; o[1] = keep.r; o[2] = w; o[3] = keep.d;
}
// the member's last `len` bases: row `row` of the task's pattern is bits [m - len + 64 row, + 64) of the forward planes, cut
// at the member's end; rows past the suffix are zeros
template <class Eq>
QE_S_HD void panel_head_planes_slot(const PanelHeadPlanesArgs& A, int t) {
    const int pair = A.o_pair[t];
    if (pair < 0) return;
    const int p = A.heads[4 * (int64_t)pair], len = A.heads[4 * (int64_t)pair + 1], nw = (len + 63) >> 6, m = A.m_len[p];
    const uint64_t* src = A.pl_m + Eq::offset(A.m_off[p]);
    uint64_t* dst = A.pool + Eq::offset(A.o_plp_off[pair]);
    for (int row = 0; row < nw + 2; ++row) {
        uint64_t x[Eq::W];
        for (int k = 0; k < Eq::W; ++k) x[k] = 0;
        if (row < nw) {
            const int left = len - 64 * row, ncols = left < 64 ? left : 64;
            search_text_words<Eq::W>(src, m - left, ncols, x);
            if (ncols < 64) for (int k = 0; k < Eq::W; ++k) x[k] &= ((uint64_t)1 << ncols) - 1;
        }
        for (int k = 0; k < Eq::W; ++k) dst[Eq::W * (int64_t)row + k] = x[k];
    }
}
// k_panel_heads_finish's slot t: the end pass's largest end is its window less o_start
QE_S_HD void panel_heads_finish_slot(int t, const int32_t* o_pair, const int32_t* o_start, int32_t* heads) {
    const int pair = o_pair[t];
    if (pair < 0) return;
    int32_t* o = heads + 4 * (int64_t)pair;
    o[2] = o_start[t] < 0 ? -1 : o[2] - o_start[t];
}

// ---- every occurrence of every member, long texts split across lanes (quicked_batch_run_panel_scan)
// A lane is a WINDOW SLOT {pair, c0, c1}: it owns the occurrences of its text whose text_end lies in (c0, c1] (c0 a multiple
// of 64, c1 = min(c0 + window, n)) and nothing else.  Per member of m bases and effective bound k it walks three stretches:
//   warm-up   (ws, c0], ws = max(0, c0 - 64 ceil((m + k) / 64)): a fresh INFIX sweep from column ws.  An occurrence of score
//             <= k that ends at e starts no earlier than e - (m + k), so the sweep's row m equals the text's wherever that is
//             <= k from column c0 on, and is above k wherever that is: min(R', k + 1) = min(R, k + 1) for every e >= c0, which
//             is all the scan reads (qe_search.h) -- c0 itself is the `prev` of the first owned column.  ws = 0 is the text's
//             own column 0.  The scan runs but owns nothing.
//   owned     (c0, c1]: a descent makes a candidate.
//   run-out   columns after c1, chunk by chunk while the candidate is still pending: a rise or the text's end emits it, a
//             descent cancels it (SearchOwnedColumns: that valley is the next window's).
// Every occurrence is owned by the one window that holds its text_end, so the lanes of a text together emit the text's set
// once.  The lane's stretch holds its slice's occurrences in (member, text_end) order, the first `cap` of them.
typedef SearchHitScanOf<PanelHitSink, SearchOwnedColumns> PanelWindowScan;
QE_S_HD void panel_window_scan_init(PanelWindowScan& H, PanelRawHit* out, int32_t cap, int32_t c0, int32_t c1) {
    H.lo = c0; H.hi = c1;
    H.prev = 0; H.pend_end = -1; H.pend_val = 0; H.found = 0; H.best = -1;
    H.sink.out = out; H.sink.cap = cap; H.sink.count = 0; H.sink.member = -1;
}
// the warm-up of a member: whole chunks, so that chunk boundaries and ownership boundaries coincide
QE_S_HD int panel_window_warmup(int m, int bound) { return 64 * ((m + search_effective(bound, m) + 63) / 64); }

// one member of NB blocks at the most against the window (c0, c1] of one text of n columns: the register form
template <int NB, class Eq>
QE_S_HD void panel_member_window(const uint64_t* pp, int m, int bound, const uint64_t* tp, int n, int c0, int c1, PanelWindowScan& H, uint32_t& steps) {
    SearchLane L;
    search_lane_init(L, m, n, SEARCH_INFIX, bound, 0);
    SearchRegStore<NB, Eq> R;
    QE_S_UNROLL
    for (int b = 0; b < NB; ++b) { R.pv[b] = R.mv[b] = 0; R.s[b] = 0; }      // (not R.clear(): profiles/panel_shells.md)
    R.load(pp, m);
    H.begin(L);
    search_store_init<NB>(R, L);
    const int warm = panel_window_warmup(m, bound);
    int col0 = c0 > warm ? c0 - warm : 0;
    // warm-up and owned columns, then the run-out while a candidate is pending (c1 is a chunk boundary or the text's end)
    for (; col0 < c1 || (col0 < n && H.pend_end >= 0); col0 += 64) {
        const int ncols = n - col0 < 64 ? n - col0 : 64;
        uint64_t t[Eq::W];
        Eq::text_chunk(tp, col0, ncols, t);
        search_chunk<NB>(R, L, t, col0, ncols, H);
    }
    H.finish();                                 // still pending: the walk reached the end of the text, where a plateau counts
    steps += L.steps;
}

// The window (c0, c1] of one text (planes tp, n columns; c1 <= c0: nothing) against the members [p0, p1): every occurrence
// the window owns goes to H's sink, H.found / H.best run on over the members; steps: block steps, added to
template <class Eq>
QE_S_HD void panel_window_hits(const PanelView& P, int p0, int p1, const uint64_t* tp, int n, int c0, int c1, PanelWindowScan& H, uint32_t& steps) {
    panel_each_member<Eq>(P, p0, p1, [&](auto NB, int p, const uint64_t* pp, int m, int bound) {
        H.sink.member = p;
        panel_member_window<NB, Eq>(pp, m, bound, tp, n, c0, c1, H, steps);
    });
}

// k_panel_scan<Eq>: k_panel_hits' shape with window slots for text slots.  Window slot w (nslots of them, a multiple of 64)
// is {text[w] (-1: an empty slot), w_c0[w], w_c1[w]}; a text's slots are contiguous and ascending by window.  Per (slice s,
// slot w): field f of {found, stored, best, steps} at part[(f nslices + s) nslots + w] and the stored occurrences as PanelRawHit
// number i at raw[(s nslots + w) max_hits + i].  A slot without a text writes nothing.
struct PanelScanArgs : PanelSweepArgs {
    const int32_t* w_c0;  const int32_t* w_c1;
    int32_t max_hits;
    int32_t* part;
    PanelRawHit* raw;
};
// The counts, in two steps so that a long text's slots are not one thread's work.  One thread per (slice s, text slot t)
// (k_panel_scan_sums; text[t] the pair, -1: none) over the text's window slots [first_slot[pair], + nwin[pair]): field f of
// {found, stored saturating at max_hits, best, steps} of that slice at sums[(f nslices + s) ntext + t].  Then one thread per
// text slot t (k_panel_scan_count) over the slices: found[pair], best[pair], len[pair] = stored - 1 and o_adv[t] as
// panel_hits_count_slot leaves them, and per slice the rank of its first record among the text's: base[s ntext + t] = the
// stored counts of the slices before s, saturating at max_hits.
struct PanelScanCountArgs {
    int32_t ntext, nslots, nslices, max_hits;
    const int32_t* text;  const int32_t* first_slot;  const int32_t* nwin;  const int32_t* part;
    int32_t* sums;
    int32_t* found;  int32_t* best;  int32_t* len;  int32_t* base;  uint32_t* o_adv;
};
// One thread per lane (slice s, window slot w) (k_panel_scan_expand).  The rank of the lane's record r = (p, e) among its
// text's records in (pattern, text_end) order is base[s][text] + the number of records with a smaller key in the lanes
// (w', s) of the text's windows: r's own index for w' = w; for w' < w every end is smaller than e, so the records with member
// <= p; for w' > w every end is larger, so those with member < p -- one binary search per window, repeated only when the
// member changes.  A record whose rank is below max_hits goes to hits[off[pair] + rank] with its start-pass task at the same
// index (as panel_hits_expand_slot writes them); the others are dropped.
// Ranks below max_hits are exact although a lane keeps only its first max_hits: every record before r in its own lane is
// before it in the text, so rank-in-lane <= rank-in-text and the text's first max_hits are all stored; and a lane that lost
// a record q < r holds max_hits stored records that are all < q < r, which puts r's computed rank at max_hits or above.
struct PanelScanExpandArgs {
    int32_t ntext, nslots, nslices, max_hits;
    const int32_t* w_pair;  const int32_t* w_text;  const int32_t* first_slot;  const int32_t* nwin;
    const int32_t* part;  const PanelRawHit* raw;  const int32_t* base;
    const int64_t* off;
    const int32_t* m_len;  const int64_t* m_off;  const int32_t* t_len;  const int64_t* t_off;
    int32_t* hits;
    int32_t* o_pair;  int32_t* o_m;  int32_t* o_n;  int32_t* o_score;  int32_t* o_end;  int64_t* o_plp_off;  int64_t* o_plt_off;
};

QE_S_HD void panel_scan_store_part(const PanelScanArgs& A, int nslices, int slice, int slot, const PanelWindowScan& H, uint32_t steps) {
    const int64_t stride = (int64_t)nslices * A.nslots;
    int32_t* q = A.part + (int64_t)slice * A.nslots + slot;
    q[0] = H.found; q[stride] = H.sink.count; q[2 * stride] = H.best; q[3 * stride] = (int32_t)steps;
}
QE_S_HD void panel_scan_sums_slice(const PanelScanCountArgs& A, int s, int t) {
    const int pair = A.text[t];
    if (pair < 0) return;
    const int64_t stride = (int64_t)A.nslices * A.nslots, tstride = (int64_t)A.nslices * A.ntext;
    const int w0 = A.first_slot[pair], w1 = w0 + A.nwin[pair];
    int32_t found = 0, stored = 0, best = -1;
    uint32_t steps = 0;
    for (int w = w0; w < w1; ++w) {
        const int32_t* q = A.part + (int64_t)s * A.nslots + w;
        const int32_t b = q[2 * stride];
        found += q[0];
        stored = stored + q[stride] < A.max_hits ? stored + q[stride] : A.max_hits;
        best = (b >= 0 && (best < 0 || b < best)) ? b : best;
        steps += (uint32_t)q[3 * stride];
    }
    int32_t* o = A.sums + (int64_t)s * A.ntext + t;
    o[0] = found; o[tstride] = stored; o[2 * tstride] = best; o[3 * tstride] = (int32_t)steps;
}
QE_S_HD void panel_scan_count_text(const PanelScanCountArgs& A, int t) {
    const int pair = A.text[t];
    if (pair < 0) return;
    const int64_t tstride = (int64_t)A.nslices * A.ntext;
    int32_t found = 0, stored = 0, best = -1;
    uint32_t steps = 0;
    for (int s = 0; s < A.nslices; ++s) {
        const int32_t* q = A.sums + (int64_t)s * A.ntext + t;
        const int32_t b = q[2 * tstride];
        A.base[(int64_t)s * A.ntext + t] = stored;
        found += q[0];
        stored = stored + q[tstride] < A.max_hits ? stored + q[tstride] : A.max_hits;
        best = (b >= 0 && (best < 0 || b < best)) ? b : best;
        steps += (uint32_t)q[3 * tstride];
    }
    A.found[pair] = found; A.best[pair] = best; A.len[pair] = stored - 1;
    A.o_adv[t] = steps;
}
// the records of a lane's stretch (sorted by member, `have` of them) with member < p (or_equal: <= p)
QE_S_HD int32_t panel_scan_members_below(const PanelRawHit* raw, int32_t have, int32_t p, bool or_equal) {
    int32_t lo = 0, hi = have;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        const int32_t q = raw[mid].pattern;
        if (q < p || (or_equal && q == p)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// TASKS: with the records' start-pass tasks; without (the mismatch-only scan, qe_panel_ham.h) text_start is left 0 and no o_* is touched
template <bool TASKS>
QE_S_HD void panel_scan_expand_lane_of(const PanelScanExpandArgs& A, int s, int w) {
    const int pair = A.w_pair[w];
    if (pair < 0) return;
    const int64_t stride = (int64_t)A.nslices * A.nslots;
    const int32_t* stored = A.part + stride + (int64_t)s * A.nslots;              // [slot], of this slice
    const int32_t have = stored[w], base = A.base[(int64_t)s * A.ntext + A.w_text[w]];
    if (have <= 0 || base >= A.max_hits) return;
    const int w0 = A.first_slot[pair], w1 = w0 + A.nwin[pair];
    const PanelRawHit* raw = A.raw + ((int64_t)s * A.nslots + w) * A.max_hits;
    const int n = A.t_len[pair];
    const int64_t j0 = A.off[pair];
    int32_t member = -1, others = 0;
    for (int32_t i = 0; i < have; ++i) {
        const PanelRawHit h = raw[i];
        if (h.pattern != member) {
            member = h.pattern; others = 0;
            for (int v = w0; v < w1 && base + i + others < A.max_hits; ++v)
                if (v != w && stored[v] > 0)
                    others += panel_scan_members_below(A.raw + ((int64_t)s * A.nslots + v) * A.max_hits, stored[v], member, v < w);
        }
        const int32_t rank = base + i + others;
        if (rank >= A.max_hits) break;          // (ranks ascend within a lane)
        const int64_t j = j0 + rank;
        int32_t start = 0;
        if (TASKS) {
            const int m = A.m_len[h.pattern];
            int32_t task_n, in_end;
            search_hit_task(m, n, h.end, h.score, task_n, in_end, start);
            A.o_pair[j] = (int32_t)j; A.o_m[j] = m; A.o_n[j] = task_n; A.o_score[j] = h.score; A.o_end[j] = in_end;
            A.o_plp_off[j] = A.m_off[h.pattern]; A.o_plt_off[j] = A.t_off[pair];
        }
        int32_t* o = A.hits + 4 * j;
        o[0] = h.pattern; o[1] = start; o[2] = h.end; o[3] = h.score;
    }
}
QE_S_HD void panel_scan_expand_lane(const PanelScanExpandArgs& A, int s, int w) { panel_scan_expand_lane_of<true>(A, s, w); }

}  // namespace qe
