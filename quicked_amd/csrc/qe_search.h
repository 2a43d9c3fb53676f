// qe_search.h -- approximate pattern search: "where in this text does the pattern fit best, and at what cost?"
// (quicked_batch_run_search).  Plain C++ with no HIP dependency: k_search<NB> (qe_kernels.hip; NB > 0 the register form, 0 the workspace form) runs it one lane
// per task, the host stand-ins of the stub build run it on the host, and the CPU suite compiles the very same source with
// g++ (tests/native/search_cpu.cpp) and checks it against a brute-force DP and edlib's HW / SHW modes.
//
// The matrix.  D is the edit-distance matrix of the pattern (rows, m) against the text (columns, n) under the library's
// equality (two symbols are equal when both are not-ACGT, or neither is and the code bits agree; qe_bounded.h).  INFIX has
// a top row of zeros -- an occurrence may start in any column --, PREFIX has D[0][j] = j.  The answer is
//   d = min over e in 1 .. n of D[m][e],   end = the smallest such e   (SEARCH_LARGEST_END: the largest),
// or "beyond" (-1, -1) when d exceeds the task's bound.  SEARCH_LAST_COLUMN reads column n only: with PREFIX that is the
// global distance.  No search distance exceeds m (D[m][1] <= m), so the bound is clamped to m.
//
// The sweep.  Myers' column sweep in the tree's carry-word convention, over blocks of 64 pattern rows and
// chunks of 64 text columns: a block over a chunk takes the horizontal deltas of the row above it as two 64-bit words (bit
// c = column c of the chunk) and leaves those of its last row.  The top block's carry-in is zero for INFIX and all-plus for
// PREFIX.  The last block takes the RAW, pre-shift deltas at bit (m - 1) & 63 -- row m's -- instead of bit 63's: the rows
// of that block below row m hold zero planes and garbage values that never reach a row above them (every cell depends on
// rows at or above its own only, and the carry of the addition runs towards higher rows).
//
// The live-block rule, one decision per chunk.  k = the task's current bound, S_b = the computed value of block b's last
// row in the chunk's start column (column 64 c; column 0 before the first chunk, where S_b = min(64 (b + 1), m)).  The
// chunk computes blocks 0 .. L + 1, L = the lowest-lying computed block with S_b <= k + 63 (-1: none; block 0 is always
// computed: a new occurrence can start in any column).  A block that (re)enters starts from "the cell above + 1" in every
// row -- Pv all ones, S = S_above + its rows --: stale state is never reused.  Why that loses no answer:
//   * computed values are costs of real paths (a skipped block's cells are never read as cheaper than they are, an
//     entering block's are a vertical run below a computed cell), so they are >= the true values;
//   * they are exact wherever the true value is <= k: the cells of a path of cost <= k all have values <= k, and by
//     induction over the chunks each of them lies in a computed block (last point);
//   * computed vertical deltas are in {-1, 0, 1}, so a block holding a cell <= k has S_b <= k + 63;
//   * values never decrease along a diagonal, so a cell <= k within the next 64 columns lies at most 64 rows below a cell
//     <= k of this column (or starts in row 0 and is in block 0): in block L + 1 at the lowest.
// At most one block enters per chunk (L + 1 <= the blocks computed so far).  Lowering k to best - 1 once a result
// best <= k is found keeps all of this -- a later column only matters when it is strictly better -- and makes "the smallest
// end among the minima" free.  SEARCH_LARGEST_END keeps k = best instead.  SEARCH_ALL_LIVE computes every block of every
// chunk (the form the rule is tested against).
//
// The end-position scan.  Row m's two delta words give its 64 values in the chunk from the value at the chunk's start; they
// are scanned only when start - popcount(minus word) <= k.
//
// Every occurrence (quicked_batch_run_search_all).  R[e] = D[m][e]; position e is an occurrence when R[e] <= k, R[e] <
// R[e - 1] (column 0 counts as higher than every value) and the first later column with another value, if there is one,
// has a higher one: the first column of a valley of row m.  SearchHitScan replaces the scan above: k stays the task's
// bound for the whole text, the lane never stops early, and the valleys go to a small sink in the order of their ends.
// The set depends on min(R[e], k + 1) only -- a value above k is no occurrence, ends a plateau as a rise whatever it is, and
// is a column every value <= k lies below -- and the sweep's values are exact wherever the true value is <= k and above k
// wherever it is not (the rule's first two points), so the scan walks w = min(computed value, k + 1).
//
// The equality is a parameter.  Everything above argues from path costs only -- what a cell costs given the cells it is
// reached from -- and never from what makes two symbols equal: the recurrence takes any Eq word, and the live-block rule,
// the two scans, the start pass over the reversed sequences (a path read backwards has the cost it has forwards: the relation
// is applied to the same two symbols) and the m + score window hold for any match relation between a pattern symbol and a
// text symbol, symmetric or not, transitive or not.  So the equality is a small policy type that the stores carry (Store::Eq):
// how many plane words a block and a chunk have (W), where a sequence's words start, how they are loaded, and how Eq is formed
// for column c.  SearchEq3 is the library's equality above over the three planes of qe_types.h and the default everywhere;
// SearchEqIupac is the set-intersection equality over the four membership planes of qe_iupac.h.
#pragma once
#include <stdint.h>

#include "qe_bounded.h"
#include "qe_iupac.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QE_S_HD __host__ __device__ __forceinline__
#else
#define QE_S_HD inline
#endif
#if defined(__HIPCC__)
#define QE_S_UNROLL _Pragma("unroll")      // before a loop over a store's blocks: hipcc's pragma, nothing for g++
#else
#define QE_S_UNROLL
#endif

namespace qe {

enum : int { SEARCH_PREFIX = 1, SEARCH_INFIX = 2 };                               // quicked_search_mode_t
enum : int { SEARCH_LARGEST_END = 1, SEARCH_LAST_COLUMN = 2, SEARCH_ALL_LIVE = 4 };
enum : int { QE_SEARCH_REG_BLOCKS = 4 };                                          // the most blocks the register form holds

QE_S_HD int search_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}
// the bound a task is decided with: no search distance exceeds the pattern's length
QE_S_HD int search_effective(int bound, int m) { return bound < m ? bound : m; }
QE_S_HD int search_blocks(int m) { return (m + 63) >> 6; }
QE_S_HD int search_rows(int b, int m) { const int r = m - 64 * b; return r < 64 ? r : 64; }      // rows of block b
// blocks 0 .. L + 1 for "L = the last block of the first `have` with S <= k + 63" (at least the top block, at most nb)
QE_S_HD int search_want(int L, int nb) { const int w = L + 2 < nb ? L + 2 : nb; return w < 1 ? 1 : w; }
// blocks that are live before the first chunk: column 0 holds S_b = min(64 (b + 1), m)
QE_S_HD int search_first_live(int k, int m, int flags) {
    const int nb = search_blocks(m);
    if (flags & SEARCH_ALL_LIVE) return nb;
    int L = -1;
    for (int b = 0; b < nb; ++b) if ((b + 1 < nb ? 64 * (b + 1) : m) <= k + 63) L = b;
    return search_want(L, nb);
}

// 64 text columns starting at bit offset `bit` of a text's planes, W words per 64 bases; words past the one that holds the
// chunk's last column (bit + ncols - 1) are not read
template <int W>
QE_S_HD void search_text_words(const uint64_t* tp, int64_t bit, int ncols, uint64_t (&t)[W]) {
    const int64_t w = bit >> 6;
    const int sh = (int)(bit & 63);
    const uint64_t* q = tp + W * w;
    for (int k = 0; k < W; ++k) t[k] = q[k] >> sh;
    if (sh && ((bit + ncols - 1) >> 6) > w) for (int k = 0; k < W; ++k) t[k] |= q[W + k] << (64 - sh);
}

// The library's equality over three planes {code bit 0, code bit 1, not-ACGT}: both not-ACGT, or neither and the codes agree
struct SearchEq3 {
    enum : int { W = 3 };
    static QE_S_HD int64_t offset(int64_t off3) { return off3; }                  // of a sequence, from its three-plane word offset
    static QE_S_HD void pattern_rows(const uint64_t* pp, int m, int b, uint64_t (&p)[W]) { bounded_pattern_rows(pp, m, 64 * b, p[0], p[1], p[2]); }
    static QE_S_HD void text_chunk(const uint64_t* tp, int64_t bit, int ncols, uint64_t (&t)[W]) { search_text_words<W>(tp, bit, ncols, t); }
    static QE_S_HD uint64_t eq(const uint64_t (&p)[W], const uint64_t (&t)[W], int c) {
        const uint64_t m0 = (uint64_t)0 - ((t[0] >> c) & 1), m1 = (uint64_t)0 - ((t[1] >> c) & 1), mn = (uint64_t)0 - ((t[2] >> c) & 1);
        const uint64_t acgt = ~(p[0] ^ m0) & ~(p[1] ^ m1) & ~p[2];
        return (mn & p[2]) | (~mn & acgt);
    }
    // position-wise: bit r is row r of p against position r of t (qe_panel_ham.h), where eq() holds one column against every row
    static QE_S_HD uint64_t eq_pos(const uint64_t (&p)[W], const uint64_t (&t)[W]) {
        return (p[2] & t[2]) | (~(p[2] | t[2]) & ~((p[0] ^ t[0]) | (p[1] ^ t[1])));
    }
};
// Set intersection over four membership planes {A, C, G, T} (qe_iupac.h): a row matches the column when they share a base
struct SearchEqIupac {
    enum : int { W = 4 };
    static QE_S_HD int64_t offset(int64_t off3) { return iupac_offset(off3); }
    static QE_S_HD void pattern_rows(const uint64_t* pp, int m, int b, uint64_t (&p)[W]) {      // rows 64 b .. of the pattern; none: zeros
        const bool in = b < ((m + 63) >> 6);
        for (int k = 0; k < W; ++k) p[k] = in ? pp[W * (int64_t)b + k] : 0;
    }
    static QE_S_HD void text_chunk(const uint64_t* tp, int64_t bit, int ncols, uint64_t (&t)[W]) { search_text_words<W>(tp, bit, ncols, t); }
    static QE_S_HD uint64_t eq(const uint64_t (&p)[W], const uint64_t (&t)[W], int c) {
        const uint64_t mA = (uint64_t)0 - ((t[0] >> c) & 1), mC = (uint64_t)0 - ((t[1] >> c) & 1);
        const uint64_t mG = (uint64_t)0 - ((t[2] >> c) & 1), mT = (uint64_t)0 - ((t[3] >> c) & 1);
        return (mA & p[0]) | (mC & p[1]) | (mG & p[2]) | (mT & p[3]);
    }
    static QE_S_HD uint64_t eq_pos(const uint64_t (&p)[W], const uint64_t (&t)[W]) {      // position-wise, as SearchEq3::eq_pos
        return (p[0] & t[0]) | (p[1] & t[1]) | (p[2] & t[2]) | (p[3] & t[3]);
    }
};

QE_S_HD void search_text_chunk(const uint64_t* tp, int64_t bit, int ncols, uint64_t& t0, uint64_t& t1, uint64_t& tn) {
    uint64_t t[3];
    SearchEq3::text_chunk(tp, bit, ncols, t);
    t0 = t[0]; t1 = t[1]; tn = t[2];
}

// One block over one chunk: Pv / Mv the block's vertical deltas, p its pattern planes, t the chunk's text planes (Eq::W words
// each), hinP / hinM the horizontal deltas of the row above.  Leaves in oP / oM the raw horizontal deltas of the block's
// row `lvl` (63: its last row = the carry words of the block below), bits >= ncols zero.
template <class Eq = SearchEq3>
QE_S_HD void search_block_chunk(uint64_t& Pv, uint64_t& Mv, const uint64_t (&p)[Eq::W], const uint64_t (&t)[Eq::W],
                                uint64_t hinP, uint64_t hinM, int lvl, int ncols, uint64_t& oP, uint64_t& oM) {
    uint64_t P = Pv, M = Mv, qP = 0, qM = 0;
    for (int c = 0; c < ncols; ++c) {
        const uint64_t E = Eq::eq(p, t, c);
        const uint64_t PHin = (hinP >> c) & 1, MHin = (hinM >> c) & 1;
        const uint64_t Xv = E | M;
        const uint64_t Eqc = E | MHin;
        const uint64_t Xh = (((Eqc & P) + P) ^ P) | Eqc;
        uint64_t Ph = M | ~(Xh | P);
        uint64_t Mh = P & Xh;
        qP |= ((Ph >> lvl) & 1) << c;
        qM |= ((Mh >> lvl) & 1) << c;
        Ph = (Ph << 1) | PHin;
        Mh = (Mh << 1) | MHin;
        P = Mh | ~(Xv | Ph);
        M = Ph & Xv;
    }
    Pv = P; Mv = M; oP = qP; oM = qM;
}
// ... with the three planes of the library's equality word by word: (a, b, nn) the block's, (T0, T1, TN) the chunk's
QE_S_HD void search_block_chunk(uint64_t& Pv, uint64_t& Mv, uint64_t a, uint64_t b, uint64_t nn, uint64_t T0, uint64_t T1, uint64_t TN,
                                uint64_t hinP, uint64_t hinM, int lvl, int ncols, uint64_t& oP, uint64_t& oM) {
    const uint64_t p[3] = {a, b, nn}, t[3] = {T0, T1, TN};
    search_block_chunk<SearchEq3>(Pv, Mv, p, t, hinP, hinM, lvl, ncols, oP, oM);
}

// what a lane carries besides its blocks' {Pv, Mv, S}
struct SearchLane {
    int32_t m, n, nb, mode, flags;
    int32_t k;              // the current bound
    int32_t live;           // blocks 0 .. live - 1 hold computed state
    int32_t best, end;      // -1, -1: nothing within the bound yet
    uint32_t steps;         // block steps (one per block per column)
};

QE_S_HD void search_lane_init(SearchLane& L, int m, int n, int mode, int bound, int flags) {
    L.m = m; L.n = n; L.nb = search_blocks(m); L.mode = mode; L.flags = flags;
    L.k = search_effective(bound, m);
    L.live = search_first_live(L.k, m, flags);
    L.best = -1; L.end = -1; L.steps = 0;
}

// row m's values in the chunk that starts at column col0 (0-based; its first column is end position col0 + 1)
QE_S_HD void search_scan(SearchLane& L, int32_t start, uint64_t oP, uint64_t oM, int col0, int ncols) {
    if (start - search_popc(oM) > L.k) return;
    int32_t v = start;
    for (int c = 0; c < ncols; ++c) {
        v += (int32_t)((oP >> c) & 1) - (int32_t)((oM >> c) & 1);
        if (v > L.k) continue;
        if ((L.flags & SEARCH_LAST_COLUMN) && col0 + c + 1 != L.n) continue;
        L.best = v; L.end = col0 + c + 1;
        L.k = (L.flags & SEARCH_LARGEST_END) ? v : v - 1;
    }
}

// The state of a lane's blocks.  NBT > 0: at most NBT blocks, every index a compile-time constant after unrolling (the
// register form: arrays that stay in registers); NBT == 0: any number (the workspace form).  A store has
//   typedef .. Eq;  uint64_t& P(int b), & M(int b);  int32_t& S(int b);  void planes(int b, uint64_t (&p)[Eq::W])
//
// One chunk: text columns [col0, col0 + ncols) of the task, planes t (Store::Eq::W words; the library's equality also as
// (T0, T1, TN)).
//
// Scan: what becomes of row m.  row(): the last block was computed, its row-m deltas are (oP, oM) from the value `start`;
// no_row(): the chunk left the last block out.
template <int NBT, class Store, class Scan>
QE_S_HD void search_chunk(Store& st, SearchLane& L, const uint64_t (&t)[Store::Eq::W], int col0, int ncols, Scan& scan) {
    typedef typename Store::Eq Eq;
    constexpr int UF = NBT ? NBT : 1;                         // the register form unrolls over its blocks; the workspace form does not
    (void)UF;
    const int nbl = NBT ? NBT : L.nb;
    // ---- the live-block rule
    int want = L.nb;
    if (!(L.flags & SEARCH_ALL_LIVE)) {
        int low = -1;
#if defined(__HIPCC__)
#pragma unroll UF
#endif
        for (int b = 0; b < nbl; ++b) if (b < L.live && st.S(b) <= L.k + 63) low = b;
        want = search_want(low, L.nb);
    }
#if defined(__HIPCC__)
#pragma unroll UF
#endif
    for (int b = 1; b < nbl; ++b)
        if (b == L.live && want > L.live) {                      // enters: the cell above + 1 in every row
            st.P(b) = ~(uint64_t)0; st.M(b) = 0;
            st.S(b) = st.S(b - 1) + search_rows(b, L.m);
        }
    L.live = want;
    // ---- the live blocks, top-down
    uint64_t hP = (L.mode == SEARCH_PREFIX) ? ~(uint64_t)0 : 0, hM = 0;
#if defined(__HIPCC__)
#pragma unroll UF
#endif
    for (int b = 0; b < nbl; ++b) {
        if (b >= L.live) continue;
        uint64_t p[Eq::W], oP, oM;
        st.planes(b, p);
        const bool last = b == L.nb - 1;
        search_block_chunk<Eq>(st.P(b), st.M(b), p, t, hP, hM, last ? ((L.m - 1) & 63) : 63, ncols, oP, oM);
        const int32_t start = st.S(b);
        st.S(b) = start + search_popc(oP) - search_popc(oM);
        if (last) scan.row(L, start, oP, oM, col0, ncols);
        hP = oP; hM = oM;
        L.steps += (uint32_t)ncols;
    }
    if (L.live < L.nb) scan.no_row(L);
}
// the scan of the best search: the default
struct SearchBestScan {
    QE_S_HD void row(SearchLane& L, int32_t start, uint64_t oP, uint64_t oM, int col0, int ncols) { search_scan(L, start, oP, oM, col0, ncols); }
    QE_S_HD void no_row(SearchLane&) {}
};
template <int NBT, class Store>
QE_S_HD void search_chunk(Store& st, SearchLane& L, const uint64_t (&t)[Store::Eq::W], int col0, int ncols) {
    SearchBestScan scan;
    search_chunk<NBT>(st, L, t, col0, ncols, scan);
}
template <int NBT, class Store, class Scan>
QE_S_HD void search_chunk(Store& st, SearchLane& L, uint64_t T0, uint64_t T1, uint64_t TN, int col0, int ncols, Scan& scan) {
    const uint64_t t[3] = {T0, T1, TN};
    search_chunk<NBT>(st, L, t, col0, ncols, scan);
}
template <int NBT, class Store>
QE_S_HD void search_chunk(Store& st, SearchLane& L, uint64_t T0, uint64_t T1, uint64_t TN, int col0, int ncols) {
    const uint64_t t[3] = {T0, T1, TN};
    search_chunk<NBT>(st, L, t, col0, ncols);
}

// ---- every occurrence.  Where a lane's occurrences go: {end, score} number i at out[i * stride], the first `cap` of them
struct SearchHit { int32_t end, score; };
struct SearchHitSink {
    SearchHit* out; int64_t stride; int32_t cap, count;
    QE_S_HD void put(int32_t end, int32_t score) {
        if (count < cap) { out[(int64_t)count * stride] = SearchHit{end, score}; ++count; }
    }
};
// what a lane carries besides SearchLane: w of the previous column, the candidate -- the first column of a plateau that was
// reached by a descent and has not risen yet (end < 0: none) --, the occurrences so far and the smallest score among them.
// Sink: where an occurrence goes, put(end, score) -- the one thing a caller may vary; what an occurrence is is decided here
// and nowhere else.  A scan may serve several patterns against one text in turn (a panel lane: qe_panel.h): begin() starts a
// pattern -- column 0, no candidate --, found / best / the sink run on.
//
// Range: which columns a descent may make a candidate in.  SearchAllColumns (the default: every column, no state) is the scan
// of a lane that walks a whole text; SearchOwnedColumns is a lane that owns the columns (lo, hi] of a text other lanes walk
// too (a window of quicked_batch_run_panel_scan): a descent outside the range clears the candidate -- the
// valley it starts is another lane's --, everything else is the same walk.
struct SearchAllColumns { QE_S_HD bool owns(int32_t) const { return true; } };
struct SearchOwnedColumns {
    int32_t lo, hi;
    QE_S_HD bool owns(int32_t end) const { return end > lo && end <= hi; }
};
template <class Sink = SearchHitSink, class Range = SearchAllColumns>
struct SearchHitScanOf : Range {
    int32_t prev, pend_end, pend_val, found, best;
    Sink sink;
    QE_S_HD void begin(const SearchLane& L) {
        prev = L.k + 1;                              // column 0: higher than every value that counts
        pend_end = -1; pend_val = 0;
    }
    QE_S_HD void init(const SearchLane& L, SearchHit* out, int64_t stride, int32_t cap) {
        begin(L);
        found = 0; best = -1;
        sink.out = out; sink.stride = stride; sink.cap = cap; sink.count = 0;
    }
    QE_S_HD void emit() {                            // the row has risen, or the text is over: the candidate is a valley
        if (pend_end < 0) return;
        sink.put(pend_end, pend_val);
        ++found;
        if (best < 0 || pend_val < best) best = pend_val;
        pend_end = -1;
    }
    QE_S_HD void row(SearchLane& L, int32_t start, uint64_t oP, uint64_t oM, int col0, int ncols) {
        // The popcount test says that every value of the chunk is above k.  With no candidate pending the chunk changes
        // nothing but `prev`, and that only to k + 1: values above k need not be exact (min(R, k + 1), above).  With one
        // pending the chunk's first column is the rise that makes it an occurrence, so the walk below has to see it.
        if (pend_end < 0 && start - search_popc(oM) > L.k) { prev = L.k + 1; return; }
        int32_t v = start;
        for (int c = 0; c < ncols; ++c) {
            v += (int32_t)((oP >> c) & 1) - (int32_t)((oM >> c) & 1);
            const int32_t w = v <= L.k ? v : L.k + 1;
            if (w < prev) { pend_end = Range::owns(col0 + c + 1) ? col0 + c + 1 : -1; pend_val = w; }      // a descent (w <= k: prev <= k + 1); an older candidate was no valley
            else if (w > prev) emit();
            prev = w;
        }
    }
    // The last block was not computed: by the rule no cell of it in this chunk is <= k (a cell <= k lies in a computed
    // block), so row m has risen above k
    QE_S_HD void no_row(SearchLane& L) { emit(); prev = L.k + 1; }
    QE_S_HD void finish() { emit(); }                // a plateau that reaches the end of the text counts
};
typedef SearchHitScanOf<> SearchHitScan;

// before the first chunk: the live blocks hold column 0
template <int NBT, class Store>
QE_S_HD void search_store_init(Store& st, const SearchLane& L) {
    constexpr int UF = NBT ? NBT : 1;
    (void)UF;
    const int nbl = NBT ? NBT : L.nb;
#if defined(__HIPCC__)
#pragma unroll UF
#endif
    for (int b = 0; b < nbl; ++b) {
        if (b >= L.live) continue;
        st.P(b) = ~(uint64_t)0; st.M(b) = 0;
        st.S(b) = b + 1 < L.nb ? 64 * (b + 1) : L.m;
    }
}

// the answer of a finished lane: {d, end}, or {-1, -1} = beyond the bound
QE_S_HD void search_answer(const SearchLane& L, int32_t& score, int32_t& end) { score = L.best; end = L.best < 0 ? -1 : L.end; }

// The workspace form's store: Pv / Mv / S of block b at stride `stride` elements (64 on the device: [block][lane]), the
// pattern planes read from memory every chunk
template <class E>
struct SearchWsStoreOf {
    typedef E Eq;
    uint64_t* pv; uint64_t* mv; int32_t* s; int64_t stride;
    const uint64_t* pp; int32_t m;
    QE_S_HD uint64_t& P(int b) { return pv[(int64_t)b * stride]; }
    QE_S_HD uint64_t& M(int b) { return mv[(int64_t)b * stride]; }
    QE_S_HD int32_t& S(int b) { return s[(int64_t)b * stride]; }
    QE_S_HD void planes(int b, uint64_t (&p)[E::W]) { E::pattern_rows(pp, m, b, p); }
};
typedef SearchWsStoreOf<SearchEq3> SearchWsStore;
// The register form's: everything of up to NB blocks in arrays
template <int NB, class E = SearchEq3>
struct SearchRegStore {
    typedef E Eq;
    uint64_t pv[NB], mv[NB], pl[NB][E::W]; int32_t s[NB];
    QE_S_HD uint64_t& P(int b) { return pv[b]; }
    QE_S_HD uint64_t& M(int b) { return mv[b]; }
    QE_S_HD int32_t& S(int b) { return s[b]; }
    QE_S_HD void planes(int b, uint64_t (&p)[E::W]) { for (int k = 0; k < E::W; ++k) p[k] = pl[b][k]; }
    QE_S_HD void clear() {
        QE_S_UNROLL
        for (int b = 0; b < NB; ++b) { pv[b] = mv[b] = 0; s[b] = 0; }
    }
    QE_S_HD void load(const uint64_t* pp, int m) {
        QE_S_UNROLL
        for (int b = 0; b < NB; ++b) E::pattern_rows(pp, m, b, pl[b]);
    }
};

// One task, lane by lane as the kernels do it: pattern planes pp (m bases, words [0, W ceil(m / 64))), the text's planes tp
// read from bit offset tbit for n columns.  A lane whose bound has dropped below zero has its answer (an exact occurrence
// at the smallest end) and stops.
template <int NBT, class Store>
QE_S_HD void search_run(Store& st, SearchLane& L, const uint64_t* tp, int64_t tbit) {
    search_store_init<NBT>(st, L);
    for (int col0 = 0; col0 < L.n && L.k >= 0; col0 += 64) {
        const int ncols = L.n - col0 < 64 ? L.n - col0 : 64;
        uint64_t t[Store::Eq::W];
        Store::Eq::text_chunk(tp, tbit + col0, ncols, t);
        search_chunk<NBT>(st, L, t, col0, ncols);
    }
}

// One task of an all-occurrences run: the bound stays, the lane walks the whole text.  flags: 0 or SEARCH_ALL_LIVE
template <int NBT, class Store, class Scan>
QE_S_HD void search_run_hits(Store& st, SearchLane& L, Scan& H, const uint64_t* tp, int64_t tbit) {
    search_store_init<NBT>(st, L);
    for (int col0 = 0; col0 < L.n; col0 += 64) {
        const int ncols = L.n - col0 < 64 ? L.n - col0 : 64;
        uint64_t t[Store::Eq::W];
        Store::Eq::text_chunk(tp, tbit + col0, ncols, t);
        search_chunk<NBT>(st, L, t, col0, ncols, H);
    }
    H.finish();
}
// the columns the start pass of an occurrence {end, score} walks: no stretch is longer than m + score
QE_S_HD int search_hit_window(int m, int end, int score) { return end < m + score ? end : m + score; }
// ... as a task of the best search's start pass (SearchArgs::in_score = score): it walks the in_end columns that end at
// column task_n of the reversed text, so task_n = n - end + window puts the window's last column on text_end; the pass leaves
// text_start - base
QE_S_HD void search_hit_task(int m, int n, int end, int score, int32_t& task_n, int32_t& in_end, int32_t& base) {
    const int w = search_hit_window(m, end, score);
    in_end = w; task_n = n - end + w; base = end - w;
}

}  // namespace qe
