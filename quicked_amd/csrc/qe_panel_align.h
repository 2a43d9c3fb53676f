// qe_panel_align.h -- the alignment (CIGAR) of every stored occurrence of an all-occurrences panel run
// (QUICKED_PANEL_CIGARS on quicked_batch_run_panel_all / _scan).  Plain C++ with no HIP dependency, like
// qe_search.h and qe_panel.h: k_panel_occ_align<Eq> (qe_kernels.hip) runs it one lane per stored occurrence, the host stand-in
// of the stub build runs it occurrence by occurrence, and the CPU suite compiles the very same source with g++
// (tests/native/panel_cigar_cpu.cpp) and checks it against the full matrix (tests/panel_cigar_lib.py).
//
// The definition.  Occurrence j = {pattern, text_start, text_end, score} gets the global alignment of its member (rows 1 .. m)
// against text[text_start, text_end) (columns 1 .. L) under the run's equality.  D is the edit-distance matrix with
// D[0][j] = j and D[i][0] = i.  From (m, L), while i > 0 and j > 0:
//   1. D[i][j] == D[i-1][j] + 1    : D (a pattern symbol against nothing), --i
//   2. D[i][j-1] == D[i-1][j-1] - 1: I (a text symbol against nothing), --j
//   3. else M where the two symbols are equal under the run's equality, X where not, --i and --j
// then the columns left as I and the rows left as D; the string is that sequence read backwards.  It is the reference's
// traceback (bpm_banded.c, banded_backtrace_matrix_cutoff) stated on the full matrix: test 1 is bit i-1 of Pv of column j,
// test 2 bit i-1 of Mv of column j-1.  Every step is an optimal move whatever makes two symbols equal:
//   1. the cell above plus one is this cell's value, so a deletion lies on an optimal path;
//   2. D[i][j-1] = D[i-1][j-1] - 1 and D[i][j] >= D[i-1][j-1] (values never decrease along a diagonal), while D[i][j] <=
//      D[i][j-1] + 1 = D[i-1][j-1]: so D[i][j] = D[i][j-1] + 1, an insertion lies on an optimal path;
//   3. where test 1 fails the vertical move does not reach the minimum.  Where test 2 fails D[i][j-1] >= D[i-1][j-1]; if the
//      horizontal move reaches the minimum, D[i][j] = D[i][j-1] + 1 >= D[i-1][j-1] + 1 >= the diagonal move's value, which is
//      never below D[i][j]: the diagonal move reaches it too.  One of the three does, so the diagonal one does.
// The string therefore has exactly D[m][L] edits; the lane checks that this is the occurrence's score.
//
// The sweep.  Myers' column sweep of qe_search.h, one column at a time (search_block_chunk over one column, carries passed
// down the blocks), with the counted top row -- the carry-in of the top block is +1 in every column -- over up to four blocks
// of 64 rows.  No live-block rule: the stretch is at most m + score columns.  {Pv, Mv} of every block after every column go
// to the HISTORY, laid out [column][block][lane] per wave of 64 occurrences, so that a wave's store of one column and block
// is 1 KiB of contiguous rows.  Column 0 is not stored: Pv all ones, Mv zero.
//
// The string is written BACKWARDS into the occurrence's slot of the pool -- the traceback produces the last operation first --
// and ends at the slot's last byte: the pool is padded in front of a string, off[j] says where it starts.  A run-length
// encoded alignment with d edits has at most 2 d + 1 runs of at most three digits and a letter (L <= 512), so a slot of
// 4 (2 score + 1) + 1 bytes holds any of them; the writer never writes below the slot's first byte whatever it is handed.
//
// Every loop is bounded: the sweep runs L columns, the traceback at most m + L steps (its loop counter).  A lane that does not
// end at (0, 0) with `score` edits, or is handed a task outside the history (text_start < 0, an empty stretch, more columns or
// blocks than the history has) reports -1 and the run returns QUICKED_ERROR: the sweeps and the aligner disagree.
#pragma once
#include <stdint.h>

#include "qe_panel.h"

namespace qe {

enum : int { ALIGN_M = 0, ALIGN_X = 1, ALIGN_I = 2, ALIGN_D = 3 };               // the order of the formatter's letters, "MXID"

struct alignas(16) AlignCell { uint64_t pv, mv; };                                // a block's vertical deltas after a column

// the bytes of occurrence j's slot without the terminator: what k_scan_offsets adds 1 to.  No score exceeds 256
QE_S_HD int32_t panel_align_len(int32_t score) {
    const int32_t s = score < 0 ? 0 : (score > PANEL_MAX_LEN ? PANEL_MAX_LEN : score);
    return 4 * (2 * s + 1);
}

// Runs, written from the slot's end towards its start.  style: quicked_batch_configure's (0 "MXID", 1 "=XID", 2 X printed as M)
struct AlignBackWriter {
    char* lo; char* pos;             // the slot's first byte; the next character goes to pos - 1
    int32_t op, len, style, nops;
    bool ok;
    QE_S_HD void init(char* slot, int32_t bytes, int32_t style_) {
        lo = slot; pos = slot + bytes; op = -1; len = 0; style = style_; nops = 0; ok = bytes > 0;
        put('\0');
    }
    QE_S_HD void put(char c) { if (pos > lo) *--pos = c; else ok = false; }
    QE_S_HD void flush() {
        if (len <= 0) return;
        const uint32_t letters = (style == 1) ? 0x4449583Du : 0x4449584Du;       // "=XID" : "MXID"
        put((char)((letters >> (8 * (op & 3))) & 0xFFu));
        uint32_t x = (uint32_t)len;
        do { put((char)('0' + x % 10)); x /= 10; } while (x);
        len = 0;
    }
    QE_S_HD void push(int o) {
        ++nops;
        if (o == op) ++len; else { flush(); op = o; len = 1; }
    }
};

// One occurrence: member planes pp (m bases), the text's planes tp, the stretch [text_start, text_end), the score the sweeps
// found.  hist: the lane's first cell, cell (column c, block b) at hist[((c - 1) hist_blocks + b) stride].  slot: slot_bytes
// bytes of the pool.  -> the string's offset within the slot, or -1; steps: block steps of the sweep, ops: operations emitted
template <class Eq>
QE_S_HD int32_t panel_align_lane(const uint64_t* pp, int m, const uint64_t* tp, int text_start, int text_end, int score,
                                 AlignCell* hist, int64_t stride, int hist_blocks, int hist_cols,
                                 char* slot, int32_t slot_bytes, int style, uint32_t& steps, uint32_t& ops) {
    const int L = text_end - text_start, nb = search_blocks(m);
    steps = 0; ops = 0;
    if (text_start < 0 || L <= 0 || m <= 0 || score < 0 || nb > QE_SEARCH_REG_BLOCKS || nb > hist_blocks || L > hist_cols) return -1;
    // ---- the sweep
    uint64_t pv[QE_SEARCH_REG_BLOCKS], mv[QE_SEARCH_REG_BLOCKS], pl[QE_SEARCH_REG_BLOCKS][Eq::W];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int b = 0; b < QE_SEARCH_REG_BLOCKS; ++b) { pv[b] = ~(uint64_t)0; mv[b] = 0; Eq::pattern_rows(pp, m, b, pl[b]); }
    for (int col0 = 0; col0 < L; col0 += 64) {
        const int ncols = L - col0 < 64 ? L - col0 : 64;
        uint64_t t[Eq::W];
        Eq::text_chunk(tp, (int64_t)text_start + col0, ncols, t);
        for (int c = 0; c < ncols; ++c) {
            uint64_t hP = 1, hM = 0;                                              // the counted top row: D[0][j] = j
            AlignCell* col = hist + (int64_t)(col0 + c) * hist_blocks * stride;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int b = 0; b < QE_SEARCH_REG_BLOCKS; ++b) {
                if (b >= nb) continue;
                uint64_t oP, oM;
                search_block_chunk<Eq>(pv[b], mv[b], pl[b], t, hP, hM, 63, 1, oP, oM);
                AlignCell cell; cell.pv = pv[b]; cell.mv = mv[b];
                col[(int64_t)b * stride] = cell;
                hP = oP; hM = oM;
                ++steps;
            }
            for (int k = 0; k < Eq::W; ++k) t[k] >>= 1;
        }
    }
    // ---- the traceback
    AlignBackWriter W;
    W.init(slot, slot_bytes, style);
    int i = m, j = L, edits = 0;
    for (int left = m + L; left > 0 && (i > 0 || j > 0); --left) {
        int op;
        if (i > 0 && j > 0) {
            const int b = (i - 1) >> 6, r = (i - 1) & 63;
            const AlignCell* at = hist + ((int64_t)(j - 1) * hist_blocks + b) * stride;
            const uint64_t up = at->pv;
            const uint64_t left_mv = j > 1 ? (at - (int64_t)hist_blocks * stride)->mv : 0;
            if ((up >> r) & 1) { op = ALIGN_D; --i; }
            else if ((left_mv >> r) & 1) { op = ALIGN_I; --j; }
            else {
                uint64_t p[Eq::W], t[Eq::W];
                Eq::pattern_rows(pp, m, b, p);
                Eq::text_chunk(tp, (int64_t)text_start + j - 1, 1, t);
                op = ((Eq::eq(p, t, 0) >> r) & 1) ? ALIGN_M : ALIGN_X;
                --i; --j;
            }
        } else if (j > 0) { op = ALIGN_I; --j; }
        else { op = ALIGN_D; --i; }
        edits += op != ALIGN_M;
        // style 2 prints X as M, except where X is the alignment's very first operation (the formatter's "1X": RunMerger)
        if (style == 2 && op == ALIGN_X && (i > 0 || j > 0)) op = ALIGN_M;
        W.push(op);
    }
    W.flush();
    ops = (uint32_t)W.nops;
    if (i != 0 || j != 0 || edits != score || !W.ok) return -1;
    return (int32_t)(W.pos - W.lo);
}

// k_panel_occ_align<Eq>: one lane per stored occurrence of the launch, occurrences [first, first + count) of the run's `total`.
// Occurrence j is hits[4 j ..] = {pattern, text_start, text_end, score}; its text is the pair whose stretch of occ_off (the
// run's offsets by pair, npairs + 1 of them) holds j.  The member's planes are at word Eq::offset(m_off[pattern]) of pl_m, the
// text's at Eq::offset(t_off[pair]) of pl_t.  The launch's wave w (64 occurrences) owns hist_cols x hist_blocks x 64 cells of
// hist.  Occurrence j's slot is pool[str_off[j], str_off[j] + panel_align_len(score) + 1); o_off[j] = where its string starts
// in the pool or -1, o_steps[j] / o_ops[j] its block steps and operations.
struct PanelAlignArgs {
    const uint64_t* pl_m;  const int64_t* m_off;  const int32_t* m_len;  int32_t n_members;
    const uint64_t* pl_t;  const int64_t* t_off;  const int32_t* t_len;
    const int64_t* occ_off;  int32_t npairs;
    const int32_t* hits;  int64_t total, first, count;
    AlignCell* hist;  int32_t hist_cols, hist_blocks;
    int32_t style;
    const int64_t* str_off;  char* pool;
    int64_t* o_off;  uint32_t* o_steps;  uint32_t* o_ops;
};
// the pair whose occurrences [off[pair], off[pair + 1]) hold j (off ascending, off[0] = 0, j < off[npairs])
QE_S_HD int32_t panel_align_pair(const int64_t* off, int32_t npairs, int64_t j) {
    int32_t lo = 0, hi = npairs;                  // the first index in (0, npairs] whose offset is above j, less one
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (off[mid + 1] > j) hi = mid; else lo = mid + 1;
    }
    return lo;
}
template <class Eq>
QE_S_HD void panel_align_occ(const PanelAlignArgs& A, int64_t k) {
    const int64_t j = A.first + k;
    if (k < 0 || k >= A.count || j >= A.total) return;
    const int32_t* h = A.hits + 4 * j;
    const int32_t pattern = h[0], start = h[1], end = h[2], score = h[3];
    const int32_t pair = panel_align_pair(A.occ_off, A.npairs, j);
    uint32_t steps = 0, ops = 0;
    int32_t at = -1;
    if (pattern >= 0 && pattern < A.n_members && pair < A.npairs && start >= 0 && end <= A.t_len[pair]) {
        AlignCell* hist = A.hist + (k >> 6) * ((int64_t)A.hist_cols * A.hist_blocks * 64) + (k & 63);
        at = panel_align_lane<Eq>(A.pl_m + Eq::offset(A.m_off[pattern]), A.m_len[pattern], A.pl_t + Eq::offset(A.t_off[pair]), start, end, score,
                                  hist, 64, A.hist_blocks, A.hist_cols, A.pool + A.str_off[j], panel_align_len(score) + 1, A.style, steps, ops);
    }
    A.o_off[j] = at < 0 ? -1 : A.str_off[j] + at;
    A.o_steps[j] = steps; A.o_ops[j] = ops;
}
// k_panel_align_sizes: occurrence j's slot without the terminator, for the offset scan
QE_S_HD void panel_align_size_one(int64_t j, const int32_t* hits, int32_t* len) { len[j] = panel_align_len(hits[4 * j + 3]); }

}  // namespace qe
