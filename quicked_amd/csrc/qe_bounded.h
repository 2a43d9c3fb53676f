// qe_bounded.h -- the diagonal-word form of a bounded edit distance: "is this pair within k edits, and if so how many?"
// for k <= 63.  Plain C++ with no HIP dependency: k_bounded_diag (qe_kernels.hip) runs it one lane per pair, and the CPU
// suite compiles the very same source with g++ (tests/native/bounded_diag_cpu.cpp) and checks it against edlib.
//
// The band.  diff = m - n is the diagonal (row - column) of the end cell.  A path of cost <= k from (0, 0) to (m, n) stays
// on the diagonals  min(0, diff) - e .. max(0, diff) + e,  e = floor((k - |diff|) / 2)  (Ukkonen): every step off the
// direct corridor has to be paid for twice.  That is |diff| + 2 e + 1 <= k + 1 diagonals, so for k <= 63 they fit one
// 64-bit word.  Bit b of the word is diagonal dlo + b, dlo = min(0, diff) - e; in text column j (1-based) that is row
// j + dlo + b: the word slides one row down per column (Hyyro's banded variant of the Myers step).
//
// Precondition (bounded_diag_takes):  k_eff = min(bound, max(m, n)) <= 63  and  |m - n| <= k_eff.  A distance never
// exceeds max(m, n), so clamping the bound changes no answer; a pair with |m - n| > bound is beyond it without a look
// at the sequences.  Lengths are unrestricted.
//
// What a result means.  Cells outside the word are never read as cheaper than they are: the row above the word is left
// out of the minimum, the row that enters at the bottom starts as "the cell above + 1" -- both are costs of real paths.
// So the value v of the end cell is the cost of a real path, v >= d; and when d <= k_eff the optimal path lies inside the
// band, so v = d.  Hence  v <= bound  <=>  d <= bound, and then v = d: the answer is v if v <= bound, else "beyond" (-1).
//
// Rows outside the pattern.  Rows <= 0 that the word covers while j is small are rows of an extended matrix
// D[i][j] = j + |i| (i <= 0): vertical delta -1, every cell "matches" (Eq forced to 1), which satisfies the recurrence and
// has D[0][j] = j, the true boundary row.  Rows > m are garbage that never reaches a row <= m: every cell depends on rows
// at or above its own only, and the carry of the addition runs towards higher rows.  The tracked cell is the one on
// diagonal diff: column 0 starts it at |diff|, each column adds its diagonal delta (1 - D0 bit), after n columns it is
// D[m][n].  Values along a diagonal never decrease, so a lane whose tracked value exceeds the bound is decided.
//
// Sequences are given as bit-planes (qe_types.h): per 64 bases three words {code bit 0, code bit 1, not-ACGT}; two
// symbols are equal when both are not-ACGT, or neither is and the code bits agree (dna_text.c:41-46).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QE_BD_HD __host__ __device__ __forceinline__
#else
#define QE_BD_HD inline
#endif

namespace qe {

enum : int { QE_BOUNDED_DIAG_MAX = 63 };   // the largest effective bound the word holds

// the bound the pair is decided with: no distance exceeds the longer sequence
QE_BD_HD int bounded_effective(int bound, int m, int n) { const int l = m > n ? m : n; return bound < l ? bound : l; }
// whether the diagonal word covers Ukkonen's band of the pair for `bound` (m, n >= 1, bound >= 0)
QE_BD_HD bool bounded_diag_takes(int bound, int m, int n) {
    const int k = bounded_effective(bound, m, n), d = m > n ? m - n : n - m;
    return k <= QE_BOUNDED_DIAG_MAX && d <= k;
}

struct BoundedDiag {
    uint64_t Pv, Mv;          // vertical deltas of the word's rows, in the NEXT column's row numbering
    uint64_t wa, wb, wn;      // pattern planes of the word's rows in the next column
    uint64_t xa, xb, xn;      // ... of the 64 rows below them (feeds the word one bit per column)
    uint64_t force;           // rows <= 0 of the word in the next column: Eq = 1
    uint64_t track;           // 1 << (bit of diagonal m - n)
    int32_t score;            // D on diagonal m - n in the last column done
    int32_t dlo;              // diagonal of bit 0
};

// 64 pattern rows starting at pattern index `start` (may be negative: those bits read 0) from planes of a pattern of m
// bases; reads words [0, ceil(m / 64)) only
QE_BD_HD void bounded_pattern_rows(const uint64_t* pp, int m, int start, uint64_t& a, uint64_t& b, uint64_t& nn) {
    const int nwords = (m + 63) >> 6;
    a = 0; b = 0; nn = 0;
    if (start <= -64) return;
    if (start < 0) {
        const int sh = -start;                       // 1 .. 63
        a = pp[0] << sh; b = pp[1] << sh; nn = pp[2] << sh;
        return;
    }
    const int w = start >> 6, sh = start & 63;
    if (w < nwords) {
        const uint64_t* q = pp + 3 * (int64_t)w;
        a = q[0] >> sh; b = q[1] >> sh; nn = q[2] >> sh;
    }
    if (sh && w + 1 < nwords) {
        const uint64_t* q = pp + 3 * (int64_t)(w + 1);
        a |= q[0] << (64 - sh); b |= q[1] << (64 - sh); nn |= q[2] << (64 - sh);
    }
}

// state before column 1; bounded_diag_takes(bound, m, n) must hold
QE_BD_HD void bounded_diag_init(BoundedDiag& S, const uint64_t* pp, int m, int n, int bound) {
    const int k = bounded_effective(bound, m, n), diff = m - n, ad = diff < 0 ? -diff : diff;
    const int e = (k - ad) >> 1;
    S.dlo = (diff < 0 ? diff : 0) - e;                 // -63 .. 0
    const int z = -S.dlo;                              // rows <= 0 of the word in column 1
    S.Mv = z ? (~(uint64_t)0 >> (64 - z)) : 0;         // D[i][0] = |i|: -1 per row down to row 0, +1 from there
    S.Pv = ~S.Mv;
    S.force = S.Mv;
    S.track = (uint64_t)1 << (diff - S.dlo);
    S.score = ad;
    bounded_pattern_rows(pp, m, S.dlo, S.wa, S.wb, S.wn);      // row 1 + dlo + b is pattern index dlo + b
    S.xa = S.xb = S.xn = 0;
}

// One text column.  Eq: the word's rows that match the column's base (rows <= 0 included).  Returns D0, the rows whose
// diagonal delta is 0.  Pv / Mv go from this column's numbering to the next one's (one row down): the delta of the row
// that enters at the bottom is +1 -- "the cell above + 1", a real path.
QE_BD_HD uint64_t bounded_diag_step(uint64_t Eq, uint64_t& Pv, uint64_t& Mv) {
    const uint64_t D0 = (((Eq & Pv) + Pv) ^ Pv) | Eq | Mv;
    const uint64_t Ph = Mv | ~(D0 | Pv);
    const uint64_t Mh = Pv & D0;
    const uint64_t X = D0 >> 1;
    Pv = Mh | ~(X | Ph) | ((uint64_t)1 << 63);
    Mv = Ph & X & ~((uint64_t)1 << 63);
    return D0;
}

// One text column whose base has plane bits (b0, b1, bn): Eq from the pattern window, the step, the tracked cell, and the
// window one row down.
QE_BD_HD void bounded_diag_column(BoundedDiag& S, uint64_t b0, uint64_t b1, uint64_t bn) {
    const uint64_t m0 = (uint64_t)0 - b0, m1 = (uint64_t)0 - b1, mn = (uint64_t)0 - bn;
    const uint64_t acgt = ~(S.wa ^ m0) & ~(S.wb ^ m1) & ~S.wn;
    const uint64_t Eq = (mn & S.wn) | (~mn & acgt) | S.force;
    const uint64_t D0 = bounded_diag_step(Eq, S.Pv, S.Mv);
    S.score += (D0 & S.track) ? 0 : 1;
    S.wa = (S.wa >> 1) | (S.xa << 63); S.xa >>= 1;
    S.wb = (S.wb >> 1) | (S.xb << 63); S.xb >>= 1;
    S.wn = (S.wn >> 1) | (S.xn << 63); S.xn >>= 1;
    S.force >>= 1;
}

// Up to 64 columns: text columns [64 chunk, 64 chunk + ncols) of the pair, whose planes are t0 / t1 / tn (bit c = column
// 64 chunk + c).  Reloads the feed words first: the 64 pattern rows below the word at the chunk's first column.
QE_BD_HD void bounded_diag_chunk(BoundedDiag& S, const uint64_t* pp, int m, int chunk, int ncols, uint64_t t0, uint64_t t1, uint64_t tn) {
    bounded_pattern_rows(pp, m, S.dlo + 64 * chunk + 64, S.xa, S.xb, S.xn);
    if (ncols == 64) {                                 // whole chunks: a fixed trip count, constant shifts
        for (int c = 0; c < 64; ++c) bounded_diag_column(S, (t0 >> c) & 1, (t1 >> c) & 1, (tn >> c) & 1);
    } else {
        for (int c = 0; c < ncols; ++c) bounded_diag_column(S, (t0 >> c) & 1, (t1 >> c) & 1, (tn >> c) & 1);
    }
}

// the answer of a finished pair
QE_BD_HD int bounded_answer(int value, int bound) { return (value >= 0 && value <= bound) ? value : -1; }

// One pair, lane by lane as the kernel does it (without the wave-wide early exit): planes of the pattern (m bases) and
// of the text (n bases), words [0, 3 ceil(len / 64)) each.  -1: beyond the bound.
QE_BD_HD int bounded_diag_pair(const uint64_t* pp, int m, const uint64_t* tp, int n, int bound) {
    BoundedDiag S;
    bounded_diag_init(S, pp, m, n, bound);
    const int nch = (n + 63) >> 6;
    for (int k = 0; k < nch; ++k) {
        const int ncols = (n - 64 * k) < 64 ? (n - 64 * k) : 64;
        const uint64_t* q = tp + 3 * (int64_t)k;
        bounded_diag_chunk(S, pp, m, k, ncols, q[0], q[1], q[2]);
    }
    return bounded_answer(S.score, bound);
}

}  // namespace qe
