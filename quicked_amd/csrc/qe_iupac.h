// qe_iupac.h -- the IUPAC equality of search runs (QUICKED_SEARCH_IUPAC, QUICKED_SEARCH_IUPAC_PATTERN).
// Plain C++ with no HIP dependency, like qe_search.h and qe_check.h: the pack kernels (k_pack_iupac, k_planes_iupac), their
// host stand-ins and the CPU suite (tests/native/search_iupac_cpu.cpp) use the same definitions.
//
// The relation.  Every byte stands for a set of bases, case folded: A C G T (U = T), the two-base codes R Y S W K M, the
// three-base codes B D H V, N = all four, any other byte the empty set.  Two symbols are equal when their sets intersect:
// symmetric, not transitive (R = A, R = G, A != G), and a byte outside the alphabet equals nothing, itself included.
// acgt_only (the text side of QUICKED_SEARCH_IUPAC_PATTERN): a byte that is not one of A C G T U has the empty set.
//
// The planes.  Per 64 bases FOUR words {A, C, G, T membership} (bit i = base 64 row + i), interleaved [row][4]; the same
// rows as the three-plane layout of qe_types.h -- ceil(len / 64) and two rows of zeros --, so a sequence that starts at
// word o of the three-plane buffer starts at word o / 3 * 4 of the four-plane one (iupac_offset; o is a multiple of 3).
// Every bit at or past the sequence's end is zero -- the empty set, which matches nothing -- whichever producer made the
// words: the packer from ASCII (iupac_pack) or the derivation from three planes (iupac_from_planes3).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QE_I_HD __host__ __device__ __forceinline__
#else
#define QE_I_HD inline
#endif

namespace qe {

enum : int { IUPAC_A = 1, IUPAC_C = 2, IUPAC_G = 4, IUPAC_T = 8 };
// the masks of the letters by (byte & 31), a nibble each: entries 0 .. 15 and 16 .. 31
//   1 A  2 B  3 C  4 D  7 G  8 H  11 K  13 M  14 N  |  18 R  19 S  20 T  21 U  22 V  23 W  25 Y
enum : uint64_t { IUPAC_TABLE_LO = 0x0F30C00B400D2E10ull, IUPAC_TABLE_HI = 0x000000A097886500ull };

// byte -> the 4-bit mask of its set
QE_I_HD uint32_t iupac_mask(uint32_t c, bool acgt_only) {
    const uint32_t l = (c | 0x20u) - 'a';                          // a letter in either case: 0 .. 25
    const uint32_t i = c & 31u;
    uint32_t k = (uint32_t)(((i & 16u) ? IUPAC_TABLE_HI : IUPAC_TABLE_LO) >> (4 * (i & 15u))) & 15u;
    if (l > 25u) k = 0;
    if (acgt_only && (k & (k - 1))) k = 0;                         // more than one base: not one of A C G T U
    return k;
}

QE_I_HD int64_t iupac_offset(int64_t off3) { return off3 / 3 * 4; }          // word offset: three-plane -> four-plane buffer
QE_I_HD int64_t iupac_rows(int len) { return ((int64_t)len + 63) / 64 + 2; }  // with the two rows of zeros
QE_I_HD int64_t iupac_words(int len) { return 4 * iupac_rows(len); }

// One sequence, forward or reversed, into its iupac_words(len) words
inline void iupac_pack(const uint8_t* s, int len, bool reverse, bool acgt_only, uint64_t* dst) {
    const int64_t nw = iupac_words(len);
    for (int64_t w = 0; w < nw; ++w) dst[w] = 0;
    for (int i = 0; i < len; ++i) {
        const uint32_t k = iupac_mask(s[reverse ? len - 1 - i : i], acgt_only);
        uint64_t* row = dst + 4 * (int64_t)(i >> 6);
        const uint64_t bit = (uint64_t)1 << (i & 63);
        if (k & IUPAC_A) row[0] |= bit;
        if (k & IUPAC_C) row[1] |= bit;
        if (k & IUPAC_G) row[2] |= bit;
        if (k & IUPAC_T) row[3] |= bit;
    }
}

// One row of 64 bases from its three planes {code bit 0, code bit 1, not-ACGT} (codes A 0, C 1, G 2, T 3): `valid` = the
// bases of the row that exist (0 .. 64); a not-ACGT base is N -- the full set, or the empty one (n_empty)
QE_I_HD void iupac_row_from_planes3(uint64_t a, uint64_t b, uint64_t nn, int valid, bool n_empty, uint64_t (&o)[4]) {
    const uint64_t mask = valid >= 64 ? ~(uint64_t)0 : (valid <= 0 ? 0 : (((uint64_t)1 << valid) - 1));
    const uint64_t n = n_empty ? 0 : nn & mask, ok = ~nn & mask;
    o[0] = (~a & ~b & ok) | n;
    o[1] = (a & ~b & ok) | n;
    o[2] = (~a & b & ok) | n;
    o[3] = (a & b & ok) | n;
}
// a whole sequence: src = its three-plane words (ceil(len / 64) rows are read), dst = its iupac_words(len) words
inline void iupac_from_planes3(const uint64_t* src, int len, bool n_empty, uint64_t* dst) {
    const int64_t rows = iupac_rows(len), nw = ((int64_t)len + 63) / 64;
    for (int64_t r = 0; r < rows; ++r) {
        uint64_t o[4] = {0, 0, 0, 0};
        if (r < nw) iupac_row_from_planes3(src[3 * r], src[3 * r + 1], src[3 * r + 2], (int)(len - 64 * r < 64 ? len - 64 * r : 64), n_empty, o);
        for (int k = 0; k < 4; ++k) dst[4 * r + k] = o[k];
    }
}

}  // namespace qe
