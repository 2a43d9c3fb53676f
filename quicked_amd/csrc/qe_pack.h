// qe_pack.h -- the span classifier of k_pack (ASCII -> the three bit planes of qe_types.h, DESIGN.md 4 "pack").
// Plain C++ with no HIP dependency and no other header of the library, like qe_iupac.h: the kernel and the CPU suite (tests/native/pack_cpu.cpp)
// run the same source; only the two one-line wrappers below differ between the device and the host.
//
// A lane of k_pack takes 16 consecutive bases as four little-endian 32-bit words (base i of the lane in byte i & 3 of word
// i >> 2) and leaves three 16-bit masks, bit i = base i:
//   a, b   the two bits of the base code: ASCII bits 1 and 2, an injective code of A, C, G, T in either case
//          (A 0, C 1, T 2, G 3; any injective code works), zero where the base is not ACGT
//   n      the base is not one of A C G T a c g t: the reference's code 4 (dna_text.c:41-46)
// The rule, four bytes at a time in SWAR: (c >> 1) & 3 indexes a 4-byte table of the upper-case letters (v_perm_b32); the
// base is ACGT iff the table byte equals its upper-cased self (the non-zero-byte test leaves bit 7 of every byte that differs).
// The gather: a word u with the flags of EIGHT bases -- bit p of every byte for the four of one word, bit p + 4 for the
// four of the next -- ORed with itself shifted left by 7, 14 and 21 has the eight flags side by side at bits p + 21 ..
// p + 28 (flag bit 8 k + q of u lands at k + q + 21; no two of the 32 shifted flags share a target there).  Two shift-ors
// per eight bases, all of them full-rate instructions.  (v_dot4_u32_u8 with the weights 1, 2, 4, 8 gathers four flags in
// one instruction and was measured first: it issues at half rate and drags the instructions around it with it -- at eight
// waves per SIMD the classifier came out 9 % SLOWER than with shift-ors; profiles/pack_lean.md.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QE_K_HD __host__ __device__ __forceinline__
#else
#define QE_K_HD inline
#endif

namespace qe {

typedef uint32_t u32;
enum : u32 { PACK_HAS_N = 1u, PACK_NONCANON = 2u };      // = FLAG_HAS_N, FLAG_NONCANON of qe_types.h (k_pack asserts it)

// v_perm_b32: byte k of the result is picked by byte k of sel -- 0 .. 3: that byte of lo, 4 .. 7: of hi, 0x0C: zero
QE_K_HD u32 pack_perm(u32 hi, u32 lo, u32 sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    u32 r = 0;
    for (int k = 0; k < 4; ++k) {
        const u32 c = (sel >> (8 * k)) & 0xFFu;
        const u32 byte = c < 4u ? (lo >> (8 * c)) & 0xFFu : c < 8u ? (hi >> (8 * (c - 4u))) & 0xFFu : 0u;
        r |= byte << (8 * k);
    }
    return r;
#endif
}
// eight flags -> one byte (above): at bits p + 21 .. p + 28
QE_K_HD u32 pack_gather8(u32 u) {
    const u32 t = u | (u << 7);
    return t | (t << 14);
}

enum : u32 { PACK_FILL = 0x41414141u };      // past a sequence's end: 'A' packs to all-zero planes and no flags

// bit 7 of every byte of w that is not one of A C G T a c g t
QE_K_HD u32 pack_not_acgt(u32 w) {
    const u32 want = pack_perm(0u, 0x47544341u, (w >> 1) & 0x03030303u);      // 'A', 'C', 'T', 'G'
    const u32 y = want ^ (w & 0xDFDFDFDFu);                                     // case-insensitive (dna_text.c:44-45)
    const u32 y7 = want ^ (w & 0x5F5F5F5Fu);                                    // = y & 0x7F7F7F7F: the table's bytes are below 0x80
    return ((y7 + 0x7F7F7F7Fu) | y) & 0x80808080u;
}

// 16 bases -> a, b, n.  hint == 0: none of the 16 bytes sets a flag (pack_flags16 would return 0) -- one test per span, and
// on upper-case ACGT it never fires.  hint != 0 decides nothing: a byte with ASCII bit 5 (lower case, digits, ...) or a
// base that is not ACGT is somewhere in the span.
QE_K_HD void pack_classify16(const u32 (&w)[4], u32& a, u32& b, u32& n, u32& hint) {
    // not ACGT: bit 7 of every byte; the first word of a pair moves to bit 3 (p = 3: the byte comes out at bits 24 .. 31)
    const u32 n0 = pack_gather8((pack_not_acgt(w[0]) >> 4) | pack_not_acgt(w[1]));
    const u32 n1 = pack_gather8((pack_not_acgt(w[2]) >> 4) | pack_not_acgt(w[3]));
    n = pack_perm(n1, n0, 0x0C0C0703u);
    // the code bits are ASCII bits 1 and 2: with the second word of a pair moved up by 4, plane a has p = 1, plane b p = 2
    const u32 m0 = (w[0] & 0x06060606u) | ((w[1] << 4) & 0x60606060u), m1 = (w[2] & 0x06060606u) | ((w[3] << 4) & 0x60606060u);
    const u32 a0 = pack_gather8(m0 & 0x22222222u), a1 = pack_gather8(m1 & 0x22222222u);
    const u32 b0 = pack_gather8(m0 & 0x44444444u), b1 = pack_gather8(m1 & 0x44444444u);
    a = (((a0 >> 22) & 0xFFu) | ((a1 >> 14) & 0xFF00u)) & ~n;      // a base that is not ACGT has code bits 0: once per span, on the masks
    b = (((b0 >> 23) & 0xFFu) | ((b1 >> 15) & 0xFF00u)) & ~n;
    hint = ((w[0] | w[1] | w[2] | w[3]) & 0x20202020u) | n;
}

// the flags of 16 bases, exactly: PACK_HAS_N for a base that is not ACGT, PACK_NONCANON for a lower-case base and for
// every symbol other than 'N' that is not a base (IUPAC and the rest, 'n' included): where the raw-byte and the encoded
// comparisons of the reference differ
QE_K_HD u32 pack_flags16(const u32 (&w)[4]) {
    u32 fl = 0;
    for (int k = 0; k < 4; ++k) {
        const u32 bad = pack_not_acgt(w[k]);
        if ((w[k] << 2) & ~bad & 0x80808080u) fl |= PACK_NONCANON;
        if (bad) {
            fl |= PACK_HAS_N;
            for (int i = 0; i < 4; ++i)
                if (((bad >> (8 * i + 7)) & 1u) && ((w[k] >> (8 * i)) & 0xFFu) != 'N') fl |= PACK_NONCANON;
        }
    }
    return fl;
}

// The 16 bytes at positions pos .. pos + 15 of the string (reverse: of the reversed string), PACK_FILL past its end: the
// byte-at-a-time form, which k_pack takes for the one ragged lane of a sequence; every other lane gets the same words from
// one 16-byte load.
QE_K_HD void pack_fetch16(const uint8_t* src, int len, int pos, bool reverse, u32 (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = PACK_FILL;
    for (int i = 0; i < 16 && pos + i < len; ++i) {
        const u32 c = reverse ? src[len - 1 - pos - i] : src[pos + i];
        w[i >> 2] = (w[i >> 2] & ~(0xFFu << (8 * (i & 3)))) | (c << (8 * (i & 3)));
    }
}

}  // namespace qe
