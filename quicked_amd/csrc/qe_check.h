// qe_check.h -- the CIGAR validator (cigar_check_alignment, cigar.c:363-434) as functions of an alignment's operations and
// the RAW bytes of its pair.  Plain C++ with no HIP dependency (as qe_bounded.h and qe_tags.h): k_check_segs and
// k_check_strings (qe_kernels.hip) run it one lane per alignment, the host-only build runs it in the kernels' place
// (tests/native/hip_stub/qe_kernels_stub.h), and the CPU suite compiles the very same source with g++ under the sanitizers
// (tests/native/check_cpu.cpp) against a restatement in Python (tests/check_lib.py).
//
// The walk: operations front to back, v bases of the pattern and h of the text consumed so far.
//   M, len   needs len more bases of both sequences, all equal byte for byte;      v += len, h += len
//   X, len   needs len more bases of both, all different byte for byte;            v += len, h += len
//   I, len   needs len more bases of the text;                                     h += len
//   D, len   needs len more bases of the pattern;                                  v += len
// The first operation that would leave a sequence, or whose bytes do not fit, fails the alignment -- as the reference's walk
// does operation by operation --, and nothing after it is looked at.  "Needs len more" is decided by subtraction
// (len > m - v), never by v + len: 0 <= v <= m and 0 <= h <= n hold throughout whatever lengths come in, so no sum can wrap
// and no byte outside the pair is ever read.  Verdict: 1 where nothing failed and both sequences are consumed exactly, else 0.
// Bytes are raw: no case folding, no wildcard (N equals N and nothing else).
//
// Strings (quicked_batch_validate): "<len><op>" repeated, up to the terminator.  op is one of M X I D, and '=' is read as M;
// len is decimal, at least 1 and at most 2147483647 (leading zeros allowed).  A longer number, a zero length, digits without
// an operation, an operation without digits and any other byte make the string invalid (0).  The empty string is the
// alignment of two empty sequences.
//
// Segments (the in-run form): literal segments and leaves as SegFormatArgs lays them out and tag_walk_segments (qe_tags.h)
// walks them; a run of length <= 0 is no operation; a leaf whose run buffer overflowed (nruns < 0) has no alignment: 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QE_CK_HD __host__ __device__ __forceinline__
#else
#define QE_CK_HD inline
#endif

namespace qe {

enum : int { CK_OP_M = 0, CK_OP_X = 1, CK_OP_I = 2, CK_OP_D = 3 };      // cigar_op_t (qe_types.h), the two low bits of a run
enum : int64_t { CK_MAX_LEN = 0x7fffffff };                              // the longest run a string may name

struct AlignCheck {
    const uint8_t* ap; const uint8_t* at; int m, n, v = 0, h = 0; bool ok = true;
    QE_CK_HD void apply(int op, int cnt) {
        if (!ok || cnt <= 0) return;
        if (op == CK_OP_I) { if (cnt > n - h) ok = false; else h += cnt; return; }
        if (op == CK_OP_D) { if (cnt > m - v) ok = false; else v += cnt; return; }
        if (cnt > m - v || cnt > n - h) { ok = false; return; }
        const uint8_t* a = ap + v; const uint8_t* b = at + h;
        int k = 0;
        if (op == CK_OP_M) {
            for (; k + 8 <= cnt; k += 8) {
                uint64_t x, y; __builtin_memcpy(&x, a + k, 8); __builtin_memcpy(&y, b + k, 8);
                if (x != y) { ok = false; return; }
            }
            for (; k < cnt; ++k) if (a[k] != b[k]) { ok = false; return; }
        } else {
            for (; k < cnt; ++k) if (a[k] == b[k]) { ok = false; return; }
        }
        v += cnt; h += cnt;
    }
    QE_CK_HD int verdict() const { return (ok && v == m && h == n) ? 1 : 0; }
};

// One NUL-terminated string into the walk (the rules above); the verdict is K.verdict()
QE_CK_HD void check_walk_string(AlignCheck& K, const char* q) {
    int64_t num = 0; bool have = false;
    for (; K.ok; ++q) {
        const char c = *q;
        if (c == 0) break;
        if (c >= '0' && c <= '9') { num = num * 10 + (c - '0'); have = true; if (num > CK_MAX_LEN) K.ok = false; continue; }
        int op = -1;
        if (c == 'M' || c == '=') op = CK_OP_M; else if (c == 'X') op = CK_OP_X;
        else if (c == 'I') op = CK_OP_I; else if (c == 'D') op = CK_OP_D;
        if (op < 0 || !have || num == 0) { K.ok = false; break; }
        K.apply(op, (int)num);
        num = 0; have = false;
    }
    if (have) K.ok = false;                 // digits without an operation
}

// The segments of alignment i (SegFormatArgs: seg_off / seg_kind / seg_a / seg_b; a leaf's runs are stored back to front)
// into the walk.  R: open(task) selects a leaf's runs, at(k) reads run k.
template <typename Runs>
QE_CK_HD void check_walk_segments(AlignCheck& K, const int64_t* seg_off, const int32_t* seg_kind, const int32_t* seg_a, const int32_t* seg_b,
                                  const int32_t* nruns, int64_t i, Runs& R) {
    for (int64_t sidx = seg_off[i]; sidx < seg_off[i + 1]; ++sidx) {
        if (seg_kind[sidx] == 1) { K.apply(seg_a[sidx], seg_b[sidx]); continue; }
        const int t = seg_a[sidx];
        if (nruns[t] < 0) { K.ok = false; return; }
        R.open(t);
        for (int k = nruns[t] - 1; k >= 0; --k) {
            const uint32_t r = R.at(k);
            K.apply((int)(r & 3), (int)(r >> 2));
        }
    }
}

}  // namespace qe
