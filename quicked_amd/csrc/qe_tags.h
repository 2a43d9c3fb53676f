// qe_tags.h -- per-pair alignment statistics and the SAM MD:Z string, as functions of an alignment's operation sequence
// and the pattern's raw bytes.  Plain C++ with no HIP dependency (as qe_bounded.h): k_tags_segs (qe_kernels.hip) runs the
// walker one lane per alignment, the host-only build runs it in place of the kernels (tests/native/hip_stub/qe_kernels_stub.h), and the CPU suite
// compiles the very same source with g++ (tests/native/tags_cpu.cpp) against a restatement in Python.
//
// The operation sequence is what the style-0 CIGAR expands to; I consumes text, D consumes pattern (AlignCheck,
// qe_kernels.hip).  Runs are maximal: equal neighbours are merged wherever they meet -- across Hirschberg leaves, literal
// segments, zero-length literals -- exactly as RunMerger::push merges them.
//
// Statistics: columns of M / X / I / D, the numbers of maximal I and D runs, the longest maximal M run, all columns.
//
// MD is over the sequence D consumes: the PATTERN (in the SAM styles this library prints, I consumes the text, so the text
// is SAM's query and the pattern SAM's reference).  Bytes are raw, no case folding.  With acc = 0, v = 0:
//   M, len   acc += len, v += len
//   X, len   per base: acc in decimal, the byte P[v]; acc = 0, v += 1   (neighbouring mismatches are separated by "0")
//   D, len   acc in decimal, '^', P[v .. v + len); acc = 0, v += len
//   I        nothing: it neither emits nor resets acc -- but it ends a D run, so "D I D" reads "^AC0^GT"
//   end      acc in decimal
//
// The bound.  A number that precedes an event has at most 1 + acc digits (acc >= 0 has at most acc + 1 of them) and the
// acc's of one string sum to at most `matches`; so with x mismatches, d deleted bases in r runs:
//   length <= (matches + x + r + 1)  [digits: one number per event and the last one]  + x  + r + d
//          <= matches + 2 x + 3 d + 1  <=  3 m + 1,   m = matches + x + d the pattern's length.
// tag_md_bound(m) = 3 m + 11 holds the string and its terminator with room to spare; the worst case is D and I alternating,
// three characters per pattern base.  A writer never passes `cap` characters whatever its input (TagSink::put).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QE_TG_HD __host__ __device__ __forceinline__
#else
#define QE_TG_HD inline
#endif

namespace qe {

enum : int { TAG_OP_M = 0, TAG_OP_X = 1, TAG_OP_I = 2, TAG_OP_D = 3 };      // cigar_op_t (qe_types.h), the two low bits of a run

// quicked_pair_stats_t (quicked_batch.h), field for field
struct TagStats { int32_t matches, mismatches, ins_bases, del_bases, ins_runs, del_runs, longest_match, columns; };

QE_TG_HD int64_t tag_md_bound(int32_t m) { return (int64_t)3 * m + 11; }      // string + terminator of a pattern of m bases
QE_TG_HD int tag_digits(uint32_t x) {
    int d = 1;
    while (x >= 10) { x /= 10; ++d; }
    return d;
}
QE_TG_HD void tag_stats_none(TagStats& s) {
    s.matches = s.mismatches = s.ins_bases = s.del_bases = s.ins_runs = s.del_runs = s.longest_match = s.columns = -1;
}

// What one maximal run adds to the statistics (the merge happens before: TagWalker::push, or the wave form's scans)
QE_TG_HD void tag_stats_run(TagStats& s, int op, int len) {
    s.columns += len;
    if (op == TAG_OP_M) { s.matches += len; if (len > s.longest_match) s.longest_match = len; }
    else if (op == TAG_OP_X) s.mismatches += len;
    else if (op == TAG_OP_I) { s.ins_bases += len; ++s.ins_runs; }
    else { s.del_bases += len; ++s.del_runs; }
}

// Characters of an MD event.  X of len bases after acc matches: "<acc>B" then len - 1 times "0B"; D: "<acc>^" and len bytes
QE_TG_HD int64_t tag_md_chars_x(int acc, int len) { return (int64_t)tag_digits((uint32_t)acc) + 1 + (int64_t)2 * (len - 1); }
QE_TG_HD int64_t tag_md_chars_d(int acc, int len) { return (int64_t)tag_digits((uint32_t)acc) + 1 + len; }

// Writes into out[0 .. cap): never beyond, whatever is asked of it; bytes of the pattern past its end read as '?'
struct TagSink {
    char* out; int64_t cap; const uint8_t* pat; int32_t m;
    QE_TG_HD void put(int64_t pos, char c) const { if (pos >= 0 && pos < cap) out[pos] = c; }
    QE_TG_HD char base(int64_t v) const { return (v >= 0 && v < m) ? (char)pat[v] : '?'; }
    QE_TG_HD int64_t number(int64_t pos, int x) const {
        const int d = tag_digits((uint32_t)x);
        uint32_t y = (uint32_t)x;
        for (int k = d - 1; k >= 0; --k) { put(pos + k, (char)('0' + y % 10)); y /= 10; }
        return pos + d;
    }
    // the text of an X run / of a D run that opens a group (caret) or continues one, at pos; returns the position behind it
    QE_TG_HD int64_t run_x(int64_t pos, int acc, int64_t v, int len) const {
        pos = number(pos, acc);
        put(pos++, base(v));
        for (int k = 1; k < len; ++k) { put(pos++, '0'); put(pos++, base(v + k)); }
        return pos;
    }
    QE_TG_HD int64_t run_d(int64_t pos, int acc, int64_t v, int len, bool opens) const {
        if (opens) { pos = number(pos, acc); put(pos++, '^'); }
        for (int k = 0; k < len; ++k) put(pos++, base(v + k));
        return pos;
    }
};

// One alignment, operation by operation.  WRITE = false counts (statistics and the MD length), WRITE = true writes the MD
// string into the sink -- like RunMerger<WRITE>.  push() takes runs in alignment order and merges equal neighbours.
template <bool WRITE>
struct TagWalker {
    bool want_md = false;
    TagSink sink{nullptr, 0, nullptr, 0};
    int op = -1, len = 0;           // the open run
    int acc = 0;                    // matches since the last MD event
    int64_t v = 0;                  // pattern bases consumed
    int64_t pos = 0;                // MD characters so far
    TagStats s{0, 0, 0, 0, 0, 0, 0, 0};

    QE_TG_HD void close() {
        if (len <= 0) return;
        if (!WRITE) tag_stats_run(s, op, len);
        if (op == TAG_OP_M) { acc += len; v += len; }
        else if (op == TAG_OP_X) {
            if (want_md) pos = WRITE ? sink.run_x(pos, acc, v, len) : pos + tag_md_chars_x(acc, len);
            acc = 0; v += len;
        } else if (op == TAG_OP_D) {
            if (want_md) pos = WRITE ? sink.run_d(pos, acc, v, len, true) : pos + tag_md_chars_d(acc, len);
            acc = 0; v += len;
        }
        len = 0;
    }
    QE_TG_HD void push(int o, int n) {
        if (n <= 0) return;
        if (o == op) { len += n; return; }
        close();
        op = o; len = n;
    }
    // the last run and the closing number; returns the MD length (without the terminator, which WRITE stores at out[cap])
    QE_TG_HD int64_t finish() {
        close();
        if (!want_md) return 0;
        if (WRITE) { pos = sink.number(pos, acc); if (sink.out) sink.out[sink.cap] = '\0'; }
        else pos += tag_digits((uint32_t)acc);
        return pos;
    }
};

// The count pass's verdict on one alignment, stored: statistics (all -1 where it has none: `bad`) and the MD length -- 0
// where it has none, or where the string would not fit tag_md_bound of its pattern, which also raises *o_md_bad (cannot
// happen for runs that consume the pattern exactly).  Null outputs are skipped.
QE_TG_HD void tag_store_counts(TagStats* o_stats, int32_t* o_md_len, int32_t* o_md_bad, bool bad, const TagStats& s, int64_t md_len, int32_t m) {
    if (o_stats) { if (bad) tag_stats_none(*o_stats); else *o_stats = s; }
    if (o_md_len) {
        const bool over = !bad && md_len + 1 > tag_md_bound(m);
        if (over) *o_md_bad = 1;
        *o_md_len = (bad || over) ? 0 : (int32_t)md_len;
    }
}

// Walks the segments of alignment i (SegFormatArgs: seg_off / seg_kind / seg_a / seg_b; a leaf's runs are stored back to
// front) into a walker.  R: open(task) selects a leaf's runs, at(k) reads run k.  False = a leaf's run buffer overflowed
// (nruns < 0): the pair has no alignment.
template <typename Walker, typename Runs>
QE_TG_HD bool tag_walk_segments(Walker& w, const int64_t* seg_off, const int32_t* seg_kind, const int32_t* seg_a, const int32_t* seg_b,
                                const int32_t* nruns, int64_t i, Runs& R) {
    for (int64_t sidx = seg_off[i]; sidx < seg_off[i + 1]; ++sidx) {
        if (seg_kind[sidx] == 1) { w.push(seg_a[sidx], seg_b[sidx]); continue; }
        const int t = seg_a[sidx];
        if (nruns[t] < 0) return false;
        R.open(t);
        for (int k = nruns[t] - 1; k >= 0; --k) {
            const uint32_t r = R.at(k);
            w.push((int)(r & 3), (int)(r >> 2));
        }
    }
    return true;
}

}  // namespace qe
