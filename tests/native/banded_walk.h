// The walk of k_banded<false[, LDS]> (BandEd score-only, one lane per task) on the CPU, the one model the
// programs pass_plan_cpu, narrow_prune_cpu, score_ring_cpu and tall_plan_cpu share: groups of 64 tasks in the order given,
// every chunk walked as the wave would walk it -- the pass heights by the kernel's own rule (qe_types.h: score_pass_height
// over pass_plan and tall_height), every K-slot pass computed slot by slot with the oracle's block step, dead slots on zeros
// and the scores by slots_pass's backward rule, the band shifted in place as the kernel shifts it, the two band-edge rules
// after every full chunk.  What a program selects (WalkOpts, Lane::prune), not copies:
//   prune   the threshold of the two band-edge rules where it is below the task's cutoff ("The pruning
//           threshold"; BandedArgs::prune); the geometry stays the cutoff's.  Not below: the geometry's clamped cutoff.
//   ring    the state in a slice laid out as the LDS form lays it out ("Band state in LDS"): Pv / Mv of
//           score_lds_cap() + 1 slots, scores[] as a ring of score_lds_ring() rows addressed by score_lds_row().  A task
//           whose band score_lds_fits() does not take sits the walk out (valid = false), as the kernel leaves it out.
//           Checked per access: the slot lies in -1 .. cap - 1 (bad_slot), the row in the chunk's window
//           first + pos_v .. last + pos_v + 1, which is shorter than the ring by two (bad_row), and a row that is read is
//           the row last written at its ring index (stale).  Without it: plain arrays sized for the task, scores[] by
//           absolute block row, as the group workspace holds it.
//   tall    the kernel's tall plan in front of the 4 / 2 / 1 plan ("Tall passes"): one pass of
//           tall_height(h) slots at the first step of a chunk whose walk is h slots long, where pass_plan has no fallback.
// Launch files: int32 count, then per pair a header of int32 and the m + n bytes of pattern and text; the header is
// m, n, cutoff (masked_lib.write_launch) or m, n, c1, p, C (narrow_prune_lib.write_launch: first-pass cutoff, threshold,
// full cutoff).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" {
#include "../../oracle/quicked_oracle.c"
}
#include <hip/hip_runtime.h>      // tests/native/hip_stub: qe_types.h is plain C++ on the host
#include "qe_types.h"

namespace {

struct Lane {
    bool valid = false, hasN = false;
    std::string p, t;
    int m = 1, n = 1, cutoff = 0, prune = 0, full = 0, nw = 1;
    pat_t pat;
    geom_t g;
    int first = 0, last = 0, pos_v = 0, pos_h = 0, max_row_init = 0;
    std::vector<uint64_t> P, M;      // slot s at [s + 1]: slot -1 is addressable, as in the kernel's workspace
    std::vector<int64_t> S;
    int64_t adv = 0;
    uint64_t hinP = ONES, hinM = 0;
    // the slice of qe_types.h instead of arrays sized for the task
    bool ring = false;
    int win_lo = 0, win_hi = -1;     // the block rows this chunk may touch
    std::vector<int> owner;          // the block row each ring index holds (-1: none yet)
    long bad_slot = 0, bad_row = 0, stale = 0, accesses = 0;

    size_t slot(int s) {
        if (ring && (s < -1 || s >= qe::score_lds_cap())) { ++bad_slot; return 0; }
        return (size_t)(s + 1);
    }
    uint64_t& Pv(int s) { return P[slot(s)]; }
    uint64_t& Mv(int s) { return M[slot(s)]; }
    size_t row(int r, bool write) {
        if (!ring) return (size_t)r;
        ++accesses;
        if (r < win_lo || r > win_hi) ++bad_row;
        const int x = qe::score_lds_row(r);
        if (write) owner[(size_t)x] = r;
        else if (owner[(size_t)x] != r) ++stale;
        return (size_t)x;
    }
    int64_t Srd(int r) { return S[row(r, false)]; }
    void Swr(int r, int64_t v) { S[row(r, true)] = v; }
    // what the chunk that starts now may touch: first + pos_v .. last + pos_v + 1
    void open_window() {
        win_lo = first + pos_v; win_hi = last + pos_v + 1;
        if (ring && win_hi - win_lo + 1 > qe::score_lds_ring() - 2) ++bad_row;
    }
};

struct WalkOpts { bool ring, tall; int lane_rel, masked; };

// chunks the wave walked; passes of 4, 2 and 1 slots; multi-slot passes with a lane on 0 < nl < K slots; live slots and
// chunks summed over the lanes; tall passes by height, the chunks one walked alone (whole) or at the head of a taller walk
// (splits), the chunks of QE_TALL_MIN or more slots left to the 4 / 2 / 1 plan, the lanes with dead slots in a tall pass
struct Stats { long chunks = 0, p4 = 0, p2 = 0, p1 = 0, masked = 0, live = 0, lane_chunks = 0, tall[qe::QE_TALL_MAX + 1] = {}, whole = 0, splits = 0, fallbacks = 0, dead = 0; };

inline int popdiff(uint64_t a, uint64_t b) { return __builtin_popcountll(a) - __builtin_popcountll(b); }

// slots_pass<K>: the lane's nl live slots from slot i (block row r), the K - nl below them on zeros
inline void slots_pass(Lane& L, int K, int nl, int i, int r, int k0, long& rule_diffs) {
    uint64_t P[qe::QE_TALL_MAX] = {}, M[qe::QE_TALL_MAX] = {};
    int v0[qe::QE_TALL_MAX], direct[qe::QE_TALL_MAX] = {};
    int64_t sc[qe::QE_TALL_MAX] = {};
    for (int k = 0; k < K; ++k) {
        if (k < nl) { P[k] = L.Pv(i + k); M[k] = L.Mv(i + k); sc[k] = L.Srd(r + k); }
        v0[k] = popdiff(P[k], M[k]);
    }
    uint64_t houtP = 0, houtM = 0;
    for (int c = 0; c < 64; ++c) {
        const int code = enc(L.t[(size_t)k0 * 64 + c]);
        uint64_t ph = (L.hinP >> c) & 1, mh = (L.hinM >> c) & 1, po = 0, mo = 0;
        for (int k = 0; k < K; ++k) {
            // a dead slot's pattern planes are zero: its rows all read 'A' (code 0)
            const uint64_t Eq = (k < nl) ? L.pat.peq[(size_t)(r + k) * ALPHA + code] : (code == 0 ? ONES : 0);
            block_step(Eq, (uint64_t)1 << 63, &P[k], &M[k], ph, mh, &po, &mo);
            direct[k] += (int)po - (int)mo;
            ph = po; mh = mo;
        }
        houtP |= po << c; houtM |= mo << c;
    }
    if (nl > 0) {
        int d = popdiff(houtP, houtM);
        for (int k = K - 1; k >= 0; --k) {
            if (k < nl) {
                if (d != direct[k]) ++rule_diffs;
                L.Swr(r + k, sc[k] + d);
                L.Pv(i + k - 1) = P[k]; L.Mv(i + k - 1) = M[k];      // band shift: slot i + k of this chunk is slot i + k - 1 of the next
            }
            d -= popdiff(P[k], M[k]) - v0[k];
        }
        L.adv += 64 * nl;
    }
    L.hinP = houtP; L.hinM = houtM;
}

// the general single-slot pass of one lane: ncols columns of slot i with the row's own level mask
inline void single_pass(Lane& L, int i, int r, int k0, int ncols) {
    uint64_t P = L.Pv(i), M = L.Mv(i), houtP = 0, houtM = 0;
    int sum = 0;
    for (int c = 0; c < ncols; ++c) {
        const int code = enc(L.t[(size_t)k0 * 64 + c]);
        uint64_t po, mo;
        block_step(L.pat.peq[(size_t)r * ALPHA + code], L.pat.level_mask[r], &P, &M, (L.hinP >> c) & 1, (L.hinM >> c) & 1, &po, &mo);
        sum += (int)po - (int)mo;
        houtP |= po << c; houtM |= mo << c;
    }
    L.Swr(r, L.Srd(r) + sum);
    const int dst = (ncols == 64) ? i - 1 : i;
    L.Pv(dst) = P; L.Mv(dst) = M;
    L.adv += ncols;
    L.hinP = houtP; L.hinM = houtM;
}

// every-64-columns bookkeeping as the kernel does it (the shift has happened in the passes)
inline void chunk_end(Lane& L) {
    const geom_t& G = L.g;
    const int64_t thr = L.prune < L.cutoff ? L.prune : G.cutoff;      // the band-edge rules alone see the threshold, and only one below the task's cutoff
    const bool c1 = (L.first + 2 < L.last) && (G.fin > 64 * (L.first + 1));
    bool cut_lo = false;
    if (c1) cut_lo = L.Srd(L.first + L.pos_v + 1) + (G.fin - 64 * (L.first + 1)) > thr;
    if (cut_lo && L.pos_h >= G.prolog) L.first++;
    else if (!cut_lo && L.pos_h < G.prolog) L.first--;
    L.Pv(L.last) = ONES; L.Mv(L.last) = 0;
    const int pos = L.last + L.pos_v;
    L.Swr(pos + 1, L.Srd(pos) + 64);
    if (pos + 1 > L.max_row_init) L.max_row_init = pos + 1;
    const bool c2 = (L.first + 2 < L.last) && (64 * (L.last - 1) > G.fin);
    bool cut_hi = false;
    if (c2) cut_hi = L.Srd(L.last + L.pos_v - 1) + (64 * (L.last - 1) - G.fin) > thr;
    if (cut_hi || (L.pos_v + L.last >= L.nw)) L.last--;
    L.pos_v++; L.pos_h++;
}

// one group of 64 lanes through the kernel's chunk loop.  Compiles the pattern of every valid lane (the caller frees it
// with pat_free, unless the lane sat a ring walk out).
inline void walk_group(Lane* W[64], const WalkOpts& o, Stats& st, long& rule_diffs) {
    int wave_chunks = 0;
    for (int l = 0; l < 64; ++l) {
        Lane& L = *W[l];
        if (!L.valid) continue;
        pat_compile(&L.pat, L.p.data(), L.m);
        L.nw = (int)L.pat.nw;
        band_geometry(L.m, L.n, L.cutoff, &L.g);
        const int nsl = (int)div_ceil(L.g.cutoff, W64) + 1;
        L.ring = o.ring;
        if (o.ring && !qe::score_lds_fits(nsl)) { pat_free(&L.pat); L.valid = false; continue; }
        L.first = (int)L.g.prolog; L.last = nsl - 1; L.pos_v = -(int)L.g.prolog; L.pos_h = 0; L.max_row_init = nsl - 1;
        if (o.ring) {
            // the slice: (cap + 1) slots of Pv and Mv, ring rows of scores[] -- score_lds_bytes(cap) in all
            const size_t ns1 = (size_t)qe::score_lds_cap() + 1, nr = (size_t)qe::score_lds_ring();
            if ((ns1 * 16 + nr * 4) * 64 != (size_t)qe::score_lds_bytes(qe::score_lds_cap())) ++L.bad_slot;
            L.P.assign(ns1, 0x5555555555555555ull); L.M.assign(ns1, 0x3333333333333333ull);
            L.S.assign(nr, -777777);
            L.owner.assign(nr, -1);
        } else {
            L.P.assign((size_t)nsl + 2, ONES); L.M.assign((size_t)nsl + 2, 0);
            L.S.assign((size_t)L.nw + nsl + 2 * L.g.prolog + 8, 0);
        }
        L.win_lo = 0; L.win_hi = nsl - 1;
        for (int s = 0; s < nsl; ++s) { L.Pv(s) = ONES; L.Mv(s) = 0; L.Swr(s, 64 * (s + 1)); }      // bpm_reset_search
        const int ch = L.n / 64 + ((L.n & 63) ? 1 : 0);
        if (ch > wave_chunks) wave_chunks = ch;
    }
    for (int k = 0; k < wave_chunks; ++k) {
        int ncols[64], rhi[64];
        bool on[64];
        int fmin = 0x7fffffff, fmax = -0x7fffffff;
        bool any_on = false;
        for (int l = 0; l < 64; ++l) {
            Lane& L = *W[l];
            const int nfull = L.n >> 6, tail = L.n & 63;
            ncols[l] = (k < nfull) ? 64 : ((k == nfull) ? tail : 0);
            on[l] = L.valid && ncols[l] > 0;
            rhi[l] = L.last < L.nw - 1 - L.pos_v ? L.last : L.nw - 1 - L.pos_v;
            if (on[l]) { any_on = true; L.open_window(); if (L.first < fmin) fmin = L.first; if (L.first > fmax) fmax = L.first; }
        }
        if (!any_on) continue;
        ++st.chunks;
        const bool rel = o.lane_rel != 0 && fmin < fmax;
        const int i0 = rel ? 0 : fmin;
        int i1 = -0x7fffffff;
        for (int l = 0; l < 64; ++l) {
            if (!on[l]) continue;
            const int v = rel ? rhi[l] - W[l]->first : rhi[l];
            if (v > i1) i1 = v;
            W[l]->hinP = ONES; W[l]->hinM = 0;
            ++st.lane_chunks;
            if (rhi[l] >= W[l]->first) st.live += rhi[l] - W[l]->first + 1;
        }
        for (int x = i0; x <= i1; ++x) {
            int ii[64], rr[64], nl[64];
            for (int l = 0; l < 64; ++l) {
                ii[l] = x + (rel ? (on[l] ? W[l]->first : 0) : 0);
                rr[l] = ii[l] + W[l]->pos_v;
                if (on[l] && ii[l] == W[l]->first) { W[l]->hinP = ONES; W[l]->hinM = 0; }
            }
            auto planned = [&](int K) {
                bool any_bad = false;
                for (int l = 0; l < 64; ++l) {
                    const int lo = on[l] ? W[l]->first : 0x7fffffff, hi = on[l] ? rhi[l] : -0x7fffffff;
                    const bool plain = !(on[l] && (ncols[l] != 64 || W[l]->hasN));
                    bool bad;
                    nl[l] = qe::pass_plan(ii[l], K, lo, hi, rr[l], W[l]->nw, plain, o.masked != 0, bad);
                    any_bad |= bad;
                }
                return !any_bad;
            };
            const int K = qe::score_pass_height(x, i0, i1, o.tall, planned);
            const bool is_tall = K >= qe::QE_TALL_MIN;
            if (o.tall && x == i0) {
                const int h = i1 - i0 + 1;
                if (is_tall) { ++st.tall[K]; (h == K ? st.whole : st.splits)++; }
                else if (h >= qe::QE_TALL_MIN) ++st.fallbacks;
            }
            if (K) {
                bool part = false;
                for (int l = 0; l < 64; ++l) {
                    if (!on[l] || nl[l] == 0) continue;      // nothing of the lane is read or written; it is past its band, or
                                                             // above it, where its carry-in is set anew at i == first
                    slots_pass(*W[l], K, nl[l], ii[l], rr[l], k, rule_diffs);
                    if (nl[l] < K) { part = true; st.dead += is_tall; }
                }
                if (K == 4) ++st.p4; else if (K == 2) ++st.p2;
                st.masked += part;
                x += K - 1;
                continue;
            }
            ++st.p1;
            for (int l = 0; l < 64; ++l)
                if (on[l] && ii[l] >= W[l]->first && ii[l] <= rhi[l]) single_pass(*W[l], ii[l], rr[l], k, ncols[l]);
        }
        for (int l = 0; l < 64; ++l)
            if (on[l] && ncols[l] == 64) chunk_end(*W[l]);
    }
}

inline int64_t read_out(Lane& L) {
    int64_t score = -1;
    // the read-out is outside every chunk's window: what it needs is row nw - 1 as last written (the ring's invariant)
    L.win_lo = L.nw - 1; L.win_hi = L.nw - 1;
    if (L.nw - 1 <= L.max_row_init) { score = L.Srd(L.nw - 1); if (L.m & 63) score -= 64 - (L.m & 63); }
    return score;
}

// a launch file's tasks; header_ints = 3: m n cutoff (no threshold: prune = full = cutoff), 5: m n c1 p C.  false: not such a file
inline bool read_launch(FILE* f, int header_ints, std::vector<Lane>& all) {
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count < 0) return false;
    all.assign((size_t)count, Lane());
    for (auto& L : all) {
        int32_t h[5];
        if (fread(h, 4, (size_t)header_ints, f) != (size_t)header_ints || h[0] < 1 || h[1] < 1) return false;
        L.m = h[0]; L.n = h[1]; L.cutoff = h[2];
        L.prune = header_ints == 5 ? h[3] : h[2]; L.full = header_ints == 5 ? h[4] : h[2];
        L.p.resize((size_t)L.m); L.t.resize((size_t)L.n);
        if (fread(&L.p[0], 1, (size_t)L.m, f) != (size_t)L.m || fread(&L.t[0], 1, (size_t)L.n, f) != (size_t)L.n) return false;
        L.valid = true;
        for (char c : L.p) L.hasN |= enc(c) == 4;
        for (char c : L.t) L.hasN |= enc(c) == 4;
    }
    return true;
}

// the command line every program has: <file> <lane_rel 0|1> <masked 0|1>.  -> 0, or the exit code (2) after the message
inline int read_args(int argc, char** argv, const char* name, int header_ints, std::vector<Lane>& all, WalkOpts& o) {
    if (argc < 4) { fprintf(stderr, "usage: %s <file> <lane_rel> <masked>\n", name); return 2; }
    o.lane_rel = atoi(argv[2]); o.masked = atoi(argv[3]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const bool ok = read_launch(f, header_ints, all);
    fclose(f);
    return ok ? 0 : 2;
}

// the last line of the programs that walk the 4 / 2 / 1 plan alone
inline void print_per_chunk(const Stats& st) {
    const double c = st.chunks ? (double)st.chunks : 1.0, lc = st.lane_chunks ? (double)st.lane_chunks : 1.0;
    printf("per chunk: live slots per lane %.2f, slots the wave walks %.2f, 4-slot passes %.2f, 2-slot %.2f, single-slot %.2f\n",
           st.live / lc, (4.0 * st.p4 + 2.0 * st.p2 + st.p1) / c, st.p4 / c, st.p2 / c, st.p1 / c);
}

// the group of 64 that starts at task g0: its lanes, `idle` where the launch has no more
inline void group_at(std::vector<Lane>& all, size_t g0, Lane& idle, Lane* W[64]) {
    for (int l = 0; l < 64; ++l) W[l] = (g0 + l < all.size()) ? &all[g0 + l] : &idle;
}

}  // namespace
