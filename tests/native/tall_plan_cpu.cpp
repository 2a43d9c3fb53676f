// Tall passes of k_banded<false, true> (qe_types.h: tall_height, pass_plan; DESIGN.md 4.1, "Tall passes"), without a GPU: the
// walk of tests/native/score_ring_cpu.cpp -- the kernel's chunk loop, pass plan and band-edge rules with the oracle's block
// step, the state in a slice laid out as the LDS form lays it out, scores[] through the ring of score_lds_row() -- run twice
// over every group of 64 tasks: with the 4 / 2 / 1 plan alone, and with the kernel's tall plan in front of it (one pass of
// tall_height(h) slots at the first step of a chunk whose walk is h slots long, where pass_plan has no fallback at that
// height).  A task whose band the slice cannot hold sits both walks out, as the kernel leaves it out.  Checked per task: score,
// first / last / pos_v, max_row_init and block advances of the two walks are equal.  Checked per access of both walks: the
// slot lies in -1 .. cap - 1, the row in the chunk's window first + pos_v .. last + pos_v + 1, and a row that is read is the
// row last written at its ring index.  Counted: the passes of every height, the chunks a tall pass walked alone, the splits
// (a tall pass at the head of a taller walk), and the chunks of five or more slots that fell back to the old plan.
//   tall_plan_cpu <file> <lane_rel 0|1> <masked 0|1>
// file: int32 count, then per pair int32 m, n, c1, p, C and the m + n bytes of pattern and text (narrow_prune_lib.write_launch).
// Prints one line per pair ("pair <index> score <..> adv <block-columns> eligible <0|1>"), then the counts.
// Exit code 1: a difference, an access outside its window, or a stale row.
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

struct Stats { long chunks = 0, p4 = 0, p2 = 0, p1 = 0, live = 0, lane_chunks = 0, tall[qe::QE_TALL_MAX + 1] = {}, whole = 0, splits = 0, fallbacks = 0, dead = 0; };

inline int popdiff(uint64_t a, uint64_t b) { return __builtin_popcountll(a) - __builtin_popcountll(b); }

// slots_pass<K>: the lane's nl live slots from slot i (block row r), the K - nl below them on zeros
void slots_pass(Lane& L, int K, int nl, int i, int r, int k0, long& rule_diffs) {
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
void single_pass(Lane& L, int i, int r, int k0, int ncols) {
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
void chunk_end(Lane& L) {
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


// one group of 64 lanes through the kernel's chunk loop; ring = the second walk (lanes the budget rejects sit it out)
void walk_group(Lane* W[64], bool ring, bool tall, int lane_rel, int mode, Stats& st, long& rule_diffs) {
    int wave_chunks = 0;
    for (int l = 0; l < 64; ++l) {
        Lane& L = *W[l];
        if (!L.valid) continue;
        pat_compile(&L.pat, L.p.data(), L.m);
        L.nw = (int)L.pat.nw;
        band_geometry(L.m, L.n, L.cutoff, &L.g);
        const int nsl = (int)div_ceil(L.g.cutoff, W64) + 1;
        L.ring = ring;
        if (ring && !qe::score_lds_fits(nsl)) { pat_free(&L.pat); L.valid = false; continue; }
        L.first = (int)L.g.prolog; L.last = nsl - 1; L.pos_v = -(int)L.g.prolog; L.pos_h = 0; L.max_row_init = nsl - 1;
        if (ring) {
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
        const bool rel = lane_rel != 0 && fmin < fmax;
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
                    nl[l] = qe::pass_plan(ii[l], K, lo, hi, rr[l], W[l]->nw, plain, mode != 0, bad);
                    any_bad |= bad;
                }
                return !any_bad;
            };
            int K = 0;
            // the kernel's tall plan: at the first step of the chunk, from the top of the band
            if (tall && x == i0) {
                const int h = i1 - i0 + 1, T = qe::tall_height(h);
                if (T && planned(T)) {
                    K = T;
                    ++st.tall[T];
                    (h == T ? st.whole : st.splits)++;
                    for (int l = 0; l < 64; ++l) st.dead += on[l] && nl[l] > 0 && nl[l] < T;
                } else if (h >= qe::QE_TALL_MIN) ++st.fallbacks;
            }
            if (!K) {
                if (x + 3 <= i1 && planned(4)) K = 4;
                else if (x + 1 <= i1 && planned(2)) K = 2;
            }
            if (K) {
                for (int l = 0; l < 64; ++l)
                    if (on[l] && nl[l] > 0) slots_pass(*W[l], K, nl[l], ii[l], rr[l], k, rule_diffs);
                if (K == 4) ++st.p4; else if (K == 2) ++st.p2;
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

int64_t read_out(Lane& L) {
    int64_t score = -1;
    // the read-out is outside every chunk's window: what it needs is row nw - 1 as last written (the ring's invariant)
    L.win_lo = L.nw - 1; L.win_hi = L.nw - 1;
    if (L.nw - 1 <= L.max_row_init) { score = L.Srd(L.nw - 1); if (L.m & 63) score -= 64 - (L.m & 63); }
    return score;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: tall_plan_cpu <file> <lane_rel> <masked>\n"); return 2; }
    const int lane_rel = atoi(argv[2]), mode = atoi(argv[3]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    std::vector<Lane> all((size_t)count);
    for (auto& L : all) {
        int32_t h[5];
        if (fread(h, 4, 5, f) != 5 || h[0] < 1 || h[1] < 1) return 2;
        L.m = h[0]; L.n = h[1]; L.cutoff = h[2]; L.prune = h[3]; L.full = h[4];
        L.p.resize((size_t)L.m); L.t.resize((size_t)L.n);
        if (fread(&L.p[0], 1, (size_t)L.m, f) != (size_t)L.m || fread(&L.t[0], 1, (size_t)L.n, f) != (size_t)L.n) return 2;
        L.valid = true;
        for (char c : L.p) L.hasN |= enc(c) == 4;
        for (char c : L.t) L.hasN |= enc(c) == 4;
    }
    fclose(f);

    Stats st, st_tall;
    long diffs = 0, rule_diffs = 0, eligible = 0, rejected = 0, bad_slot = 0, bad_row = 0, stale = 0, accesses = 0;
    for (size_t g0 = 0; g0 < all.size(); g0 += 64) {
        Lane idle_a, idle_b;
        std::vector<Lane> tall_copy;
        tall_copy.reserve(64);
        Lane *A[64], *B[64];
        for (int l = 0; l < 64; ++l) {
            A[l] = (g0 + l < all.size()) ? &all[g0 + l] : &idle_a;
            if (g0 + l < all.size()) { tall_copy.push_back(all[g0 + l]); B[l] = &tall_copy.back(); } else B[l] = &idle_b;
        }
        walk_group(A, true, false, lane_rel, mode, st, rule_diffs);
        walk_group(B, true, true, lane_rel, mode, st_tall, rule_diffs);
        for (int l = 0; l < 64; ++l) {
            Lane &L = *A[l], &R = *B[l];
            if (g0 + l >= all.size()) continue;
            int64_t score = -1;
            if (L.valid) {
                ++eligible;
                score = read_out(L);
                const int64_t rs = read_out(R);
                if (!R.valid || rs != score || R.adv != L.adv || R.first != L.first || R.last != L.last || R.pos_v != L.pos_v || R.max_row_init != L.max_row_init) {
                    if (diffs < 10) fprintf(stderr, "pair %zu: the tall walk has %lld adv %lld first %d last %d, the old plan %lld adv %lld first %d last %d (m %d n %d c1 %d p %d)\n", g0 + l,
                                            (long long)rs, (long long)R.adv, R.first, R.last, (long long)score, (long long)L.adv, L.first, L.last, L.m, L.n, L.cutoff, L.prune);
                    ++diffs;
                }
                bad_slot += R.bad_slot + L.bad_slot; bad_row += R.bad_row + L.bad_row; stale += R.stale + L.stale; accesses += R.accesses;
                pat_free(&R.pat);
                pat_free(&L.pat);
            } else ++rejected;
            printf("pair %zu score %lld adv %lld eligible %d\n", g0 + l, (long long)score, (long long)L.adv, L.valid ? 1 : 0);
            L.valid = false;
        }
    }
    printf("pairs %d lane_rel %d masked %d diffs %ld rule_diffs %ld eligible %ld rejected %ld bad_slot %ld bad_row %ld stale %ld accesses %ld chunks %ld "
           "old4 %ld old2 %ld old1 %ld passes4 %ld passes2 %ld passes1 %ld tall5 %ld tall6 %ld tall7 %ld tall8 %ld tall9 %ld tall10 %ld whole %ld splits %ld "
           "fallbacks %ld dead_lanes %ld live %ld lane_chunks %ld\n",
           (int)count, lane_rel, mode, diffs, rule_diffs, eligible, rejected, bad_slot, bad_row, stale, accesses, st_tall.chunks,
           st.p4, st.p2, st.p1, st_tall.p4, st_tall.p2, st_tall.p1, st_tall.tall[5], st_tall.tall[6], st_tall.tall[7], st_tall.tall[8], st_tall.tall[9],
           st_tall.tall[10], st_tall.whole, st_tall.splits, st_tall.fallbacks, st_tall.dead, st_tall.live, st_tall.lane_chunks);
    return (diffs || rule_diffs || bad_slot || bad_row || stale || st.chunks != st_tall.chunks) ? 1 : 0;
}
