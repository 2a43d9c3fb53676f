// The walk of tests/native/pass_plan_cpu.cpp with a pruning threshold per task ("The pruning threshold"): the
// band geometry is that of the task's first-pass cutoff c1, the two band-edge rules compare against p where p < c1 (else
// against the geometry's clamped cutoff) as k_banded<false> does with BandedArgs::prune, everything else is the kernel's walk with the oracle's block step.  Per
// pair the result goes through qe_types.h's narrow_accepts_pruned(m, n, c1, C, p, .) and is compared with the oracle's pass
// at the full cutoff C: an ACCEPTED result that differs is an error (exit code 1).  `lost` counts the pairs whose distance
// the threshold allows (the oracle's score at C passes the same rule) and whose walk did not return it.  A task whose
// threshold is not below its cutoff c1 must also advance the oracle's block-columns at c1.
//   narrow_prune_cpu <file> <lane_rel 0|1> <masked 0|1>
// file: int32 count, then per pair int32 m, n, c1, p, C and the m + n bytes of pattern and text.
// Prints one line per pair ("pair <index> score <walk's> adv <block-columns> accepted <0|1>"), then the counts and the
// passes per chunk.
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
};

struct Stats { long chunks = 0, p4 = 0, p2 = 0, p1 = 0, masked = 0, live = 0, lane_chunks = 0; };

inline int popdiff(uint64_t a, uint64_t b) { return __builtin_popcountll(a) - __builtin_popcountll(b); }

// slots_pass<K>: the lane's nl live slots from slot i (block row r), the K - nl below them on zeros
void slots_pass(Lane& L, int K, int nl, int i, int r, int k0, long& rule_diffs) {
    uint64_t P[4] = {0, 0, 0, 0}, M[4] = {0, 0, 0, 0};
    int v0[4], direct[4] = {0, 0, 0, 0};
    int64_t sc[4] = {0, 0, 0, 0};
    for (int k = 0; k < K; ++k) {
        if (k < nl) { P[k] = L.P[i + k + 1]; M[k] = L.M[i + k + 1]; sc[k] = L.S[r + k]; }
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
                L.S[r + k] = sc[k] + d;
                L.P[i + k] = P[k]; L.M[i + k] = M[k];      // band shift: slot i + k of this chunk is slot i + k - 1 of the next
            }
            d -= popdiff(P[k], M[k]) - v0[k];
        }
        L.adv += 64 * nl;
    }
    L.hinP = houtP; L.hinM = houtM;
}

// the general single-slot pass of one lane: ncols columns of slot i with the row's own level mask
void single_pass(Lane& L, int i, int r, int k0, int ncols) {
    uint64_t P = L.P[i + 1], M = L.M[i + 1], houtP = 0, houtM = 0;
    int sum = 0;
    for (int c = 0; c < ncols; ++c) {
        const int code = enc(L.t[(size_t)k0 * 64 + c]);
        uint64_t po, mo;
        block_step(L.pat.peq[(size_t)r * ALPHA + code], L.pat.level_mask[r], &P, &M, (L.hinP >> c) & 1, (L.hinM >> c) & 1, &po, &mo);
        sum += (int)po - (int)mo;
        houtP |= po << c; houtM |= mo << c;
    }
    L.S[r] += sum;
    const int dst = (ncols == 64) ? i - 1 : i;
    L.P[dst + 1] = P; L.M[dst + 1] = M;
    L.adv += ncols;
    L.hinP = houtP; L.hinM = houtM;
}

// every-64-columns bookkeeping as the kernel does it (the shift has happened in the passes)
void chunk_end(Lane& L) {
    const geom_t& G = L.g;
    const int64_t thr = L.prune < L.cutoff ? L.prune : G.cutoff;      // the band-edge rules alone see the threshold, and only one below the task's cutoff
    const bool c1 = (L.first + 2 < L.last) && (G.fin > 64 * (L.first + 1));
    bool cut_lo = false;
    if (c1) cut_lo = L.S[L.first + L.pos_v + 1] + (G.fin - 64 * (L.first + 1)) > thr;
    if (cut_lo && L.pos_h >= G.prolog) L.first++;
    else if (!cut_lo && L.pos_h < G.prolog) L.first--;
    L.P[L.last + 1] = ONES; L.M[L.last + 1] = 0;
    const int pos = L.last + L.pos_v;
    L.S[pos + 1] = L.S[pos] + 64;
    if (pos + 1 > L.max_row_init) L.max_row_init = pos + 1;
    const bool c2 = (L.first + 2 < L.last) && (64 * (L.last - 1) > G.fin);
    bool cut_hi = false;
    if (c2) cut_hi = L.S[L.last + L.pos_v - 1] + (64 * (L.last - 1) - G.fin) > thr;
    if (cut_hi || (L.pos_v + L.last >= L.nw)) L.last--;
    L.pos_v++; L.pos_h++;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: narrow_prune_cpu <file> <lane_rel> <masked>\n"); return 2; }
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

    Stats st;
    long diffs = 0, rule_diffs = 0, accepted = 0, rejected = 0, lost = 0;
    for (size_t g0 = 0; g0 < all.size(); g0 += 64) {
        Lane idle;
        Lane* W[64];
        int wave_chunks = 0;
        for (int l = 0; l < 64; ++l) {
            W[l] = (g0 + l < all.size()) ? &all[g0 + l] : &idle;
            Lane& L = *W[l];
            if (!L.valid) continue;
            pat_compile(&L.pat, L.p.data(), L.m);
            L.nw = (int)L.pat.nw;
            band_geometry(L.m, L.n, L.cutoff, &L.g);
            const int nsl = (int)div_ceil(L.g.cutoff, W64) + 1;
            L.first = (int)L.g.prolog; L.last = nsl - 1; L.pos_v = -(int)L.g.prolog; L.pos_h = 0; L.max_row_init = nsl - 1;
            L.P.assign((size_t)nsl + 2, ONES); L.M.assign((size_t)nsl + 2, 0);
            L.S.assign((size_t)L.nw + nsl + 2 * L.g.prolog + 8, 0);
            for (int s = 0; s < nsl; ++s) L.S[s] = 64 * (s + 1);
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
                if (on[l]) { any_on = true; if (L.first < fmin) fmin = L.first; if (L.first > fmax) fmax = L.first; }
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
                if (x + 3 <= i1 && planned(4)) K = 4;
                else if (x + 1 <= i1 && planned(2)) K = 2;
                if (K) {
                    bool part = false;
                    for (int l = 0; l < 64; ++l) {
                        if (!on[l] || nl[l] == 0) continue;      // nothing of the lane is read or written; it is past its band, or
                                                                 // above it, where its carry-in is set anew at i == first
                        slots_pass(*W[l], K, nl[l], ii[l], rr[l], k, rule_diffs);
                        part |= nl[l] > 0 && nl[l] < K;
                    }
                    (K == 4 ? st.p4 : st.p2)++;
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
        for (int l = 0; l < 64; ++l) {
            Lane& L = *W[l];
            if (!L.valid) continue;
            int64_t score = -1;
            if (L.nw - 1 <= L.max_row_init) { score = L.S[L.nw - 1]; if (L.m & 63) score -= 64 - (L.m & 63); }
            const int64_t osc = qo_banded_score(L.p.data(), L.m, L.t.data(), L.n, L.full, L.n, nullptr, nullptr, nullptr);
            const bool ok = qe::narrow_accepts_pruned(L.m, L.n, L.cutoff, L.full, L.prune, (int)score);
            (ok ? accepted : rejected)++;
            if (ok && score != osc) {
                if (diffs < 10) fprintf(stderr, "pair %zu: accepted %lld, the oracle at %d has %lld (c1 %d p %d)\n", g0 + l, (long long)score, L.full, (long long)osc, L.cutoff, L.prune);
                ++diffs;
            }
            if (!ok && qe::narrow_accepts_pruned(L.m, L.n, L.cutoff, L.full, L.prune, (int)osc)) ++lost;
            if (L.prune >= L.cutoff) {
                int64_t oadv = 0;
                const int64_t s1 = qo_banded_score(L.p.data(), L.m, L.t.data(), L.n, L.cutoff, L.n, nullptr, nullptr, &oadv);
                if (s1 != score || oadv != L.adv) {
                    if (diffs < 10) fprintf(stderr, "pair %zu: unpruned walk %lld / %lld adv %lld / %lld\n", g0 + l, (long long)score, (long long)s1, (long long)L.adv, (long long)oadv);
                    ++diffs;
                }
            }
            printf("pair %zu score %lld adv %lld accepted %d\n", g0 + l, (long long)score, (long long)L.adv, ok ? 1 : 0);
            pat_free(&L.pat);
            L.valid = false;
        }
    }
    const double c = st.chunks ? (double)st.chunks : 1.0, lc = st.lane_chunks ? (double)st.lane_chunks : 1.0;
    printf("pairs %d lane_rel %d masked %d diffs %ld rule_diffs %ld accepted %ld rejected %ld lost %ld live %ld lane_chunks %ld chunks %ld passes4 %ld passes2 %ld passes1 %ld partial_passes %ld\n",
           (int)count, lane_rel, mode, diffs, rule_diffs, accepted, rejected, lost, st.live, st.lane_chunks, st.chunks, st.p4, st.p2, st.p1, st.masked);
    printf("per chunk: live slots per lane %.2f, slots the wave walks %.2f, 4-slot passes %.2f, 2-slot %.2f, single-slot %.2f\n",
           st.live / lc, (4.0 * st.p4 + 2.0 * st.p2 + st.p1) / c, st.p4 / c, st.p2 / c, st.p1 / c);
    return (diffs || rule_diffs) ? 1 : 0;
}
