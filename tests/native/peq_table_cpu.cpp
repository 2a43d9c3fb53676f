// Eq from a table (qe_types.h: peq_*; DESIGN.md 4.1, "Eq from a table"), without a GPU.
//   peq_table_cpu layout
// checks the layout functions alone: every entry against the plane formula for all (a, b, sym) bit cases, the offsets of
// distinct (sym, slot, lane) apart and inside the slice, four slices within half a CU's LDS, lane l on bank 2 l mod 64.
//   peq_table_cpu <file> <lane_rel 0|1> <masked 0|1>
// walks every group of 64 tasks twice with the tall plan, the state in plain arrays by absolute block row as the table form
// keeps it: once through tests/native/banded_walk.h as it is (Eq of a live slot from the compiled pattern, a dead slot on
// zero planes), and once with every TALL pass taking Eq from a table built as the kernel builds it -- the planes a, b of the
// pass's slots (zeros for a dead slot) through peq_entry into a wave's slice at peq_offset, then one read per block step at
// the column's symbol.  The chunk loop below is walk_group's with that one pass exchanged; everything else is the header's.
// Checked per task: score, first / last / pos_v, max_row_init and block advances of the two walks are equal.  Checked per
// access of the table: the offset lies in the slice (bad_off), the entry was written by THIS pass (unwritten), the column's
// symbol is one of four (bad_sym), and a live slot's entry equals the compiled pattern's Eq word (mismatch).
// file: int32 count, then per pair int32 m, n, c1, p, C and the m + n bytes of pattern and text (narrow_prune_lib.write_launch).
// Prints one line per pair ("pair <index> score <..> adv <block-columns> eligible 1"), then the counts.  Exit code 1: a difference.
#include "banded_walk.h"

namespace {

const int CU_LDS = 160 * 1024;

struct Table {                       // a wave's slice and what was seen of its accesses
    std::vector<uint64_t> w;
    std::vector<long> gen;           // the pass that wrote each word
    long pass = 0, bad_off = 0, unwritten = 0, bad_sym = 0, mismatch = 0, reads = 0, writes = 0;
    Table() : w((size_t)qe::peq_bytes() / 8, 0xDEADDEADDEADDEADull), gen((size_t)qe::peq_bytes() / 8, -1) {}
    bool inside(int off) const { return off >= 0 && off % 8 == 0 && off + 8 <= qe::peq_bytes(); }
    void write(int off, uint64_t v) {
        ++writes;
        if (!inside(off)) { ++bad_off; return; }
        w[(size_t)off / 8] = v; gen[(size_t)off / 8] = pass;
    }
    uint64_t read(int off) {
        ++reads;
        if (!inside(off)) { ++bad_off; return 0; }
        if (gen[(size_t)off / 8] != pass) ++unwritten;
        return w[(size_t)off / 8];
    }
};

// the two code planes of block row r of the lane's pattern, as k_pack lays them out: bit j of a / b = bit 0 / 1 of the code
// of pattern[64 r + j]
inline void planes_of(const Lane& L, int r, uint64_t& a, uint64_t& b) {
    a = 0; b = 0;
    for (int j = 0; j < 64; ++j) {
        const size_t x = (size_t)r * 64 + (size_t)j;
        if (x >= (size_t)L.m) break;
        const int code = enc(L.p[x]);
        a |= (uint64_t)(code & 1) << j; b |= (uint64_t)((code >> 1) & 1) << j;
    }
}

// slots_pass of banded_walk.h for a tall pass of the table form: same state, same score rule, Eq from the table
inline void slots_pass_table(Lane& L, int lane, Table& T, int K, int nl, int i, int r, int k0, long& rule_diffs) {
    uint64_t P[qe::QE_TALL_MAX] = {}, M[qe::QE_TALL_MAX] = {};
    int v0[qe::QE_TALL_MAX], direct[qe::QE_TALL_MAX] = {};
    int64_t sc[qe::QE_TALL_MAX] = {};
    ++T.pass;
    for (int k = 0; k < K; ++k) {
        uint64_t a = 0, b = 0;
        if (k < nl) { P[k] = L.Pv(i + k); M[k] = L.Mv(i + k); sc[k] = L.Srd(r + k); planes_of(L, r + k, a, b); }
        v0[k] = popdiff(P[k], M[k]);
        for (int sym = 0; sym < 4; ++sym) {
            const uint64_t e = qe::peq_entry(a, b, sym);
            if (k < nl && e != L.pat.peq[(size_t)(r + k) * ALPHA + sym]) ++T.mismatch;
            T.write(qe::peq_offset(sym, k, lane), e);
        }
    }
    uint64_t houtP = 0, houtM = 0;
    for (int c = 0; c < 64; ++c) {
        int code = enc(L.t[(size_t)k0 * 64 + c]);
        if (code < 0 || code > 3) { ++T.bad_sym; code = 0; }       // (a lane with another symbol never takes a multi-slot pass)
        uint64_t ph = (L.hinP >> c) & 1, mh = (L.hinM >> c) & 1, po = 0, mo = 0;
        for (int k = 0; k < K; ++k) {
            const uint64_t Eq = T.read(qe::peq_offset(code, k, lane));
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
                L.Pv(i + k - 1) = P[k]; L.Mv(i + k - 1) = M[k];
            }
            d -= popdiff(P[k], M[k]) - v0[k];
        }
        L.adv += 64 * nl;
    }
    L.hinP = houtP; L.hinM = houtM;
}

// walk_group of banded_walk.h (plain arrays, the tall plan) with the tall passes through slots_pass_table
inline void walk_group_table(Lane* W[64], const WalkOpts& o, Table& T, Stats& st, long& rule_diffs) {
    int wave_chunks = 0;
    for (int l = 0; l < 64; ++l) {
        Lane& L = *W[l];
        if (!L.valid) continue;
        pat_compile(&L.pat, L.p.data(), L.m);
        L.nw = (int)L.pat.nw;
        band_geometry(L.m, L.n, L.cutoff, &L.g);
        const int nsl = (int)div_ceil(L.g.cutoff, W64) + 1;
        L.ring = false;
        L.first = (int)L.g.prolog; L.last = nsl - 1; L.pos_v = -(int)L.g.prolog; L.pos_h = 0; L.max_row_init = nsl - 1;
        L.P.assign((size_t)nsl + 2, ONES); L.M.assign((size_t)nsl + 2, 0);
        L.S.assign((size_t)L.nw + nsl + 2 * L.g.prolog + 8, 0);
        for (int s = 0; s < nsl; ++s) { L.Pv(s) = ONES; L.Mv(s) = 0; L.Swr(s, 64 * (s + 1)); }
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
        const bool rel = o.lane_rel != 0 && fmin < fmax;
        const int i0 = rel ? 0 : fmin;
        int i1 = -0x7fffffff;
        for (int l = 0; l < 64; ++l) {
            if (!on[l]) continue;
            const int v = rel ? rhi[l] - W[l]->first : rhi[l];
            if (v > i1) i1 = v;
            W[l]->hinP = ONES; W[l]->hinM = 0;
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
            const int K = qe::score_pass_height(x, i0, i1, true, planned);
            if (K >= qe::QE_TALL_MIN) {
                ++st.tall[K];
                // the kernel's table has peq_cap() slots: no taller pass may be planned
                if (K > qe::peq_cap()) ++T.bad_off;
                for (int l = 0; l < 64; ++l) {
                    if (!on[l] || nl[l] == 0) continue;
                    slots_pass_table(*W[l], l, T, K, nl[l], ii[l], rr[l], k, rule_diffs);
                    if (nl[l] < K) ++st.dead;
                }
                x += K - 1;
                continue;
            }
            if (K) {
                for (int l = 0; l < 64; ++l)
                    if (on[l] && nl[l] != 0) slots_pass(*W[l], K, nl[l], ii[l], rr[l], k, rule_diffs);
                if (K == 4) ++st.p4; else ++st.p2;
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

int check_layout() {
    long bad = 0;
    // every entry against the plane formula, all sixteen (a, b, t0, t1) bit cases in one word and its complement patterns
    const uint64_t as[] = {0, ONES, 0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0x0123456789ABCDEFull}, bs[] = {0, ONES, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull, 0xFEDCBA9876543210ull};
    for (uint64_t a : as) for (uint64_t b : bs) for (int sym = 0; sym < 4; ++sym) {
        const uint64_t e = qe::peq_entry(a, b, sym);
        for (int j = 0; j < 64; ++j) {
            const int abit = (int)((a >> j) & 1), bbit = (int)((b >> j) & 1), t0 = sym & 1, t1 = sym >> 1;
            if ((int)((e >> j) & 1) != ((abit == t0) && (bbit == t1))) ++bad;
        }
        // the kernel's plane arithmetic with the column's masks m0 = -t0, m1 = -t1: ~(a ^ m0) & ~(b ^ m1)
        const uint64_t m0 = (sym & 1) ? ONES : 0, m1 = (sym & 2) ? ONES : 0;
        if (e != (~(a ^ m0) & ~(b ^ m1))) ++bad;
    }
    // offsets: distinct, 8-byte words inside the slice; lane l on bank 2 l mod 64 (4-byte banks, 64 of them)
    std::vector<int> seen((size_t)qe::peq_bytes() / 8, 0);
    for (int sym = 0; sym < 4; ++sym) for (int s = 0; s < qe::peq_cap(); ++s) for (int l = 0; l < 64; ++l) {
        const int off = qe::peq_offset(sym, s, l);
        if (off < 0 || off % 8 || off + 8 > qe::peq_bytes()) { ++bad; continue; }
        if (seen[(size_t)off / 8]++) ++bad;
        if ((off / 4) % 64 != (2 * l) % 64) ++bad;
    }
    if (qe::peq_sym_stride() % 256) ++bad;
    if (qe::peq_cap() != qe::QE_TALL_MAX) ++bad;                     // every tall pass has its slots in the table
    if (4 * qe::peq_bytes() * 2 > CU_LDS) ++bad;                     // two workgroups of four slices per CU
    printf("layout cap %d sym_stride %d bytes %d workgroup %d bad %ld\n", qe::peq_cap(), qe::peq_sym_stride(), qe::peq_bytes(), 4 * qe::peq_bytes(), bad);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && strcmp(argv[1], "layout") == 0) return check_layout();
    std::vector<Lane> all;
    WalkOpts plan = {false, true, 0, 0};
    if (const int rc = read_args(argc, argv, "peq_table_cpu", 5, all, plan)) return rc;

    Stats st, st_tab;
    Table T;
    long diffs = 0, rule_diffs = 0;
    for (size_t g0 = 0; g0 < all.size(); g0 += 64) {
        const size_t g1 = g0 + 64 < all.size() ? g0 + 64 : all.size();
        std::vector<Lane> tab_copy(all.begin() + (long)g0, all.begin() + (long)g1);
        Lane idle_a, idle_b;
        Lane *A[64], *B[64];
        group_at(all, g0, idle_a, A);
        group_at(tab_copy, 0, idle_b, B);
        walk_group(A, plan, st, rule_diffs);
        walk_group_table(B, plan, T, st_tab, rule_diffs);
        for (size_t l = 0; l < g1 - g0; ++l) {
            Lane &L = *A[l], &R = *B[l];
            const int64_t score = read_out(L), rs = read_out(R);
            if (rs != score || R.adv != L.adv || R.first != L.first || R.last != L.last || R.pos_v != L.pos_v || R.max_row_init != L.max_row_init) {
                if (diffs < 10) fprintf(stderr, "pair %zu: the table walk has %lld adv %lld first %d last %d, the walk without %lld adv %lld first %d last %d (m %d n %d c1 %d p %d)\n", g0 + l,
                                        (long long)rs, (long long)R.adv, R.first, R.last, (long long)score, (long long)L.adv, L.first, L.last, L.m, L.n, L.cutoff, L.prune);
                ++diffs;
            }
            pat_free(&R.pat);
            pat_free(&L.pat);
            printf("pair %zu score %lld adv %lld eligible 1\n", g0 + l, (long long)score, (long long)L.adv);
            L.valid = false;
        }
    }
    long tall_diff = 0;
    for (int h = qe::QE_TALL_MIN; h <= qe::QE_TALL_MAX; ++h) tall_diff += st.tall[h] != st_tab.tall[h];
    printf("pairs %zu lane_rel %d masked %d diffs %ld rule_diffs %ld bad_off %ld unwritten %ld bad_sym %ld mismatch %ld reads %ld writes %ld chunks %ld "
           "passes4 %ld passes2 %ld passes1 %ld tall5 %ld tall6 %ld tall7 %ld tall8 %ld tall9 %ld tall10 %ld tall_diff %ld dead_lanes %ld\n",
           all.size(), plan.lane_rel, plan.masked, diffs, rule_diffs, T.bad_off, T.unwritten, T.bad_sym, T.mismatch, T.reads, T.writes, st_tab.chunks,
           st_tab.p4, st_tab.p2, st_tab.p1, st_tab.tall[5], st_tab.tall[6], st_tab.tall[7], st_tab.tall[8], st_tab.tall[9], st_tab.tall[10], tall_diff, st_tab.dead);
    return (diffs || rule_diffs || T.bad_off || T.unwritten || T.bad_sym || T.mismatch || tall_diff || st.chunks != st_tab.chunks || st.p4 != st_tab.p4 ||
            st.p2 != st_tab.p2 || st.p1 != st_tab.p1) ? 1 : 0;
}
