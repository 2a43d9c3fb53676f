// Host stand-ins for the kernels of quicked_amd/csrc/qe_kernels.hip, for the sanitizer build of the library's HOST layer
// (see hip/hip_runtime.h next to this file).  The kernels the host logic depends on for its control flow are real code here
// (in-stream copies, the offsets scan, the stage-1 rule, the cut-off hand-over, the CIGAR validator); the bounded, search, panel
// and tag kernels and k_narrow run the per-lane source of the qe_*.h headers task by task; the alignment kernels leave plausible
// zeros -- a bound of `QE_STUB_BOUND` and, for every `QE_STUB_SKIP_EVERY`-th task, the "goes on to stage 2" flag, so that
// the fast flow's overflow path, the early-finish threads and the merged flows all get work.  TEST INFRASTRUCTURE.
#pragma once
#define QE_STUB_HAS_EVERY_STAND_IN 1      // qe_driver.hip then looks for no satellite header
#include <algorithm>
#include "qe_types.h"
#include "qe_check.h"
#include "qe_panel_ham.h"      // and through it qe_panel.h, qe_search.h, qe_bounded.h, qe_iupac.h
#include "qe_panel_align.h"
#include "qe_tags.h"

namespace qe {

struct CopyTable {
    enum { MAX = 16 };
    int32_t n;
    uint4* dst[MAX]; const uint4* src[MAX]; int64_t n_u4[MAX];
};
static inline int stub_env(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

static void k_copy_multi(CopyTable T) { for (int i = 0; i < T.n; ++i) if (T.n_u4[i] > 0) memmove(T.dst[i], T.src[i], (size_t)T.n_u4[i] * 16); }
static void k_gather_words(int nspans, const int64_t* src_addr, const int64_t* dst_off, const int32_t* nwords, u64* dst) {
    for (int e = 0; e < nspans; ++e) memmove(dst + dst_off[e], reinterpret_cast<const u64*>(src_addr[e]), (size_t)nwords[e] * 8);
}
static void k_copy_total(uint4* dst, const uint4* src, const int64_t* total, int64_t cap_u4) {
    const int64_t n = std::min((*total + 15) >> 4, cap_u4);
    if (n > 0) memmove(dst, src, (size_t)n * 16);
}
static void k_scan_offsets(const int32_t* len, const int32_t* pair, int64_t* off, int64_t* total, int n) {
    int64_t carry = 0;
    for (int i = 0; i < n; ++i) { off[i] = carry; if (pair[i] >= 0) carry += (int64_t)len[i] + 1; }
    *total = carry;
}
static void k_stage1_decide(Stage1Args A) {
    const int every = stub_env("QE_STUB_SKIP_EVERY", 0);
    for (int t = 0; t < A.nt; ++t) {
        int cut = 0, skip = 1;
        u32 steps = 0;
        if (A.pair[t] >= 0) {
            cut = A.score[t];
            skip = ((every > 0 && t % every == 0) ? 1 : 0) | ((cut > A.est[t]) ? 2 : 0);
            steps = A.steps[t];
        }
        A.o_cut[t] = cut; A.o_skip[t] = skip; A.o_steps[t] = steps;
    }
}
static void k_apply_cutoffs(int nt, int32_t* cutoff, int32_t* pair, const int32_t* cut, const int32_t* skip) {
    for (int t = 0; t < nt; ++t) { cutoff[t] = cut[t]; if (skip[t] != 0) pair[t] = -1; }
}
// WindowEd: a bound per task (what stage 1 hands the align step), no high-error windows
static void stub_windowed(const WindowArgs& A) {
    const int bound = stub_env("QE_STUB_BOUND", 70);
    for (int t = 0; t < A.T.ntasks; ++t) {
        if (A.T.pair[t] < 0 || (A.only_if && A.only_if[t] == 0)) continue;
        A.o_score[t] = bound; A.o_hew[t] = 0; A.o_steps[t] = 1;
        if (!A.score_only) { A.o_nruns[t] = 0; A.o_nops[t] = 0; A.o_edits[t] = 0; }
    }
}
static void k_windowed(WindowArgs A) { stub_windowed(A); }
static void k_windowed_cp(WindowArgs A) { stub_windowed(A); }
static void k_windowed_sys(WindowArgs A) {
    for (int t = 0; t < A.T.ntasks; ++t) if (A.T.pair[t] >= 0 && A.o_abort) A.o_abort[t] = 0;
    stub_windowed(A);
}
static void k_windowed_quad(WindowArgs A) { if (A.state) memset(A.state, 0, (size_t)5 * A.T.ntasks * sizeof(int32_t)); }
// BandEd: a score per task, nothing flagged
static void stub_banded(const BandedArgs& A) {
    for (int t = 0; t < A.T.ntasks; ++t) {
        if (A.T.pair[t] < 0 || (A.only_if && A.only_if[t] == 0)) continue;
        A.o_score[t] = stub_env("QE_STUB_BOUND", 70) / 2; A.o_first[t] = 0; A.o_last[t] = 0; A.o_posv[t] = 0; A.o_adv[t] = 1; A.o_maxrow[t] = 1 << 20;
    }
}
constexpr bool QE_K_BANDED_LDS = false;      // the workspace form only: score_lds_slots declines (tests/test_host_narrow*.py rely on it)
template <bool FILL, bool LDS = false> static void k_banded(BandedArgs A) { stub_banded(A); }
static void k_banded_wave(BandedArgs A) { stub_banded(A); }
template <int LG, bool FILL> static void k_banded_sys(BandedArgs A) {
    for (int t = 0; t < A.T.ntasks; ++t) if (A.T.pair[t] >= 0 && A.o_abort) A.o_abort[t] = 0;
    stub_banded(A);
}
template <bool FILL> static void k_banded_sys2(BandedArgs A) {
    for (int t = 0; t < A.T.ntasks; ++t) if (A.T.pair[t] >= 0 && A.o_abort && !(A.only_if && A.only_if[t] == 0)) A.o_abort[t] = 0;
    stub_banded(A);
}
static void k_banded_coop(CoopArgs A) {
    for (int t = 0; t < A.T.ntasks; ++t) {
        if (A.T.pair[t] < 0) continue;
        A.o_score[t] = stub_env("QE_STUB_BOUND", 70) / 2; A.o_first[t] = 0; A.o_last[t] = 0; A.o_posv[t] = 0; A.o_adv[t] = 1; A.o_maxrow[t] = 1 << 20;
    }
}
template <bool FILL> static void k_banded_coop_lds(CoopLdsArgs X) { k_banded_coop(X.A); }
static void stub_trace(const TraceArgs& A) {
    for (int t = 0; t < A.T.ntasks; ++t) {
        if (A.T.pair[t] < 0 || (A.only_if && A.only_if[t] == 0)) continue;
        A.o_nruns[t] = 0; A.o_nops[t] = 0; A.o_edits[t] = 0; A.o_steps[t] = 1;
    }
}
static void k_traceback(TraceArgs A) { stub_trace(A); }
template <int LG> static void k_traceback_sys(TraceArgs A) {
    for (int t = 0; t < A.T.ntasks; ++t) if (A.T.pair[t] >= 0 && A.o_abort) A.o_abort[t] = 0;
    stub_trace(A);
}
static void k_join(JoinArgs A) { for (int j = 0; j < A.nnodes; ++j) { A.o_best[j] = A.m[j] / 2; A.o_score_l[j] = 1; A.o_score_r[j] = 1; A.o_ok[j] = 1; } }
// CIGAR strings: one "1M" per entry, so that string pools, offsets and the D2H of the strings are exercised
template <bool WRITE> static void k_format_segs(SegFormatArgs A) {
    for (int i = 0; i < A.npairs; ++i) {
        if (!WRITE) { A.o_len[i] = 2; A.o_edits[i] = 0; A.o_nops[i] = 1; }
        else if (A.pool && A.str_off) { char* s = A.pool + A.str_off[i]; s[0] = '1'; s[1] = 'M'; s[2] = 0; }
    }
}
template <bool WRITE> static void k_format_segs_wave(SegFormatArgs A) { k_format_segs<WRITE>(A); }
// The validator: the walk of qe_check.h, the kernels' own source, one alignment after the other -- real verdicts (of the
// stand-in alignments above: no runs, so 0 for every pair that has bases)
struct StubRuns {                  // a leaf's runs in either layout (run_view, qe_kernels.hip)
    const SegFormatArgs& A; const u32* base = nullptr; int64_t stride = 1;
    void open(int t) {
        const int g = t >> 6, lane = t & 63;
        if (A.runs_by_task) { base = A.runs + A.g_runs_off[g] + (int64_t)lane * A.g_runs_cap[g]; stride = 1; }
        else { base = A.runs + A.g_runs_off[g] + lane; stride = 64; }
    }
    u32 at(int k) const { return base[(int64_t)k * stride]; }
};
static AlignCheck stub_check_of_pair(const PairView& P, int pair) {
    AlignCheck K;
    K.ap = P.asc_p + P.asc_p_off[pair]; K.at = P.asc_t + P.asc_t_off[pair];
    K.m = P.p_len[pair]; K.n = P.t_len[pair];
    return K;
}
static void k_check_segs(SegCheckArgs C) {
    const SegFormatArgs& A = C.F;
    for (int i = 0; i < A.npairs; ++i) {
        AlignCheck K = stub_check_of_pair(C.P, C.root_pair[i]);
        StubRuns R{A};
        check_walk_segments(K, A.seg_off, A.seg_kind, A.seg_a, A.seg_b, A.nruns, i, R);
        C.o_ok[i] = K.verdict();
    }
}
static void k_check_strings(PairView P, int npairs, const char* pool, const int64_t* off, int32_t* o_ok) {
    for (int i = 0; i < npairs; ++i) {
        if (off[i] < 0) { o_ok[i] = -1; continue; }
        AlignCheck K = stub_check_of_pair(P, i);
        check_walk_string(K, pool + off[i]);
        o_ok[i] = K.verdict();
    }
}
static void k_pack(PackArgs A) { if (A.flags) for (int i = 0; i < A.nseq; ++i) A.flags[i] |= 0u; }
static void k_unpack_wire(WireArgs) {}
static void k_reverse_planes(RevArgs) {}

// k_narrow: the same phases on the host
static void k_narrow(NarrowArgs A) {
    const int nt = A.T.ntasks;
    if (A.phase == 0) {
        for (int q = 0; q < QE_NARROW_STAT; ++q) A.stat[q] = 0;
        for (int g = 0; g < nt; g += 64) {
            int sg = 0;
            if (A.q > 0)
                for (int t = g; t < std::min(nt, g + 64); ++t)
                    if (A.T.pair[t] >= 0) sg = std::max(sg, narrow_fit_slots(A.T.m[t], A.T.n[t], A.T.cutoff[t], narrow_rhat(A.q, A.T.cutoff[t])));
            for (int t = g; t < std::min(nt, g + 64); ++t) {
                A.q_pair[t] = -1;
                A.cut1[t] = (A.T.pair[t] >= 0) ? narrow_fit_lane(A.T.m[t], A.T.n[t], A.T.cutoff[t], A.q, sg) : A.T.cutoff[t];
                if (A.prune1) A.prune1[t] = (A.T.pair[t] >= 0) ? narrow_prune(A.T.m[t], A.T.n[t], A.T.cutoff[t], A.cut1[t], A.qp) : A.cut1[t];
            }
        }
    } else if (A.phase == 1) {
        for (int t = 0; t < nt; ++t) {
            if (A.T.pair[t] < 0 || A.cut1[t] == A.T.cutoff[t]) continue;
            A.stat[1] += A.adv[t]; ++A.stat[3];
            if (narrow_accepts_pruned(A.T.m[t], A.T.n[t], A.cut1[t], A.T.cutoff[t], A.prune1 ? A.prune1[t] : A.cut1[t], A.score[t])) {
                A.stat[4] = std::max(A.stat[4], (unsigned long long)std::max(0, narrow_ratio(A.T.m[t], A.T.n[t], A.T.cutoff[t], A.score[t])));
                continue;
            }
            const int j = (int)A.stat[0]++;
            A.q_pair[j] = A.T.pair[t]; A.q_p0[j] = A.T.p0[t]; A.q_m[j] = A.T.m[t]; A.q_t0[j] = A.T.t0[t]; A.q_n[j] = A.T.n[t];
            A.q_cutoff[j] = A.T.cutoff[t]; A.q_tfin[j] = A.T.tfin[t]; A.q_src[j] = t;
        }
    } else if (A.phase == 2) {
        for (int j = 0; j < (int)A.stat[0]; ++j) {
            A.score[A.q_src[j]] = A.q_score[j]; A.adv[A.q_src[j]] += A.q_adv[j]; A.stat[2] += A.q_adv[j];
            const int ratio = narrow_ratio(A.q_m[j], A.q_n[j], A.q_cutoff[j], A.q_score[j]);
            if (ratio >= 0) { ++A.stat[5]; A.stat[4] = std::max(A.stat[4], (unsigned long long)ratio); }
        }
    } else {
        for (int t = 0; t < nt; ++t) {
            if (A.T.pair[t] < 0) continue;
            const int src = (((t >> 6) * A.stride) << 6) + (t & 63);
            A.stat[1] += A.q_adv[t]; ++A.stat[3];
            if (!narrow_accepts(A.T.m[t], A.T.n[t], A.T.cutoff[t], A.main_cutoff[src], A.q_score[t])) { ++A.stat[0]; A.stat[2] += A.adv[src]; }
            A.adv[src] += A.q_adv[t];
        }
    }
}
// Bounded runs: the same source (qe_bounded.h) on the host
static void k_bounded_diag(BoundedArgs A) {
    for (int t = 0; t < A.T.ntasks; ++t) {
        const int pr = A.T.pair[t];
        if (pr < 0) continue;
        A.o_score[t] = bounded_diag_pair(A.P.pl_p + A.P.pl_p_off[pr], A.T.m[t], A.P.pl_t + A.P.pl_t_off[pr], A.T.n[t], A.T.cutoff[t]);
        A.o_adv[t] = (u32)A.T.n[t];
    }
}
static void k_bounded_threshold(int nt, const int32_t* score, const u32* adv, const int32_t* bound, int32_t* o_score, u32* o_adv) {
    for (int t = 0; t < nt; ++t) { o_score[t] = bounded_answer(score[t], bound[t]); o_adv[t] = adv[t]; }
}
// Search runs: the same source (qe_search.h) on the host, task by task, in the layout and with the arguments of the device form
template <int NB, class Eq = SearchEq3>
static void k_search(SearchArgs A) {
    for (int t = 0; t < A.T.ntasks; ++t) {
        const int pair = A.T.pair[t];
        if (pair < 0) continue;
        const int g = t >> 6, lane = t & 63, m = A.T.m[t];
        int n = A.T.n[t], bound = A.T.cutoff[t], in_end = 0;
        int64_t tbit = 0;
        bool valid = true;
        if (A.in_score) {
            bound = A.in_score[t]; in_end = A.in_end[t];
            valid = bound >= 0 && in_end >= 1 && in_end <= n;
            tbit = n - in_end; n = in_end;
        }
        const int nbg = NB == 0 ? A.g_nb[g] : NB;
        valid = valid && search_blocks(m) <= nbg;
        SearchLane L;
        search_lane_init(L, m, valid ? n : 0, A.mode, valid ? bound : 0, A.flags);
        const u64* pp = A.P.pl_p + Eq::offset(A.P.pl_p_off[pair]);
        const u64* tp = A.P.pl_t + Eq::offset(A.P.pl_t_off[pair]);
        if (valid) {
            if constexpr (NB > 0) {
                SearchRegStore<(NB > 0 ? NB : 1), Eq> R;
                R.clear();
                R.load(pp, m);
                search_run<NB>(R, L, tp, tbit);
            } else {
                u64* base = (u64*)(A.ws + A.g_ws_off[g]);
                SearchWsStoreOf<Eq> W{base + lane, base + (int64_t)nbg * 64 + lane, (int32_t*)(base + (int64_t)2 * nbg * 64) + lane, 64, pp, m};
                search_run<0>(W, L, tp, tbit);
            }
        }
        int32_t score, end;
        search_answer(L, score, end);
        if (!valid) { score = -1; end = -1; }
        if (A.in_score) {
            if (valid) A.o_start[t] = (score == bound) ? in_end - end : -1;
        } else {
            A.o_score[t] = score; A.o_end[t] = end;
            A.o_start[t] = (score >= 0 && A.mode == SEARCH_PREFIX) ? 0 : -1;
        }
        A.o_adv[t] += L.steps;
    }
}
// ... and of the all-occurrences kernels (SearchHitsArgs, HitExpandArgs)
template <int NB, class Eq = SearchEq3>
static void k_search_hits(SearchHitsArgs X) {
    const SearchArgs& A = X.S;
    for (int t = 0; t < A.T.ntasks; ++t) {
        const int pair = A.T.pair[t];
        if (pair < 0) continue;
        const int g = t >> 6, lane = t & 63, m = A.T.m[t], n = A.T.n[t], bound = A.T.cutoff[t];
        const int nbg = NB == 0 ? A.g_nb[g] : NB;
        if (bound < 0 || search_blocks(m) > nbg) continue;
        SearchLane L;
        search_lane_init(L, m, n, A.mode, bound, 0);
        SearchHitScan H;
        H.init(L, reinterpret_cast<SearchHit*>(X.raw) + (int64_t)t * X.max_hits, 1, X.max_hits);
        const u64* pp = A.P.pl_p + Eq::offset(A.P.pl_p_off[pair]);
        const u64* tp = A.P.pl_t + Eq::offset(A.P.pl_t_off[pair]);
        if constexpr (NB > 0) {
            SearchRegStore<(NB > 0 ? NB : 1), Eq> R;
            R.clear();
            R.load(pp, m);
            search_run_hits<NB>(R, L, H, tp, 0);
        } else {
            u64* base = (u64*)(A.ws + A.g_ws_off[g]);
            SearchWsStoreOf<Eq> W{base + lane, base + (int64_t)nbg * 64 + lane, (int32_t*)(base + (int64_t)2 * nbg * 64) + lane, 64, pp, m};
            search_run_hits<0>(W, L, H, tp, 0);
        }
        X.o_found[pair] = H.found; X.o_best[pair] = H.best; X.o_len[pair] = H.sink.count - 1;
        A.o_adv[t] += L.steps;
    }
}
static void k_hits_expand(HitExpandArgs A) {
    for (int t = 0; t < A.T.ntasks; ++t) {
        const int pair = A.T.pair[t];
        if (pair < 0) continue;
        const int stored = std::min(A.len[pair] + 1, A.max_hits), m = A.T.m[t], n = A.T.n[t];
        const int32_t* raw = A.raw + 2 * (int64_t)t * A.max_hits;
        for (int i = 0; i < stored; ++i) {
            const int64_t j = A.off[pair] + i;
            const int32_t end = raw[2 * i], score = raw[2 * i + 1];
            int32_t task_n, in_end, base;
            search_hit_task(m, n, end, score, task_n, in_end, base);
            A.hits[3 * j] = A.infix ? base : 0; A.hits[3 * j + 1] = end; A.hits[3 * j + 2] = score;
            if (A.infix) { A.o_pair[j] = pair; A.o_m[j] = m; A.o_n[j] = task_n; A.o_score[j] = score; A.o_end[j] = in_end; }
        }
    }
}
static void k_hits_finish(int64_t total, const int32_t* o_start, int32_t* hits) {
    for (int64_t j = 0; j < total; ++j) hits[3 * j] = o_start[j] < 0 ? -1 : hits[3 * j] + o_start[j];
}
// ... and of the two producers of a flagged run's four planes: the scalar code of qe_iupac.h, so the host-only build of a
// flagged run gives true answers (of an ASCII batch; a packed one derives them from the zeros k_unpack_wire's stand-in leaves)
static void k_pack_iupac(IupacPackArgs A) {
    for (int i = 0; i < A.nseq; ++i)
        iupac_pack(A.asc + A.asc_off[i], A.len[i], A.reverse != 0, A.acgt_only != 0, A.planes + iupac_offset(A.pl_off[i]));
}
static void k_planes_iupac(IupacPlanesArgs A) {
    for (int i = 0; i < A.nseq; ++i) iupac_from_planes3(A.src + A.pl_off[i], A.len[i], A.n_empty != 0, A.dst + iupac_offset(A.pl_off[i]));
}
// Panel runs: the per-slot functions of qe_panel.h, qe_panel_ham.h and qe_panel_align.h that the device kernels call, with the
// arguments of the device forms.  The seven per-text sweeps run through one loop over the kernels' own opener: f(S, T) for
// every slice S and every slot T that has a text, slice by slice
template <class Eq, class F>
static void stub_panel_sweep(const PanelSweepArgs& A, F f) {
    const int nslices = panel_slice(A, 0).nslices;
    for (int slice = 0; slice < nslices; ++slice) {
        const PanelSlice S = panel_slice(A, slice);
        for (int slot = 0; slot < A.nslots; ++slot) {
            const PanelLane T = panel_lane<Eq>(A, slot);
            if (T.pair >= 0) f(S, T);
        }
    }
}
// the best member per text (PanelArgs), by edits (k_search_panel) and by mismatches only (k_panel_ham: TEXT = panel_ham_text)
template <class Eq, class Text>
static void stub_panel_best(const PanelArgs& A, Text text) {
    stub_panel_sweep<Eq>(A, [&](const PanelSlice& S, const PanelLane& T) {
        PanelKeeper keep;
        keep.init();
        u32 steps = 0;
        text(S.P, S.p0, S.p1, T.tp, T.n, A.mode, keep, steps, A.m_score ? A.m_score + (int64_t)T.pair * A.n_members : nullptr,
             A.m_score ? A.m_end + (int64_t)T.pair * A.n_members : nullptr);
        panel_store_part(A, S.nslices, S.slice, T.slot, keep, steps);
    });
}
template <class Eq> static void k_search_panel(PanelArgs A) { stub_panel_best<Eq>(A, [](auto&&... a) { panel_text<Eq>(a...); }); }
template <class Eq> static void k_panel_ham(PanelArgs A) { stub_panel_best<Eq>(A, [](auto&&... a) { panel_ham_text<Eq>(a...); }); }
static void k_panel_wire_codes(u64* planes, int64_t rows) { for (int64_t r = 0; r < rows; ++r) planes[3 * r] ^= planes[3 * r + 1]; }
static void k_panel_reduce(PanelReduceArgs A) { for (int t = 0; t < A.nslots; ++t) panel_reduce_slot(A, t); }
static void k_panel_finish(int nslots, const int32_t* text, const int32_t* o_pair, const int32_t* o_start, int32_t* hits) {
    for (int t = 0; t < nslots; ++t) panel_finish_slot(t, text, o_pair, o_start, hits);
}
static void k_panel_ham_finish(int64_t npairs, const int32_t* m_len, int32_t* hits) { for (int64_t i = 0; i < npairs; ++i) panel_ham_finish_pair(i, m_len, hits); }
// ... of the all-occurrences panel kernels (PanelHitsArgs, PanelHitsCountArgs, PanelHitsExpandArgs), the mismatch-only one and
// the 3' tails among them
template <class Eq>
static void k_panel_hits(PanelHitsArgs A) {
    stub_panel_sweep<Eq>(A, [&](const PanelSlice& S, const PanelLane& T) {
        PanelHitScan H;
        panel_hit_scan_init(H, panel_lane_raw(A, S, T), A.max_hits);
        u32 steps = 0;
        panel_text_hits<Eq>(S.P, S.p0, S.p1, T.tp, T.n, A.mode, H, steps);
        panel_hits_store_part(A, S.nslices, S.slice, T.slot, H, steps);
    });
}
template <class Eq>
static void k_panel_ham_hits(PanelHitsArgs A) {
    stub_panel_sweep<Eq>(A, [&](const PanelSlice& S, const PanelLane& T) {
        PanelHamScan H;
        panel_hit_scan_init(H, panel_lane_raw(A, S, T), A.max_hits);
        u32 steps = 0;
        panel_ham_text_hits<Eq>(S.P, S.p0, S.p1, T.tp, T.n, A.mode, H, steps);
        panel_hits_store_part(A, S.nslices, S.slice, T.slot, H, steps);
    });
}
template <class Eq>
static void k_panel_tails(PanelTailsArgs X) {
    const PanelHitsArgs& A = X.H;
    stub_panel_sweep<Eq>(A, [&](const PanelSlice& S, const PanelLane& T) {
        PanelHitScan H;
        panel_hit_scan_init(H, panel_lane_raw(A, S, T), A.max_hits);
        PanelTailKeeper keep;
        keep.init();
        u32 steps = 0, rows = 0;
        panel_text_tails<Eq>(S.P, S.p0, S.p1, T.tp, T.n, A.mode, X.min_overlap, H, keep, steps, rows);
        panel_hits_store_part(A, S.nslices, S.slice, T.slot, H, steps);
        panel_tails_store_part(X, S.nslices, S.slice, T.slot, keep, rows);
    });
}
static void k_panel_hits_count(PanelHitsCountArgs A) { for (int t = 0; t < A.nslots; ++t) panel_hits_count_slot(A, t); }
static void k_panel_hits_expand(PanelHitsExpandArgs A) { for (int t = 0; t < A.nslots; ++t) panel_hits_expand_slot(A, t); }
static void k_panel_hits_finish(int64_t total, const int32_t* o_start, int32_t* hits) { for (int64_t j = 0; j < total; ++j) panel_hits_finish_one(j, o_start, hits); }
static void k_panel_ham_hits_finish(int64_t total, const int32_t* m_len, int32_t* hits) { for (int64_t j = 0; j < total; ++j) panel_ham_hits_finish_one(j, m_len, hits); }
// ... of the queued run's three steps behind the offset scan (quicked_batch_configure_panel_queue)
static void k_panel_queue_expand(PanelHitsExpandArgs A, int64_t cap) { for (int t = 0; t < A.nslots; ++t) panel_queue_expand_slot(A, t, cap); }
static void k_panel_queue_finish(const int64_t* total, int64_t cap, const int32_t* o_start, int32_t* hits) {
    for (int64_t j = 0; j < cap; ++j) panel_queue_finish_one(j, total, cap, o_start, hits);
}
static void k_panel_queue_clamp(int64_t n, int64_t cap, int64_t* off, int64_t* q) {
    for (int64_t i = 0; i <= n; ++i) panel_queue_clamp_one(i, n, cap, off, q);
}
// ... of the steps behind k_panel_tails (QUICKED_PANEL_TAILS), and of the 5' heads (QUICKED_PANEL_HEADS)
static void k_panel_tails_merge(PanelTailsMergeArgs A) { for (int t = 0; t < A.nslots; ++t) panel_tails_merge_slot(A, t); }
template <class Eq>
static void k_panel_tail_planes(PanelTailPlanesArgs A) { for (int t = 0; t < A.nslots; ++t) panel_tail_planes_slot<Eq>(A, t); }
static void k_panel_tails_finish(int nslots, const int32_t* o_pair, const int32_t* o_start, int32_t* tails) {
    for (int t = 0; t < nslots; ++t) panel_tails_finish_slot(t, o_pair, o_start, tails);
}
template <class Eq>
static void k_panel_heads(PanelHeadsArgs A) {
    stub_panel_sweep<Eq>(A, [&](const PanelSlice& S, const PanelLane& T) {
        PanelTailKeeper keep;
        keep.init();
        u32 steps = 0, rows = 0;
        panel_text_heads<Eq>(S.P, S.p0, S.p1, T.tp, T.n, A.min_overlap, keep, steps, rows);
        panel_heads_store_part(A, S.nslices, S.slice, T.slot, keep, rows, steps);
    });
}
static void k_panel_heads_merge(PanelHeadsMergeArgs A) { for (int t = 0; t < A.nslots; ++t) panel_heads_merge_slot(A, t); }
template <class Eq>
static void k_panel_head_planes(PanelHeadPlanesArgs A) { for (int t = 0; t < A.nslots; ++t) panel_head_planes_slot<Eq>(A, t); }
static void k_panel_heads_finish(int nslots, const int32_t* o_pair, const int32_t* o_start, int32_t* heads) {
    for (int t = 0; t < nslots; ++t) panel_heads_finish_slot(t, o_pair, o_start, heads);
}
// ... of the windowed run (quicked_batch_run_panel_scan): window slots for text slots
template <class Eq>
static void k_panel_scan(PanelScanArgs A) {
    stub_panel_sweep<Eq>(A, [&](const PanelSlice& S, const PanelLane& T) {
        const int c0 = A.w_c0[T.slot], c1 = A.w_c1[T.slot];
        PanelWindowScan H;
        panel_window_scan_init(H, panel_lane_raw(A, S, T), A.max_hits, c0, c1);
        u32 steps = 0;
        panel_window_hits<Eq>(S.P, S.p0, S.p1, T.tp, T.n, c0, c1, H, steps);
        panel_scan_store_part(A, S.nslices, S.slice, T.slot, H, steps);
    });
}
static void k_panel_scan_sums(PanelScanCountArgs A) { for (int s = 0; s < A.nslices; ++s) for (int t = 0; t < A.ntext; ++t) panel_scan_sums_slice(A, s, t); }
static void k_panel_scan_count(PanelScanCountArgs A) { for (int t = 0; t < A.ntext; ++t) panel_scan_count_text(A, t); }
static void k_panel_scan_expand(PanelScanExpandArgs A) {
    for (int s = 0; s < A.nslices; ++s) for (int w = 0; w < A.nslots; ++w) panel_scan_expand_lane(A, s, w);
}
// ... and of the occurrence aligner (QUICKED_PANEL_CIGARS; qe_panel_align.h), occurrence by occurrence
template <class Eq>
static void k_panel_occ_align(PanelAlignArgs A) { for (int64_t k = 0; k < A.count; ++k) panel_align_occ<Eq>(A, k); }
static void k_panel_align_sizes(int64_t total, const int32_t* hits, int32_t* len) { for (int64_t j = 0; j < total; ++j) panel_align_size_one(j, hits, len); }
// The tag kernels: the walker of qe_tags.h on the host, both forms
template <bool WRITE> static void k_tags_segs(SegTagArgs T) {
    const SegFormatArgs& A = T.F;
    for (int i = 0; i < A.npairs; ++i) {
        const int pair = T.root_pair[i];
        const int m = T.P.p_len[pair];
        TagWalker<WRITE> W;
        W.want_md = T.want_md != 0;
        if (WRITE) {
            char* out = T.md_pool + T.md_off[i];
            if (T.o_md_len[i] <= 0) { out[0] = '\0'; continue; }
            W.sink = TagSink{out, T.o_md_len[i], T.P.asc_p + T.P.asc_p_off[pair], m};
        }
        StubRuns R{A};
        const bool ok = tag_walk_segments(W, A.seg_off, A.seg_kind, A.seg_a, A.seg_b, A.nruns, i, R);
        const int64_t md_len = W.finish();
        if (!WRITE) tag_store_counts(T.want_stats ? T.o_stats + i : nullptr, T.want_md ? T.o_md_len + i : nullptr, T.o_md_bad, !ok, W.s, md_len, m);
    }
}
template <bool WRITE> static void k_tags_segs_wave(SegTagArgs T) { k_tags_segs<WRITE>(T); }

}  // namespace qe
