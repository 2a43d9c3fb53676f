// Host stand-ins for the kernels of the mismatch-only panel runs (QUICKED_PANEL_NO_INDELS; k_panel_ham, k_panel_ham_hits,
// k_panel_ham_finish and k_panel_ham_hits_finish of quicked_amd/csrc/qe_kernels.hip), beside qe_kernels_stub_heads.h and in its
// style: the per-lane and per-record functions of qe_panel_ham.h that the device kernels call, run slot by slot and slice by
// slice with the arguments of the device forms.  The host-only translation unit picks this header up right after its kernels
// header where the tree has it.
// TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>

#include "qe_types.h"
#include "qe_panel_ham.h"

namespace qe {

template <class Eq>
static void k_panel_ham(PanelArgs A) {
    const int nslices = (A.n_members + A.per_slice - 1) / A.per_slice;
    PanelView P;
    P.pl = A.pl_m; P.off = A.m_off; P.len = A.m_len; P.bound = A.m_bound;
    for (int slice = 0; slice < nslices; ++slice)
        for (int slot = 0; slot < A.nslots; ++slot) {
            const int pair = A.text[slot];
            if (pair < 0) continue;
            const int p0 = slice * A.per_slice, p1 = std::min(A.n_members, p0 + A.per_slice);
            PanelKeeper keep;
            keep.init();
            u32 steps = 0;
            panel_ham_text<Eq>(P, p0, p1, A.pl_t + Eq::offset(A.pl_t_off[pair]), A.t_len[pair], A.mode, keep, steps,
                               A.m_score ? A.m_score + (int64_t)pair * A.n_members : nullptr, A.m_score ? A.m_end + (int64_t)pair * A.n_members : nullptr);
            panel_store_part(A, nslices, slice, slot, keep, steps);
        }
}
template <class Eq>
static void k_panel_ham_hits(PanelHitsArgs A) {
    const int nslices = (A.n_members + A.per_slice - 1) / A.per_slice;
    PanelView P;
    P.pl = A.pl_m; P.off = A.m_off; P.len = A.m_len; P.bound = A.m_bound;
    for (int slice = 0; slice < nslices; ++slice)
        for (int slot = 0; slot < A.nslots; ++slot) {
            const int pair = A.text[slot];
            if (pair < 0) continue;
            const int p0 = slice * A.per_slice, p1 = std::min(A.n_members, p0 + A.per_slice);
            PanelHamScan H;
            panel_hit_scan_init(H, A.raw + ((int64_t)slice * A.nslots + slot) * A.max_hits, A.max_hits);
            u32 steps = 0;
            panel_ham_text_hits<Eq>(P, p0, p1, A.pl_t + Eq::offset(A.pl_t_off[pair]), A.t_len[pair], A.mode, H, steps);
            panel_hits_store_part(A, nslices, slice, slot, H, steps);
        }
}
static void k_panel_ham_finish(int64_t npairs, const int32_t* m_len, int32_t* hits) { for (int64_t i = 0; i < npairs; ++i) panel_ham_finish_pair(i, m_len, hits); }
static void k_panel_ham_hits_finish(int64_t total, const int32_t* m_len, int32_t* hits) { for (int64_t j = 0; j < total; ++j) panel_ham_hits_finish_one(j, m_len, hits); }

}  // namespace qe
