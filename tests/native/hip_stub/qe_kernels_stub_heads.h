// Host stand-ins for the kernels of the 5' heads (QUICKED_PANEL_HEADS; k_panel_heads, k_panel_heads_merge, k_panel_head_planes
// and k_panel_heads_finish of quicked_amd/csrc/qe_kernels.hip), beside qe_kernels_stub_tails.h and in its style: the per-lane and
// per-slot functions of qe_panel.h that the device kernels call, run slot by slot and slice by slice with the arguments of the
// device forms.  The host-only translation unit picks this header up right after its kernels header where the tree has it.
// TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>

#include "qe_types.h"
#include "qe_panel.h"

namespace qe {

template <class Eq>
static void k_panel_heads(PanelHeadsArgs A) {
    const int nslices = (A.n_members + A.per_slice - 1) / A.per_slice;
    PanelView P;
    P.pl = A.pl_m_rev; P.off = A.m_off; P.len = A.m_len; P.bound = A.m_bound;
    for (int slice = 0; slice < nslices; ++slice)
        for (int slot = 0; slot < A.nslots; ++slot) {
            const int pair = A.text[slot];
            if (pair < 0) continue;
            const int p0 = slice * A.per_slice, p1 = std::min(A.n_members, p0 + A.per_slice);
            PanelTailKeeper keep;
            keep.init();
            u32 steps = 0, rows = 0;
            panel_text_heads<Eq>(P, p0, p1, A.pl_t + Eq::offset(A.pl_t_off[pair]), A.t_len[pair], A.min_overlap, keep, steps, rows);
            panel_heads_store_part(A, nslices, slice, slot, keep, rows, steps);
        }
}
static void k_panel_heads_merge(PanelHeadsMergeArgs A) { for (int t = 0; t < A.nslots; ++t) panel_heads_merge_slot(A, t); }
template <class Eq>
static void k_panel_head_planes(PanelHeadPlanesArgs A) { for (int t = 0; t < A.nslots; ++t) panel_head_planes_slot<Eq>(A, t); }
static void k_panel_heads_finish(int nslots, const int32_t* o_pair, const int32_t* o_start, int32_t* heads) {
    for (int t = 0; t < nslots; ++t) panel_heads_finish_slot(t, o_pair, o_start, heads);
}

}  // namespace qe
