// Host stand-ins for the windowed panel search's kernels (quicked_batch_run_panel_scan; k_panel_scan, k_panel_scan_sums,
// k_panel_scan_count and k_panel_scan_expand of quicked_amd/csrc/qe_kernels.hip), beside qe_kernels_stub.h and in its style: the per-lane functions of
// qe_panel.h that the device kernels call, run slot by slot and slice by slice with the arguments of the device forms.  The
// host-only translation unit picks this header up right after its kernels header where the tree has it.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include "qe_types.h"
#include "qe_panel.h"

namespace qe {

template <class Eq>
static void k_panel_scan(PanelScanArgs A) {
    const int nslices = (A.n_members + A.per_slice - 1) / A.per_slice;
    PanelView P;
    P.pl = A.pl_m; P.off = A.m_off; P.len = A.m_len; P.bound = A.m_bound;
    for (int slice = 0; slice < nslices; ++slice)
        for (int slot = 0; slot < A.nslots; ++slot) {
            const int pair = A.w_pair[slot];
            if (pair < 0) continue;
            const int p0 = slice * A.per_slice, p1 = std::min(A.n_members, p0 + A.per_slice);
            PanelWindowScan H;
            panel_window_scan_init(H, A.raw + ((int64_t)slice * A.nslots + slot) * A.max_hits, A.max_hits, A.w_c0[slot], A.w_c1[slot]);
            u32 steps = 0;
            panel_window_hits<Eq>(P, p0, p1, A.pl_t + Eq::offset(A.pl_t_off[pair]), A.t_len[pair], A.w_c0[slot], A.w_c1[slot], H, steps);
            panel_scan_store_part(A, nslices, slice, slot, H, steps);
        }
}
static void k_panel_scan_sums(PanelScanCountArgs A) { for (int s = 0; s < A.nslices; ++s) for (int t = 0; t < A.ntext; ++t) panel_scan_sums_slice(A, s, t); }
static void k_panel_scan_count(PanelScanCountArgs A) { for (int t = 0; t < A.ntext; ++t) panel_scan_count_text(A, t); }
static void k_panel_scan_expand(PanelScanExpandArgs A) {
    for (int s = 0; s < A.nslices; ++s) for (int w = 0; w < A.nslots; ++w) panel_scan_expand_lane(A, s, w);
}

}  // namespace qe
