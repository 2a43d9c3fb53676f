// qe_kernels_stub_noindels_scan.h -- the host stand-ins of the windowed mismatch-only panel run's two kernels
// (quicked_batch_run_panel_scan_no_indels), beside qe_kernels_stub.h, which holds every other one and is
// included first.  The kernels' own source (qe_panel_ham.h, qe_panel.h) run slot by slot through stub_panel_sweep.
#pragma once

namespace qe {

template <class Eq>
static void k_panel_ham_scan(PanelScanArgs A) {
    stub_panel_sweep<Eq>(A, [&](const PanelSlice& S, const PanelLane& T) {
        const int c0 = A.w_c0[T.slot], c1 = A.w_c1[T.slot];
        PanelHamWindowScan H;
        panel_ham_window_scan_init(H, panel_lane_raw(A, S, T), A.max_hits, c0, c1);
        u32 steps = 0;
        panel_ham_window_hits<Eq>(S.P, S.p0, S.p1, T.tp, T.n, c0, c1, H, steps);
        panel_scan_store_part(A, S.nslices, S.slice, T.slot, H, steps);
    });
}
static void k_panel_ham_scan_expand(PanelScanExpandArgs A) {
    for (int s = 0; s < A.nslices; ++s) for (int w = 0; w < A.nslots; ++w) panel_scan_expand_lane_of<false>(A, s, w);
}

}  // namespace qe
