// Host stand-ins for the kernels of the queued all-occurrences panel run (quicked_batch_configure_panel_queue;
// k_panel_queue_expand, k_panel_queue_finish and k_panel_queue_clamp of quicked_amd/csrc/qe_kernels.hip), beside
// qe_kernels_stub_heads.h and in its style: the per-slot functions of qe_panel.h that the device kernels call, run slot by slot
// with the arguments of the device forms.  The host-only translation unit picks this header up right after its kernels header
// where the tree has it.
// TEST INFRASTRUCTURE.
#pragma once
#include "qe_types.h"
#include "qe_panel.h"

namespace qe {

static void k_panel_queue_expand(PanelHitsExpandArgs A, int64_t cap) { for (int t = 0; t < A.nslots; ++t) panel_queue_expand_slot(A, t, cap); }
static void k_panel_queue_finish(const int64_t* total, int64_t cap, const int32_t* o_start, int32_t* hits) {
    for (int64_t j = 0; j < cap; ++j) panel_queue_finish_one(j, total, cap, o_start, hits);
}
static void k_panel_queue_clamp(int64_t n, int64_t cap, int64_t* off, int64_t* q) {
    for (int64_t i = 0; i <= n; ++i) panel_queue_clamp_one(i, n, cap, off, q);
}

}  // namespace qe
