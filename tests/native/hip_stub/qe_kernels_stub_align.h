// Host stand-ins for the occurrence aligner's kernels (QUICKED_PANEL_CIGARS; k_panel_occ_align and k_panel_align_sizes of
// quicked_amd/csrc/qe_kernels.hip), beside qe_kernels_stub.h and in its style: the per-lane functions of qe_panel_align.h that
// the device kernels call, run occurrence by occurrence with the arguments of the device forms.  The host-only translation unit
// picks this header up right after its kernels header where the tree has it.  TEST INFRASTRUCTURE.
#pragma once
#include "qe_types.h"
#include "qe_panel_align.h"

namespace qe {

template <class Eq>
static void k_panel_occ_align(PanelAlignArgs A) { for (int64_t k = 0; k < A.count; ++k) panel_align_occ<Eq>(A, k); }
static void k_panel_align_sizes(int64_t total, const int32_t* hits, int32_t* len) { for (int64_t j = 0; j < total; ++j) panel_align_size_one(j, hits, len); }

}  // namespace qe
