// The ring and the slot budget of k_banded<false, true> (qe_types.h: score_lds_*), without a GPU: the walk of
// tests/native/banded_walk.h with the 4 / 2 / 1 plan, run twice over every group of 64 tasks -- through plain arrays and
// through the slice of the LDS form (ring).  A task is ELIGIBLE when score_lds_fits() takes its band's slot count; the others
// are left out of the second walk.  Checked per eligible task: score, first / last / pos_v, max_row_init and block advances
// of both walks are equal, and the read-out of the second finds row nw - 1.  Checked per access of the second walk: the
// model's bad_slot, bad_row and stale stay 0.
//   score_ring_cpu <file> <lane_rel 0|1> <masked 0|1>
// file: int32 count, then per pair int32 m, n, c1, p, C and the m + n bytes of pattern and text (narrow_prune_lib.write_launch).
// Prints one line per pair ("pair <index> score <plain walk's> adv <block-columns> eligible <0|1>"), then the counts.
// Exit code 1: a difference, an access outside its window, or a stale row.
#include "banded_walk.h"

int main(int argc, char** argv) {
    std::vector<Lane> all;
    WalkOpts plain = {false, false, 0, 0};
    if (const int rc = read_args(argc, argv, "score_ring_cpu", 5, all, plain)) return rc;
    WalkOpts ring = plain;
    ring.ring = true;

    Stats st, st_ring;
    long diffs = 0, rule_diffs = 0, eligible = 0, rejected = 0, bad_slot = 0, bad_row = 0, stale = 0, accesses = 0, max_rows = 0;
    for (size_t g0 = 0; g0 < all.size(); g0 += 64) {
        const size_t g1 = g0 + 64 < all.size() ? g0 + 64 : all.size();
        std::vector<Lane> ring_copy(all.begin() + (long)g0, all.begin() + (long)g1);
        Lane idle_a, idle_b;
        Lane *A[64], *B[64];
        group_at(all, g0, idle_a, A);
        group_at(ring_copy, 0, idle_b, B);
        walk_group(A, plain, st, rule_diffs);
        walk_group(B, ring, st_ring, rule_diffs);
        for (int l = 0; l < 64; ++l) {
            Lane &L = *A[l], &R = *B[l];
            if (!L.valid) continue;
            const int64_t score = read_out(L);
            if (R.valid) {
                ++eligible;
                const int64_t rs = read_out(R);
                if (rs != score || R.adv != L.adv || R.first != L.first || R.last != L.last || R.pos_v != L.pos_v || R.max_row_init != L.max_row_init) {
                    if (diffs < 10) fprintf(stderr, "pair %zu: the ring walk has %lld adv %lld, plain arrays %lld adv %lld (m %d n %d c1 %d p %d)\n", g0 + l,
                                            (long long)rs, (long long)R.adv, (long long)score, (long long)L.adv, L.m, L.n, L.cutoff, L.prune);
                    ++diffs;
                }
                bad_slot += R.bad_slot; bad_row += R.bad_row; stale += R.stale; accesses += R.accesses;
                if (R.max_row_init > max_rows) max_rows = R.max_row_init;
                pat_free(&R.pat);
            } else ++rejected;
            printf("pair %zu score %lld adv %lld eligible %d\n", g0 + l, (long long)score, (long long)L.adv, R.valid ? 1 : 0);
            pat_free(&L.pat);
            L.valid = false;
        }
    }
    printf("pairs %zu lane_rel %d masked %d diffs %ld rule_diffs %ld eligible %ld rejected %ld bad_slot %ld bad_row %ld stale %ld accesses %ld max_rows %ld chunks %ld ring_chunks %ld\n",
           all.size(), plain.lane_rel, plain.masked, diffs, rule_diffs, eligible, rejected, bad_slot, bad_row, stale, accesses, max_rows, st.chunks, st_ring.chunks);
    return (diffs || rule_diffs || bad_slot || bad_row || stale) ? 1 : 0;
}
