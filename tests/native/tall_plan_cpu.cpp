// Tall passes of k_banded<false, true> (qe_types.h: tall_height, pass_plan), without a GPU: the walk of
// tests/native/banded_walk.h through the slice of the LDS form (ring), run twice over every group of 64 tasks -- with the
// 4 / 2 / 1 plan alone, and with the kernel's tall plan in front of it.  A task whose band the slice cannot hold sits both
// walks out.  Checked per task: score, first / last / pos_v, max_row_init and block advances of the two walks are equal.
// Checked per access of both walks: the model's bad_slot, bad_row and stale stay 0.  Counted: the passes of every height, the
// chunks a tall pass walked alone, the splits (a tall pass at the head of a taller walk), and the chunks of five or more
// slots that fell back to the old plan.
//   tall_plan_cpu <file> <lane_rel 0|1> <masked 0|1>
// file: int32 count, then per pair int32 m, n, c1, p, C and the m + n bytes of pattern and text (narrow_prune_lib.write_launch).
// Prints one line per pair ("pair <index> score <..> adv <block-columns> eligible <0|1>"), then the counts.
// Exit code 1: a difference, an access outside its window, or a stale row.
#include "banded_walk.h"

int main(int argc, char** argv) {
    std::vector<Lane> all;
    WalkOpts old_plan = {true, false, 0, 0};
    if (const int rc = read_args(argc, argv, "tall_plan_cpu", 5, all, old_plan)) return rc;
    WalkOpts tall_plan = old_plan;
    tall_plan.tall = true;

    Stats st, st_tall;
    long diffs = 0, rule_diffs = 0, eligible = 0, rejected = 0, bad_slot = 0, bad_row = 0, stale = 0, accesses = 0;
    for (size_t g0 = 0; g0 < all.size(); g0 += 64) {
        const size_t g1 = g0 + 64 < all.size() ? g0 + 64 : all.size();
        std::vector<Lane> tall_copy(all.begin() + (long)g0, all.begin() + (long)g1);
        Lane idle_a, idle_b;
        Lane *A[64], *B[64];
        group_at(all, g0, idle_a, A);
        group_at(tall_copy, 0, idle_b, B);
        walk_group(A, old_plan, st, rule_diffs);
        walk_group(B, tall_plan, st_tall, rule_diffs);
        for (size_t l = 0; l < g1 - g0; ++l) {
            Lane &L = *A[l], &R = *B[l];
            int64_t score = -1;
            if (L.valid) {
                ++eligible;
                score = read_out(L);
                const int64_t rs = read_out(R);
                if (!R.valid || rs != score || R.adv != L.adv || R.first != L.first || R.last != L.last || R.pos_v != L.pos_v || R.max_row_init != L.max_row_init) {
                    if (diffs < 10) fprintf(stderr, "pair %zu: the tall walk has %lld adv %lld first %d last %d, the old plan %lld adv %lld first %d last %d (m %d n %d c1 %d p %d)\n", g0 + l,
                                            (long long)rs, (long long)R.adv, R.first, R.last, (long long)score, (long long)L.adv, L.first, L.last, L.m, L.n, L.cutoff, L.prune);
                    ++diffs;
                }
                bad_slot += R.bad_slot + L.bad_slot; bad_row += R.bad_row + L.bad_row; stale += R.stale + L.stale; accesses += R.accesses;
                pat_free(&R.pat);
                pat_free(&L.pat);
            } else ++rejected;
            printf("pair %zu score %lld adv %lld eligible %d\n", g0 + l, (long long)score, (long long)L.adv, L.valid ? 1 : 0);
            L.valid = false;
        }
    }
    printf("pairs %zu lane_rel %d masked %d diffs %ld rule_diffs %ld eligible %ld rejected %ld bad_slot %ld bad_row %ld stale %ld accesses %ld chunks %ld "
           "old4 %ld old2 %ld old1 %ld passes4 %ld passes2 %ld passes1 %ld tall5 %ld tall6 %ld tall7 %ld tall8 %ld tall9 %ld tall10 %ld whole %ld splits %ld "
           "fallbacks %ld dead_lanes %ld live %ld lane_chunks %ld\n",
           all.size(), old_plan.lane_rel, old_plan.masked, diffs, rule_diffs, eligible, rejected, bad_slot, bad_row, stale, accesses, st_tall.chunks,
           st.p4, st.p2, st.p1, st_tall.p4, st_tall.p2, st_tall.p1, st_tall.tall[5], st_tall.tall[6], st_tall.tall[7], st_tall.tall[8], st_tall.tall[9],
           st_tall.tall[10], st_tall.whole, st_tall.splits, st_tall.fallbacks, st_tall.dead, st_tall.live, st_tall.lane_chunks);
    return (diffs || rule_diffs || bad_slot || bad_row || stale || st.chunks != st_tall.chunks) ? 1 : 0;
}
