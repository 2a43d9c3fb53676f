// The walk of tests/native/banded_walk.h over plain arrays with the 4 / 2 / 1 plan and a pruning threshold per task.  Per
// pair the result goes through qe_types.h's narrow_accepts_pruned(m, n, c1, C, p, .) and is compared with the oracle's pass
// at the full cutoff C: an ACCEPTED result that differs is an error (exit code 1).  `lost` counts the pairs whose distance
// the threshold allows (the oracle's score at C passes the same rule) and whose walk did not return it.  A task whose
// threshold is not below its cutoff c1 must also advance the oracle's block-columns at c1.
//   narrow_prune_cpu <file> <lane_rel 0|1> <masked 0|1>
// file: int32 count, then per pair int32 m, n, c1, p, C and the m + n bytes of pattern and text.
// Prints one line per pair ("pair <index> score <walk's> adv <block-columns> accepted <0|1>"), then the counts and the
// passes per chunk.
#include "banded_walk.h"

int main(int argc, char** argv) {
    std::vector<Lane> all;
    WalkOpts o = {false, false, 0, 0};
    if (const int rc = read_args(argc, argv, "narrow_prune_cpu", 5, all, o)) return rc;

    Stats st;
    long diffs = 0, rule_diffs = 0, accepted = 0, rejected = 0, lost = 0;
    for (size_t g0 = 0; g0 < all.size(); g0 += 64) {
        Lane idle;
        Lane* W[64];
        group_at(all, g0, idle, W);
        walk_group(W, o, st, rule_diffs);
        for (int l = 0; l < 64; ++l) {
            Lane& L = *W[l];
            if (!L.valid) continue;
            const int64_t score = read_out(L);
            const int64_t osc = qo_banded_score(L.p.data(), L.m, L.t.data(), L.n, L.full, L.n, nullptr, nullptr, nullptr);
            const bool ok = qe::narrow_accepts_pruned(L.m, L.n, L.cutoff, L.full, L.prune, (int)score);
            (ok ? accepted : rejected)++;
            if (ok && score != osc) {
                if (diffs < 10) fprintf(stderr, "pair %zu: accepted %lld, the oracle at %d has %lld (c1 %d p %d)\n", g0 + l, (long long)score, L.full, (long long)osc, L.cutoff, L.prune);
                ++diffs;
            }
            if (!ok && qe::narrow_accepts_pruned(L.m, L.n, L.cutoff, L.full, L.prune, (int)osc)) ++lost;
            if (L.prune >= L.cutoff) {
                int64_t oadv = 0;
                const int64_t s1 = qo_banded_score(L.p.data(), L.m, L.t.data(), L.n, L.cutoff, L.n, nullptr, nullptr, &oadv);
                if (s1 != score || oadv != L.adv) {
                    if (diffs < 10) fprintf(stderr, "pair %zu: unpruned walk %lld / %lld adv %lld / %lld\n", g0 + l, (long long)score, (long long)s1, (long long)L.adv, (long long)oadv);
                    ++diffs;
                }
            }
            printf("pair %zu score %lld adv %lld accepted %d\n", g0 + l, (long long)score, (long long)L.adv, ok ? 1 : 0);
            pat_free(&L.pat);
            L.valid = false;
        }
    }
    printf("pairs %zu lane_rel %d masked %d diffs %ld rule_diffs %ld accepted %ld rejected %ld lost %ld live %ld lane_chunks %ld chunks %ld passes4 %ld passes2 %ld passes1 %ld partial_passes %ld\n",
           all.size(), o.lane_rel, o.masked, diffs, rule_diffs, accepted, rejected, lost, st.live, st.lane_chunks, st.chunks, st.p4, st.p2, st.p1, st.masked);
    print_per_chunk(st);
    return (diffs || rule_diffs) ? 1 : 0;
}
