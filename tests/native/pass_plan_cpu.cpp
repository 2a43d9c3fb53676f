// The walk of tests/native/banded_walk.h over plain arrays with the 4 / 2 / 1 plan and no threshold, checked per pair against
// the oracle's own pass (qo_banded_score, score_pass_run): score, first / last / pos_v, block advances.  Prints the counts
// and the passes per chunk.
//   pass_plan_cpu <file> <lane_rel 0|1> <masked 0|1>
// file: int32 count, then per pair int32 m, n, cutoff and the m + n bytes of pattern and text.
// Exit code 1: a difference.
#include "banded_walk.h"

int main(int argc, char** argv) {
    std::vector<Lane> all;
    WalkOpts o = {false, false, 0, 0};
    if (const int rc = read_args(argc, argv, "pass_plan_cpu", 3, all, o)) return rc;

    Stats st;
    long diffs = 0, rule_diffs = 0;
    for (size_t g0 = 0; g0 < all.size(); g0 += 64) {
        Lane idle;
        Lane* W[64];
        group_at(all, g0, idle, W);
        walk_group(W, o, st, rule_diffs);
        for (int l = 0; l < 64; ++l) {
            Lane& L = *W[l];
            if (!L.valid) continue;
            const int64_t score = read_out(L);
            score_pass_t sp;
            score_pass_run(&sp, &L.pat, L.t.data(), L.n, L.cutoff, L.n);
            int64_t ofirst = 0, olast = 0, oadv = 0;
            const int64_t osc = qo_banded_score(L.p.data(), L.m, L.t.data(), L.n, L.cutoff, L.n, &ofirst, &olast, &oadv);
            const bool same = score == osc && sp.score == osc && L.first == ofirst && L.last == olast && L.pos_v == sp.b.pos_v && L.adv == oadv;
            if (!same) {
                if (diffs < 10)
                    fprintf(stderr, "pair %zu: score %lld / %lld first %d / %lld last %d / %lld pos_v %d / %lld adv %lld / %lld\n", g0 + l,
                            (long long)score, (long long)osc, L.first, (long long)ofirst, L.last, (long long)olast, L.pos_v, (long long)sp.b.pos_v,
                            (long long)L.adv, (long long)oadv);
                ++diffs;
            }
            score_pass_free(&sp);
            pat_free(&L.pat);
            L.valid = false;
        }
    }
    printf("pairs %zu lane_rel %d masked %d diffs %ld rule_diffs %ld chunks %ld passes4 %ld passes2 %ld passes1 %ld partial_passes %ld\n",
           all.size(), o.lane_rel, o.masked, diffs, rule_diffs, st.chunks, st.p4, st.p2, st.p1, st.masked);
    print_per_chunk(st);
    return (diffs || rule_diffs) ? 1 : 0;
}
