// Queued panel runs (quicked_batch_configure_panel_queue) on the HOST, under sanitizers: the library's host layer built with g++
// against the fake HIP runtime of tests/native/hip_stub.  The stand-ins of the new kernels (hip_stub/qe_kernels_stub.h) are
// the device kernels' own per-slot source (qe_panel.h); the stand-in of k_pack_iupac is the scalar packer, so the runs under an
// IUPAC flag give true answers here.  They are compared with the definitions tests/test_host_panel_queue.py wrote (file `cases`
// in the directory given; tests/panel_queue_lib.py's format): occurrence lists, tails and heads, the best member derived from
// the lists by the header's consequence 1, a sub-panel's by dropping the other members' records.
//
// Checked: the configure call's refusals and that they leave the setting alone; an unconfigured and a re-zeroed batch; every
// combination that stays refused with the setting on; QUICKED_ERROR before QUICKED_UNIMPLEMENTED; every getter unchanged between
// queue and fetch after a sync panel run, after a pair run and after nothing; the fetch against the definitions in both base
// modes, with and without QUICKED_PANEL_TAILS and QUICKED_PANEL_HEADS, at max_hits 1, 2 and 64, QE_PANEL_SLICES unset, 1 and
// 4096, counter [0] against the sync run's; the overflow rule at max_total 1, 2, W - 1, W, W + 1; a second queued run
// superseding the first; reload and destroy with a run pending; the fetch from another thread; six batch objects with six
// panels queued before the first fetch and fetched in reverse; `wanted` after each kind of run.
#include <thread>

#define PANEL_HOST_NAME "panel_queue_host"
#include "panel_host_common.h"

static const int INFIX = QUICKED_SEARCH_INFIX, PREFIX = QUICKED_SEARCH_PREFIX, TL = QUICKED_PANEL_TAILS, HD = QUICKED_PANEL_HEADS;
static const int FLAGS[3] = {0, QUICKED_SEARCH_IUPAC, QUICKED_SEARCH_IUPAC_PATTERN};

struct Occ { int32_t pattern, start, end, score; bool operator==(const Occ& o) const { return !memcmp(this, &o, sizeof(Occ)); } };
struct Four { int32_t a, b, c, d; bool operator==(const Four& o) const { return !memcmp(this, &o, sizeof(Four)); } };
typedef std::vector<std::vector<Occ>> Lists;
struct Group {
    std::vector<std::string> panel, texts; std::vector<int32_t> bound;
    Lists hits[3][2];                                      // [flag][PREFIX, INFIX], uncapped
    std::vector<std::vector<Four>> tails[3], heads[3];     // [flag][min_overlap index]
};
static std::vector<int32_t> g_overlaps;

// ---- what every getter answers, status and data: equal snapshots = nothing the caller can see has changed
struct Snapshot {
    std::vector<int64_t> v;
    bool operator==(const Snapshot& o) const { return v == o.v; }
    bool operator!=(const Snapshot& o) const { return !(v == o.v); }
};
static Snapshot snapshot(quicked_batch_t* b, int64_t n, int K) {
    Snapshot S;
    auto put = [&](int64_t x) { S.v.push_back(x); };
    std::vector<int32_t> a((size_t)n + 1), c((size_t)n + 1);
    put(quicked_batch_scores(b, a.data(), c.data()));
    for (int64_t i = 0; i < n; ++i) { put(a[(size_t)i]); put(c[(size_t)i]); }
    int64_t cn[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    put(quicked_batch_counters(b, cn));
    for (int q = 0; q < 8; ++q) if (q != 5) put(cn[q]);
    std::vector<quicked_panel_hit_t> ph((size_t)n + 1, quicked_panel_hit_t{-7, -7, -7, -7, -7, -7});
    put(quicked_batch_panel_results(b, ph.data()));
    for (int64_t i = 0; i < n; ++i) { put(ph[(size_t)i].pattern); put(ph[(size_t)i].score); put(ph[(size_t)i].text_start); put(ph[(size_t)i].text_end); put(ph[(size_t)i].second_pattern); put(ph[(size_t)i].second_score); }
    (void)K;
    put(quicked_batch_panel_matrix(b, nullptr, nullptr));
    put(quicked_batch_panel_hit_counts(b, a.data(), c.data()));
    const int64_t total = quicked_batch_panel_hit_total(b);
    put(total);
    if (total >= 0) {
        for (int64_t i = 0; i < n; ++i) { put(a[(size_t)i]); put(c[(size_t)i]); }
        std::vector<quicked_panel_occ_t> occ((size_t)total + 1);
        std::vector<int64_t> off((size_t)n + 1);
        put(quicked_batch_panel_hits(b, occ.data(), off.data()));
        for (int64_t j = 0; j < total; ++j) { put(occ[(size_t)j].pattern); put(occ[(size_t)j].text_start); put(occ[(size_t)j].text_end); put(occ[(size_t)j].score); }
        for (const int64_t o : off) put(o);
    }
    std::vector<quicked_panel_tail_t> t((size_t)n + 1, quicked_panel_tail_t{-7, -7, -7, -7});
    put(quicked_batch_panel_tails(b, t.data()));
    for (int64_t i = 0; i < n; ++i) { put(t[(size_t)i].pattern); put(t[(size_t)i].overlap); put(t[(size_t)i].text_start); put(t[(size_t)i].score); }
    std::vector<quicked_panel_head_t> h((size_t)n + 1, quicked_panel_head_t{-7, -7, -7, -7});
    put(quicked_batch_panel_heads(b, h.data()));
    for (int64_t i = 0; i < n; ++i) { put(h[(size_t)i].pattern); put(h[(size_t)i].overlap); put(h[(size_t)i].text_end); put(h[(size_t)i].score); }
    put(quicked_batch_locations(b, a.data(), c.data()));
    put(quicked_batch_hit_total(b));
    put(quicked_batch_panel_hit_cigar_bytes(b));
    put(quicked_batch_cigar_bytes(b));
    put(quicked_batch_panel_queue_wanted(b));
    return S;
}

// ---- the definitions' side
// a sub-panel's lists: the records of the members kept, renumbered (a member's occurrences do not depend on the others)
static Lists sub_lists(const Lists& L, const std::vector<int>& members) {
    Lists out(L.size());
    for (size_t i = 0; i < L.size(); ++i)
        for (size_t q = 0; q < members.size(); ++q)
            for (const Occ& o : L[i]) if (o.pattern == members[q]) out[i].push_back(Occ{(int32_t)q, o.start, o.end, o.score});
    return out;
}
// consequence 1 of the header: the smallest key (score, pattern) with the first occurrence that has it; the runner-up among the others
static quicked_panel_hit_t best_two(const std::vector<Occ>& h) {
    quicked_panel_hit_t r{-1, -1, -1, -1, -1, -1};
    for (const Occ& o : h) if (r.pattern < 0 || o.score < r.score || (o.score == r.score && o.pattern < r.pattern)) r = quicked_panel_hit_t{o.pattern, o.score, o.start, o.end, -1, -1};
    for (const Occ& o : h) if (o.pattern != r.pattern && (r.second_pattern < 0 || o.score < r.second_score || (o.score == r.second_score && o.pattern < r.second_pattern))) { r.second_pattern = o.pattern; r.second_score = o.score; }
    return r;
}

struct Run { quicked_batch_t* b; int64_t n; Pool M; std::vector<int32_t> bound; int K; };
static quicked_status_t run_all(const Run& R, int mode, int32_t max_hits, int sync) {
    return quicked_batch_run_panel_all(R.b, mode, R.K, R.M.bytes.data(), R.M.off.data(), R.M.len.data(), R.bound.data(), 0, max_hits, sync);
}
static quicked_status_t run_best(const Run& R, int mode, int sync) {
    return quicked_batch_run_panel(R.b, mode, R.K, R.M.bytes.data(), R.M.off.data(), R.M.len.data(), R.bound.data(), 0, sync);
}
static Run make_run(quicked_batch_t* b, const Group& G, const std::vector<int>& members) {
    Run R;
    R.b = b; R.n = (int64_t)G.texts.size(); R.K = (int)members.size();
    std::vector<std::string> pan;
    for (const int p : members) { pan.push_back(G.panel[(size_t)p]); R.bound.push_back(G.bound[(size_t)p]); }
    R.M = pool_of(pan);
    return R;
}
static std::vector<int> all_members(const Group& G) { std::vector<int> m(G.panel.size()); for (size_t p = 0; p < m.size(); ++p) m[p] = (int)p; return m; }
static quicked_batch_t* batch_of(const Group& G, bool with_patterns = false) {
    const int n = (int)G.texts.size();
    const std::vector<std::string> none((size_t)n);
    const Pool E = pool_of(with_patterns ? G.texts : none), T = pool_of(G.texts);
    quicked_batch_t* b = quicked_batch_create(n, E.bytes.data(), E.off.data(), E.len.data(), T.bytes.data(), T.off.data(), T.len.data());
    CHECK(b);
    return b;
}

static long g_checked = 0, g_overflows = 0;
// the fetched results of a queued quicked_batch_run_panel against the lists
static void check_best(quicked_batch_t* b, const Group& G, const Lists& L) {
    const size_t n = G.texts.size();
    std::vector<quicked_panel_hit_t> got(n + 1, quicked_panel_hit_t{-7, -7, -7, -7, -7, -7});
    CHECK(quicked_batch_panel_results(b, got.data()) == QUICKED_OK && got[n].pattern == -7);
    std::vector<int32_t> sc(n), st(n);
    CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
    for (size_t i = 0; i < n; ++i) {
        const quicked_panel_hit_t w = best_two(L[i]);
        if (memcmp(&got[i], &w, sizeof(w))) fprintf(stderr, "text %zu: got {%d %d %d %d %d %d}, expected {%d %d %d %d %d %d}\n", i, got[i].pattern, got[i].score, got[i].text_start, got[i].text_end, got[i].second_pattern, got[i].second_score, w.pattern, w.score, w.text_start, w.text_end, w.second_pattern, w.second_score);
        CHECK(!memcmp(&got[i], &w, sizeof(w)));
        CHECK(sc[i] == w.score && st[i] == (G.texts[i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
        ++g_checked;
    }
    CHECK(quicked_batch_panel_queue_wanted(b) == -1 && quicked_batch_panel_hit_total(b) == -1);
    int64_t c[8];
    CHECK(quicked_batch_counters(b, c) >= 0 && (c[0] > 0 || L.empty()));
}
// ... of a queued quicked_batch_run_panel_all: the cap per text, then the room per run.  -> W
static int64_t check_all(quicked_batch_t* b, const Group& G, const Lists& L, int32_t max_hits, int64_t max_total,
                         const std::vector<Four>* tails, const std::vector<Four>* heads) {
    const size_t n = G.texts.size();
    std::vector<int64_t> off(n + 1, 0);
    std::vector<Occ> recs;
    for (size_t i = 0; i < n; ++i) {
        const size_t keep = std::min(L[i].size(), (size_t)max_hits);
        recs.insert(recs.end(), L[i].begin(), L[i].begin() + (long)keep);
        off[i + 1] = off[i] + (int64_t)keep;
    }
    const int64_t W = off[n], total = std::min(W, max_total);
    std::vector<int32_t> found(n), stored(n), sc(n), st(n);
    CHECK(quicked_batch_panel_hit_counts(b, found.data(), stored.data()) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_total(b) == total && quicked_batch_panel_queue_wanted(b) == W);
    std::vector<Occ> got((size_t)total + 1, Occ{-7, -7, -7, -7});
    std::vector<int64_t> goff(n + 1, -7);
    CHECK(quicked_batch_panel_hits(b, (quicked_panel_occ_t*)got.data(), goff.data()) == QUICKED_OK && got[(size_t)total].pattern == -7);
    CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
    for (size_t i = 0; i < n; ++i) {
        int32_t bestv = -1;
        for (const Occ& o : L[i]) bestv = (bestv < 0 || o.score < bestv) ? o.score : bestv;
        CHECK(found[i] == (int32_t)L[i].size() && sc[i] == bestv && st[i] == (G.texts[i].empty() ? QUICKED_EMPTY_SEQUENCE : QUICKED_OK));
        CHECK(goff[i] == std::min(off[i], max_total) && stored[i] == (int32_t)(std::min(off[i + 1], max_total) - std::min(off[i], max_total)));
    }
    CHECK(goff[n] == total);
    for (int64_t j = 0; j < total; ++j) {
        if (!(got[(size_t)j] == recs[(size_t)j])) fprintf(stderr, "record %lld: got {%d %d %d %d}, expected {%d %d %d %d}\n", (long long)j, got[(size_t)j].pattern, got[(size_t)j].start, got[(size_t)j].end, got[(size_t)j].score, recs[(size_t)j].pattern, recs[(size_t)j].start, recs[(size_t)j].end, recs[(size_t)j].score);
        CHECK(got[(size_t)j] == recs[(size_t)j]);
        ++g_checked;
    }
    std::vector<Four> t(n + 1, Four{-7, -7, -7, -7});
    if (tails) { CHECK(quicked_batch_panel_tails(b, (quicked_panel_tail_t*)t.data()) == QUICKED_OK && t[n].a == -7); for (size_t i = 0; i < n; ++i) CHECK(t[i] == (*tails)[i]); }
    else CHECK(quicked_batch_panel_tails(b, (quicked_panel_tail_t*)t.data()) == QUICKED_ERROR);
    if (heads) { CHECK(quicked_batch_panel_heads(b, (quicked_panel_head_t*)t.data()) == QUICKED_OK && t[n].a == -7); for (size_t i = 0; i < n; ++i) CHECK(t[i] == (*heads)[i]); }
    else CHECK(quicked_batch_panel_heads(b, (quicked_panel_head_t*)t.data()) == QUICKED_ERROR);
    quicked_panel_hit_t ph[1];
    CHECK(quicked_batch_panel_results(b, ph) == QUICKED_ERROR && quicked_batch_panel_hit_cigar_bytes(b) == -1 && quicked_batch_hit_total(b) == -1);
    return W;
}

// ---- the definitions, group by group: both base modes, the bits, the caps, the slices
static void run_definitions(const Group& G) {
    quicked_batch_t* b = batch_of(G);
    const Run R = make_run(b, G, all_members(G));
    CHECK(quicked_batch_configure_panel_queue(b, (int64_t)1 << 20) == QUICKED_OK);
    int64_t cs[8], cq[8];
    for (const char* slices : {(const char*)nullptr, "1", "4096"}) {
        set_env("QE_PANEL_SLICES", slices);
        for (int f = 1; f < 3; ++f)
            for (int base : {PREFIX, INFIX}) {
                const Lists& L = G.hits[f][base == INFIX];
                CHECK(run_best(R, base | FLAGS[f], 0) == QUICKED_OK);
                CHECK(quicked_batch_fetch(b) == QUICKED_OK);
                check_best(b, G, L);
                for (size_t mo = 0; mo < g_overlaps.size(); ++mo) {
                    // (the tails and the heads keep a min_overlap each: one takes this one, the other the next)
                    const size_t mo_h = (mo + 1) % g_overlaps.size();
                    CHECK(quicked_batch_configure_panel_tails(b, g_overlaps[mo]) == QUICKED_OK && quicked_batch_configure_panel_heads(b, g_overlaps[mo_h]) == QUICKED_OK);
                    for (int tl : {0, TL})
                        for (int hd : {0, HD})
                            for (int32_t cap : {1, 2, 64}) {
                                if (base == PREFIX && tl) { CHECK(run_all(R, base | FLAGS[f] | tl | hd, cap, 0) == QUICKED_ERROR); continue; }
                                if ((mo || slices) && cap == 2) continue;
                                CHECK(run_all(R, base | FLAGS[f] | tl | hd, cap, 1) == QUICKED_OK);
                                CHECK(quicked_batch_counters(b, cs) >= 0 && quicked_batch_panel_queue_wanted(b) == -1);
                                CHECK(run_all(R, base | FLAGS[f] | tl | hd, cap, 0) == QUICKED_OK);
                                CHECK(quicked_batch_fetch(b) == QUICKED_OK);
                                check_all(b, G, L, cap, (int64_t)1 << 20, tl ? &G.tails[f][mo] : nullptr, hd ? &G.heads[f][mo_h] : nullptr);
                                CHECK(quicked_batch_counters(b, cq) >= 0);
                                for (int q : {0, 1, 2, 3, 6, 7}) CHECK(cs[q] == cq[q]);       // roomy: the block steps are the sync run's
                            }
                }
            }
    }
    set_env("QE_PANEL_SLICES", nullptr);
    CHECK(quicked_batch_configure_panel_tails(b, 3) == QUICKED_OK && quicked_batch_configure_panel_heads(b, 3) == QUICKED_OK);
    // ---- overflow: the first max_total records of the array, the clamped offsets, W
    {
        const Lists& L = G.hits[1][1];
        int64_t W = 0;
        for (const auto& h : L) W += (int64_t)std::min<size_t>(h.size(), 4);
        for (int64_t room : {(int64_t)1, (int64_t)2, W - 1, W, W + 1}) {
            if (W <= 4) break;
            ++g_overflows;
            CHECK(quicked_batch_configure_panel_queue(b, room) == QUICKED_OK);
            CHECK(run_all(R, INFIX | FLAGS[1] | TL | HD, 4, 0) == QUICKED_OK && quicked_batch_fetch(b) == QUICKED_OK);
            const size_t mo3 = (size_t)(std::find(g_overlaps.begin(), g_overlaps.end(), 3) - g_overlaps.begin());
            CHECK(check_all(b, G, L, 4, room, &G.tails[1][mo3], &G.heads[1][mo3]) == W);
            CHECK(run_all(R, PREFIX | FLAGS[1], 4, 0) == QUICKED_OK && quicked_batch_fetch(b) == QUICKED_OK);
            check_all(b, G, G.hits[1][0], 4, room, nullptr, nullptr);
        }
    }
    quicked_batch_destroy(b);
}

// ---- the rules of the interface, on one group
static void run_rules(const Group& G) {
    const int64_t n = (int64_t)G.texts.size();
    const int K = (int)G.panel.size(), IU = QUICKED_SEARCH_IUPAC;
    quicked_batch_t* b = batch_of(G, true);
    const Run R = make_run(b, G, all_members(G));
    const Lists& LI = G.hits[1][1];
    // ---- after nothing: a batch as it is created refuses, and a configured one queues; the getters stay as they were
    const Snapshot fresh = snapshot(b, n, K);
    CHECK(quicked_batch_panel_queue_wanted(b) == -1 && quicked_batch_panel_queue_wanted(nullptr) == -1);
    CHECK(run_best(R, INFIX | IU, 0) == QUICKED_UNIMPLEMENTED && run_all(R, INFIX | IU, 16, 0) == QUICKED_UNIMPLEMENTED && run_all(R, PREFIX | IU | HD, 16, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_fetch(b) == QUICKED_OK && snapshot(b, n, K) == fresh);
    // ---- the configure call
    CHECK(quicked_batch_configure_panel_queue(nullptr, 16) == QUICKED_ERROR);
    for (int64_t bad : {(int64_t)-1, ((int64_t)1 << 26) + 1, (int64_t)INT64_MAX, (int64_t)INT64_MIN}) {
        CHECK(quicked_batch_configure_panel_queue(b, bad) == QUICKED_ERROR);
        CHECK(run_best(R, INFIX | IU, 0) == QUICKED_UNIMPLEMENTED);                     // still off
    }
    CHECK(quicked_batch_configure_panel_queue(b, (int64_t)1 << 26) == QUICKED_OK && quicked_batch_configure_panel_queue(b, 1) == QUICKED_OK);
    CHECK(quicked_batch_configure_panel_queue(b, 4096) == QUICKED_OK);
    for (int64_t bad : {(int64_t)-1, ((int64_t)1 << 26) + 1}) CHECK(quicked_batch_configure_panel_queue(b, bad) == QUICKED_ERROR);
    CHECK(run_best(R, INFIX | IU, 0) == QUICKED_OK);                                    // still on
    CHECK(snapshot(b, n, K) == fresh);
    CHECK(quicked_batch_fetch(b) == QUICKED_OK);
    check_best(b, G, LI);
    CHECK(snapshot(b, n, K) != fresh);
    // ---- re-zeroed: as created
    CHECK(quicked_batch_configure_panel_queue(b, 0) == QUICKED_OK);
    CHECK(run_best(R, INFIX | IU, 0) == QUICKED_UNIMPLEMENTED && run_all(R, INFIX | IU, 16, 0) == QUICKED_UNIMPLEMENTED);
    CHECK(quicked_batch_configure_panel_queue(b, 4096) == QUICKED_OK);
    // ---- after a sync panel run: what stays refused with the setting on, and QUICKED_ERROR first; nothing queued, nothing changed
    CHECK(run_all(R, INFIX | IU | TL | HD, 16, 1) == QUICKED_OK);
    const Snapshot sync_all = snapshot(b, n, K);
    {
        CHECK(run_best(R, INFIX | IU | QUICKED_PANEL_MATRIX, 0) == QUICKED_UNIMPLEMENTED && run_best(R, PREFIX | QUICKED_PANEL_MATRIX, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(run_all(R, INFIX | IU | QUICKED_PANEL_CIGARS, 16, 0) == QUICKED_UNIMPLEMENTED && run_all(R, INFIX | IU | QUICKED_PANEL_CIGARS | TL | HD, 16, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_panel_scan(b, INFIX | IU, R.K, R.M.bytes.data(), R.M.off.data(), R.M.len.data(), R.bound.data(), 0, 16, 64, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_search_all(b, INFIX, nullptr, 3, 4, 0) == QUICKED_UNIMPLEMENTED);
        const std::string big((size_t)QUICKED_PANEL_MAX_LEN + 1, 'A');
        const int64_t o2[2] = {0, 0};
        const int32_t len[2] = {4, QUICKED_PANEL_MAX_LEN + 1};
        CHECK(quicked_batch_run_panel_all(b, INFIX, 2, big.data(), o2, len, nullptr, 3, 16, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_run_panel(b, INFIX, 2, big.data(), o2, len, nullptr, 3, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
        CHECK(run_all(R, INFIX | IU, 16, 0) == QUICKED_UNIMPLEMENTED && run_best(R, INFIX | IU, 0) == QUICKED_UNIMPLEMENTED);
        CHECK(quicked_batch_configure(b, 0, 0) == QUICKED_OK);
        // QUICKED_ERROR comes first, whatever else would refuse the run
        for (int on = 0; on < 2; ++on) {
            CHECK(quicked_batch_configure_panel_queue(b, on ? 4096 : 0) == QUICKED_OK);
            CHECK(run_all(R, PREFIX | IU | TL, 16, 0) == QUICKED_ERROR && run_all(R, INFIX | IU, 0, 0) == QUICKED_ERROR && run_all(R, INFIX | IU | 1024, 16, 0) == QUICKED_ERROR);
            CHECK(run_all(R, INFIX | IU | QUICKED_PANEL_MATRIX, 16, 0) == QUICKED_ERROR && run_all(R, INFIX | IU | QUICKED_PANEL_CIGARS, 4097, 0) == QUICKED_ERROR);
            CHECK(run_best(R, INFIX | IU | HD, 0) == QUICKED_ERROR && run_best(R, 3 | QUICKED_PANEL_MATRIX, 0) == QUICKED_ERROR);
            CHECK(quicked_batch_run_panel(b, INFIX | QUICKED_PANEL_MATRIX, 0, R.M.bytes.data(), R.M.off.data(), R.M.len.data(), nullptr, 3, 0) == QUICKED_ERROR);
            CHECK(quicked_batch_run_panel_all(b, INFIX | QUICKED_PANEL_CIGARS, R.K, R.M.bytes.data(), R.M.off.data(), R.M.len.data(), nullptr, -1, 16, 0) == QUICKED_ERROR);
            CHECK(quicked_batch_run_panel_all(b, INFIX, 2, big.data(), o2, len, nullptr, -1, 16, 0) == QUICKED_ERROR);      // (over 256 bases too)
        }
        CHECK(quicked_batch_fetch(b) == QUICKED_OK);
        CHECK(snapshot(b, n, K) == sync_all);
    }
    // ---- queued behind that sync run: the getters show the sync run's results until the fetch; a second queued run supersedes
    const std::vector<int> one = {K - 1};
    const Run R1 = make_run(b, G, one);
    CHECK(run_all(R, PREFIX | IU | HD, 2, 0) == QUICKED_OK);
    CHECK(snapshot(b, n, K) == sync_all);
    CHECK(run_best(R1, INFIX | IU, 0) == QUICKED_OK);
    CHECK(snapshot(b, n, K) == sync_all);
    CHECK(quicked_batch_fetch(b) == QUICKED_OK);
    check_best(b, G, sub_lists(LI, one));
    CHECK(quicked_batch_fetch(b) == QUICKED_OK);                                        // nothing pending any more
    check_best(b, G, sub_lists(LI, one));
    CHECK(run_best(R1, INFIX | IU, 0) == QUICKED_OK && run_all(R, INFIX | IU | TL, 64, 0) == QUICKED_OK && quicked_batch_fetch(b) == QUICKED_OK);
    check_all(b, G, LI, 64, 4096, &G.tails[1][(size_t)(std::find(g_overlaps.begin(), g_overlaps.end(), 3) - g_overlaps.begin())], nullptr);
    // ---- after a pair run
    CHECK(quicked_batch_run_search(b, INFIX, nullptr, 3, 1, 1) >= QUICKED_EMPTY_SEQUENCE);
    const Snapshot pair_run = snapshot(b, n, K);
    CHECK(quicked_batch_panel_queue_wanted(b) == -1);
    CHECK(run_all(R, INFIX | IU, 16, 0) == QUICKED_OK);
    CHECK(snapshot(b, n, K) == pair_run);
    std::vector<int32_t> ts((size_t)n), te((size_t)n);
    CHECK(quicked_batch_locations(b, ts.data(), te.data()) == QUICKED_OK);             // the last run is still the search run
    // ---- the fetch from another thread
    {
        quicked_status_t st = QUICKED_ERROR;
        std::thread th([&] { st = quicked_batch_fetch(b); });
        th.join();
        CHECK(st == QUICKED_OK);
    }
    check_all(b, G, LI, 16, 4096, nullptr, nullptr);
    CHECK(quicked_batch_locations(b, ts.data(), te.data()) == QUICKED_ERROR);
    // ---- `wanted`: -1 after a sync run of the same kind, and after a reload; a reload discards a pending run
    CHECK(run_all(R, INFIX | IU, 16, 1) == QUICKED_OK && quicked_batch_panel_queue_wanted(b) == -1);
    CHECK(run_all(R, INFIX | IU, 16, 0) == QUICKED_OK && quicked_batch_fetch(b) == QUICKED_OK && quicked_batch_panel_queue_wanted(b) >= 0);
    CHECK(run_all(R, INFIX | IU, 16, 0) == QUICKED_OK);
    {
        const Pool T = pool_of(G.texts);
        CHECK(quicked_batch_reload(b, n, T.bytes.data(), T.off.data(), T.len.data(), T.bytes.data(), T.off.data(), T.len.data()) >= 0);
    }
    CHECK(quicked_batch_fetch(b) == QUICKED_OK);
    CHECK(quicked_batch_panel_queue_wanted(b) == -1 && quicked_batch_panel_hit_total(b) == -1);
    CHECK(run_best(R, INFIX | IU, 0) == QUICKED_OK && quicked_batch_fetch(b) == QUICKED_OK);      // the setting outlives the reload
    check_best(b, G, LI);
    // ---- destroy with a run pending
    CHECK(run_all(R, INFIX | IU | TL | HD, 16, 0) == QUICKED_OK);
    quicked_batch_destroy(b);
    // ---- six batch objects with six panels, queued before the first fetch, fetched in reverse (more than the rotation's five sets)
    {
        std::vector<quicked_batch_t*> bs;
        std::vector<std::vector<int>> members;
        for (int q = 0; q < 6; ++q) {
            std::vector<int> m = {q % K};
            if (q >= 2 && (q + 1) % K != q % K) m.push_back((q + 1) % K);
            std::sort(m.begin(), m.end());
            members.push_back(m);
            bs.push_back(batch_of(G));
            CHECK(quicked_batch_configure_panel_queue(bs.back(), 1 << 16) == QUICKED_OK);
        }
        for (int q = 0; q < 6; ++q) {
            const Run Rq = make_run(bs[(size_t)q], G, members[(size_t)q]);      // (the panel and the bounds are gone when the call returns)
            CHECK((q % 2 ? run_best(Rq, INFIX | IU, 0) : run_all(Rq, INFIX | IU, 8, 0)) == QUICKED_OK);
        }
        for (int q = 5; q >= 0; --q) {
            CHECK(quicked_batch_fetch(bs[(size_t)q]) == QUICKED_OK);
            const Lists L = sub_lists(LI, members[(size_t)q]);
            if (q % 2) check_best(bs[(size_t)q], G, L); else check_all(bs[(size_t)q], G, L, 8, 1 << 16, nullptr, nullptr);
        }
        for (quicked_batch_t* q : bs) quicked_batch_destroy(q);
    }
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream f(std::string(argv[1]) + "/cases");
    int ngroups = 0, nover = 0;
    f >> ngroups >> nover;
    CHECK(!f.fail() && ngroups >= 1 && nover >= 1);
    g_overlaps.resize((size_t)nover);
    std::vector<Group> groups((size_t)ngroups);
    for (Group& G : groups) {
        int K = 0, n = 0;
        f >> K >> n;
        CHECK(!f.fail() && K >= 1 && n >= 1);
        G.panel.resize((size_t)K); G.texts.resize((size_t)n); G.bound.resize((size_t)K);
        for (int p = 0; p < K; ++p) f >> G.panel[(size_t)p] >> G.bound[(size_t)p];
        for (int i = 0; i < n; ++i) { f >> G.texts[(size_t)i]; if (G.texts[(size_t)i] == ".") G.texts[(size_t)i].clear(); }
        for (int fl = 0; fl < 3; ++fl) {
            for (int mode = 0; mode < 2; ++mode) {
                G.hits[fl][mode].resize((size_t)n);
                for (auto& h : G.hits[fl][mode]) {
                    int found = 0;
                    f >> found;
                    h.resize((size_t)found);
                    for (Occ& o : h) f >> o.pattern >> o.start >> o.end >> o.score;
                }
            }
            G.tails[fl].resize((size_t)nover); G.heads[fl].resize((size_t)nover);
            for (int mo = 0; mo < nover; ++mo) {
                G.tails[fl][(size_t)mo].resize((size_t)n); G.heads[fl][(size_t)mo].resize((size_t)n);
                for (Four& t : G.tails[fl][(size_t)mo]) f >> t.a >> t.b >> t.c >> t.d;
                for (Four& t : G.heads[fl][(size_t)mo]) f >> t.a >> t.b >> t.c >> t.d;
            }
            CHECK(!f.fail());
        }
    }
    for (int mo = 0; mo < nover; ++mo) f >> g_overlaps[(size_t)mo];
    CHECK(!f.fail());
    run_rules(groups[0]);
    for (const Group& G : groups) run_definitions(G);
    CHECK(g_checked > 4000 && g_overflows >= 10);
    printf("panel_queue_host ok %ld\n", g_checked);
    return 0;
}
