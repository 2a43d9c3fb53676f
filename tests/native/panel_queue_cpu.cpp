// The per-slot steps of the queued all-occurrences panel run (quicked_batch_configure_panel_queue; qe_panel.h:
// panel_queue_expand_slot, panel_queue_finish_one, panel_queue_clamp_one -- the source k_panel_queue_expand, _finish and _clamp
// run per thread) on the HOST, against a restatement: lay the slices' stored records out pair by pair, keep the first `cap`.
// Random counts per (slice, slot), slots in an order that is not the pairs', slices of 1, 2 and K, PREFIX and INFIX, and for
// every layout cap = 1, 2, W - 1, W, W + 1, 2 W + 64, one inside a text's stretch and one exactly on a text's boundary.
// Every array the steps write stands between guard words, and its indices >= min(W, cap) are checked to be untouched.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "qe_panel.h"

using namespace qe;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "panel_queue_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

static const int GUARD = 8;
// an array of `n` elements of T filled with `fill`, GUARD elements of a pattern before and behind it
template <class T> struct Guarded {
    std::vector<T> v; size_t n; T fill;
    Guarded(size_t n_, T fill_) : v(n_ + 2 * GUARD, fill_), n(n_), fill(fill_) { for (int g = 0; g < GUARD; ++g) { v[(size_t)g] = (T)(0x5A5A5A00 + g); v[GUARD + n + (size_t)g] = (T)(0x6B6B6B00 + g); } }
    T* data() { return v.data() + GUARD; }
    const T& operator[](size_t i) const { return v[GUARD + i]; }
    void check_guards() const { for (int g = 0; g < GUARD; ++g) CHECK(v[(size_t)g] == (T)(0x5A5A5A00 + g) && v[GUARD + n + (size_t)g] == (T)(0x6B6B6B00 + g)); }
    void check_untouched_from(size_t first) const { for (size_t i = first; i < n; ++i) CHECK(v[GUARD + i] == fill); }
};

struct Layout {
    int nslots, nslices, max_hits, npairs, K;
    std::vector<int32_t> text, part, m_len, t_len;
    std::vector<int64_t> m_off, t_off, off;          // off: [npairs + 1], the scan over the stored counts in the order of the pairs
    std::vector<PanelRawHit> raw;
};

static Layout make_layout(std::mt19937& rng, int npairs, int nslices, int max_hits, int density) {
    Layout L;
    L.npairs = npairs; L.nslices = nslices; L.max_hits = max_hits; L.K = 8;
    // some pairs have no slot (an empty text); the slots are in an order of their own and padded to a multiple of 64 with -1
    std::vector<int32_t> live;
    for (int i = 0; i < npairs; ++i) if (rng() % 5) live.push_back(i);
    std::shuffle(live.begin(), live.end(), rng);
    L.text = live;
    while (L.text.size() % 64) L.text.push_back(-1);
    L.nslots = (int)L.text.size();
    const int64_t stride = (int64_t)nslices * L.nslots;
    L.part.assign((size_t)(4 * stride), -9);
    L.raw.assign((size_t)(stride * max_hits), PanelRawHit{-9, -9, -9});
    L.m_len.resize((size_t)L.K); L.m_off.resize((size_t)L.K);
    for (int p = 0; p < L.K; ++p) { L.m_len[(size_t)p] = 1 + (int)(rng() % 200); L.m_off[(size_t)p] = 1000 + 17 * p; }
    L.t_len.resize((size_t)npairs); L.t_off.resize((size_t)npairs);
    for (int i = 0; i < npairs; ++i) { L.t_len[(size_t)i] = 1 + (int)(rng() % 300); L.t_off[(size_t)i] = 5000 + 13 * i; }
    std::vector<int64_t> stored((size_t)npairs, 0);
    for (int t = 0; t < L.nslots; ++t) {
        const int pair = L.text[(size_t)t];
        if (pair < 0) continue;
        int64_t sum = 0;
        for (int s = 0; s < nslices; ++s) {
            const int have = (int)(rng() % 100) < density ? (int)(rng() % (unsigned)(max_hits + 1)) : 0;
            L.part[(size_t)(stride + (int64_t)s * L.nslots + t)] = have;
            for (int i = 0; i < have; ++i) {
                const int p = (int)(rng() % (unsigned)L.K), n = L.t_len[(size_t)pair];
                L.raw[(size_t)(((int64_t)s * L.nslots + t) * max_hits + i)] = PanelRawHit{p, 1 + (int)(rng() % (unsigned)n), (int)(rng() % 5)};
            }
            sum += have;
        }
        stored[(size_t)pair] = std::min<int64_t>(sum, max_hits);
    }
    L.off.assign((size_t)npairs + 1, 0);
    for (int i = 0; i < npairs; ++i) L.off[(size_t)i + 1] = L.off[(size_t)i] + stored[(size_t)i];
    return L;
}

struct Task { int32_t m, n, score, end; int64_t plp, plt; };
// the restatement: pair by pair, a pair's slices in order, at most max_hits per pair -- the whole array, uncapped
static void restate(const Layout& L, bool infix, std::vector<int32_t>& hits, std::vector<Task>& tasks) {
    std::vector<int> slot_of((size_t)L.npairs, -1);
    for (int t = 0; t < L.nslots; ++t) if (L.text[(size_t)t] >= 0) slot_of[(size_t)L.text[(size_t)t]] = t;
    const int64_t stride = (int64_t)L.nslices * L.nslots;
    for (int pair = 0; pair < L.npairs; ++pair) {
        const int t = slot_of[(size_t)pair];
        int left = L.max_hits;
        for (int s = 0; t >= 0 && s < L.nslices; ++s)
            for (int i = 0; i < L.part[(size_t)(stride + (int64_t)s * L.nslots + t)] && left > 0; ++i, --left) {
                const PanelRawHit h = L.raw[(size_t)(((int64_t)s * L.nslots + t) * L.max_hits + i)];
                int32_t task_n = 0, in_end = 0, base = 0;
                if (infix) search_hit_task(L.m_len[(size_t)h.pattern], L.t_len[(size_t)pair], h.end, h.score, task_n, in_end, base);
                hits.insert(hits.end(), {h.pattern, base, h.end, h.score});
                tasks.push_back(Task{L.m_len[(size_t)h.pattern], task_n, h.score, in_end, L.m_off[(size_t)h.pattern], L.t_off[(size_t)pair]});
            }
        CHECK((int64_t)tasks.size() == L.off[(size_t)pair + 1]);
    }
}

static long run_layout(std::mt19937& rng, const Layout& L, bool infix) {
    std::vector<int32_t> want_hits; std::vector<Task> want_tasks;
    restate(L, infix, want_hits, want_tasks);
    const int64_t W = L.off[(size_t)L.npairs];
    std::vector<int64_t> caps = {1, 2, W - 1, W, W + 1, 2 * W + 64};
    for (int i = 1; i <= L.npairs; ++i) {
        const int64_t a = L.off[(size_t)i - 1], b = L.off[(size_t)i];
        if (b - a >= 2) { caps.push_back(a + 1 + (int64_t)(rng() % (unsigned)(b - a - 1))); break; }      // inside a text's stretch
    }
    for (int i = L.npairs / 2; i <= L.npairs; ++i) if (L.off[(size_t)i] > 0 && L.off[(size_t)i] < W) { caps.push_back(L.off[(size_t)i]); break; }      // on a boundary
    long checked = 0;
    for (const int64_t cap : caps) {
        if (cap < 1) continue;
        const size_t nc = (size_t)cap, stored = (size_t)std::min(W, cap);
        Guarded<int32_t> hits(4 * nc, -7), o_pair(nc, -1), o_m(nc, -7), o_n(nc, -7), o_score(nc, -7), o_end(nc, -7), o_start(nc, -1);
        Guarded<int64_t> o_plp(nc, -7), o_plt(nc, -7);
        PanelHitsExpandArgs e{};
        e.nslots = L.nslots; e.nslices = L.nslices; e.max_hits = L.max_hits; e.infix = infix ? 1 : 0;
        e.text = L.text.data(); e.part = L.part.data(); e.raw = L.raw.data(); e.off = L.off.data();
        e.m_len = L.m_len.data(); e.m_off = L.m_off.data(); e.t_len = L.t_len.data(); e.t_off = L.t_off.data(); e.hits = hits.data();
        if (infix) { e.o_pair = o_pair.data(); e.o_m = o_m.data(); e.o_n = o_n.data(); e.o_score = o_score.data(); e.o_end = o_end.data(); e.o_plp_off = o_plp.data(); e.o_plt_off = o_plt.data(); }
        // the slots in a scrambled order: the result may not depend on which thread runs first
        std::vector<int> order((size_t)L.nslots);
        for (int t = 0; t < L.nslots; ++t) order[(size_t)t] = t;
        std::shuffle(order.begin(), order.end(), rng);
        for (const int t : order) panel_queue_expand_slot(e, t, cap);
        for (size_t j = 0; j < stored; ++j) {
            CHECK(!memcmp(hits.data() + 4 * j, want_hits.data() + 4 * j, 16));
            if (infix) {
                const Task& k = want_tasks[j];
                CHECK(o_pair[j] == (int32_t)j && o_m[j] == k.m && o_n[j] == k.n && o_score[j] == k.score && o_end[j] == k.end && o_plp[j] == k.plp && o_plt[j] == k.plt);
            }
            ++checked;
        }
        hits.check_untouched_from(4 * stored);
        for (Guarded<int32_t>* g : {&o_pair, &o_m, &o_n, &o_score, &o_end}) { g->check_untouched_from(infix ? stored : 0); g->check_guards(); }
        for (Guarded<int64_t>* g : {&o_plp, &o_plt}) { g->check_untouched_from(infix ? stored : 0); g->check_guards(); }
        hits.check_guards();
        // ---- the finish step: o_start of the pass (-1: not found) onto the window's base, below min(total, cap) only
        if (infix) {
            std::vector<int32_t> before(hits.data(), hits.data() + 4 * nc);
            for (size_t j = 0; j < nc; ++j) o_start.data()[j] = (rng() % 4) ? (int32_t)(rng() % 50) : -1;      // (past `stored` too: the step may not read them into a record)
            const int64_t total = W;
            for (int64_t j = (int64_t)nc - 1; j >= 0; --j) panel_queue_finish_one(j, &total, cap, o_start.data(), hits.data());
            for (size_t j = 0; j < nc; ++j) {
                int32_t want[4] = {before[4 * j], before[4 * j + 1], before[4 * j + 2], before[4 * j + 3]};
                if (j < stored) want[1] = o_start[j] < 0 ? -1 : want[1] + o_start[j];
                CHECK(!memcmp(hits.data() + 4 * j, want, 16));
            }
            hits.check_guards(); o_start.check_guards();
        }
        // ---- the clamp: off' = min(off, cap), and {W, the records' bytes, the step counts' bytes}
        Guarded<int64_t> off((size_t)L.npairs + 1, 0), q(3, -7);
        memcpy(off.data(), L.off.data(), ((size_t)L.npairs + 1) * sizeof(int64_t));
        for (int64_t i = L.npairs; i >= 0; --i) panel_queue_clamp_one(i, L.npairs, cap, off.data(), q.data());
        for (int i = 0; i <= L.npairs; ++i) CHECK(off[(size_t)i] == std::min(L.off[(size_t)i], cap));
        CHECK(q[0] == W && q[1] == 16 * (int64_t)stored && q[2] == 4 * (int64_t)stored);
        for (int i = 0; i < L.npairs; ++i) {      // stored'[i]: what of the pair's stretch lies below the cap
            const int64_t a = L.off[(size_t)i], b = L.off[(size_t)i + 1];
            CHECK(off[(size_t)i + 1] - off[(size_t)i] == std::max<int64_t>(0, std::min(b, cap) - std::min(a, cap)));
        }
        off.check_guards(); q.check_guards();
    }
    return checked;
}

int main() {
    std::mt19937 rng(20261020);
    long checked = 0, layouts = 0, empty = 0;
    for (int npairs : {1, 3, 63, 64, 65, 130, 300})
        for (int nslices : {1, 2, 8})
            for (int max_hits : {1, 2, 16})
                for (int density : {0, 30, 100})
                    for (int infix = 0; infix < 2; ++infix) {
                        const Layout L = make_layout(rng, npairs, nslices, max_hits, density);
                        if (L.nslots == 0) continue;
                        empty += L.off[(size_t)npairs] == 0;
                        checked += run_layout(rng, L, infix != 0);
                        ++layouts;
                    }
    // the sync run's step is the same function without the cap
    {
        const Layout L = make_layout(rng, 130, 2, 16, 100);
        std::vector<int32_t> want_hits; std::vector<Task> want_tasks;
        restate(L, false, want_hits, want_tasks);
        std::vector<int32_t> hits(want_hits.size(), -7);
        PanelHitsExpandArgs e{};
        e.nslots = L.nslots; e.nslices = L.nslices; e.max_hits = L.max_hits; e.infix = 0;
        e.text = L.text.data(); e.part = L.part.data(); e.raw = L.raw.data(); e.off = L.off.data();
        e.m_len = L.m_len.data(); e.m_off = L.m_off.data(); e.t_len = L.t_len.data(); e.t_off = L.t_off.data(); e.hits = hits.data();
        for (int t = 0; t < L.nslots; ++t) panel_hits_expand_slot(e, t);
        CHECK(hits == want_hits && !hits.empty());
    }
    CHECK(layouts > 300 && checked > 100000 && empty > 50);
    printf("panel_queue_cpu ok layouts %ld records %ld without_occurrence %ld\n", layouts, checked, empty);
    return 0;
}
