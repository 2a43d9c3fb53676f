// search_hits_cpu.cpp -- the all-occurrences recurrence of quicked_amd/csrc/qe_search.h compiled for the host: the very
// source k_search_hits<NB> runs per lane, driven task by task through the steps of the run_search_hits stage (the forward
// pass into a sink of `cap` entries, then for INFIX one PREFIX pass per stored occurrence over the reversed sequences, on the
// window of search_hit_window columns).  A stand-alone program, built by tests/test_search_hits_cpu.py once plain and once
// with -fsanitize=address,undefined; it reads its cases from files and is compared with a brute force and with edlib there.
//
// search_hits_cpu <dir>: {plen,tlen,bound,mode,form,cap}.i32, {poff,toff}.i64, {ppool,tpool}.bin -> <dir>/out.i32, per entry
// found, best score, stored, block steps of the forward pass, then stored x {text_start, text_end, score}.
//   form: 0 the workspace store with every block live, 1 the workspace store with the live-block rule, 2 the register
//         store with the rule (patterns of up to QE_SEARCH_REG_BLOCKS blocks; longer ones: as 1)
// The sink is an array of exactly `stored capacity` = min(cap, tlen) entries with a guard value behind it: a write past a
// task's capacity is an error here even without the sanitizers.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "qe_search.h"

static std::vector<uint64_t> planes_of(const char* s, int len, bool reverse) {
    std::vector<uint64_t> pl((size_t)3 * (size_t)((len + 63) / 64), 0);
    for (int i = 0; i < len; ++i) {
        int code;
        switch (s[reverse ? len - 1 - i : i]) {
            case 'A': case 'a': code = 0; break;
            case 'C': case 'c': code = 1; break;
            case 'G': case 'g': code = 2; break;
            case 'T': case 't': code = 3; break;
            default: code = 4; break;
        }
        uint64_t* row = pl.data() + 3 * (size_t)(i >> 6);
        const uint64_t bit = (uint64_t)1 << (i & 63);
        if (code == 4) row[2] |= bit;
        else { if (code & 1) row[0] |= bit; if (code & 2) row[1] |= bit; }
    }
    return pl;
}

// the forward pass in the given form; exactly the blocks of the pattern as workspace
static void forward(const uint64_t* pp, int m, const uint64_t* tp, int n, int mode, int bound, int form, qe::SearchHitScan& H,
                    qe::SearchHit* out, int cap, uint32_t& steps) {
    qe::SearchLane L;
    qe::search_lane_init(L, m, n, mode, bound, form == 0 ? qe::SEARCH_ALL_LIVE : 0);
    H.init(L, out, 1, cap);
    if (form == 2 && L.nb <= qe::QE_SEARCH_REG_BLOCKS) {
        qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS> st;
        for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { st.pv[b] = st.mv[b] = 0; st.s[b] = 0; }
        st.load(pp, m);
        qe::search_run_hits<qe::QE_SEARCH_REG_BLOCKS>(st, L, H, tp, 0);
    } else {
        std::vector<uint64_t> pv((size_t)L.nb, 0x5a5a5a5a5a5a5a5aull), mv((size_t)L.nb, 0xa5a5a5a5a5a5a5a5ull);     // (stale state must never be read)
        std::vector<int32_t> s((size_t)L.nb, -12345);
        qe::SearchWsStore st{pv.data(), mv.data(), s.data(), 1, pp, m};
        qe::search_run_hits<0>(st, L, H, tp, 0);
    }
    steps = L.steps;
}

// the start of one occurrence: the PREFIX form over the reversed planes, the largest end, on the window that ends at `end`
static int32_t start_of(const uint64_t* pr, int m, const uint64_t* tr, int n, int end, int score, int form) {
    const int w = qe::search_hit_window(m, end, score);
    qe::SearchLane L;
    qe::search_lane_init(L, m, w, qe::SEARCH_PREFIX, score, qe::SEARCH_LARGEST_END | (form == 0 ? qe::SEARCH_ALL_LIVE : 0));
    if (form == 2 && L.nb <= qe::QE_SEARCH_REG_BLOCKS) {
        qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS> st;
        for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { st.pv[b] = st.mv[b] = 0; st.s[b] = 0; }
        st.load(pr, m);
        qe::search_run<qe::QE_SEARCH_REG_BLOCKS>(st, L, tr, (int64_t)n - end);
    } else {
        std::vector<uint64_t> pv((size_t)L.nb, 0), mv((size_t)L.nb, 0);
        std::vector<int32_t> s((size_t)L.nb, 0);
        qe::SearchWsStore st{pv.data(), mv.data(), s.data(), 1, pr, m};
        qe::search_run<0>(st, L, tr, (int64_t)n - end);
    }
    int32_t s2, e2;
    qe::search_answer(L, s2, e2);
    return s2 == score ? end - e2 : -99;
}

template <typename T> static std::vector<T> slurp(const std::string& path) {
    std::vector<T> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); return v; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (bytes > 0 && fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<int32_t> plen = slurp<int32_t>(d + "plen.i32"), tlen = slurp<int32_t>(d + "tlen.i32"), bound = slurp<int32_t>(d + "bound.i32"),
                               mode = slurp<int32_t>(d + "mode.i32"), form = slurp<int32_t>(d + "form.i32"), cap = slurp<int32_t>(d + "cap.i32");
    const std::vector<int64_t> poff = slurp<int64_t>(d + "poff.i64"), toff = slurp<int64_t>(d + "toff.i64");
    const std::vector<char> ppool = slurp<char>(d + "ppool.bin"), tpool = slurp<char>(d + "tpool.bin");
    const size_t n = plen.size();
    if (n == 0 || tlen.size() != n || bound.size() != n || mode.size() != n || form.size() != n || cap.size() != n || poff.size() != n || toff.size() != n) return 3;
    std::vector<int32_t> out;
    for (size_t i = 0; i < n; ++i) {
        const char* p = ppool.data() + poff[i];
        const char* t = tpool.data() + toff[i];
        const int m = plen[i], tn = tlen[i];
        const std::vector<uint64_t> pp = planes_of(p, m, false), tp = planes_of(t, tn, false);
        const int room = cap[i] < tn ? cap[i] : tn;                      // (a text of n columns has at most n occurrences)
        std::vector<qe::SearchHit> sink((size_t)room + 1, qe::SearchHit{-77, -77});
        qe::SearchHitScan H;
        uint32_t steps = 0;
        forward(pp.data(), m, tp.data(), tn, mode[i], bound[i], form[i], H, sink.data(), room, steps);
        if (sink[(size_t)room].end != -77 || sink[(size_t)room].score != -77 || H.sink.count > room) { fprintf(stderr, "entry %zu: a write past the sink's capacity\n", i); return 5; }
        out.push_back(H.found); out.push_back(H.best); out.push_back(H.sink.count); out.push_back((int32_t)steps);
        std::vector<uint64_t> pr, tr;
        if (mode[i] == qe::SEARCH_INFIX && H.sink.count) { pr = planes_of(p, m, true); tr = planes_of(t, tn, true); }
        for (int h = 0; h < H.sink.count; ++h) {
            const qe::SearchHit x = sink[(size_t)h];
            out.push_back(mode[i] == qe::SEARCH_PREFIX ? 0 : start_of(pr.data(), m, tr.data(), tn, x.end, x.score, form[i]));
            out.push_back(x.end); out.push_back(x.score);
        }
    }
    FILE* f = fopen((d + "out.i32").c_str(), "wb");
    if (!f || fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) return 4;
    fclose(f);
    printf("search hits ok: %zu entries\n", n);
    return 0;
}
