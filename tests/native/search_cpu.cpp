// search_cpu.cpp -- the search recurrence of quicked_amd/csrc/qe_search.h compiled for the host: the very source
// k_search<NB> runs per lane, driven task by task through the run_search stage's steps (forward pass, then for
// INFIX the PREFIX pass over the reversed sequences).  A stand-alone program, built by tests/test_search_cpu.py once plain
// and once with -fsanitize=address,undefined; it reads its cases from files and is compared with a brute-force DP and
// with edlib there.
//
// search_cpu <dir>: {plen,tlen,bound,mode,form}.i32, {poff,toff}.i64, {ppool,tpool}.bin -> <dir>/out.i32, four values per
// entry: score, text_start, text_end, block steps of the forward pass.
//   form & 3: 0 the workspace store with every block live, 1 the workspace store with the live-block rule, 2 the register
//             store with the rule (patterns of up to QE_SEARCH_REG_BLOCKS blocks; longer ones: as 1)
//   form & 8: SEARCH_LAST_COLUMN on the forward pass, no start pass (PREFIX: the global distance)
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "qe_search.h"

// ASCII -> planes with the library's symbol rule (case folded, every non-ACGT byte one symbol); exactly ceil(len / 64)
// rows, no padding: the recurrence must not read beyond them
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

// one pass in the given form; exactly the blocks of the pattern as workspace
static void one_pass(const uint64_t* pp, int m, const uint64_t* tp, int64_t tbit, int n, int mode, int bound, int flags, int form,
                     int32_t& score, int32_t& end, uint32_t& steps) {
    qe::SearchLane L;
    qe::search_lane_init(L, m, n, mode, bound, flags | (form == 0 ? qe::SEARCH_ALL_LIVE : 0));
    if (form == 2 && L.nb <= qe::QE_SEARCH_REG_BLOCKS) {
        qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS> st;
        for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { st.pv[b] = st.mv[b] = 0; st.s[b] = 0; }
        st.load(pp, m);
        qe::search_run<qe::QE_SEARCH_REG_BLOCKS>(st, L, tp, tbit);
    } else {
        std::vector<uint64_t> pv((size_t)L.nb, 0x5a5a5a5a5a5a5a5aull), mv((size_t)L.nb, 0xa5a5a5a5a5a5a5a5ull);     // (stale state must never be read)
        std::vector<int32_t> s((size_t)L.nb, -12345);
        qe::SearchWsStore st{pv.data(), mv.data(), s.data(), 1, pp, m};
        qe::search_run<0>(st, L, tp, tbit);
    }
    qe::search_answer(L, score, end);
    steps = L.steps;
}

static void locate(const char* p, int m, const char* t, int n, int mode, int bound, int form, int32_t* out) {
    const std::vector<uint64_t> pp = planes_of(p, m, false), tp = planes_of(t, n, false);
    int32_t score = -1, end = -1, start = -1;
    uint32_t steps = 0;
    const int f = form & 3;
    one_pass(pp.data(), m, tp.data(), 0, n, mode, bound, (form & 8) ? qe::SEARCH_LAST_COLUMN : 0, f, score, end, steps);
    if (score >= 0 && !(form & 8)) {
        if (mode == qe::SEARCH_PREFIX) start = 0;
        else {
            // the PREFIX form over the reversed planes, on the sub-range that ends at text_end: reversed text [n - end, n)
            const std::vector<uint64_t> pr = planes_of(p, m, true), tr = planes_of(t, n, true);
            int32_t s2 = -1, e2 = -1;
            uint32_t st2 = 0;
            one_pass(pr.data(), m, tr.data(), (int64_t)n - end, end, qe::SEARCH_PREFIX, score, qe::SEARCH_LARGEST_END, f, s2, e2, st2);
            start = (s2 == score) ? end - e2 : -99;
        }
    }
    out[0] = score; out[1] = start; out[2] = end; out[3] = (int32_t)steps;
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
                               mode = slurp<int32_t>(d + "mode.i32"), form = slurp<int32_t>(d + "form.i32");
    const std::vector<int64_t> poff = slurp<int64_t>(d + "poff.i64"), toff = slurp<int64_t>(d + "toff.i64");
    const std::vector<char> ppool = slurp<char>(d + "ppool.bin"), tpool = slurp<char>(d + "tpool.bin");
    const size_t n = plen.size();
    if (n == 0 || tlen.size() != n || bound.size() != n || mode.size() != n || form.size() != n || poff.size() != n || toff.size() != n) return 3;
    std::vector<int32_t> out(4 * n, -7);
    for (size_t i = 0; i < n; ++i)
        locate(ppool.data() + poff[i], plen[i], tpool.data() + toff[i], tlen[i], mode[i], bound[i], form[i], out.data() + 4 * i);
    FILE* f = fopen((d + "out.i32").c_str(), "wb");
    if (!f || fwrite(out.data(), sizeof(int32_t), 4 * n, f) != 4 * n) return 4;
    fclose(f);
    printf("search ok: %zu entries\n", n);
    return 0;
}
