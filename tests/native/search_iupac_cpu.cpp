// search_iupac_cpu.cpp -- the IUPAC equality of search runs compiled for the host: the table and the two plane producers of
// quicked_amd/csrc/qe_iupac.h, and the recurrence of qe_search.h under SearchEqIupac -- the very source k_search<NB, Eq> and
// k_search_hits<NB, Eq> run per lane -- driven task by task through the stage's steps.  A stand-alone program, built by
// tests/test_search_iupac_cpu.py once plain and once with -fsanitize=address,undefined.
//
// search_iupac_cpu table <file>       256 x 2 bytes: iupac_mask(c, false), iupac_mask(c, true)
// search_iupac_cpu producers          the scalar packer against three planes -> four planes over ACGTN, forward and reversed,
//                                     both text tables; bits past the end; prints "producers ok"
// search_iupac_cpu search <dir>       {plen,tlen,bound,mode,form,flag,cap}.i32, {poff,toff}.i64, {ppool,tpool}.bin -> <dir>/out.i32
//   flag: 0 the library's equality over three planes, 16 QUICKED_SEARCH_IUPAC, 32 QUICKED_SEARCH_IUPAC_PATTERN
//   form: 0 the workspace store with every block live, 1 the workspace store with the live-block rule, 2 the register store
//         with the rule (patterns of up to QE_SEARCH_REG_BLOCKS blocks; longer ones: as 1)
//   cap 0: the best search -- score, text_start, text_end, block steps of the forward pass
//   cap > 0: every occurrence -- found, best score, stored, block steps, then stored x {text_start, text_end, score}; the sink
//         has exactly min(cap, tlen) entries and a guard behind them
// Plane buffers hold exactly ceil(len / 64) rows: the recurrence must not read beyond them.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "qe_search.h"

// three planes with the library's symbol rule (case folded, every non-ACGT byte one symbol) in the packed batches' codes
// A 0, C 1, G 2, T 3 -- what iupac_from_planes3 reads
static std::vector<uint64_t> planes3_of(const char* s, int len, bool reverse) {
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
// four planes from the packer, cut to the rows of the sequence
static std::vector<uint64_t> planes4_of(const char* s, int len, bool reverse, bool acgt_only) {
    std::vector<uint64_t> full((size_t)qe::iupac_words(len));
    qe::iupac_pack(reinterpret_cast<const uint8_t*>(s), len, reverse, acgt_only, full.data());
    full.resize((size_t)4 * (size_t)((len + 63) / 64));
    return std::vector<uint64_t>(full.begin(), full.end());      // a tight allocation
}

template <class Eq> struct Planes;
template <> struct Planes<qe::SearchEq3> {
    static std::vector<uint64_t> of(const char* s, int len, bool reverse, bool) { return planes3_of(s, len, reverse); }
};
template <> struct Planes<qe::SearchEqIupac> {
    static std::vector<uint64_t> of(const char* s, int len, bool reverse, bool acgt_only) { return planes4_of(s, len, reverse, acgt_only); }
};

// one pass of the best search in the given form; exactly the blocks of the pattern as workspace
template <class Eq>
static void one_pass(const uint64_t* pp, int m, const uint64_t* tp, int64_t tbit, int n, int mode, int bound, int flags, int form,
                     int32_t& score, int32_t& end, uint32_t& steps) {
    qe::SearchLane L;
    qe::search_lane_init(L, m, n, mode, bound, flags | (form == 0 ? qe::SEARCH_ALL_LIVE : 0));
    if (form == 2 && L.nb <= qe::QE_SEARCH_REG_BLOCKS) {
        qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS, Eq> st;
        for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { st.pv[b] = st.mv[b] = 0; st.s[b] = 0; }
        st.load(pp, m);
        qe::search_run<qe::QE_SEARCH_REG_BLOCKS>(st, L, tp, tbit);
    } else {
        std::vector<uint64_t> pv((size_t)L.nb, 0x5a5a5a5a5a5a5a5aull), mv((size_t)L.nb, 0xa5a5a5a5a5a5a5a5ull);     // (stale state must never be read)
        std::vector<int32_t> s((size_t)L.nb, -12345);
        qe::SearchWsStoreOf<Eq> st{pv.data(), mv.data(), s.data(), 1, pp, m};
        qe::search_run<0>(st, L, tp, tbit);
    }
    qe::search_answer(L, score, end);
    steps = L.steps;
}

template <class Eq>
static void locate(const char* p, int m, const char* t, int n, int mode, int bound, int form, bool text_acgt, std::vector<int32_t>& out) {
    const std::vector<uint64_t> pp = Planes<Eq>::of(p, m, false, false), tp = Planes<Eq>::of(t, n, false, text_acgt);
    int32_t score = -1, end = -1, start = -1;
    uint32_t steps = 0;
    one_pass<Eq>(pp.data(), m, tp.data(), 0, n, mode, bound, 0, form, score, end, steps);
    if (score >= 0) {
        if (mode == qe::SEARCH_PREFIX) start = 0;
        else {
            const std::vector<uint64_t> pr = Planes<Eq>::of(p, m, true, false), tr = Planes<Eq>::of(t, n, true, text_acgt);
            int32_t s2 = -1, e2 = -1;
            uint32_t st2 = 0;
            one_pass<Eq>(pr.data(), m, tr.data(), (int64_t)n - end, end, qe::SEARCH_PREFIX, score, qe::SEARCH_LARGEST_END, form, s2, e2, st2);
            start = (s2 == score) ? end - e2 : -99;
        }
    }
    out.push_back(score); out.push_back(start); out.push_back(end); out.push_back((int32_t)steps);
}

template <class Eq>
static bool all_hits(const char* p, int m, const char* t, int n, int mode, int bound, int form, int cap, bool text_acgt, std::vector<int32_t>& out) {
    const std::vector<uint64_t> pp = Planes<Eq>::of(p, m, false, false), tp = Planes<Eq>::of(t, n, false, text_acgt);
    const int room = cap < n ? cap : n;
    std::vector<qe::SearchHit> sink((size_t)room + 1, qe::SearchHit{-77, -77});
    qe::SearchLane L;
    qe::search_lane_init(L, m, n, mode, bound, form == 0 ? qe::SEARCH_ALL_LIVE : 0);
    qe::SearchHitScan H;
    H.init(L, sink.data(), 1, room);
    if (form == 2 && L.nb <= qe::QE_SEARCH_REG_BLOCKS) {
        qe::SearchRegStore<qe::QE_SEARCH_REG_BLOCKS, Eq> st;
        for (int b = 0; b < qe::QE_SEARCH_REG_BLOCKS; ++b) { st.pv[b] = st.mv[b] = 0; st.s[b] = 0; }
        st.load(pp.data(), m);
        qe::search_run_hits<qe::QE_SEARCH_REG_BLOCKS>(st, L, H, tp.data(), 0);
    } else {
        std::vector<uint64_t> pv((size_t)L.nb, 0x5a5a5a5a5a5a5a5aull), mv((size_t)L.nb, 0xa5a5a5a5a5a5a5a5ull);
        std::vector<int32_t> s((size_t)L.nb, -12345);
        qe::SearchWsStoreOf<Eq> st{pv.data(), mv.data(), s.data(), 1, pp.data(), m};
        qe::search_run_hits<0>(st, L, H, tp.data(), 0);
    }
    if (sink[(size_t)room].end != -77 || sink[(size_t)room].score != -77 || H.sink.count > room) return false;
    out.push_back(H.found); out.push_back(H.best); out.push_back(H.sink.count); out.push_back((int32_t)L.steps);
    std::vector<uint64_t> pr, tr;
    if (mode == qe::SEARCH_INFIX && H.sink.count) { pr = Planes<Eq>::of(p, m, true, false); tr = Planes<Eq>::of(t, n, true, text_acgt); }
    for (int h = 0; h < H.sink.count; ++h) {
        const qe::SearchHit x = sink[(size_t)h];
        int32_t start = 0;
        if (mode == qe::SEARCH_INFIX) {
            const int w = qe::search_hit_window(m, x.end, x.score);
            int32_t s2 = -1, e2 = -1;
            uint32_t st2 = 0;
            one_pass<Eq>(pr.data(), m, tr.data(), (int64_t)n - x.end, w, qe::SEARCH_PREFIX, x.score, qe::SEARCH_LARGEST_END, form, s2, e2, st2);
            start = s2 == x.score ? x.end - e2 : -99;
        }
        out.push_back(start); out.push_back(x.end); out.push_back(x.score);
    }
    return true;
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

static int do_table(const char* path) {
    uint8_t out[512];
    for (int c = 0; c < 256; ++c) { out[2 * c] = (uint8_t)qe::iupac_mask((uint32_t)c, false); out[2 * c + 1] = (uint8_t)qe::iupac_mask((uint32_t)c, true); }
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(out, 1, sizeof out, f) != sizeof out) return 4;
    fclose(f);
    printf("table ok\n");
    return 0;
}

static int do_producers() {
    static const int lens[] = {1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4097};
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int len : lens) {
        std::string s((size_t)len, 'A');
        for (int i = 0; i < len; ++i) { x = x * 6364136223846793005ull + 1442695040888963407ull; s[(size_t)i] = "ACGTN"[(x >> 33) % 5]; }
        s[(size_t)len - 1] = 'N';                                 // the last base of the last row: the mask's edge
        for (int reverse = 0; reverse < 2; ++reverse)
            for (int text_acgt = 0; text_acgt < 2; ++text_acgt) {
                const size_t nw = (size_t)qe::iupac_words(len), rows = (size_t)((len + 63) / 64);
                std::vector<uint64_t> a(nw, ~(uint64_t)0), b(nw, ~(uint64_t)0);
                qe::iupac_pack(reinterpret_cast<const uint8_t*>(s.data()), len, reverse != 0, text_acgt != 0, a.data());
                // the three planes with garbage at and past the sequence's end: the derivation masks to the length
                std::vector<uint64_t> p3 = planes3_of(s.data(), len, reverse != 0);
                if (len & 63) for (int k = 0; k < 3; ++k) p3[3 * (rows - 1) + (size_t)k] |= ~(uint64_t)0 << (len & 63);
                qe::iupac_from_planes3(p3.data(), len, text_acgt != 0, b.data());
                if (a != b) { fprintf(stderr, "producers differ: len %d reverse %d acgt_only %d\n", len, reverse, text_acgt); return 6; }
                for (size_t r = 0; r < nw / 4; ++r)
                    for (int k = 0; k < 4; ++k) {
                        const uint64_t w = a[4 * r + (size_t)k];
                        const int valid = r < rows ? (len - 64 * (int)r < 64 ? len - 64 * (int)r : 64) : 0;
                        if (valid < 64 && (w >> valid)) { fprintf(stderr, "bits past the end: len %d row %zu\n", len, r); return 7; }
                    }
                // every base is in exactly the planes of its set
                for (int i = 0; i < len; ++i) {
                    const uint32_t want = qe::iupac_mask((uint8_t)s[(size_t)(reverse ? len - 1 - i : i)], text_acgt != 0);
                    uint32_t got = 0;
                    for (int k = 0; k < 4; ++k) got |= (uint32_t)((a[4 * (size_t)(i >> 6) + (size_t)k] >> (i & 63)) & 1) << k;
                    if (got != want) { fprintf(stderr, "base %d of %d: planes %u, table %u\n", i, len, got, want); return 8; }
                }
            }
    }
    printf("producers ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "table")) return do_table(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "producers")) return do_producers();
    if (argc != 3 || strcmp(argv[1], "search")) return 2;
    const std::string d = std::string(argv[2]) + "/";
    const std::vector<int32_t> plen = slurp<int32_t>(d + "plen.i32"), tlen = slurp<int32_t>(d + "tlen.i32"), bound = slurp<int32_t>(d + "bound.i32"),
                               mode = slurp<int32_t>(d + "mode.i32"), form = slurp<int32_t>(d + "form.i32"), flag = slurp<int32_t>(d + "flag.i32"),
                               cap = slurp<int32_t>(d + "cap.i32");
    const std::vector<int64_t> poff = slurp<int64_t>(d + "poff.i64"), toff = slurp<int64_t>(d + "toff.i64");
    const std::vector<char> ppool = slurp<char>(d + "ppool.bin"), tpool = slurp<char>(d + "tpool.bin");
    const size_t n = plen.size();
    if (n == 0 || tlen.size() != n || bound.size() != n || mode.size() != n || form.size() != n || flag.size() != n || cap.size() != n ||
        poff.size() != n || toff.size() != n) return 3;
    std::vector<int32_t> out;
    for (size_t i = 0; i < n; ++i) {
        const char* p = ppool.data() + poff[i];
        const char* t = tpool.data() + toff[i];
        bool ok = true;
        if (flag[i] == 0) {
            if (cap[i] == 0) locate<qe::SearchEq3>(p, plen[i], t, tlen[i], mode[i], bound[i], form[i], false, out);
            else ok = all_hits<qe::SearchEq3>(p, plen[i], t, tlen[i], mode[i], bound[i], form[i], cap[i], false, out);
        } else if (flag[i] == 16 || flag[i] == 32) {
            if (cap[i] == 0) locate<qe::SearchEqIupac>(p, plen[i], t, tlen[i], mode[i], bound[i], form[i], flag[i] == 32, out);
            else ok = all_hits<qe::SearchEqIupac>(p, plen[i], t, tlen[i], mode[i], bound[i], form[i], cap[i], flag[i] == 32, out);
        } else return 3;
        if (!ok) { fprintf(stderr, "entry %zu: a write past the sink's capacity\n", i); return 5; }
    }
    FILE* f = fopen((d + "out.i32").c_str(), "wb");
    if (!f || fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) return 4;
    fclose(f);
    printf("search ok: %zu entries\n", n);
    return 0;
}
