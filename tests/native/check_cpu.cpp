// The CIGAR validator of quicked_amd/csrc/qe_check.h -- the source k_check_strings and k_check_segs run per lane -- compiled
// for the host and driven over cases from a file (tests/test_check_cpu.py writes it and checks the verdicts against its own
// restatement of the rules, tests/check_lib.py).  A stand-alone program, so that the same cases run under the sanitizers:
// every pattern, text and string lies in a heap block of exactly its size, so a read outside a pair is an error, not luck.
//
//   check_cpu <cases> <results>        ("-" for <cases>: standard input)
// cases:   "<ncases>", then per case one of
//          "S <pattern> <text> <string>"          a string case; all three as hex, "-" = empty
//          "G <pattern> <text> <nsegments>"       a segment case, then per segment
//              "L <op> <len>"                     a literal segment (kind 1)
//              "R <n> <r0> ... <rn-1>"            a leaf: n runs, packed len << 2 | op, stored back to front
//              "B"                                a leaf whose run buffer overflowed (nruns = -1)
// results: per case its verdict, 1 or 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qe_check.h"

using namespace qe;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "check_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

static int hexval(char ch) { return ch <= '9' ? ch - '0' : ch - 'a' + 10; }

// a hex word -> a malloc'ed block of exactly its bytes (+ extra zero bytes: a string's terminator); *len = the bytes
static uint8_t* read_block(FILE* f, size_t extra, size_t* len) {
    char* w = nullptr;
    CHECK(fscanf(f, " %ms", &w) == 1);
    const size_t n = strcmp(w, "-") == 0 ? 0 : strlen(w) / 2;
    uint8_t* b = (uint8_t*)malloc(n + extra);
    CHECK(b || n + extra == 0);
    for (size_t k = 0; k < n; ++k) b[k] = (uint8_t)(hexval(w[2 * k]) * 16 + hexval(w[2 * k + 1]));
    for (size_t k = 0; k < extra; ++k) b[n + k] = 0;
    free(w);
    *len = n;
    return b;
}

struct Segments {
    std::vector<int64_t> seg_off;                 // one alignment: {0, nseg}
    std::vector<int32_t> kind, a, b, nruns;
    std::vector<uint32_t*> runs;                  // per leaf task, a block of exactly its runs
};
struct Runs {                                     // what check_walk_segments reads a leaf's runs through
    const Segments& s; const uint32_t* base = nullptr;
    void open(int t) { base = s.runs[(size_t)t]; }
    uint32_t at(int k) const { return base[k]; }
};

static void read_segments(FILE* f, int nseg, Segments& s) {
    s.seg_off = {0, nseg};
    for (int q = 0; q < nseg; ++q) {
        char tag = 0;
        CHECK(fscanf(f, " %c", &tag) == 1);
        if (tag == 'L') {
            int op = 0, len = 0;
            CHECK(fscanf(f, "%d %d", &op, &len) == 2);
            s.kind.push_back(1); s.a.push_back(op); s.b.push_back(len);
            continue;
        }
        s.kind.push_back(0); s.a.push_back((int32_t)s.runs.size()); s.b.push_back(0);
        if (tag == 'B') { s.runs.push_back(nullptr); s.nruns.push_back(-1); continue; }
        CHECK(tag == 'R');
        int n = 0;
        CHECK(fscanf(f, "%d", &n) == 1 && n >= 0);
        uint32_t* r = (uint32_t*)malloc((size_t)n * sizeof(uint32_t));
        for (int k = 0; k < n; ++k) CHECK(fscanf(f, "%u", &r[k]) == 1);
        s.runs.push_back(r); s.nruns.push_back(n);
    }
}

int main(int argc, char** argv) {
    CHECK(argc == 3);
    FILE* in = strcmp(argv[1], "-") == 0 ? stdin : fopen(argv[1], "r");
    FILE* out = fopen(argv[2], "w");
    CHECK(in && out);
    int ncases = 0;
    CHECK(fscanf(in, "%d", &ncases) == 1);
    int valid = 0;
    for (int q = 0; q < ncases; ++q) {
        char form = 0;
        CHECK(fscanf(in, " %c", &form) == 1 && (form == 'S' || form == 'G'));
        size_t m = 0, n = 0;
        uint8_t* p = read_block(in, 0, &m);
        uint8_t* t = read_block(in, 0, &n);
        AlignCheck K;
        K.ap = p; K.at = t; K.m = (int)m; K.n = (int)n;
        if (form == 'S') {
            size_t len = 0;
            char* s = (char*)read_block(in, 1, &len);
            check_walk_string(K, s);
            free(s);
        } else {
            int nseg = 0;
            CHECK(fscanf(in, "%d", &nseg) == 1 && nseg >= 0);
            Segments s;
            read_segments(in, nseg, s);
            Runs R{s};
            check_walk_segments(K, s.seg_off.data(), s.kind.data(), s.a.data(), s.b.data(), s.nruns.data(), 0, R);
            for (uint32_t* r : s.runs) free(r);
        }
        // whatever came in, the walk stays inside the pair
        CHECK(K.v >= 0 && K.v <= K.m && K.h >= 0 && K.h <= K.n);
        const int verdict = K.verdict();
        valid += verdict;
        fprintf(out, "%d\n", verdict);
        free(p); free(t);
    }
    if (in != stdin) fclose(in);
    CHECK(fclose(out) == 0);
    printf("check_cpu ok: %d cases, %d valid\n", ncases, valid);
    return 0;
}
