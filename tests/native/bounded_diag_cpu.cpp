// bounded_diag_cpu.cpp -- the diagonal-word recurrence of quicked_amd/csrc/qe_bounded.h compiled for the host: the very
// source k_bounded_diag runs per lane, driven pair by pair.  Built by tests/test_bounded_cpu.py -- as a shared library, and
// with -DBD_MAIN -fsanitize=address,undefined as a program that reads its cases from files -- and compared against edlib there.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "qe_bounded.h"

// ASCII -> planes with the library's symbol rule (case folded, every non-ACGT byte one symbol); exactly ceil(len / 64)
// rows, no padding: the recurrence must not read beyond them
static std::vector<uint64_t> planes_of(const char* s, int len) {
    std::vector<uint64_t> pl((size_t)3 * (size_t)((len + 63) / 64), 0);
    for (int i = 0; i < len; ++i) {
        int code;
        switch (s[i]) {
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

extern "C" {

int bd_max_bound(void) { return qe::QE_BOUNDED_DIAG_MAX; }

int bd_takes(int bound, int m, int n) { return (m >= 1 && n >= 1 && bound >= 0 && qe::bounded_diag_takes(bound, m, n)) ? 1 : 0; }

// the pair's distance if it is <= bound, -1 if it is beyond, -2 if the kernel's precondition does not admit the pair
int bd_distance(const char* p, int m, const char* t, int n, int bound) {
    if (!bd_takes(bound, m, n)) return -2;
    const std::vector<uint64_t> pp = planes_of(p, m), tp = planes_of(t, n);
    return qe::bounded_diag_pair(pp.data(), m, tp.data(), n, bound);
}

// the same for npairs pairs laid out back to back (offsets in bytes), one bound each
void bd_distance_batch(int npairs, const char* ppool, const int64_t* poff, const int32_t* plen,
                       const char* tpool, const int64_t* toff, const int32_t* tlen, const int32_t* bound, int32_t* out) {
    for (int i = 0; i < npairs; ++i) out[i] = bd_distance(ppool + poff[i], plen[i], tpool + toff[i], tlen[i], bound[i]);
}

}

#ifdef BD_MAIN
// bounded_diag <dir>: the arrays of bd_distance_batch from <dir>/{plen,tlen,bound}.i32, {poff,toff}.i64, {ppool,tpool}.bin;
// the results to <dir>/out.i32
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
    const std::vector<int32_t> plen = slurp<int32_t>(d + "plen.i32"), tlen = slurp<int32_t>(d + "tlen.i32"), bound = slurp<int32_t>(d + "bound.i32");
    const std::vector<int64_t> poff = slurp<int64_t>(d + "poff.i64"), toff = slurp<int64_t>(d + "toff.i64");
    const std::vector<char> ppool = slurp<char>(d + "ppool.bin"), tpool = slurp<char>(d + "tpool.bin");
    const size_t n = plen.size();
    if (n == 0 || tlen.size() != n || bound.size() != n || poff.size() != n || toff.size() != n) return 3;
    std::vector<int32_t> out(n, -7);
    bd_distance_batch((int)n, ppool.data(), poff.data(), plen.data(), tpool.data(), toff.data(), tlen.data(), bound.data(), out.data());
    FILE* f = fopen((d + "out.i32").c_str(), "wb");
    if (!f || fwrite(out.data(), sizeof(int32_t), n, f) != n) return 4;
    fclose(f);
    printf("bounded_diag ok: %zu entries\n", n);
    return 0;
}
#endif
