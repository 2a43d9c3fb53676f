// Alignment tags (quicked_batch_configure_tags) on the HOST, under sanitizers: the library's host layer built with g++
// against the fake HIP runtime of tests/native/hip_stub.  The stub's traceback leaves no runs, so every alignment is the
// empty operation sequence -- statistics of zeros, MD "0" -- which the host stand-ins of the tag kernels (qe_stages.hip:
// the walker of qe_tags.h) produce; what is checked is the host side around them: the pools and offsets of both branches
// of fetch_alignments (few alignments: one copy launch; many: the arrays and one D2H of the MD pool), the getters' rules,
// NO_CIGAR, and that tags 0 leaves no tag data; and the validator's entry points (validator_scenario).  Built and run by tests/test_host_tags.py with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "quicked.h"
#include "quicked_batch.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "tags_host: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

struct Pairs { std::string pp, tp; std::vector<int64_t> po, to; std::vector<int32_t> pl, tl; int64_t n = 0; };
static Pairs make_pairs(int n, int len) {
    Pairs P;
    P.n = n;
    unsigned x = 777;
    for (int i = 0; i < n; ++i) {
        const int l = (i % 7 == 3) ? 0 : len + i % 5;                       // some empty patterns: pairs without an alignment
        P.po.push_back((int64_t)P.pp.size()); P.to.push_back((int64_t)P.tp.size());
        for (int k = 0; k < l; ++k) { x = x * 1664525u + 1013904223u; P.pp.push_back("ACGT"[x >> 30]); }
        for (int k = 0; k < len; ++k) { x = x * 1664525u + 1013904223u; P.tp.push_back("ACGT"[x >> 30]); }
        P.pl.push_back(l); P.tl.push_back(len);
    }
    return P;
}

static void expect_no_tag_data(quicked_batch_t* b, int64_t n) {
    std::vector<quicked_pair_stats_t> st((size_t)n);
    std::vector<int64_t> off((size_t)n);
    CHECK(quicked_batch_pair_stats(b, st.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_md(b, nullptr, off.data()) == QUICKED_ERROR);
    CHECK(quicked_batch_md_bytes(b) == 0);
}

static void scenario(int n, int len, int algo) {
    const Pairs P = make_pairs(n, len);
    quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
    CHECK(b);
    quicked_params_t p = quicked_default_params();
    p.algo = (quicked_algo_t)algo;
    std::vector<int32_t> sc0((size_t)n), st0((size_t)n), sc((size_t)n), st((size_t)n);
    std::vector<int64_t> coff((size_t)n), moff((size_t)n);
    std::vector<quicked_pair_stats_t> ps((size_t)n);
    // tags 0
    CHECK(quicked_batch_run(b, &p, 1) >= 0);
    CHECK(quicked_batch_scores(b, sc0.data(), st0.data()) >= 0);
    const int64_t cigar_bytes = quicked_batch_cigar_bytes(b);
    CHECK(cigar_bytes > 0);
    expect_no_tag_data(b, n);
    // unknown bits; a queued run that aligns
    CHECK(quicked_batch_configure_tags(b, 8) == QUICKED_ERROR);
    CHECK(quicked_batch_configure_tags(b, QUICKED_TAG_STATS | QUICKED_TAG_MD) == QUICKED_OK);
    CHECK(quicked_batch_run(b, &p, 0) == QUICKED_UNIMPLEMENTED);
    // STATS | MD, then the same with NO_CIGAR
    for (int pass = 0; pass < 2; ++pass) {
        CHECK(quicked_batch_configure_tags(b, QUICKED_TAG_STATS | QUICKED_TAG_MD | (pass ? QUICKED_TAG_NO_CIGAR : 0)) == QUICKED_OK);
        CHECK(quicked_batch_run(b, &p, 1) >= 0);
        CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);
        CHECK(sc == sc0 && st == st0);
        CHECK(quicked_batch_cigar_bytes(b) == (pass ? 0 : cigar_bytes));
        std::vector<char> cpool((size_t)cigar_bytes + 1);
        CHECK(quicked_batch_cigars(b, cpool.data(), coff.data()) >= 0);
        CHECK(quicked_batch_pair_stats(b, ps.data()) == QUICKED_OK);
        const int64_t mb = quicked_batch_md_bytes(b);
        std::vector<char> mpool((size_t)mb + 1);
        CHECK(quicked_batch_md(b, mpool.data(), moff.data()) == QUICKED_OK);
        int64_t aligned = 0;
        for (int64_t i = 0; i < n; ++i) {
            const bool has = st[(size_t)i] >= 0;
            const quicked_pair_stats_t& s = ps[(size_t)i];
            if (pass) CHECK(coff[(size_t)i] == -1);
            if (!has) { CHECK(s.matches == -1 && s.columns == -1 && s.longest_match == -1 && moff[(size_t)i] == -1); continue; }
            ++aligned;
            CHECK(s.matches == 0 && s.mismatches == 0 && s.ins_bases == 0 && s.del_bases == 0 && s.ins_runs == 0 && s.del_runs == 0 &&
                  s.longest_match == 0 && s.columns == 0);
            CHECK(moff[(size_t)i] >= 0 && moff[(size_t)i] + 2 <= mb && strcmp(mpool.data() + moff[(size_t)i], "0") == 0);
        }
        CHECK(aligned > 0 && aligned < n && mb == 2 * aligned);
    }
    // an only_score run and a tags-0 run leave no tag data; a tags-0 queued run works again
    p.only_score = true;
    CHECK(quicked_batch_run(b, &p, 1) >= 0);
    expect_no_tag_data(b, n);
    p.only_score = false;
    CHECK(quicked_batch_configure_tags(b, 0) == QUICKED_OK);
    CHECK(quicked_batch_run(b, &p, 0) >= 0 && quicked_batch_fetch(b) >= 0);
    CHECK(quicked_batch_scores(b, sc.data(), st.data()) >= 0);      // (the stub's queued flows give other stand-in scores)
    expect_no_tag_data(b, n);
    quicked_batch_destroy(b);
}

// The validator's host stand-ins run the walk of qe_check.h (tests/native/hip_stub/qe_kernels_stub.h), so the host-only build
// gives real verdicts: quicked_batch_validate end to end -- pool and offsets up, verdicts down -- and the in-run form on the
// stub's alignments, which have no runs and so consume nothing.
static void validator_scenario() {
    const char* pat[] = {"ACGTACG", "ACGT", "ACGT", "ACGTACG", "ACG", "ACGTACG", "ACGTACGTAC"};
    const char* txt[] = {"ACGTACG", "ACGA", "ACGA", "ACGTACG", "ACGG", "ACGTACG", "ACGTACGTAC"};
    const char* str[] = {"7M", "3M1X", "4M", nullptr, "3M1I", "2147483647I2147483647I2I7M", "0000000010="};
    const int32_t want[] = {1, 1, 0, -1, 1, 0, 1};
    const int n = 7;
    Pairs P;
    P.n = n;
    std::string pool;
    std::vector<int64_t> off;
    for (int i = 0; i < n; ++i) {
        P.po.push_back((int64_t)P.pp.size()); P.to.push_back((int64_t)P.tp.size());
        P.pp += pat[i]; P.tp += txt[i];
        P.pl.push_back((int32_t)strlen(pat[i])); P.tl.push_back((int32_t)strlen(txt[i]));
        if (!str[i]) { off.push_back(-1); continue; }
        off.push_back((int64_t)pool.size());
        pool.append(str[i]); pool.push_back('\0');
    }
    quicked_batch_t* b = quicked_batch_create(P.n, P.pp.data(), P.po.data(), P.pl.data(), P.tp.data(), P.to.data(), P.tl.data());
    CHECK(b);
    std::vector<int32_t> ok((size_t)n, 7);
    CHECK(quicked_batch_validate(b, pool.data(), (int64_t)pool.size(), off.data(), ok.data()) == QUICKED_OK);
    for (int i = 0; i < n; ++i) CHECK(ok[(size_t)i] == want[i]);
    // the last terminator left out; an offset at the end of the pool: an error that writes nothing
    CHECK(quicked_batch_validate(b, pool.data(), (int64_t)pool.size() - 1, off.data(), ok.data()) == QUICKED_OK);
    for (int i = 0; i < n; ++i) CHECK(ok[(size_t)i] == want[i]);
    std::fill(ok.begin(), ok.end(), 7);
    off[2] = (int64_t)pool.size();
    CHECK(quicked_batch_validate(b, pool.data(), (int64_t)pool.size(), off.data(), ok.data()) == QUICKED_ERROR);
    for (int i = 0; i < n; ++i) CHECK(ok[(size_t)i] == 7);
    // in-run: an alignment without operations is valid for no pair that has bases
    quicked_params_t p = quicked_default_params();
    p.algo = BANDED;
    CHECK(quicked_batch_configure(b, 0, 1) == QUICKED_OK);
    CHECK(quicked_batch_run(b, &p, 1) >= 0);
    CHECK(quicked_batch_check_results(b, ok.data()) == QUICKED_OK);
    for (int i = 0; i < n; ++i) CHECK(ok[(size_t)i] == 0);
    quicked_batch_destroy(b);
}

int main() {
    CHECK(quicked_batch_configure_tags(nullptr, 1) == QUICKED_ERROR);
    validator_scenario();
    for (int algo : {(int)QUICKED, (int)BANDED, (int)WINDOWED, (int)HIRSCHBERG}) {
        scenario(5, 300, algo);             // few alignments: everything in one copy launch
        scenario(9000, 120, algo);          // many: the per-root arrays, then one D2H of the MD pool
    }
    printf("tags_host ok\n");
    return 0;
}
