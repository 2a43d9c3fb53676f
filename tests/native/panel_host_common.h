// What the host programs of the panel runs (search_panel_host.cpp, panel_*_host.cpp) share: the headers, CHECK -- it names the
// program through PANEL_HOST_NAME, which the program defines before it includes this file --, and the helpers that were the same
// text in every one of them.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quicked.h"
#include "quicked_batch.h"

extern "C" quicked_status_t quicked_debug_reload_env(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, PANEL_HOST_NAME ": %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

// sequences as the batch and panel calls take them: one pool of bytes, offsets and lengths
struct Pool { std::string bytes; std::vector<int64_t> off; std::vector<int32_t> len; };
static inline Pool pool_of(const std::vector<std::string>& seqs) {
    Pool P;
    for (const std::string& s : seqs) { P.off.push_back((int64_t)P.bytes.size()); P.len.push_back((int32_t)s.size()); P.bytes += s; }
    P.bytes.push_back('\0');
    return P;
}
// a switch of the library set (v null: unset) and read again
static inline void set_env(const char* name, const char* v) {
    if (v) setenv(name, v, 1); else unsetenv(name);
    CHECK(quicked_debug_reload_env() >= 0);
}
// counter [0]: the block steps of the last run
static inline int64_t steps_of(quicked_batch_t* b) {
    int64_t c[8];
    CHECK(quicked_batch_counters(b, c) >= 0);
    return c[0];
}
// the strings of the last QUICKED_PANEL_CIGARS run, one per stored occurrence; the getter writes nothing past what it reports
static inline std::vector<std::string> strings_of(quicked_batch_t* b) {
    const int64_t bytes = quicked_batch_panel_hit_cigar_bytes(b), total = quicked_batch_panel_hit_total(b);
    CHECK(bytes >= 0 && total >= 0);
    std::vector<char> pool((size_t)bytes + 1, 'Z');
    std::vector<int64_t> off((size_t)total + 1, -7);
    CHECK(quicked_batch_panel_hit_cigars(b, pool.data(), off.data()) == QUICKED_OK);
    CHECK(quicked_batch_panel_hit_cigars(b, nullptr, nullptr) == QUICKED_OK);
    CHECK(pool[(size_t)bytes] == 'Z' && off[(size_t)total] == -7);
    std::vector<std::string> out;
    for (int64_t j = 0; j < total; ++j) {
        CHECK(off[(size_t)j] >= 0 && off[(size_t)j] < bytes);
        CHECK(memchr(pool.data() + off[(size_t)j], 0, (size_t)(bytes - off[(size_t)j])) != nullptr);
        out.emplace_back(pool.data() + off[(size_t)j]);
    }
    return out;
}
