// The alignment-tag walker of quicked_amd/csrc/qe_tags.h -- the source k_tags_segs runs per lane -- compiled for the host
// and driven over segment lists from a file (tests/test_tags_cpu.py writes it and checks the answers against its own
// restatement of the definitions).  A stand-alone program, so that the same cases also run under the sanitizers.
//
//   tags_cpu <cases> <results>
// cases:   "<ncases>", then per case "<pattern as hex, or -> <nsegments>" and per segment
//          "L <op> <len>"            a literal segment (kind 1)
//          "R <n> <r0> ... <rn-1>"   a leaf: n runs, packed len << 2 | op, stored back to front as the traceback leaves them
//          "B"                       a leaf whose run buffer overflowed (nruns = -1)
// results: per case "<ok> <8 statistics> <md length> <md as hex>"
// Every case is walked three times: counted, written with the counted length as its capacity, and written with a capacity
// three characters short; both writers work inside guard bytes that must survive.  Then a host model of the wave form's
// step (wave_model) must give the same statistics and string.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "qe_tags.h"

using namespace qe;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "tags_cpu: %s failed at line %d\n", #cond, __LINE__); exit(1); } } while (0)

struct Case {
    std::vector<uint8_t> pattern;
    std::vector<int64_t> seg_off;                 // one alignment: {0, nseg}
    std::vector<int32_t> kind, a, b, nruns;
    std::vector<std::vector<uint32_t>> runs;      // per leaf task
};
struct Runs {                                     // what tag_walk_segments reads a leaf's runs through
    const Case& c; const uint32_t* base = nullptr;
    void open(int t) { base = c.runs[(size_t)t].data(); }
    uint32_t at(int k) const { return base[k]; }
};

static int hexval(char ch) { return ch <= '9' ? ch - '0' : ch - 'a' + 10; }

static bool read_case(FILE* f, Case& c) {
    char* pat = nullptr;
    int nseg = 0;
    if (fscanf(f, " %ms %d", &pat, &nseg) != 2) return false;
    if (strcmp(pat, "-") != 0) for (size_t k = 0; pat[k] && pat[k + 1]; k += 2) c.pattern.push_back((uint8_t)(hexval(pat[k]) * 16 + hexval(pat[k + 1])));
    free(pat);
    c.seg_off = {0, nseg};
    for (int s = 0; s < nseg; ++s) {
        char tag = 0;
        CHECK(fscanf(f, " %c", &tag) == 1);
        if (tag == 'L') {
            int op = 0, len = 0;
            CHECK(fscanf(f, "%d %d", &op, &len) == 2);
            c.kind.push_back(1); c.a.push_back(op); c.b.push_back(len);
        } else {
            const int t = (int)c.runs.size();
            c.kind.push_back(0); c.a.push_back(t); c.b.push_back(0);
            c.runs.emplace_back();
            if (tag == 'B') { c.nruns.push_back(-1); continue; }
            CHECK(tag == 'R');
            int n = 0;
            CHECK(fscanf(f, "%d", &n) == 1 && n >= 0);
            for (int k = 0; k < n; ++k) { unsigned r = 0; CHECK(fscanf(f, "%u", &r) == 1); c.runs.back().push_back(r); }
            c.nruns.push_back(n);
        }
    }
    return true;
}

template <bool WRITE>
static bool walk(const Case& c, TagWalker<WRITE>& W, int64_t& md_len) {
    Runs R{c};
    const bool ok = tag_walk_segments(W, c.seg_off.data(), c.kind.data(), c.a.data(), c.b.data(), c.nruns.data(), 0, R);
    md_len = W.finish();
    return ok;
}

// writes the string with capacity `cap` into a buffer of cap + 1 bytes between guards
static std::string write_md(const Case& c, int64_t cap) {
    const size_t G = 64;
    std::vector<char> buf((size_t)cap + 1 + 2 * G, (char)0x5A);
    TagWalker<true> W;
    W.want_md = true;
    W.sink = TagSink{buf.data() + G, cap, c.pattern.data(), (int32_t)c.pattern.size()};
    int64_t len = 0;
    CHECK(walk(c, W, len));
    for (size_t k = 0; k < G; ++k) CHECK(buf[k] == (char)0x5A && buf[G + (size_t)cap + 1 + k] == (char)0x5A);
    CHECK(buf[G + (size_t)cap] == '\0');
    return std::string(buf.data() + G, (size_t)cap);
}

// A host model of k_tags_segs_wave's step (qe_kernels.hip), lane for lane: 64 consecutive runs per step as they lie --
// unmerged --, the same shuffles (an array per register, shfl_up as an index shift), the same carries from step to step.
// The kernel itself is covered on the GPU; this pins the step's arithmetic to the walker on every case of the CPU suite.
struct Lanes {
    int v[64];
    Lanes up(int d) const { Lanes r; for (int l = 0; l < 64; ++l) r.v[l] = v[l >= d ? l - d : l]; return r; }
};
static void wave_model(const Case& c, TagStats& s, std::string& md) {
    std::vector<std::pair<int, int>> runs;                                  // the sequence SegCursor yields
    for (size_t sg = 0; sg < c.kind.size(); ++sg) {
        if (c.kind[sg] == 1) { if (c.b[sg] > 0) runs.push_back({c.a[sg], c.b[sg]}); continue; }
        const std::vector<uint32_t>& r = c.runs[(size_t)c.a[sg]];
        for (int k = (int)r.size() - 1; k >= 0; --k) runs.push_back({(int)(r[(size_t)k] & 3), (int)(r[(size_t)k] >> 2)});
    }
    const int64_t total_runs = (int64_t)runs.size();
    std::vector<char> out((size_t)tag_md_bound((int32_t)c.pattern.size()) + 64, 0);
    const TagSink sink{out.data(), (int64_t)out.size() - 1, c.pattern.data(), (int32_t)c.pattern.size()};
    s = TagStats{0, 0, 0, 0, 0, 0, 0, 0};
    int64_t written = 0, v_base = 0;
    int carry_op = -1, carry_len = 0, carry_acc = 0;
    for (int64_t base = 0; base < total_runs; base += 64) {
        Lanes op, len, x, flag, a, pv, off;
        bool valid[64];
        for (int l = 0; l < 64; ++l) {
            valid[l] = base + l < total_runs;
            op.v[l] = valid[l] ? runs[(size_t)(base + l)].first : -1;
            len.v[l] = x.v[l] = valid[l] ? runs[(size_t)(base + l)].second : 0;
        }
        const Lanes left = op.up(1);
        int op_prev[64];
        for (int l = 0; l < 64; ++l) op_prev[l] = l == 0 ? carry_op : left.v[l];
        const int last = (int)std::min<int64_t>(63, total_runs - 1 - base);
        // group: segmented inclusive scan of the lengths
        for (int l = 0; l < 64; ++l) flag.v[l] = valid[l] && op.v[l] != op_prev[l];
        for (int d = 1; d < 64; d <<= 1) {
            const Lanes y = x.up(d), f = flag.up(d);
            for (int l = 0; l < 64; ++l) if (l >= d && !flag.v[l]) { x.v[l] += y.v[l]; flag.v[l] = f.v[l] != 0; }
        }
        for (int l = 0; l < 64; ++l) if (valid[l] && !flag.v[l]) x.v[l] += carry_len;
        carry_len = x.v[last];
        for (int l = 0; l < 64; ++l) {
            if (!valid[l]) continue;
            s.columns += len.v[l];
            if (op.v[l] == TAG_OP_M) { s.matches += len.v[l]; s.longest_match = std::max(s.longest_match, x.v[l]); }
            else if (op.v[l] == TAG_OP_X) s.mismatches += len.v[l];
            else if (op.v[l] == TAG_OP_I) { s.ins_bases += len.v[l]; if (op.v[l] != op_prev[l]) ++s.ins_runs; }
            else { s.del_bases += len.v[l]; if (op.v[l] != op_prev[l]) ++s.del_runs; }
        }
        // acc and v, one loop of shuffles
        bool event[64];
        for (int l = 0; l < 64; ++l) {
            event[l] = valid[l] && (op.v[l] == TAG_OP_X || op.v[l] == TAG_OP_D);
            a.v[l] = (valid[l] && op.v[l] == TAG_OP_M) ? len.v[l] : 0;
            flag.v[l] = event[l];
            pv.v[l] = (valid[l] && op.v[l] != TAG_OP_I) ? len.v[l] : 0;
        }
        for (int d = 1; d < 64; d <<= 1) {
            const Lanes y = a.up(d), f = flag.up(d), w = pv.up(d);
            for (int l = 0; l < 64; ++l) if (l >= d) { pv.v[l] += w.v[l]; if (!flag.v[l]) { a.v[l] += y.v[l]; flag.v[l] = f.v[l] != 0; } }
        }
        for (int l = 0; l < 64; ++l) if (!flag.v[l]) a.v[l] += carry_acc;
        const Lanes a_left = a.up(1);
        int acc[64], chars[64]; bool opens[64];
        for (int l = 0; l < 64; ++l) {
            acc[l] = l == 0 ? carry_acc : a_left.v[l];
            opens[l] = !(op.v[l] == TAG_OP_D && op_prev[l] == TAG_OP_D);
            chars[l] = 0;
            if (event[l]) chars[l] = (int)(op.v[l] == TAG_OP_X ? tag_md_chars_x(acc[l], len.v[l]) : (opens[l] ? tag_md_chars_d(acc[l], len.v[l]) : (int64_t)len.v[l]));
            off.v[l] = chars[l];
        }
        for (int d = 1; d < 64; d <<= 1) { const Lanes y = off.up(d); for (int l = 0; l < 64; ++l) if (l >= d) off.v[l] += y.v[l]; }
        for (int l = 0; l < 64; ++l) {
            if (!event[l]) continue;
            const int64_t q = written + (off.v[l] - chars[l]), v = v_base + (pv.v[l] - len.v[l]);
            if (op.v[l] == TAG_OP_X) sink.run_x(q, acc[l], v, len.v[l]); else sink.run_d(q, acc[l], v, len.v[l], opens[l]);
        }
        written += off.v[63]; v_base += pv.v[63];
        carry_acc = a.v[last]; carry_op = op.v[last];
    }
    written = sink.number(written, carry_acc);
    md.assign(out.data(), (size_t)written);
}

int main(int argc, char** argv) {
    CHECK(argc == 3);
    FILE* in = fopen(argv[1], "r");
    FILE* out = fopen(argv[2], "w");
    CHECK(in && out);
    int ncases = 0;
    CHECK(fscanf(in, "%d", &ncases) == 1);
    for (int q = 0; q < ncases; ++q) {
        Case c;
        CHECK(read_case(in, c));
        TagWalker<false> W;
        W.want_md = true;
        int64_t md_len = 0;
        const bool ok = walk(c, W, md_len);
        TagStats s = W.s;
        std::string md;
        if (!ok) { tag_stats_none(s); md_len = 0; }
        else {
            md = write_md(c, md_len);
            CHECK((int64_t)strlen(md.c_str()) == md_len);                     // no terminator inside, every character written
            if (md_len >= 3) { const std::string cut = write_md(c, md_len - 3); CHECK(md.compare(0, (size_t)md_len - 3, cut) == 0); }
            // statistics alone walk the same way and never touch a sink
            TagWalker<false> S;
            int64_t none = 0;
            CHECK(walk(c, S, none) && none == 0 && memcmp(&S.s, &s, sizeof(s)) == 0);
            // the wave form's step, modelled lane for lane, agrees with the walker
            TagStats ws; std::string wmd;
            wave_model(c, ws, wmd);
            CHECK(memcmp(&ws, &s, sizeof(s)) == 0 && wmd == md);
        }
        fprintf(out, "%d %d %d %d %d %d %d %d %d %lld ", ok ? 1 : 0, s.matches, s.mismatches, s.ins_bases, s.del_bases, s.ins_runs, s.del_runs,
                s.longest_match, s.columns, (long long)md_len);
        if (md.empty()) fputc('-', out);
        for (unsigned char ch : md) fprintf(out, "%02x", ch);
        fputc('\n', out);
    }
    fclose(in);
    CHECK(fclose(out) == 0);
    printf("tags_cpu ok: %d cases, bound of a pattern of 100 bases %lld\n", ncases, (long long)tag_md_bound(100));
    return 0;
}
