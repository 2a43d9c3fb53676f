// k_pack's span classifier (quicked_amd/csrc/qe_pack.h) on the HOST: sequences are packed span by span as the kernel's lanes
// pack them -- lane l of span s takes the 16 bytes at 1024 s + 16 l (pack_fetch16), pack_classify16 gives its three 16-bit
// masks, four neighbouring lanes make a row, the flags come from pack_flags16 in every lane of a span in which some lane's
// hint fires -- and compared with a scalar packer that goes byte by byte through the reference's code table
// (dna_text.c:41-46), which shares nothing with the header.  Planes, the two padding rows and the flags must be equal, forward
// and reversed.  A stand-alone program (built plain and under ASan + UBSan by tests/test_pack_cpu.py); every sequence lives
// in a heap block of exactly its length, so a byte read outside it is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qe_pack.h"

using qe::u32;
typedef uint64_t u64;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { if (++g_failed <= 20) fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// ---- the scalar rule ---------------------------------------------------------------------------------------------------
struct Packed { std::vector<u64> words; u32 flags = 0; };
static uint8_t g_encode[256];      // the reference's table: A C G T in either case 0 .. 3, everything else 4
static void init_table() {
    memset(g_encode, 4, sizeof g_encode);
    const char* up = "ACGT"; const char* lo = "acgt";
    for (int k = 0; k < 4; ++k) { g_encode[(uint8_t)up[k]] = (uint8_t)k; g_encode[(uint8_t)lo[k]] = (uint8_t)k; }
}
static size_t rows_of(int len) { return (size_t)((len + 63) / 64 + 2); }
static Packed scalar_pack(const uint8_t* s, int len, bool reverse) {
    Packed P;
    P.words.assign(3 * rows_of(len), 0);
    static const int plane_code[4] = {0, 1, 3, 2};      // the planes' code of A, C, G, T: ASCII bits 1 and 2 of the letter
    for (int i = 0; i < len; ++i) {
        const uint8_t c = s[reverse ? len - 1 - i : i];
        const int r = g_encode[c];
        u64* row = &P.words[3 * (size_t)(i / 64)];
        const u64 bit = (u64)1 << (i % 64);
        if (r == 4) {
            row[2] |= bit;
            P.flags |= qe::PACK_HAS_N;
            if (c != 'N') P.flags |= qe::PACK_NONCANON;
        } else {
            if (plane_code[r] & 1) row[0] |= bit;
            if (plane_code[r] & 2) row[1] |= bit;
            if (c != "ACGT"[r]) P.flags |= qe::PACK_NONCANON;
        }
    }
    return P;
}

// ---- the kernel's walk -------------------------------------------------------------------------------------------------
static Packed lane_pack(const uint8_t* s, int len, bool reverse) {
    Packed P;
    const int nrows = (int)rows_of(len), nspan = (nrows + 15) / 16;
    P.words.assign(3 * (size_t)nrows, ~(u64)0);          // what the walk does not write shows
    std::vector<char> written((size_t)nrows, 0);
    for (int span = 0; span < nspan; ++span) {
        u32 w[64][4], a[64], b[64], n[64], hint[64];
        bool any = false;
        for (int lane = 0; lane < 64; ++lane) {
            qe::pack_fetch16(s, len, span * 1024 + 16 * lane, reverse, w[lane]);
            qe::pack_classify16(w[lane], a[lane], b[lane], n[lane], hint[lane]);
            CHECK((a[lane] | b[lane] | n[lane]) < 0x10000u);
            CHECK(((a[lane] | b[lane]) & n[lane]) == 0);
            if (hint[lane] == 0) CHECK(qe::pack_flags16(w[lane]) == 0);
            any = any || hint[lane] != 0;
        }
        for (int lane = 0; lane < 64; ++lane) {
            if (any) P.flags |= qe::pack_flags16(w[lane]);
            const int row = span * 16 + lane / 4, sh = 16 * (lane & 3);
            if (row >= nrows) { CHECK((a[lane] | b[lane] | n[lane]) == 0); continue; }
            u64* q = &P.words[3 * (size_t)row];
            if (!written[(size_t)row]) { q[0] = q[1] = q[2] = 0; written[(size_t)row] = 1; }
            q[0] |= (u64)a[lane] << sh; q[1] |= (u64)b[lane] << sh; q[2] |= (u64)n[lane] << sh;
        }
    }
    for (char c : written) CHECK(c);
    return P;
}

static long g_cases = 0;
static void compare(const std::vector<uint8_t>& seq) {
    const int len = (int)seq.size();
    uint8_t* heap = (uint8_t*)malloc(len ? (size_t)len : 1);      // exactly the sequence: no slack behind it
    if (len) memcpy(heap, seq.data(), (size_t)len);
    for (int rev = 0; rev < 2; ++rev) {
        const Packed e = scalar_pack(heap, len, rev != 0), g = lane_pack(heap, len, rev != 0);
        ++g_cases;
        const bool same = e.words == g.words && e.flags == g.flags;
        if (!same && g_failed < 20) fprintf(stderr, "mismatch: len %d reversed %d flags %u / %u\n", len, rev, g.flags, e.flags);
        CHECK(same);
        const size_t nw = e.words.size();
        for (size_t k = nw - 6; k < nw; ++k) CHECK(g.words[k] == 0);      // the two padding rows
    }
    free(heap);
}

static u64 g_rng = 0x9E3779B97F4A7C15ull;
static u32 rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (u32)(g_rng >> 32); }

int main() {
    init_table();
    // the host forms of the two wrappers
    CHECK(qe::pack_perm(0u, 0x47544341u, 0x03020100u) == 0x47544341u && qe::pack_perm(0u, 0x47544341u, 0x00010203u) == 0x41435447u);
    CHECK(qe::pack_perm(0xD4C3B2A1u, 0x44332211u, 0x0C0C0703u) == 0x0000D444u && qe::pack_perm(0xD4C3B2A1u, 0x44332211u, 0x07060302u) == 0xD4C34433u);
    for (u32 p = 0; p < 4; ++p)          // the gather: eight flags at bits p and p + 4 of the four bytes -> the byte at p + 21
        for (u32 v = 0; v < 256; ++v) {
            u32 u = 0;
            for (u32 k = 0; k < 4; ++k) u |= (((v >> k) & 1u) << (8 * k + p)) | (((v >> (4 + k)) & 1u) << (8 * k + p + 4));
            CHECK(((qe::pack_gather8(u) >> (p + 21)) & 0xFFu) == v);
        }
    const int lengths[] = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1007, 1008, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4097};
    const uint8_t raw_bytes[] = {'A', 'C', 'G', 'T', 'a', 'c', 'g', 't', 0x00, 0x7F, 0x80, 0xFF};
    struct Alphabet { const uint8_t* sym; int n; };
    const Alphabet alphabets[] = {
        {(const uint8_t*)"ACGT", 4}, {(const uint8_t*)"ACGTacgt", 8}, {(const uint8_t*)"ACGTACGTACGTNn", 14},
        {(const uint8_t*)"ACGTRYSWKMBDHVNUryswkmbdhvnu", 28}, {raw_bytes, 12}, {nullptr, 256}};
    for (const Alphabet& al : alphabets)
        for (int len : lengths)
            for (int rep = 0; rep < 2; ++rep) {
                std::vector<uint8_t> s((size_t)len);
                for (auto& c : s) c = al.sym ? al.sym[rnd() % (u32)al.n] : (uint8_t)rnd();
                if (rep == 1 && len > 0) {      // a single symbol of the alphabet in a run of upper-case bases: one lane's hint, a whole span's flags
                    const uint8_t one = s[0];
                    for (auto& c : s) c = "ACGT"[rnd() & 3];
                    s[rnd() % (u32)len] = one;
                }
                compare(s);
            }
    // all 256 byte values at every position of a lane, in upper-case and in lower-case company
    for (int lower = 0; lower < 2; ++lower)
        for (int pos = 0; pos < 16; ++pos)
            for (int v = 0; v < 256; ++v) {
                const char* bg = lower ? "acgttgcaacgttgca" : "ACGTTGCAACGTTGCA";
                std::vector<uint8_t> s(bg, bg + 16);
                s[(size_t)pos] = (uint8_t)v;
                compare(s);
                s.insert(s.begin(), 1030, 'G');      // ... and the same lane as the ragged end behind a span that is loaded whole
                compare(s);
            }
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("pack ok: %ld packs\n", g_cases);
    return 0;
}
