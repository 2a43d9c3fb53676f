// qe_types.h -- argument blocks shared by the host driver and the gfx950 kernels.
//
// Data model (DESIGN.md "Data layout in HBM"):
//   pair    one (pattern, text) of the batch; owns ASCII bytes and bit-planes.
//   planes  per pair and per sequence, 3 x u64 per 64 bases, interleaved
//           [row][plane]: plane 0/1 = the two bits of the base code, plane 2 =
//           "not ACGT" (the reference's code 4, dna_text.c:41-46).  Two zero
//           rows of padding follow every sequence (funnel-shift over-read).
//   task    one unit of kernel work = a sub-rectangle of a pair:
//           pattern[p0, p0+m) x text[t0, t0+n) with a cutoff.  Whole-pair
//           alignments are tasks with p0 = t0 = 0; Hirschberg children are not.
//   group   64 consecutive tasks = one wavefront; lane l of group g owns task
//           64 g + l for the whole kernel (one lane per alignment, no cross-lane
//           traffic; all per-task state is addressed [..][lane] so that every
//           global access of a wave is one contiguous 256/512/1024-byte row).
#pragma once
#include <stdint.h>

namespace qe {

typedef uint64_t u64;
typedef uint32_t u32;

enum : u32 { FLAG_HAS_N = 1u, FLAG_NONCANON = 2u };
// The BandEd fill leaves a checkpoint {Pv, Mv} every QE_CP_COLS columns of every band slot, QE_CPC per 64-column chunk: the
// width of the tile the traceback rebuilds in one round (k_traceback's TW).  Round 2 stored one every 8 columns and the
// traceback read every other one.
enum : int { QE_CP_COLS = 16, QE_CPC = 64 / QE_CP_COLS };
enum : u32 { OP_M = 0, OP_X = 1, OP_I = 2, OP_D = 3 };

struct PairView {
    const uint8_t* asc_p;  const int64_t* asc_p_off;  const int32_t* p_len;
    const uint8_t* asc_t;  const int64_t* asc_t_off;  const int32_t* t_len;
    const u64* pl_p;  const int64_t* pl_p_off;     // forward planes, word offsets
    const u64* pl_t;  const int64_t* pl_t_off;
    const u32* flags;
};

struct TaskView {
    int32_t ntasks;
    const int32_t* pair;     // -1 = empty slot
    const int32_t* p0;  const int32_t* m;
    const int32_t* t0;  const int32_t* n;
    const int32_t* cutoff;   // cutoff_in of banded_matrix_allocate
    const int32_t* tfin;     // text_finish_pos (score-only passes)
};

// pack: ASCII -> planes (+ flags).  reverse != 0 packs the reversed string.  One launch packs one set of nseq sequences
// or two of them (a batch's patterns and its texts): the grid has (nseq + 3) / 4 blocks per set, the block index picks
// the set, and sequence i of either set ORs its flags into flags[i] -- a pair's flags are those of both its sequences.
struct PackSet {
    const uint8_t* asc;  const int64_t* asc_off;  const int32_t* len;
    u64* planes;  const int64_t* pl_off;
};
struct PackArgs {
    int32_t nseq;        // sequences per set
    PackSet set[2];      // set[1] is read only by a grid of two sets' blocks
    u32* flags;          // OR-ed into (may be null)
    int32_t reverse;
};

// packed wire format -> planes (quicked_batch_create_packed).  wire 2: 2 bits per base, base i of a sequence in bits
// 2(i%32).. of word i/32, codes A0 C1 G2 T3 (dna_text.c:41-46), no N; wire 3: the plane layout itself, [row][3] =
// {code bit 0, code bit 1, not-ACGT} per 64 bases, without the padding rows
struct WireArgs {
    int32_t nseq, wire;
    const u64* words;  const int64_t* w_off;  const int32_t* len;
    u64* planes;  const int64_t* pl_off;
    u32* flags;          // FLAG_HAS_N is OR-ed in (may be null)
};
// planes of the reversed sequences from the forward planes (what k_pack(reverse) makes from ASCII)
struct RevArgs {
    int32_t nseq;
    const u64* fwd;  u64* rev;  const int64_t* pl_off;  const int32_t* len;
};

// The four membership planes of a flagged search run (qe_iupac.h; k_pack_iupac from resident ASCII, k_planes_iupac from the
// three planes of a packed batch): [row][4] = {A, C, G, T} per 64 bases, two zero rows behind every sequence, a sequence at
// word iupac_offset(pl_off[seq]) -- pl_off are the three-plane offsets.  No pack flags are written.
struct IupacPackArgs {
    int32_t nseq;
    const uint8_t* asc;  const int64_t* asc_off;  const int32_t* len;
    u64* planes;  const int64_t* pl_off;
    int32_t reverse;         // != 0: the reversed string
    int32_t acgt_only;       // != 0: a byte that is not A C G T U (either case) has the empty set
};
struct IupacPlanesArgs {
    int32_t nseq;
    const u64* src;  u64* dst;  const int64_t* pl_off;  const int32_t* len;      // src: forward or reversed three planes
    int32_t n_empty;         // != 0: the not-ACGT symbol has the empty set (else the full one)
};

// BandEd, score-only or fill (bpm_banded.c:791-964 / 199-316)
struct BandedArgs {
    PairView P;
    TaskView T;
    // per-group workspace: Pv[(ns+1)][64] u64 | Mv[(ns+1)][64] u64 | S[nrows][64] i32 | cf[nch][64] i16 | cl[nch][64] i16
    uint8_t* ws;  const int64_t* g_ws_off;  const int32_t* g_nslots;  const int32_t* g_nrows;  const int32_t* g_nch;
    // fill only: checkpoints {Pv,Mv} every QE_CP_COLS columns [(QE_CPC chunk + j) * g_nslots + slot][64] x 16 B, then the carry-in
    // words of every (chunk, slot) [(chunk * g_nslots + slot)][64] x 16 B
    uint4* mat;  const int64_t* g_mat_off;
    // outputs per task
    int32_t* o_score;  int32_t* o_first;  int32_t* o_last;  int32_t* o_posv;  u32* o_adv;  int32_t* o_maxrow;
    const int32_t* only_if;  // run only tasks whose flag is non-zero (fallback pass after k_banded_coop); may be null
    int32_t fill_multi = 1;  // fill: K-slot skewed passes where no lane needs the general form (0: single-slot passes only; tests)
    int32_t lane_rel = 1;    // every lane walks ITS band (slot first + j at step j of a chunk) instead of the wave walking the union of its lanes' bands (0: tests)
    int32_t score_masked = 1;     // k_banded<false>: a lane joins a multi-slot pass with the slots of it that are in its band (pass_plan; 0: all of them or none)
    int32_t* o_abort = nullptr;   // k_banded_sys: 1 where a task is left to k_banded<true> (N in the pair, a band of more than 15 slots)
    int32_t doubling = 0;         // k_banded_sys<.., false>: QuickEd's stage-3 band doubling in the launch (quicked.c:248-278)
    int32_t* o_cutoff = nullptr;  // ... the cutoff of every task's last pass (or, flagged, of the pass it was handed back before)
    int32_t prio = 0;             // the cooperative forms: s_setprio 3 (few waves on a serial chain, next to chip-filling launches)
    int32_t fill_geom = 0;        // k_banded<false>: the FILL's band geometry (a6's ebb, stop rule nw - 1: bpm_banded.c:121-135, 295) instead of
                                  // the score-only kernel's narrower one (801-803, 917): the cells, hence the end value, of the fill -- QuickEd with
                                  // only_score takes its score from such a pass instead of filling, tracing back and counting edits
    const int32_t* prune = nullptr;   // k_banded<false>: per task, beside T.cutoff: where prune[t] < T.cutoff[t] the band-edge rules compare against it
                                  // instead of the geometry's cutoff -- the fitted first launch of a two-pass run (narrow_prune); null, or a value
                                  // that is not below the task's cutoff: the geometry's (clamped) cutoff, as every other launch
    int32_t lds_slots = 0;        // k_banded<false, true> only: the band slots every wave's slice of the LDS holds (score_lds_bytes(lds_slots)
                                  // per wave); the group workspace is not touched
    int32_t score_tall = 0;       // k_banded<false, true> and the table form k_banded<false, false, true> only: one pass of tall_height() slots at the head of every chunk (0: the 4 / 2 / 1 plan alone)
};

// Bounded edit distance, diagonal-word form (k_bounded_diag, qe_bounded.h): whole pairs (p0 = t0 = 0), T.cutoff = the pair's
// bound; no workspace
struct BoundedArgs {
    PairView P;
    TaskView T;
    int32_t* o_score;        // the distance if it is within the bound, else -1
    u32* o_adv;              // text columns walked (one block step each)
};

// Approximate pattern search (k_search<NB>, qe_search.h): whole pairs (p0 = t0 = 0, T.m / T.n = the pair's lengths), T.cutoff =
// the pair's bound.  The forward pass (in_score == null) leaves o_score / o_end = {d, text_end} or {-1, -1} = beyond, and
// o_start = 0 for a PREFIX task within its bound, else -1.  The start pass of an INFIX run (in_score / in_end = the forward
// pass's outputs, P = the REVERSED planes, mode = SEARCH_PREFIX, flags = SEARCH_LARGEST_END) runs the tasks with
// in_score >= 0, bound in_score, over the in_end columns that end at text_end, and leaves o_start.  Both add their block
// steps to o_adv.
struct SearchArgs {
    PairView P;
    TaskView T;
    int32_t mode, flags;                     // SEARCH_PREFIX / SEARCH_INFIX; SEARCH_* flags
    const int32_t* in_score;  const int32_t* in_end;
    // the workspace form (k_search<0>), per group: Pv[nb][64] u64 | Mv[nb][64] u64 | S[nb][64] i32, nb = g_nb[group] >= the
    // blocks of every pattern of the group; null for the register forms
    uint8_t* ws;  const int64_t* g_ws_off;  const int32_t* g_nb;
    int32_t* o_score;  int32_t* o_end;  int32_t* o_start;  u32* o_adv;
};

// Every occurrence within the bound (k_search_hits<NB>, qe_search.h: SearchHitScan): the forward pass of k_search with the
// bound kept -- S.P / S.T / S.mode / S.ws .. S.g_nb / S.o_adv as there, S.flags 0, the other fields of S unused.  Per task t
// up to max_hits {end, score} at raw[2 (t max_hits + i)], ordered by end; per PAIR o_found = the occurrences, o_best = the
// smallest score among them (-1: none), o_len = the stored ones - 1 (what k_scan_offsets adds 1 to).  A lane without a task
// writes nothing.
struct SearchHitsArgs {
    SearchArgs S;
    int32_t max_hits;
    int32_t* raw;
    int32_t* o_found;  int32_t* o_best;  int32_t* o_len;
};
// The stored occurrences of a task list become one start-pass task each (k_hits_expand), in the order of the pairs: occurrence
// i of the list's task t is number j = off[pair] + i of the run.  hits[j] = {text_end - window (PREFIX: 0), text_end, score};
// o_pair[j] / o_m[j] / o_n[j] / o_score[j] / o_end[j] = T.pair / T.m / T.n / in_score / in_end of a start pass over the
// occurrence's window (search_hit_task; INFIX only: a PREFIX run has no start pass).  k_hits_finish then adds the pass's o_start to text_start (or leaves -1).
struct HitExpandArgs {
    TaskView T;                              // the forward pass's list
    int32_t max_hits, infix;
    const int32_t* raw;                      // of the list's first task
    const int32_t* len;  const int64_t* off; // per pair: stored - 1, the offset scan over it
    int32_t* hits;                           // quicked_hit_t[total] as {text_start, text_end, score}
    int32_t* o_pair;  int32_t* o_m;  int32_t* o_n;  int32_t* o_score;  int32_t* o_end;
};

// (the argument blocks of the panel kernels -- PanelArgs and PanelReduceArgs, and PanelHitsArgs, PanelHitsCountArgs and
// PanelHitsExpandArgs of the all-occurrences run -- are in qe_panel.h: plain C++, next to the
// per-slot functions that the kernels and their host stand-ins share)

// BandEd score-only, G lanes per alignment (cooperative form of k_banded<false>)
struct CoopArgs {
    PairView P;
    TaskView T;
    int32_t G;                               // lanes per alignment: 2, 4, ..., 64; a wave owns 64 / G tasks
    // per-WAVE workspace (A = 64 / G): Pv[(ns+1)][A] u64 | Mv[(ns+1)][A] u64 | S[nrows][A] i32 |
    //                                  CF[nch][A] i16 | CL[nch][A] i16 | KF[A] i32 | KL[A] i32
    uint8_t* ws;  const int64_t* w_ws_off;  const int32_t* w_nslots;  const int32_t* w_nrows;  const int32_t* w_nch;
    int32_t* o_score;  int32_t* o_first;  int32_t* o_last;  int32_t* o_posv;  u32* o_adv;  int32_t* o_maxrow;
    int32_t* o_abort;                        // 1: a band-edge decision could not be resolved in time; rerun with k_banded<false>
};

// the same with the band state of a wave's tasks in LDS (k_banded_coop_lds): what the whole launch is sized for
struct CoopLdsArgs {
    CoopArgs A;
    int32_t lgG;             // log2(A.G)
    int32_t ns;              // band slots per task the LDS holds (>= every task's band height)
    int32_t rr;              // scores[] ring: ns + G + 4 block rows per task and parity
    int32_t cr;              // band-edge rings: a power of two >= G + 4 chunks
    int32_t lds_per_wave;    // bytes
    // FILL form only (k_banded_coop_lds<true>): where the traceback expects the fill's checkpoints, carry words and band
    // edges -- BandedArgs' per-GROUP layout (64 tasks per group, column = task & 63); a wave's 64 / G tasks lie in one group
    uint4* mat;  const int64_t* g_mat_off;
    uint8_t* gws;  const int64_t* g_ws_off;  const int32_t* g_nslots;  const int32_t* g_nrows;  const int32_t* g_nch;
};

// BandEd traceback over a filled matrix (bpm_banded.c:967-1036) -> RLE runs, back to front
struct TraceArgs {
    PairView P;
    TaskView T;
    const uint8_t* ws;  const int64_t* g_ws_off;  const int32_t* g_nslots;  const int32_t* g_nrows;  const int32_t* g_nch;
    const uint4* mat;  const int64_t* g_mat_off;
    u32* runs;  const int64_t* g_runs_off;  const int32_t* g_runs_cap;   // [idx][64] u32 = len << 2 | op
    int32_t* o_nruns;  int32_t* o_nops;  int32_t* o_edits;  u32* o_steps;
    int32_t runs_by_task;    // != 0: task (g, lane) has the stretch [lane * cap, (lane + 1) * cap) of its group's buffer to itself
                             // (the wave-per-alignment formatter reads it sequentially; [idx][lane] rows cost it a 256-byte row per run)
    const int32_t* only_if = nullptr;   // k_traceback: walk only tasks whose flag is non-zero (what k_traceback_sys left)
    int32_t* o_abort = nullptr;         // k_traceback_sys: 1 where a task is left to k_traceback (N / non-canonical symbols)
    int32_t prio = 0;                   // k_traceback_sys: s_setprio 3
};

// WindowEd chain (bpm_windowed.c:563-628)
struct WindowArgs {
    PairView P;
    TaskView T;
    int32_t W, O, hew_threshold, score_only, sse, reversed;
    int32_t cp_path;       // k_windowed_cp: checkpoints + carry words instead of the full history (0: the history path, for tests)
    // per-group workspace: Pv[W][64] u64 | Mv[W][64] u64 ; history {Pv,Mv}[(64W+3)*W][64] x 16 B (k_windowed_cp uses a prefix:
    // checkpoints [8W][W][64] + carry words [W][W][64], 16 B each)
    uint8_t* ws;  const int64_t* g_ws_off;
    u32* runs;  const int64_t* g_runs_off;  const int32_t* g_runs_cap;
    int32_t* o_score;  int32_t* o_hew;  int32_t* o_nruns;  int32_t* o_nops;  int32_t* o_edits;  u32* o_steps;
    // chain state [5][ntasks] = {pos_v, pos_h, score, hew, steps} per task: k_windowed_quad (four lanes per alignment, full
    // (2, 1) windows only) leaves every task's chain where its first clamped window begins, k_windowed takes it up from
    // there; null: k_windowed runs the whole chain
    int32_t* state = nullptr;
    // k_windowed_sys (16 lanes per alignment, any window shape of up to 15 blocks, score only) flags what it leaves to
    // k_windowed_cp -- N / non-canonical symbols -- in o_abort; k_windowed_cp then runs only the tasks whose flag is set
    int32_t* o_abort = nullptr;  const int32_t* only_if = nullptr;
    int32_t prio = 0;      // k_windowed_quad / k_windowed_sys: s_setprio 3
};
// k_windowed_quad: LDS per wave = {Pv after, Mv before} of the traceback's 64 columns, [slot][lane] x 8 B, 65 slots
// (the lanes of a quad run one column apart)
enum : int { QE_WQ_SLOTS = 65, QE_WQ_LDS_PER_WAVE = QE_WQ_SLOTS * 64 * 8 };

// QuickEd's stage-1 rule on the device (quicked.c:201-202): the WindowEd(2,1) score of a task is its bound unless too many
// of its windows were high-error ones; est = the cutoff the host sized the align step for
struct Stage1Args {
    int32_t nt;
    const int32_t* pair;  const int32_t* m;  const int32_t* n;
    const int32_t* score;  const int32_t* hew;  const u32* steps;   // k_windowed's outputs
    const int32_t* est;
    u32 hew_percentage;
    int32_t* o_cut;      // the bound = the align step's cutoff
    int32_t* o_skip;     // bit 0: the pair goes on to stage 2; bit 1: its bound exceeds the estimate the buffers were sized for; bit 2: see flags
    u32* o_steps;        // copy of steps (the stage's buffers are recycled before the run is fetched)
    const u32* flags = nullptr;   // the pack flags by pair, where a score pass follows instead of the align step (only_score): a pair with
                                  // FLAG_NONCANON leaves the list too (bit 2 of o_skip) -- its edit count is not the matrix's end value
};

// BandEd score-only in two passes (run_banded_score): a first pass of k_banded<false> at half of every
// task's cutoff, then the full band only for the tasks whose first result proves nothing.  The cutoff a task's first pass
// runs at: C / 2 where that band has fewer slots than the band at C, else C itself (such a task's first result is final).
// Host and device decide with the same functions.
#if defined(__HIPCC__) || defined(__CUDACC__)
#define QE_T_HD __host__ __device__ __forceinline__
#else
#define QE_T_HD inline
#endif
QE_T_HD int narrow_effective(int m, int n, int cutoff_in) {          // banded_matrix_allocate's clamps (band_geometry)
    const int d = n > m ? n - m : m - n;
    const int c = d + 1 > cutoff_in ? d + 1 : cutoff_in;
    return c < 65 ? 65 : c;
}
QE_T_HD int narrow_slots(int m, int n, int cutoff_in) {
    return ((narrow_effective(m, n, cutoff_in) + 63) >> 6) + 1;      // the score-only band (bpm_banded.c:801-803)
}
QE_T_HD int narrow_cutoff(int m, int n, int cutoff_in) {
    const int half = cutoff_in / 2;
    return narrow_slots(m, n, half) < narrow_slots(m, n, cutoff_in) ? half : cutoff_in;
}
// The diagonals i - j below the main one that the score-only band at this cutoff holds in EVERY column.  The band starts
// `prolog` blocks above row 0 and moves down a block per 64 columns, so in the last column of a chunk it ends 64 (slots -
// prolog - 1) rows below the main diagonal.  The fill's geometry has a slot more wherever the two roundings to whole blocks
// add up to more than the rounding of the sum; the score-only one (slots = ceil(cutoff / 64) + 1) then holds fewer diagonals
// below the corridor than Ukkonen's band for the cutoff needs (cutoff 127, m - n = -3: none at all).
QE_T_HD int narrow_cover(int m, int n, int cutoff_in) {
    const int ce = narrow_effective(m, n, cutoff_in), diff = m - n, ad = diff < 0 ? -diff : diff;
    const int rel = (ce - ad + 1) / 2, prolog = (rel + (diff < 0 ? -diff : 0) + 63) / 64;
    return 64 * (((ce + 63) >> 6) - prolog);
}
// A first-pass result r at cutoff c1 stands for the pass at `cutoff` when it is the cost of a path within c1 AND both bands
// hold every diagonal a path of that cost can touch: max(0, diff) + floor((r - |diff|) / 2) below the main one (above it both
// always do: prolog is sized for the cutoff).  Then both passes return the distance.
QE_T_HD bool narrow_accepts(int m, int n, int c1, int cutoff_in, int r) {
    const int diff = m - n, ad = diff < 0 ? -diff : diff;
    if (r < ad || r > c1) return false;          // (no path costs less than |diff|; -1: the band never reached the end cell)
    const int need = (diff > 0 ? diff : 0) + (r - ad) / 2;
    const int a = narrow_cover(m, n, c1), b = narrow_cover(m, n, cutoff_in);
    return need <= (a < b ? a : b);
}
// The fit: narrow_accepts() holds for ANY first-pass cutoff c1, so where the distances of a stream are known
// -- as a ratio q of distance to cutoff in 1/1024ths -- the first pass takes the band of the fewest slots that still proves
// them instead of the band at half the cutoff.  r_hat = the result the fit is made for.
QE_T_HD int narrow_rhat(int q, int cutoff_in) { return (int)(((long long)q * cutoff_in + 1023) >> 10); }
// the largest result narrow_accepts(m, n, c1, cutoff_in, .) takes, -1 if it takes none
QE_T_HD int narrow_room(int m, int n, int c1, int cutoff_in) {
    const int diff = m - n, ad = diff < 0 ? -diff : diff;
    const int a = narrow_cover(m, n, c1), b = narrow_cover(m, n, cutoff_in);
    const int k = (a < b ? a : b) - (diff > 0 ? diff : 0);
    if (k < 0 || c1 < ad) return -1;
    const int r = ad + 2 * k + 1;
    return r < c1 ? r : c1;
}
// The candidates of the fit are the cutoffs c = narrow_effective(m, n, c) below cutoff_in whose band has fewer slots than the
// band at cutoff_in (a cutoff under the floor max(|m - n| + 1, 65) walks the floor's band and only accepts less).
// -> the least slot count among the candidates c >= r_hat that accept r_hat; 0: there is none
QE_T_HD int narrow_fit_slots(int m, int n, int cutoff_in, int r_hat) {
    const int diff = m - n, ad = diff < 0 ? -diff : diff;
    if (r_hat < ad) return 0;                                                // (no cutoff accepts it)
    if ((diff > 0 ? diff : 0) + (r_hat - ad) / 2 > narrow_cover(m, n, cutoff_in)) return 0;
    const int full = narrow_slots(m, n, cutoff_in), floor_c = narrow_effective(m, n, 0);
    for (int c = r_hat > floor_c ? r_hat : floor_c; c < cutoff_in; ++c) {
        const int s = ((c + 63) >> 6) + 1;
        if (s >= full) return 0;
        if (narrow_accepts(m, n, c, cutoff_in, r_hat)) return s;
    }
    return 0;
}
// -> among the candidates of exactly s slots (at most 64 cutoffs) the one that accepts the largest result, the smallest such;
// 0: no candidate has s slots.  This choice is the fit's margin: a lane gets all the room its slot count holds.
QE_T_HD int narrow_fit_cutoff(int m, int n, int cutoff_in, int s) {
    const int floor_c = narrow_effective(m, n, 0), hi = 64 * (s - 1) < cutoff_in - 1 ? 64 * (s - 1) : cutoff_in - 1;
    int c = 64 * (s - 2) + 1, best = 0, room = -2;
    if (s >= narrow_slots(m, n, cutoff_in)) return 0;
    for (c = c > floor_c ? c : floor_c; c <= hi; ++c) {
        const int r = narrow_room(m, n, c, cutoff_in);
        if (r > room) { room = r; best = c; }
    }
    return best;
}
// The cutoff of a lane whose group of 64 walks s_g slots (the largest narrow_fit_slots of its lanes that have one): the fitted
// one where that band is lower than the band at half the cutoff and proves the lane's own r_hat, else narrow_cutoff as ever.
QE_T_HD int narrow_fit_lane(int m, int n, int cutoff_in, int q, int s_g) {
    const int half = narrow_cutoff(m, n, cutoff_in);
    if (s_g <= 0 || s_g >= narrow_slots(m, n, half)) return half;
    const int c = narrow_fit_cutoff(m, n, cutoff_in, s_g);
    return (c > 0 && narrow_accepts(m, n, c, cutoff_in, narrow_rhat(q, cutoff_in))) ? c : half;
}
// The pruning threshold: the fitted cutoff is the roomiest its slot count holds, and every unit of that room
// is rows the band-edge rules of k_banded keep (they compare against the cutoff).  A lane that took the fitted cutoff prunes
// at min(c1, r_hat of the ratio qp) instead -- the geometry stays c1's -- and a first result above the threshold proves
// nothing: the rules drop a slot only when no path within the threshold passes through what is no longer computed.
// c1 = the lane's first-pass cutoff (narrow_fit_lane): it is the fit's exactly when it differs from narrow_cutoff (the fitted
// band has fewer slots than the band at half the cutoff); qp = the prune ratio in 1/1024ths of the cutoff, 0: none.
// A fitted band of three slots (the least there is) keeps its cutoff: its edges cannot move.
QE_T_HD int narrow_prune(int m, int n, int cutoff_in, int c1, int qp) {
    if (qp <= 0 || c1 == cutoff_in || c1 == narrow_cutoff(m, n, cutoff_in)) return c1;
    if (narrow_slots(m, n, c1) <= 3) return c1;      // first + 2 < last never holds in such a band: no rule fires, a threshold could only add misses
    const int r = narrow_rhat(qp, cutoff_in);
    return r < c1 ? r : c1;
}
QE_T_HD bool narrow_accepts_pruned(int m, int n, int c1, int cutoff_in, int p, int r) {
    return narrow_accepts(m, n, c1, cutoff_in, r) && r <= p;
}
// what a run reports of a task with a lowered cutoff and the final score r: ceil(1024 r / cutoff) where the pass at
// narrow_cutoff would have accepted r (the ratio the next fit is made from), else -1
QE_T_HD int narrow_ratio(int m, int n, int cutoff_in, int r) {
    if (!narrow_accepts(m, n, narrow_cutoff(m, n, cutoff_in), cutoff_in, r)) return -1;
    return (int)(((long long)r * 1024 + cutoff_in - 1) / cutoff_in);
}

// The pass plan of k_banded<false> ("Masked passes"): the part one lane takes in a K-slot pass over the slots
// i .. i + K - 1 of a chunk.  lo .. hi are the band slots the lane computes in this chunk (first .. min(last, nw - 1 - pos_v);
// lo > hi for a lane without columns here), r = the block row of slot i, nw = the pattern's block rows, plain = a full chunk
// of 64 columns of a pair without N.  -> nl, the lane's live slots: i .. i + nl - 1, always a prefix of the pass (the slots
// below them compute on zeros and are never loaded or stored: carries only flow downwards).  `fallback` = the wave must not
// take this pass because of this lane: its live slots start inside the pass (the slots above them would feed the band's top
// slot, whose carry-in is (1, 0)) or one of them needs the general form (partial chunk, N, the pattern's last block row).
// The wave takes the pass when no lane says fallback.  masked = false is the all-or-none rule: a lane has all K slots or
// none of them, anything else is a fallback.
QE_T_HD int pass_plan(int i, int K, int lo, int hi, int r, int nw, bool plain, bool masked, bool& fallback) {
    if (!masked) {
        const bool all = i >= lo && i + K - 1 <= hi, none = i + K - 1 < lo || i > hi;
        fallback = !(all || none) || (all && (!plain || r + K - 1 >= nw - 1));
        return all ? K : 0;
    }
    const int a0 = i > lo ? i : lo, a1 = i + K - 1 < hi ? i + K - 1 : hi;
    const int nl = a1 >= a0 ? a1 - a0 + 1 : 0;
    fallback = nl > 0 && (a0 != i || !plain || r + nl - 1 >= nw - 1);
    return nl;
}
// Tall passes of k_banded<false, true> ("Tall passes"): at the first step of a chunk whose walk is h slots
// long the wave takes ONE pass of tall_height(h) slots from the top of the band -- a prefix, as masked passes need -- where
// pass_plan at that height has no fallback; the 4 / 2 / 1 plan walks what is left, and the whole chunk where this says 0.
// h = 5 .. 10: the walk itself.  A taller walk: the largest height whose remainder the old plan takes in whole passes
// (0, 1, 2 or at least 4 slots; 3 would be a 2-slot and a single-slot pass).
enum : int { QE_TALL_MIN = 5, QE_TALL_MAX = 10 };
QE_T_HD int tall_height(int h) {
    for (int K = QE_TALL_MAX; K >= QE_TALL_MIN; --K) {
        const int rem = h - K;
        if (rem >= 0 && rem != 3) return K;
    }
    return 0;
}
// the height of the pass that starts at step x of a chunk walked i0 .. i1: the tall height at the first step where `tall`
// and planned(K) holds, else 4, else 2 where that many steps are left and planned, else 0 (a single-slot pass)
template <class Planned> QE_T_HD int score_pass_height(int x, int i0, int i1, bool tall, Planned&& planned) {
    if (tall && x == i0) {
        const int K = tall_height(i1 - i0 + 1);
        if (K && planned(K)) return K;
    }
    if (x + 3 <= i1 && planned(4)) return 4;
    if (x + 1 <= i1 && planned(2)) return 2;
    return 0;
}

// Band state in LDS (k_banded<false, true>; DESIGN.md 4.1, "Band state in LDS"): the budget, one definition for the launch
// and the kernel.  A wave's slice holds Pv[s + 1][64] u64 | Mv[s + 1][64] u64 (slot -1 included) for bands of up to s slots
// and scores[] as a ring of score_lds_ring() block rows x 64 lanes, row r at index r & (ring - 1).
// The ring's invariant: with the score-only geometry (stop rule nw) a chunk reads and writes the rows
// first + pos_v .. last + pos_v + 1 only -- at most slots + 1 consecutive rows, first + pos_v and last + pos_v never decrease
// from chunk to chunk -- and no row above nw + 1 is ever written (last-- once pos_v + last reaches nw).  So with
// slots + 1 <= ring - 2 no two rows of a chunk share an index, and row nw - 1 shares one only with rows nw - 1 -+ ring:
// the lower one left the window before nw - 1 entered it, the upper one does not exist.  The read-out finds row nw - 1
// as it was last written.
QE_T_HD int score_lds_ring() { return 16; }
QE_T_HD int score_lds_cap() { return score_lds_ring() - 3; }        // 13 slots: a window of 14 rows
QE_T_HD bool score_lds_fits(int slots) { return slots >= 1 && slots <= score_lds_cap(); }
QE_T_HD int score_lds_row(int r) { return r & (score_lds_ring() - 1); }
QE_T_HD int score_lds_bytes(int slots) { return 2 * (slots + 1) * 64 * 8 + score_lds_ring() * 64 * 4; }      // per wave: 18 KB at the cap

// Eq from a table (the table form of the fitted first launch; DESIGN.md 4.1, "Eq from a table"): a wave's slice of the LDS
// holds E[sym][slot][lane], one u64 each -- the 64 Eq bits of that lane's pattern block row at slot `slot` of the pass for the
// text symbol sym = t0 + 2 t1, (a == t0) & (b == t1) per bit of the two code planes.  2 KB per slot, 20 KB per wave, 80 KB per
// workgroup of four: two workgroups share a CU's 160 KB.  The sym stride is a multiple of 256 B and lanes are 8 B apart, so
// lane l reads bank 2 l mod 64 (and the one above it) whatever sym and slot: no ds_read_b64 of a wave meets a bank conflict.
QE_T_HD int peq_cap() { return QE_TALL_MAX; }                                   // the slots of the tallest pass
QE_T_HD int peq_slot_stride() { return 64 * 8; }                               // bytes
QE_T_HD int peq_sym_stride() { return peq_cap() * peq_slot_stride(); }         // bytes
QE_T_HD int peq_bytes() { return 4 * peq_sym_stride(); }                       // per wave
QE_T_HD int peq_offset(int sym, int slot, int lane) { return sym * peq_sym_stride() + slot * peq_slot_stride() + lane * 8; }
QE_T_HD u64 peq_entry(u64 a, u64 b, int sym) { return ((sym & 1) ? a : ~a) & ((sym & 2) ? b : ~b); }

// k_narrow, one thread per task of the list T (whole-text passes: tfin = n).  phase 0: cut1 = narrow_cutoff of every task,
// the packed list emptied, the statistics zeroed.  phase 1, after the first pass: a task whose cutoff was halved and whose
// score narrow_accepts() does not take is a miss; the misses go, with their original cutoffs, into the packed list q_* in dense
// groups of 64 (order: as the waves get there; nothing depends on it), q_src = the task's index.  phase 2, after the second
// pass over the packed list: the misses' scores replace the first pass's at q_src, their block-columns are added there.
// phase 3, a probe of the policy (no result depends on it): T is a SAMPLE of a list that ran its single pass -- the tasks of
// every stride-th group of 64, at halved cutoffs -- whose pass beside that launch left q_score / q_adv; score / adv and
// main_cutoff are the whole list's.  It counts what two passes would have cost the sample (stat; [2] from what the single
// pass did advance for the misses) and adds the sample pass's block-columns to the tasks' own (work really done).
// With q > 0 (the fit, see above) phase 0 works per group of 64 tasks = one wave of k_banded: s_g = the largest narrow_fit_slots
// of the group's live lanes that have one, cut1 = narrow_fit_lane(.., q, s_g); q = 0 is narrow_cutoff for every task.
// With a prune ratio qp > 0 the lanes that took the fit get prune1 = narrow_prune(..) <= cut1, the band-edge threshold of
// the first launch, and phase 1 takes a first result only up to it; the misses this adds are accepted by narrow_cutoff's
// pass, so phase 2 counts them in stat[5] and reports their ratios like every miss owed to the fit.
enum : int { QE_NARROW_STAT = 6 };               // words of NarrowArgs::stat
struct NarrowArgs {
    int32_t phase, stride, q;
    TaskView T;
    int32_t* cut1;
    int32_t qp = 0;  int32_t* prune1 = nullptr;  // the fit's pruning threshold: phase 0 writes narrow_prune(.., cut1, qp) beside cut1, phase 1
                                                 // accepts with narrow_accepts_pruned (null: no thresholds; phase 3 has none)
    int32_t* score;  u32* adv;                   // the list's outputs (first pass; phase 2 merges the second into them)
    int32_t *q_pair, *q_p0, *q_m, *q_t0, *q_n, *q_cutoff, *q_tfin, *q_src;
    const int32_t* q_score;  const u32* q_adv;   // the second pass's outputs, by packed index
    const int32_t* main_cutoff;
    // [0] misses  [1] block-columns the tasks with a halved cutoff advanced in the first pass  [2] block-columns of the second
    // pass  [3] tasks with a halved cutoff  [4] the largest narrow_ratio() of the lowered tasks' final scores (phases 1 and 2)
    // [5] the misses among them that the pass at narrow_cutoff would have accepted: the misses owed to the fit alone
    unsigned long long* stat;
};

// Where a stopped score-only BandEd launch left its band (what the Hirschberg join reads)
struct BandState {
    int32_t G;     // 1: k_banded<false> layout (per 64-task group, column = lane); >= 2: k_banded_coop layout (per wave of 64/G tasks)
    const uint8_t* ws;  const int64_t* g_ws_off;  const int32_t* g_nslots;  const int32_t* g_nrows;  const int32_t* g_nch;
    const int32_t* first;  const int32_t* last;  const int32_t* posv;  const int32_t* maxrow;
    const int32_t* abort;  // coop only: tasks recomputed by the fallback pass live in fb's layout
};

// Hirschberg midpoint join (bpm_hirschberg.c:102-200, re-derived: SURVEY A.5 / A.7(12)); node j of
// the split list is task j of both the forward and the reverse half-pass launch
struct JoinArgs {
    int32_t nnodes;
    const int32_t* m;  const int32_t* n1;  const int32_t* n2;
    BandState F, R;       // cooperative launches (or the only ones when G == 1)
    BandState Ffb, Rfb;   // their k_banded<false> fallback passes (G == 1 layout); used where abort[j] != 0
    int32_t* o_best;  int32_t* o_score_l;  int32_t* o_score_r;  int32_t* o_ok;
};

// CIGAR of a pair = its segments in order, each either the RLE runs of a leaf alignment
// (kind 0: a = leaf task index) or a literal run (kind 1: a = op, b = count), merged across
// segment borders exactly like cigar_sprint over one operations buffer (cigar.c:453-488)
struct SegFormatArgs {
    int32_t npairs;
    const int64_t* seg_off;      // [npairs + 1]
    const int32_t* seg_kind;  const int32_t* seg_a;  const int32_t* seg_b;
    const u32* runs;  const int64_t* g_runs_off;  const int32_t* nruns;   // per leaf task
    const int32_t* g_runs_cap;  int32_t runs_by_task;                      // layout of `runs` (TraceArgs::runs_by_task)
    int32_t* o_len;  int32_t* o_edits;  int32_t* o_nops;                  // per pair-list entry
    const int64_t* str_off;  char* pool;
    // 0: the reference's RLE "MXID" (cigar_sprint, cigar.c:453-488); 1: SAM with mismatches "=XID";
    // 2: SAM "MID", X folded into M before runs are merged (cigar_compute_CIGAR, cigar.c:194-240, 504-529)
    int32_t style;
};

// cigar_check_alignment (cigar.c:363-434) of every entry's alignment against the raw bytes of its pair
struct SegCheckArgs {
    SegFormatArgs F;
    PairView P;
    const int32_t* root_pair;
    int32_t* o_ok;               // 1 valid, 0 not
};

// Per-pair statistics and MD strings of every entry's alignment (qe_tags.h; quicked_batch_configure_tags).  The count pass
// leaves o_stats / o_md_len (string length without the terminator; 0 where the pair has no alignment), the write pass
// fills md_pool at md_off: F.o_* / F.pool / F.str_off are not touched
struct TagStats;
struct SegTagArgs {
    SegFormatArgs F;
    PairView P;
    const int32_t* root_pair;
    int32_t want_stats, want_md;
    TagStats* o_stats;           // [npairs], all -1 where the pair has no alignment
    int32_t* o_md_len;
    int32_t* o_md_bad;           // one flag: set when a string would not fit tag_md_bound of its pattern
    const int64_t* md_off;  char* md_pool;
};

}  // namespace qe
