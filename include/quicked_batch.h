/*
 * quicked_batch.h -- additive batch surface of libquicked_hip.so.
 *
 * Not in the reference (its only batch mode is an OpenMP loop over
 * quicked_align calls, tools/align_benchmark/align_benchmark.c:269-284, fed
 * from sequence_buffer_t, quicked_utils/include/sequence_buffer.h:30-50).
 * Per-pair semantics are those of quicked_align() with the aligner's params;
 * the six reference signatures and both struct layouts are untouched.
 * Plain pointers and sizes only.
 */
#ifndef QUICKED_BATCH_H
#define QUICKED_BATCH_H

#include <stddef.h>

#include "quicked.h"

#ifdef __cplusplus
extern "C" {
#endif

/* selects the HIP device used by subsequent calls of this thread (default 0).  One process may drive every GPU of a node:
 * a host thread per device, each with its own aligner / batch objects (tools/align_benchmark.cpp -t N: the reference's one
 * aligner per thread, align_benchmark.c:246-249, mapped to devices); pairs are sharded, there is no data-path collective. */
quicked_status_t quicked_set_device(int device);
/* HIP devices this process sees (0 if there is no usable runtime) */
int quicked_device_count(void);

/* Convenience form: n pairs given as host pointers.  scores_out[n];
 * cigars_out may be NULL (scores only); otherwise cigars_out[i] is a
 * NUL-terminated RLE string owned by the aligner until the next batch call or
 * quicked_free() (NULL for pairs whose status is an error).  status_out may be
 * NULL.  Returns the first error status, else the common success status. */
quicked_status_t quicked_align_batch(quicked_aligner_t* aligner, int n,
                                     const char* const* patterns, const int* pattern_lens,
                                     const char* const* texts, const int* text_lens,
                                     int* scores_out, char** cigars_out,
                                     quicked_status_t* status_out);

/* Pinned host memory for sequence pools: quicked_batch_create() DMAs straight from it (pageable pools
 * are pipelined through pinned staging instead). */
void* quicked_host_alloc(size_t bytes);
void quicked_host_free(void* p);

/* ---- resident batches: upload once, run many times (what bench.py times) --- */
typedef struct quicked_batch quicked_batch_t;

/* Pairs stored back to back in two host byte pools (the batch wire format):
 * pattern i = pattern_pool[pattern_off[i] .. +pattern_len[i]).  Copies the
 * pools to HBM (H2D) and sizes the device pool; no alignment work. */
quicked_batch_t* quicked_batch_create(int64_t n,
                                      const char* pattern_pool, const int64_t* pattern_off, const int32_t* pattern_len,
                                      const char* text_pool, const int64_t* text_off, const int32_t* text_len);
void quicked_batch_destroy(quicked_batch_t* batch);
/* Loads n new pairs into an existing batch object: same arguments as quicked_batch_create, but the object's device
 * arena is kept when it is large enough (no hipMalloc / hipFree, which synchronise the device).  Waits for the runs of
 * the batch that are still on the device; may be called from another thread than the one that runs the batch -- a
 * client streams by reloading batch k+1 on an uploader thread while batch k runs (bench.py's end-to-end leg). */
quicked_status_t quicked_batch_reload(quicked_batch_t* batch, int64_t n,
                                      const char* pattern_pool, const int64_t* pattern_off, const int32_t* pattern_len,
                                      const char* text_pool, const int64_t* text_off, const int32_t* text_len);

/* ---- packed wire format (supersedes sequence_buffer_t, tools/align_benchmark/utils/sequence_buffer.h:30-50)
 * For sequences over upper-case A, C, G, T (and N in PLANES3) -- the symbols whose raw-byte and encoded
 * comparisons agree (dna_text.c:41-46, bpm_banded.c:1012); everything else must use the ASCII form.
 *   QUICKED_WIRE_2BIT     2 bits per base: base i of a sequence in bits 2(i%32).. of its word i/32,
 *                         codes A 0, C 1, G 2, T 3; ceil(len/32) words
 *   QUICKED_WIRE_PLANES3  per 64 bases three words {code bit 0, code bit 1, not-ACGT}; 3 ceil(len/64) words
 * A packed batch uploads 4x / 2.7x fewer bytes than ASCII, keeps no bytes in HBM and skips the pack stage of
 * every run; scores and CIGARs are identical to the ASCII batch of the same sequences.  The raw-byte
 * validator is not available for it (QUICKED_UNIMPLEMENTED). */
typedef enum { QUICKED_WIRE_2BIT = 2, QUICKED_WIRE_PLANES3 = 3 } quicked_wire_t;
int64_t quicked_wire_words(int32_t len, int wire);
/* host-side serializer of one sequence; QUICKED_ERROR if a symbol is not representable in `wire` */
quicked_status_t quicked_wire_pack(const char* seq, int32_t len, int wire, uint64_t* out);
/* The same serializer over a whole pool in one call: sequence i = pool[off[i] .. +len[i]) goes to out_words + out_off[i]
 * (quicked_wire_words(len[i], wire) words; quicked_wire_offsets lays the sequences out back to back and returns the
 * total).  SIMD (AVX-512BW or AVX2, with BMI2; picked at run time, scalar otherwise) on `threads` host threads (0: the
 * CPUs the process may use, at most 32).  This is how a caller that holds ASCII -- what the reference's API consumes,
 * quicked.c:405-437 -- gets under the PCIe bound: 2 GB of ASCII per 100 k pairs of 10 kb become 0.5 GB on the wire.
 * Words identical to quicked_wire_pack's.  QUICKED_ERROR if a sequence holds a symbol `wire` cannot represent;
 * *bad_seq (may be NULL) = the first such sequence, else -1. */
quicked_status_t quicked_wire_pack_pool(int64_t n, const char* pool, const int64_t* off, const int32_t* len, int wire,
                                        uint64_t* out_words, const int64_t* out_off, int threads, int64_t* bad_seq);
int64_t quicked_wire_offsets(int64_t n, const int32_t* len, int wire, int64_t* out_off);
/* which kernel quicked_wire_pack_pool uses: 0 scalar, 1 AVX2, 2 AVX-512BW; force >= 0 pins a kernel the CPU has (tests),
 * force < 0 restores the run-time choice; returns the kernel in use, or -1 if the CPU lacks the one asked for */
int quicked_wire_pack_isa(int force);
quicked_batch_t* quicked_batch_create_packed(int64_t n, int wire,
                                             const uint64_t* pattern_words, const int64_t* pattern_word_off, const int32_t* pattern_len,
                                             const uint64_t* text_words, const int64_t* text_word_off, const int32_t* text_len);

quicked_status_t quicked_batch_reload_packed(quicked_batch_t* batch, int64_t n, int wire,
                                             const uint64_t* pattern_words, const int64_t* pattern_word_off, const int32_t* pattern_len,
                                             const uint64_t* text_words, const int64_t* text_word_off, const int32_t* text_len);

/* Runs the hot path for every pair with `params` (algo, only_score, ...), from
 * the ASCII bytes resident in HBM to scores (and CIGAR runs) resident in HBM.
 * sync != 0: waits for the run and copies scores / statuses / CIGARs / counters
 * to the host, where the getters below read them.
 * sync == 0: returns once the run is queued; nothing is copied to the host until quicked_batch_fetch().  HIRSCHBERG, and
 * QUICKED where a pair may split or the batch runs for the first time, return once their host-driven stages are done;
 * otherwise QUICKED queues stage 1 and the align step together (the stage-1 rule of quicked.c:201-202 runs on the
 * device) and aligns the pairs that go on to stages 2 / 3 when the run is fetched.  Consecutive runs of a thread rotate over several sets of stream, device
 * pool and bit-planes -- three for batches that fill the chip, up to twelve for small ones (quicked_pool_stats()[2]) --
 * so the kernels of the next runs overlap those of run k. */
quicked_status_t quicked_batch_run(quicked_batch_t* batch, const quicked_params_t* params, int sync);
/* Bounded distances: "is pair i within k edits, and if so, how many?".  Pair i's bound is max_dist[i] (n values, read during
 * the call) or, where max_dist is NULL, max_dist_all.  Result of pair i: its edit distance d if d <= bound, else "beyond":
 * score -1 with the status QUICKED_OK -- an answer, not an error -- and no CIGAR.  The distance is the library's own (what
 * algo = QUICKED computes: case folded, every non-ACGT byte one symbol, dna_text.c:41-46).  only_score == 0: a CIGAR with
 * exactly d edits for every pair within its bound (cigar_off -1 for the others), in the style and with the validator of
 * quicked_batch_configure; such a run needs sync != 0 (sync == 0: QUICKED_UNIMPLEMENTED, nothing is queued).  only_score != 0
 * with sync == 0 queues the run like quicked_batch_run does; quicked_batch_fetch brings its results.  Results through the
 * getters below.  Empty sequences keep QUICKED_EMPTY_SEQUENCE; a NULL batch or a negative bound: QUICKED_ERROR, nothing is
 * launched.  ASCII and packed batches alike.  A pair whose bound (at most max(pattern, text) counts) is <= 63 can be
 * decided by a kernel that keeps the pair's whole band in one 64-bit word: the library picks it for pairs of 2000 bases and more,
 * QE_BOUNDED_DIAG=1 wherever it applies, QE_BOUNDED_DIAG=0 never; the others, and the CIGARs, go through the BandEd
 * kernels with the bound as the cutoff.  Pairs with lower-case / IUPAC bytes get their distance from the QUICKED flow
 * itself (its alignment's edit count), on the host's schedule: when a sync != 0 run ends, or in the fetch. */
quicked_status_t quicked_batch_run_bounded(quicked_batch_t* batch, const int32_t* max_dist, int32_t max_dist_all,
                                           int only_score, int sync);
/* Approximate pattern search: "where in this text does the pattern fit best, and at what cost?" -- edlib's SHW (prefix) and HW
 * (infix) modes.  D is the edit-distance matrix of pair i's pattern (rows, m) against its text (columns, n) under the library's
 * own equality (case folded, every non-ACGT byte one symbol: two symbols are equal when both are non-ACGT or when their codes
 * agree).  QUICKED_SEARCH_INFIX has a top row of zeros (the pattern may start anywhere in the text),
 * QUICKED_SEARCH_PREFIX has D[0][j] = j (it starts at the text's start).  The result of pair i:
 *   score      d = min over e in 1 .. n of D[m][e]
 *   text_end   the smallest such e; exclusive: the located stretch is text[text_start, text_end)
 *   text_start 0 for PREFIX; for INFIX the smallest s < text_end for which the global distance of the pattern against
 *              text[s, text_end) equals d -- the longest stretch
 * which is edlib's editDistance, endLocations[0] + 1 and startLocations[0] with EDLIB_TASK_LOC; where edlib reports the end
 * location -1 (d == m: "the pattern before the text") the rule above is the definition.
 * Bounds as in quicked_batch_run_bounded: pair i's bound is max_dist[i] (n values, read during the call) or, where max_dist is
 * NULL, max_dist_all; it is clamped to m, which no search distance exceeds, so INT32_MAX means "no bound".  d > bound: the
 * pair is "beyond" -- score -1 with the status QUICKED_OK, both locations -1, no CIGAR.  Empty sequences keep
 * QUICKED_EMPTY_SEQUENCE (locations -1); a NULL batch, an unknown mode or a negative bound: QUICKED_ERROR, nothing is launched.
 * ASCII and packed batches alike.
 * only_score != 0 with sync == 0 queues the run like quicked_batch_run does; quicked_batch_fetch brings scores and locations.
 * only_score == 0 needs sync != 0 (sync == 0: QUICKED_UNIMPLEMENTED, nothing is queued, as a queued bounded CIGAR run): every
 * pair within its bound gets the CIGAR of the global alignment of the pattern against its located stretch, with exactly d
 * edits, in the style of quicked_batch_configure (a status other than QUICKED_OK on a located pair means its alignment failed:
 * the score and the locations stand, the CIGAR does not).  The alignment tags of quicked_batch_configure_tags apply unchanged -- they
 * read the alignment and the whole pattern -- with one difference in the identities of quicked_pair_stats_t:
 *   matches + mismatches + ins_bases == text_end - text_start   (the stretch, not text_len).
 * The in-run validator walks the text from its origin: a search run on a batch configured with check != 0 returns
 * QUICKED_UNIMPLEMENTED and queues nothing.  Pairs with lower-case / IUPAC bytes are scored and located like every other
 * pair, but in a CIGAR run they get no alignment (cigar_off -1, statistics of all -1, md_off -1): the traceback compares raw
 * bytes, so the edit count of their CIGAR would not be d.
 * Two kernel forms, one lane per pair: the workspace form for any pattern length (the library's choice), and a form that
 * keeps the whole state of a pattern of up to 256 bases in registers; QE_SEARCH_FORM=0 the workspace form always, 1 the
 * register form wherever it applies.
 * quicked_batch_locations: text_start / text_end (n values each, either may be NULL) of the last sync != 0 search run or of
 * the fetch of a queued one; QUICKED_ERROR after any run that was not a search run, as the tag getters.
 *
 * IUPAC degenerate bases (primers and adapters written with R, Y, N ...): one of the two flags below, OR-ed into `mode` of
 * quicked_batch_run_search or quicked_batch_run_search_all, replaces the equality.  Every byte then stands for a set of bases,
 * case folded -- A, C, G, T (U = T); R = AG, Y = CT, S = CG, W = AT, K = GT, M = AC; B = CGT, D = AGT, H = ACT, V = ACG;
 * N = ACGT; any other byte the empty set -- and two symbols are equal when their sets intersect.  The relation is symmetric
 * and not transitive (R = A, R = G, A != G); a byte outside the alphabet equals nothing, itself included.
 *   QUICKED_SEARCH_IUPAC          both sequences are read through the table: a text N matches every pattern symbol
 *   QUICKED_SEARCH_IUPAC_PATTERN  the pattern only: a text byte that is not one of A C G T U (either case) has the empty
 *                                 set, so a poly-N read does not match every adapter
 * On input of upper- or lower-case ACGT only both give exactly the results of the unflagged run.  Everything else -- D, the
 * modes, the results and their tie rules, the bounds, "beyond", empty sequences, the occurrence definition, max_hits, found /
 * stored, queued only_score != 0 runs and their fetch, counters [0], kernel_times slot [0], QE_SEARCH_FORM -- is that of the
 * unflagged run described above and below.  The base mode (mode & 15) must be PREFIX or INFIX, at most one of the two flags
 * may be set and no other bit: anything else is QUICKED_ERROR, nothing is launched.  A flagged quicked_batch_run_search with
 * only_score == 0 returns QUICKED_UNIMPLEMENTED and queues nothing (the traceback and the formatter compare raw bytes: a
 * CIGAR's edit count would not be d).  Packed batches: QUICKED_WIRE_2BIT holds ACGT only; the fifth symbol of
 * QUICKED_WIRE_PLANES3 is N -- the full set under QUICKED_SEARCH_IUPAC, under QUICKED_SEARCH_IUPAC_PATTERN the full set in
 * patterns and the empty set in texts -- so a packed batch and the ASCII batch of the same sequences over ACGTN agree.
 * A flagged run packs four base-membership planes of the batch into its own pool first. */
typedef enum { QUICKED_SEARCH_PREFIX = 1, QUICKED_SEARCH_INFIX = 2 } quicked_search_mode_t;
enum { QUICKED_SEARCH_IUPAC = 16, QUICKED_SEARCH_IUPAC_PATTERN = 32 };
quicked_status_t quicked_batch_run_search(quicked_batch_t* batch, int mode,
                                          const int32_t* max_dist, int32_t max_dist_all,
                                          int only_score, int sync);
quicked_status_t quicked_batch_locations(quicked_batch_t* batch, int32_t* text_start, int32_t* text_end); /* n each */
/* Every occurrence within the bound, not only the best: "where does the pattern occur in this text within k edits?" -- a primer
 * in a window of a genome, an adapter that occurs twice in a chimeric read, a barcode in a read with a tandem repeat.
 * D, the modes, the equality, the per-pair bound (max_dist / max_dist_all, clamped to m) and the treatment of empty sequences
 * are those of quicked_batch_run_search.  Let R[e] = D[m][e] for e = 1 .. n and k the pair's effective bound; column 0 counts as
 * higher than every value.  Position e is an occurrence when
 *   R[e] <= k,
 *   R[e] < R[e-1]  (which holds for e = 1 by the convention above), and
 *   the first e' > e with R[e'] != R[e], if there is one, has R[e'] > R[e]:
 * e is the first column of a valley of row m; a valley's plateau counts once, and a plateau that reaches the end of the text
 * counts.  The occurrence's score is R[e], its text_end is e (exclusive, as above); text_start is 0 for PREFIX, for INFIX the
 * smallest s for which the global distance of the pattern against text[s, e) is score -- the rule of the best search.  A
 * pair's occurrences are ordered by text_end.  Two consequences: the set depends on min(R[e], k + 1) only; and the smallest
 * score among a pair's occurrences, with the first occurrence that has it, is exactly {score, text_start, text_end} of
 * quicked_batch_run_search for the same bound (d == m included).  For upper-case ACGT input with d != m the occurrences of
 * score d are edlib's endLocations + 1 with every member whose predecessor is also in the list removed, and its startLocations
 * of those.
 * Results: quicked_batch_hit_counts gives found[i], the number of occurrences of pair i -- exact whatever the cap -- and
 * stored[i] = min(found[i], max_hits): the stored occurrences are the first ones by text_end, hits[hit_off[i] .. hit_off[i+1])
 * of quicked_batch_hits (hit_off has n + 1 entries; quicked_batch_hit_total = hit_off[n] sizes the array).  quicked_batch_scores
 * after such a run gives the smallest score among ALL found occurrences, stored or not, so "is pair i within k?" stays exact
 * under any cap; a pair without an occurrence gets -1 with QUICKED_OK.  Empty sequences keep QUICKED_EMPTY_SEQUENCE and have no
 * occurrences.  quicked_batch_locations, the CIGAR getters and the tag getters return what they return after any run that
 * produced none of their data; the three getters here return QUICKED_ERROR (the total: -1) after any run that was not an
 * all-occurrences run.
 * max_hits must be in 1 .. 4096 and (the number of pairs without an empty sequence) x max_hits at most 2^26; otherwise, and for
 * a NULL batch, an unknown mode or a negative bound: QUICKED_ERROR, nothing is launched.  sync == 0: QUICKED_UNIMPLEMENTED,
 * nothing is queued (the start pass is sized from a total that the host reads between the two passes); so is a batch configured
 * with check != 0, as for quicked_batch_run_search.  The tags of quicked_batch_configure_tags are ignored: these runs produce
 * no alignments.  ASCII and packed batches alike; N, lower-case and IUPAC bytes under the library's equality.  Counters [0] and
 * kernel_times slot [0] count the passes, as for a search run.  Both kernel forms of quicked_batch_run_search (QE_SEARCH_FORM);
 * the forward pass cannot lower its bound or stop at an exact occurrence, so it walks every text to its end. */
typedef struct { int32_t text_start, text_end, score; } quicked_hit_t;          /* 12 bytes */
quicked_status_t quicked_batch_run_search_all(quicked_batch_t* batch, int mode,
                                              const int32_t* max_dist, int32_t max_dist_all,
                                              int32_t max_hits, int sync);
quicked_status_t quicked_batch_hit_counts(quicked_batch_t* batch, int32_t* found, int32_t* stored); /* n each, either may be NULL */
int64_t          quicked_batch_hit_total(quicked_batch_t* batch);               /* sum of stored; -1 after any other run */
quicked_status_t quicked_batch_hits(quicked_batch_t* batch, quicked_hit_t* hits, int64_t* hit_off /* n + 1 */);
/* Panel search: every text of the batch against ONE shared set of patterns -- n reads against a panel of barcodes, adapters or
 * primers: "which panel member fits this text best, how well, where, and how far behind is the runner-up?"
 * Texts and patterns.  The texts are the texts of the batch's pairs; the batch's own patterns are ignored and may all be empty.
 * The panel is host ASCII, read during the call, laid out like a batch pool: member p is the panel_len[p] bytes at
 * panel_pool + panel_off[p].
 * Per text i and panel member p, {d, text_end} is exactly what quicked_batch_run_search defines for that pattern against that
 * text: the same mode, the same equality, the bound clamped to m.  Member p's bound is max_dist[p] (n_patterns values), or
 * max_dist_all where max_dist is NULL; d > bound means p is beyond for this text.
 * Per text result.  The members within their bound are ordered by the key (score, panel index), ascending.  pattern / score are
 * the smallest key; second_pattern / second_score are the smallest key among the other members -- a duplicate of the best, at a
 * higher index, is the runner-up with the same score; -1 is reported where there is none.  text_end is the best member's;
 * text_start is 0 for PREFIX, for INFIX it follows the best search's rule (the longest stretch with distance score), and it is
 * computed for the best member only.
 * Other getters.  quicked_batch_scores gives score per text, or -1 with QUICKED_OK when no member is within its bound;
 * QUICKED_EMPTY_SEQUENCE is reported for an empty text only (every field of its result is -1): the batch pattern's length
 * plays no part.
 * QUICKED_PANEL_MATRIX, OR-ed into mode, additionally keeps every {d or -1, text_end or -1}: quicked_batch_panel_matrix copies
 * them as [text][pattern], n * n_patterns values each (the rows of empty texts are -1).  Without the flag the matrix getter
 * returns QUICKED_ERROR.
 * QUICKED_SEARCH_IUPAC and QUICKED_SEARCH_IUPAC_PATTERN apply as in a search run; panel members are the "pattern" side.  ASCII
 * and packed batches alike, with the same reading of the fifth symbol of QUICKED_WIRE_PLANES3 as in flagged search runs.
 * QUICKED_ERROR, nothing launched: a NULL batch; a base mode that is not PREFIX or INFIX; both IUPAC flags, or an unknown bit;
 * n_patterns outside 1 .. QUICKED_PANEL_MAX_PATTERNS; a member of length 0; a negative bound; with the matrix flag, (texts) x
 * n_patterns above 2^28 (every text of the batch has a row in the matrix, the empty ones too).
 * QUICKED_UNIMPLEMENTED, nothing queued: a member longer than QUICKED_PANEL_MAX_LEN bases (the register form's limit); sync == 0;
 * a batch configured with check != 0 (as for the other search runs).  (sync == 0 is accepted on a batch object that
 * quicked_batch_configure_panel_queue, below, switched on -- never with QUICKED_PANEL_MATRIX.)
 * No alignments: the tags of quicked_batch_configure_tags are ignored; the CIGAR, tag, location and hit getters return what
 * they return after any run that produced none of their data.  The two panel getters return QUICKED_ERROR after any run that
 * was not a panel run.  Counters [0] and kernel_times slot [0] count the passes' block steps and launches, as for a search
 * run. */
enum { QUICKED_PANEL_MAX_PATTERNS = 4096, QUICKED_PANEL_MAX_LEN = 256 };
enum { QUICKED_PANEL_MATRIX = 64 };            /* OR-ed into mode, beside the two IUPAC flags */
typedef struct { int32_t pattern, score, text_start, text_end, second_pattern, second_score; } quicked_panel_hit_t; /* 24 bytes */
quicked_status_t quicked_batch_run_panel(quicked_batch_t* batch, int mode,
                                         int32_t n_patterns, const char* panel_pool, const int64_t* panel_off, const int32_t* panel_len,
                                         const int32_t* max_dist /* n_patterns values, or NULL */, int32_t max_dist_all, int sync);
quicked_status_t quicked_batch_panel_results(quicked_batch_t* batch, quicked_panel_hit_t* out /* n */);
quicked_status_t quicked_batch_panel_matrix(quicked_batch_t* batch, int32_t* scores, int32_t* text_ends /* n * n_patterns each, [text][pattern]; either may be NULL */);

/* Panel search, every occurrence: per text, every occurrence of every panel member -- both primers of an amplicon with start and
 * end, an adapter that occurs twice in a chimeric read, a 5' and a 3' barcode from one panel.
 *
 * Texts, the panel, the modes, both IUPAC flags and packed batches are exactly those of quicked_batch_run_panel (the reading of
 * the fifth symbol of PLANES3 and "the batch's own patterns are ignored" included).  A member's bound is max_dist[p] or
 * max_dist_all, clamped to m.  For text i and member p the occurrences are exactly those quicked_batch_run_search_all defines
 * for that pattern against that text with that bound: the valley rule, plateaus, text_start by the best search's rule, 0 for
 * PREFIX.  A text's occurrences are ordered by (pattern, text_end), ascending.  found[i] is their exact number over all members,
 * whatever the cap; stored[i] = min(found[i], max_hits), and the stored ones are the first in that order, at
 * hits[hit_off[i] .. hit_off[i + 1]).  quicked_batch_scores after such a run gives the smallest score among all found
 * occurrences of the text, stored or not, and -1 with QUICKED_OK when there are none.  An empty text keeps
 * QUICKED_EMPTY_SEQUENCE and has no occurrences.
 *
 * Two consequences (tests/test_gpu_panel_hits.py checks both):
 *  1. the smallest key (score, pattern) among a text's occurrences, with the first occurrence that has it, is {pattern, score,
 *     text_start, text_end} of quicked_batch_run_panel for the same panel and bounds; the smallest key among the occurrences of
 *     the other members is its {second_pattern, second_score};
 *  2. member p's smallest score, and the first end that has it, is the QUICKED_PANEL_MATRIX entry [i][p].
 *
 * QUICKED_ERROR, nothing launched: a NULL batch; a base mode that is not PREFIX or INFIX; both IUPAC flags or any other bit but
 * QUICKED_PANEL_CIGARS (QUICKED_PANEL_MATRIX too: it has no meaning here); n_patterns outside 1 .. QUICKED_PANEL_MAX_PATTERNS; a member of length 0;
 * a negative bound; max_hits outside 1 .. 4096; (non-empty texts) x max_hits above 2^26.
 * QUICKED_UNIMPLEMENTED, nothing queued: a member longer than QUICKED_PANEL_MAX_LEN bases; sync == 0 (the host reads the total
 * between the passes; a batch object that quicked_batch_configure_panel_queue, below, switched on gives the room instead and
 * is accepted); a batch configured with check != 0.
 * The three getters below return QUICKED_ERROR (the total: -1) after any run that was not of this kind;
 * quicked_batch_panel_results, quicked_batch_panel_matrix, quicked_batch_hits, quicked_batch_hit_counts,
 * quicked_batch_locations and the CIGAR and tag getters return what they return after any run that produced none of their
 * data.  Tags are ignored.  Counters [0] and kernel_times slot [0] count both passes, as for the other search runs.  A reload
 * clears the results.  QUICKED_PANEL_TAILS and QUICKED_PANEL_HEADS (below) add the members a text's end or start cuts off.
 * Not built: members over 256 bases, alignments for quicked_batch_run_panel and
 * quicked_batch_run_search_all (this run has them: QUICKED_PANEL_CIGARS below), statistics and MD tags per occurrence. */
typedef struct { int32_t pattern, text_start, text_end, score; } quicked_panel_occ_t;   /* 16 bytes */
quicked_status_t quicked_batch_run_panel_all(quicked_batch_t* batch, int mode,
                                             int32_t n_patterns, const char* panel_pool, const int64_t* panel_off, const int32_t* panel_len,
                                             const int32_t* max_dist /* n_patterns values, or NULL */, int32_t max_dist_all,
                                             int32_t max_hits, int sync);
quicked_status_t quicked_batch_panel_hit_counts(quicked_batch_t* batch, int32_t* found, int32_t* stored /* n each; either may be NULL */);
int64_t          quicked_batch_panel_hit_total(quicked_batch_t* batch);   /* the sum of stored; -1 after any other run */
quicked_status_t quicked_batch_panel_hits(quicked_batch_t* batch, quicked_panel_occ_t* hits, int64_t* hit_off /* n + 1 */);
/* Windowed panel search: quicked_batch_run_panel_all for a few LONG texts -- contigs, a bacterial genome, 100 kb reads.  That
 * run gives every text one lane; this one cuts every text into windows of `window` columns and gives every window a lane, so a
 * 5 Mb text occupies the chip instead of one lane of one wave.
 *
 * The contract is one sentence: for every input it accepts it leaves exactly the results quicked_batch_run_panel_all leaves for
 * the same batch, panel, mode, bounds and max_hits, whatever `window` is -- found, stored, every stored occurrence in (pattern,
 * text_end) order and which ones the cap keeps; quicked_batch_scores, the statuses, empty texts; both IUPAC flags; ASCII and
 * packed batches with the same reading of PLANES3's fifth symbol.  A lane owns the occurrences whose text_end lies in its window;
 * it warms up over the 64 ceil((m + k) / 64) columns before the window (no occurrence of a member of m bases within its bound k
 * is longer than m + k) and follows a plateau that is still pending at the window's end until it rises, falls or the text ends
 * (DESIGN.md 4.14.2 has the argument).  The three getters above serve it: a scan run is a run of their kind; every other getter
 * behaves as after quicked_batch_run_panel_all.  Counters [0] and kernel_times slot [0] count both passes; the block steps are
 * the ones really walked, warm-up and run-out columns included.
 *
 * window: the text columns a lane owns.  0: the library's choice (a multiple of 64, at least 1024 and eight warm-ups, small
 * enough that the windows and the panel's slices fill the chip about twice, widened until the rule below holds).  Otherwise a
 * multiple of 64 that is at least 64.
 *
 * QUICKED_ERROR, nothing launched: everything quicked_batch_run_panel_all answers so (a NULL batch; a base mode that is not PREFIX
 * or INFIX; unknown bits, QUICKED_PANEL_MATRIX; n_patterns out of range; an empty member; a negative bound; max_hits outside
 * 1 .. 4096; (non-empty texts) x max_hits above 2^26); a window that is negative, not a multiple of 64 or above 2^31 - 64; with a
 * forced window, (window slots of the batch = the sum of ceil(n / window) over the texts) x max_hits above 2^26.
 * QUICKED_UNIMPLEMENTED, nothing queued: the base mode QUICKED_SEARCH_PREFIX (a PREFIX occurrence within the bound ends in the
 * first m + k columns: quicked_batch_run_panel_all serves it); a member longer than QUICKED_PANEL_MAX_LEN bases; sync == 0; a
 * batch configured with check != 0.
 * Not built: a cap above 4096 per text, queued runs, members over 256 bases, alignments of occurrences of
 * quicked_batch_run_panel and _run_search_all (this run and quicked_batch_run_panel_all have them: QUICKED_PANEL_CIGARS below),
 * statistics and MD tags per occurrence, and windows for quicked_batch_run_panel / _run_search / _run_search_all. */
quicked_status_t quicked_batch_run_panel_scan(quicked_batch_t* batch, int mode,
                                              int32_t n_patterns, const char* panel_pool, const int64_t* panel_off, const int32_t* panel_len,
                                              const int32_t* max_dist /* n_patterns values, or NULL */, int32_t max_dist_all,
                                              int32_t max_hits, int32_t window, int sync);
/* The alignment of every stored occurrence.  QUICKED_PANEL_CIGARS is OR-ed into `mode` of quicked_batch_run_panel_all and
 * quicked_batch_run_panel_scan, beside the two IUPAC flags.  Without the bit nothing about either run changes.  With it every
 * result the unflagged run leaves is left unchanged -- found, stored, the records and their order, scores, statuses, counter
 * [0], the refusals of the other getters; quicked_batch_cigars still returns -1 for every pair -- and every stored occurrence j
 * (the index into quicked_batch_panel_hits' array) gets the CIGAR of the GLOBAL alignment of its member against
 * text[text_start, text_end), in the cigar_style of quicked_batch_configure (0, 1, 2, style 2 with the "1X" of a leading mismatch
 * as the pair runs print it).
 *
 * Which alignment.  D is the edit-distance matrix of the member (rows 1 .. m) against the stretch (columns 1 .. L) with
 * D[0][j] = j and D[i][0] = i.  From (m, L), while i > 0 and j > 0: D[i][j] == D[i-1][j] + 1 emits D and decrements i; else
 * D[i][j-1] == D[i-1][j-1] - 1 emits I and decrements j; else M where the two symbols are equal, X where not, and both are
 * decremented.  The columns left are I, the rows left D; the string is that sequence reversed.  This is the traceback of the pair
 * runs (the reference's) on the full matrix: on ACGT input the string is the one quicked_batch_run_bounded gives for (member,
 * stretch) with bound = score.  It has exactly `score` edits, consumes m member symbols (M X D) and text_end - text_start text
 * symbols (M X I), and never ends with I; an INFIX string never begins with I either (a PREFIX stretch starts at column 0
 * wherever the occurrence does, so its string may).
 * M means "equal under the run's equality": under the flags the sets intersect (R against A is M; a text N under
 * QUICKED_SEARCH_IUPAC_PATTERN is X); unflagged, case is folded and any two bytes that are not A C G T are equal.  I consumes
 * text, D consumes the member, as in every CIGAR of this library.
 *
 * quicked_batch_panel_hit_cigars copies the pool (quicked_batch_panel_hit_cigar_bytes bytes) and one offset per stored
 * occurrence (quicked_batch_panel_hit_total of them); the string of occurrence j is NUL-terminated at pool + off[j].  off[j]
 * is never -1 for a stored occurrence of a run that returned QUICKED_OK.  The pool is padded between the strings (with unspecified bytes): only off and
 * the strings are the contract.  Both getters return QUICKED_ERROR / -1 after any run without the bit and after a reload.
 * A run returns QUICKED_ERROR with off[j] = -1 where the aligner did not reach (0, 0) with the occurrence's score: the sweeps
 * and the aligner disagree, which is a defect of the library and is not hidden.
 *
 * QUICKED_ERROR, nothing launched: the bit on quicked_batch_run_panel (any unknown bit there: the best member's alignment is the
 * first record with the smallest key of quicked_batch_run_panel_all); the bit together with QUICKED_PANEL_MATRIX.  Every other
 * refusal of the two runs stands.  The tags of quicked_batch_configure_tags stay ignored.
 * Counters: [0] and kernel_times slot [0] are the unflagged run's; counter [1] is the block steps of the alignment sweep,
 * counter [3] the operations emitted, kernel_times slot [1] the alignment launches (QE_PANEL_ALIGN_WS_KB bounds the pass's
 * workspace; more occurrences than fit are aligned in several launches).
 * Not built: alignments for quicked_batch_run_panel and quicked_batch_run_search_all (whose patterns may exceed 256 bases),
 * statistics and MD tags per occurrence, queued runs. */
enum { QUICKED_PANEL_CIGARS = 512 };           /* OR-ed into mode of quicked_batch_run_panel_all / _scan, beside the two IUPAC flags (128 and 256 stay unknown bits) */
int64_t          quicked_batch_panel_hit_cigar_bytes(quicked_batch_t* batch);   /* -1 unless the last run was a flagged run */
quicked_status_t quicked_batch_panel_hit_cigars(quicked_batch_t* batch, char* pool, int64_t* off /* hit_total entries */);
/* A member cut off by the text's end (3' tails).  QUICKED_PANEL_TAILS is OR-ed into `mode` of quicked_batch_run_panel_all,
 * beside the two IUPAC flags and QUICKED_PANEL_CIGARS.  Without the bit nothing about the run changes.  With it every result the
 * unflagged run leaves is left unchanged -- found, stored, the records and their order, quicked_batch_scores, the statuses,
 * counter [0], the strings of a QUICKED_PANEL_CIGARS run, the refusals of the other getters -- and every text gets one record
 * besides: the panel member whose beginning the text ends in.  A read that runs into its 3' adapter ends with the adapter's
 * first r < m bases; row m of the matrix never comes within the bound there, so the occurrences above do not see it.
 *
 * The definition.  Text i has n >= 1 bases, member p has m bases and the effective bound k = min(bound, m); D is the INFIX
 * matrix (D[0][j] = 0) under the run's equality, IUPAC flags included.  Row r is a tail of p in i when
 *     min_overlap <= r <= m - 1   and   D[r][n] <= floor(r * k / m):
 * the member's first r bases fit a stretch that ends at the text's end, at the member's own error rate.  The member's tail is
 * the tail row with the largest matched length r - D[r][n]; on a tie the smaller D[r][n] (r is then determined).  The text's
 * tail is the best member's by the same two keys, then the smaller member index.  The record is {pattern, overlap = r,
 * text_start, score = D[r][n]}: text_start is the smallest s with ed(member[0:r], text[s:n]) == score -- the longest stretch, the
 * best search's rule --, the stretch's end is always n.  Every field is -1 where no member has a tail; an empty text has none.
 * Tails say nothing about full occurrences and full occurrences nothing about tails: a text may have both, and the caller
 * decides.  Row m is not a tail; it is the occurrence scan's.
 *
 * quicked_batch_configure_panel_tails sets min_overlap for the runs to come (default 3); QUICKED_ERROR outside
 * 1 .. QUICKED_PANEL_MAX_LEN.  quicked_batch_panel_tails copies the n records; QUICKED_ERROR after any run without the bit and
 * after a reload.  A run returns QUICKED_ERROR with text_start = -1 where the start pass did not find the tail's score: the
 * two passes disagree, which is a defect of the library and is not hidden.
 *
 * QUICKED_ERROR, nothing launched: the bit with the base mode QUICKED_SEARCH_PREFIX (D[0][n] = n there: a tail means nothing);
 * the bit on quicked_batch_run_panel, _run_panel_scan, _run_search and _run_search_all (an unknown bit there).  Every other
 * refusal of quicked_batch_run_panel_all stands (sync == 0, members over 256 bases, check != 0).
 * Counters: [2] is the row steps of the walk down the last column; [0], [1] and [3] keep their meaning.
 * Counters [6] and [7] are a QUICKED_PANEL_HEADS run's (below), 0 otherwise.
 * Not built: tails on quicked_batch_run_panel_scan; one tail per member instead of one per text; tail CIGARs.  (5' tails, a
 * member's suffix at the text's start, are QUICKED_PANEL_HEADS below.) */
enum { QUICKED_PANEL_TAILS = 2048 };           /* OR-ed into mode of quicked_batch_run_panel_all (1024 stays an unknown bit) */
typedef struct { int32_t pattern, overlap, text_start, score; } quicked_panel_tail_t;   /* 16 bytes */
quicked_status_t quicked_batch_configure_panel_tails(quicked_batch_t* batch, int32_t min_overlap);
quicked_status_t quicked_batch_panel_tails(quicked_batch_t* batch, quicked_panel_tail_t* out /* n */);
/* A member cut off by the text's start (5' heads).  QUICKED_PANEL_HEADS is OR-ed into `mode` of quicked_batch_run_panel_all,
 * beside the two IUPAC flags, QUICKED_PANEL_CIGARS and QUICKED_PANEL_TAILS; all three bits may be set in one run.  Without the
 * bit nothing about any run changes: no launch, no allocation, no copy.  With it every result the unflagged run leaves is left
 * unchanged -- found, stored, the records and their order, quicked_batch_scores, the statuses, counters [0] .. [3], the strings
 * of a QUICKED_PANEL_CIGARS run, the tails of a QUICKED_PANEL_TAILS run, the refusals of the other getters -- and every text
 * gets one record besides: the panel member whose end the text begins with.  A read whose 5' adapter, barcode or primer was
 * partly clipped, or that starts mid-adapter, begins with the member's last r < m bases; row m of the matrix never comes within
 * the bound there, so the occurrences above do not see it.  With the tails one run answers all three questions of a trimming
 * tool: is the whole member there, does the read run into it at its end, does the read start inside it.
 *
 * The definition.  Text i has n >= 1 bases, member p has m bases and the effective bound k = min(bound, m); rev() is plain
 * reversal, no complement (every equality of the library is position-wise symmetric); D^R is the INFIX matrix (D^R[0][j] = 0)
 * of rev(member) against rev(text) under the run's equality, IUPAC flags included.  Row r is a head of p in i when
 *     min_overlap <= r <= m - 1   and   D^R[r][n] <= floor(r * k / m):
 * the member's last r bases, member[m-r:m], fit a stretch text[0:e) at the member's own error rate.  The tie rules are the
 * tails': the member's head is the head row with the largest matched length r - D^R[r][n]; on a tie the smaller score.  The
 * text's head is the best member's by the same two keys, then the smaller member index.  The record is {pattern, overlap = r,
 * text_end, score = D^R[r][n]}: text_end is the largest e with ed(member[m-r:m], text[0:e)) == score -- the longest stretch,
 * the best search's rule mirrored --, the stretch's start is always 0.  Every field is -1 where no member has a head; an empty
 * text has none.  In one sentence: the heads of (texts, panel) are the tails of (reversed texts, reversed members) with
 * text_end = n - text_start.  Row m is not a head; it is the occurrence scan's.
 *
 * The base mode may be INFIX or PREFIX: the heads' matrix is its own and does not depend on the occurrences' (PREFIX together
 * with QUICKED_PANEL_TAILS stays QUICKED_ERROR, because of the tails).  A head of member p depends only on the first m + k
 * columns of the text, however long the text is, and that is all the run walks for it.
 *
 * quicked_batch_configure_panel_heads sets min_overlap for the runs to come (default 3), independently of the tails' setting;
 * QUICKED_ERROR outside 1 .. QUICKED_PANEL_MAX_LEN.  quicked_batch_panel_heads copies the n records; QUICKED_ERROR after any run
 * without the bit and after a reload.  A run returns QUICKED_ERROR with text_end = -1 where the end pass did not find the
 * head's score: the two passes disagree, which is a defect of the library and is not hidden.
 *
 * QUICKED_ERROR, nothing launched: the bit on quicked_batch_run_panel, _run_panel_scan, _run_search and _run_search_all (an
 * unknown bit there).  Every other refusal of quicked_batch_run_panel_all stands (sync == 0, members over 256 bases,
 * check != 0).
 * Counters, in a flagged run only (0 otherwise): [6] is the block steps of the head sweep, [7] the row steps of its walk;
 * [0] .. [3] keep their meaning and their values.  kernel_times slot [0] includes the head kernels.
 * Not built: heads or tails on quicked_batch_run_panel_scan; one head per member instead of one per text; head and tail CIGARs;
 * reverse-complement members.  (For queued (sync == 0) panel runs see quicked_batch_configure_panel_queue below.) */
enum { QUICKED_PANEL_HEADS = 8192 };           /* OR-ed into mode of quicked_batch_run_panel_all (128, 256, 1024 and 4096 stay unknown bits) */
typedef struct { int32_t pattern, overlap, text_end, score; } quicked_panel_head_t;   /* 16 bytes */
quicked_status_t quicked_batch_configure_panel_heads(quicked_batch_t* batch, int32_t min_overlap);
quicked_status_t quicked_batch_panel_heads(quicked_batch_t* batch, quicked_panel_head_t* out /* n */);
/* Queued panel runs.  Every panel run is sync != 0 only on a batch object as it is created.  A demultiplexing or trimming job --
 * thousands of batches against one fixed panel -- wants what pair runs have: runs that rotate over sets of {stream, pool,
 * planes}, a thread that reloads the next batch object meanwhile, quicked_batch_fetch later.  That is opt-in per batch object:
 *
 * quicked_batch_configure_panel_queue(batch, max_total).  0, the default of every batch, is off: every panel run with
 * sync == 0 answers QUICKED_UNIMPLEMENTED with nothing queued.  1 .. 2^26 is on.  Anything else, or a NULL batch, is
 * QUICKED_ERROR and leaves the setting unchanged.  Runs with sync != 0 never look at the setting: no launch, no allocation, no
 * copy of theirs changes.  A reload keeps the setting.
 *
 * With the setting on, sync == 0 is accepted by quicked_batch_run_panel (PREFIX and INFIX, both IUPAC flags) and by
 * quicked_batch_run_panel_all (PREFIX and INFIX, both IUPAC flags, QUICKED_PANEL_TAILS, QUICKED_PANEL_HEADS, in every combination
 * the sync run accepts).  Every QUICKED_ERROR rule of the two runs comes first, as before; a member over 256 bases and
 * check != 0 stay QUICKED_UNIMPLEMENTED.  The run returns what a queued quicked_batch_run_search returns.  The panel and
 * max_dist are read during the call: the caller may free them on return.  Between the call and quicked_batch_fetch every
 * getter answers exactly as before the call -- panel getters, scores, counters, and which kind of run the last one was.  The
 * rules of queued runs hold: the results move into the batch's own result arena at the end of the run; any number of runs of
 * OTHER batch objects may be queued before the fetch; the batch's next run, a reload or destroy discards the run; any thread
 * may fetch.
 *
 * What the fetch brings.  quicked_batch_run_panel: everything the sync run leaves, bit for bit.  quicked_batch_run_panel_all:
 * let W be the total the sync run would store, its hit_off[n].  found, quicked_batch_scores, the statuses, the tails, the
 * heads and counters [2], [6], [7] are the sync run's whatever max_total is.  If W <= max_total so is everything else: stored,
 * hit_off, every record, counter [0].  If W > max_total the fetch still returns QUICKED_OK and the records are the first
 * max_total of the sync run's array -- which is in the order of the pairs, then (pattern, text_end) --:
 *     hit_off'[i] = min(hit_off[i], max_total),   stored'[i] = hit_off'[i + 1] - hit_off'[i],
 * and counter [0] counts the block steps really walked.  This is the library's cap rule one level up: a cap per text shows as
 * stored < found, a cap per run as wanted > total.  quicked_batch_panel_queue_wanted returns W after such a fetch, and -1
 * after anything else: a sync run, a fetched quicked_batch_run_panel, a reload, before the fetch.
 * The run takes its records' room -- min(max_total, non-empty texts x max_hits) of them, 16 bytes each, 60 with INFIX -- from
 * its pool whatever W turns out to be, and the start pass launches a lane per record of that room: lanes past W leave at once
 * (DESIGN.md 4.14.6 has what they cost).  max_total also sizes the batch object's own result arena, where the run's results wait
 * for the fetch: 20 bytes per record of that room with INFIX, 16 with PREFIX -- up to 1.3 GB at 2^26 --, allocated at the first
 * queued run that needs it and kept for the object's life.  A caller that rotates several batch objects budgets for one each.
 *
 * QUICKED_UNIMPLEMENTED with sync == 0 as before, nothing queued, setting on or off: QUICKED_PANEL_MATRIX; QUICKED_PANEL_CIGARS
 * (the host reads the strings' total); quicked_batch_run_panel_scan; quicked_batch_run_search_all.
 * Not built: queued runs with the matrix or the strings, of the windowed run and of quicked_batch_run_search_all; a room that
 * grows by itself (a run that overflowed is run again with max_total >= wanted). */
quicked_status_t quicked_batch_configure_panel_queue(quicked_batch_t* batch, int64_t max_total);
int64_t          quicked_batch_panel_queue_wanted(quicked_batch_t* batch);
/* Panel search by mismatches only.  QUICKED_PANEL_NO_INDELS is OR-ed into `mode` of quicked_batch_run_panel and
 * quicked_batch_run_panel_all, beside the two IUPAC flags; on quicked_batch_run_panel it also stands beside
 * QUICKED_PANEL_MATRIX.  Without the bit nothing about any run changes: no launch, no allocation, no copy.  With it the two
 * runs answer under the other distance a panel job comes with: index reads and inline barcodes at a fixed position, guide
 * counting, UMI whitelists, a trimmer's "no indels".  Edit distance is a lower bound of the mismatch count, so the unflagged
 * runs report members and positions this run must not, and their results cannot be turned into its.
 *
 * The definition.  Text i has n bases, member p has m bases and the effective bound k = min(bound[p], m); the bounds are
 * max_dist / max_dist_all as in the unflagged runs.  For a start s with 0 <= s <= n - m
 *     H[s] = #{ r in [0, m) : member[r] and text[s + r] are NOT equal under the run's equality },
 * the equality being the unflagged run's: case folded and any two non-ACGT bytes equal; QUICKED_SEARCH_IUPAC: the base sets
 * intersect; QUICKED_SEARCH_IUPAC_PATTERN: a text byte outside ACGTU is the empty set and mismatches everything.  R[e] =
 * H[e - m] for the ends e in E: INFIX E = {m, .., n}, PREFIX E = {m}, n < m: E is empty.  Every column outside E counts as
 * higher than every value.  From here every sentence of the two runs' contracts above holds with D[m][e] read as R[e]:
 *   quicked_batch_run_panel: member p's d = min over E of R, text_end the smallest e that has it; d > k or an empty E: p is
 *     beyond for this text.  Keys, best, runner-up, quicked_batch_scores, empty texts and QUICKED_PANEL_MATRIX as there.
 *     text_start = text_end - m always (0 with PREFIX); no start pass is launched.
 *   quicked_batch_run_panel_all: e is an occurrence when R[e] <= k, R[e] < R[e - 1], and the first e' > e in E with R[e'] !=
 *     R[e], if there is one, has R[e'] > R[e] -- the valley rule, a plateau counted once.  The record is {p, e - m, e, R[e]};
 *     the order, found / stored, the max_hits cap and quicked_batch_scores as there.  Both consequences listed there hold
 *     between the two flagged runs.
 * ASCII and packed batches alike, with the unflagged runs' reading of PLANES3's fifth symbol; QE_PANEL_SLICES as there.
 *
 * Every QUICKED_ERROR rule of the two runs comes first, unchanged.  QUICKED_UNIMPLEMENTED, nothing launched, with the bit:
 * QUICKED_PANEL_CIGARS, QUICKED_PANEL_TAILS or QUICKED_PANEL_HEADS beside it; sync == 0, also on a batch object that
 * quicked_batch_configure_panel_queue switched on; a member over QUICKED_PANEL_MAX_LEN; check != 0.
 * QUICKED_ERROR, nothing launched: the bit on quicked_batch_run_panel_scan, _run_search and _run_search_all (an unknown bit
 * there).
 * Counters: [0] is the block steps walked -- per (text, member) the start positions (n - m + 1, or 1 with PREFIX, or 0) x
 * ceil(m / 64) --, [1] .. [7] are 0 ([5] too: the kernels' time is kernel_times slot [0]'s).  kernel_times slot [0] holds the
 * launches.
 * Not built: CIGARs, tails and heads under the bit; queued flagged runs; the windowed run under the bit; the bit for
 * quicked_batch_run_search / _run_search_all; members over 256 bases; reverse-complement members; a per-member choice of
 * distance within one run. */
enum { QUICKED_PANEL_NO_INDELS = 32768 };      /* OR-ed into mode of quicked_batch_run_panel / _run_panel_all (4, 8, 128, 256, 1024, 4096 and 16384 stay unknown bits) */
/* Windowed panel search by mismatches only: the flagged quicked_batch_run_panel_all for a few LONG texts -- a panel of guides,
 * primers or probes against a genome or the contigs of an assembly: every site within k mismatches, no bulges, a PAM written
 * with IUPAC N.  A function of its own with quicked_batch_run_panel_scan's argument list; QUICKED_PANEL_NO_INDELS on
 * quicked_batch_run_panel_scan itself stays an unknown bit, as said above.  Here the bit in `mode` is accepted and means
 * nothing more: a caller may pass the mode it gives quicked_batch_run_panel_all.
 *
 * The contract is one sentence: for every input it accepts it leaves exactly what quicked_batch_run_panel_all leaves for the
 * same batch, panel, mode | QUICKED_PANEL_NO_INDELS, bounds and max_hits, whatever `window` is -- found, stored, the records
 * in (pattern, text_end) order and which ones the cap keeps; text_start = text_end - m; quicked_batch_scores, the statuses,
 * empty texts; texts shorter than a member; both IUPAC flags; ASCII and both packed wires.  The three getters of
 * quicked_batch_run_panel_all serve it; every other getter behaves as after a flagged quicked_batch_run_panel_all.
 * A lane owns the ends in its window (c0, c1].  R[e] reads text[e - m, e) only, so a lane needs no warm-up: per member it
 * computes the one start c0 - m, whose value is the previous column of its first owned end (c0 < m: no such column, the first
 * owned end is m; c1 < m: the window owns nothing), then its owned ends, then the ends past c1 only while a valley that began
 * in the window is still pending.
 * Counters: [0] is the block steps really walked -- per (window slot, member) the starts from max(0, c0 - m) to the last one
 * of the run-out, x ceil(m / 64) --, [1] .. [7] are 0; the kernels' time is in kernel_times slot [0].
 *
 * window: quicked_batch_run_panel_scan's rules -- 0 (the library's choice) or a multiple of 64, with the same 2^26 rules.
 * QUICKED_ERROR, nothing launched: everything quicked_batch_run_panel_scan answers so; QUICKED_PANEL_MATRIX, QUICKED_PANEL_TAILS
 * and QUICKED_PANEL_HEADS (unknown bits of the scan).
 * QUICKED_UNIMPLEMENTED, nothing launched: the base mode QUICKED_SEARCH_PREFIX; QUICKED_PANEL_CIGARS; sync == 0, also on a batch
 * object that quicked_batch_configure_panel_queue switched on; a member over QUICKED_PANEL_MAX_LEN; check != 0.
 * Not built: CIGARs, tails and heads; queued runs; members over 256 bases; reverse-complement members. */
quicked_status_t quicked_batch_run_panel_scan_no_indels(quicked_batch_t* batch, int mode,
                                              int32_t n_patterns, const char* panel_pool, const int64_t* panel_off, const int32_t* panel_len,
                                              const int32_t* max_dist /* n_patterns values, or NULL */, int32_t max_dist_all,
                                              int32_t max_hits, int32_t window, int sync);
quicked_status_t quicked_batch_sync(quicked_batch_t* batch);
/* Brings the results of the batch's last sync == 0 run to the host: waits for that run (only that one: later runs of
 * this or other batches keep executing) and copies scores / statuses / CIGARs / counters to where the getters read
 * them.  A sync == 0 run itself leaves the getters' data untouched.  At its end such a run moves its results from the
 * queueing thread's rotating pools into memory of the batch object (device to device), so the thread may queue any number
 * of runs of OTHER batch objects before this one is fetched; the batch's own next run, reload or destroy discards them.
 * Any thread may fetch (bench.py's end-to-end leg fetches on a thread of its own) as long as no other call on this batch
 * object runs at the same time; what the fetch itself has to compute runs on the calling thread's streams and pools.
 * QUICKED: the pairs a queued run left for the host-driven stages (those past stage 1, those above the bound estimate)
 * are aligned by library threads as soon as the run is over ("early finish": up to QE_FINISHERS = 3 threads with streams
 * and pools of their own, started when first needed); the fetch then only waits for that.  Calls on one batch object are
 * serialised against such a thread by the library, and such a thread writes into a second set of host-side result buffers
 * that the fetch makes visible: the getters and the zero-copy views keep showing the previous results until the fetch. */
quicked_status_t quicked_batch_fetch(quicked_batch_t* batch);

/* results of the last sync != 0 run or of the last quicked_batch_fetch (host copies) */
quicked_status_t quicked_batch_scores(quicked_batch_t* batch, int32_t* scores_out, int32_t* status_out);
/* total bytes of all CIGAR strings incl. terminators, then the strings themselves
 * (cigar_off[i] = offset of string i in cigar_pool, -1 if none) */
int64_t quicked_batch_cigar_bytes(quicked_batch_t* batch);
quicked_status_t quicked_batch_cigars(quicked_batch_t* batch, char* cigar_pool, int64_t* cigar_off);
/* the same without the copy: pointers into the batch's own (pinned) result buffers, valid until the next sync != 0 run,
 * fetch, reload or destroy of the batch */
quicked_status_t quicked_batch_cigar_view(quicked_batch_t* batch, const char** cigar_pool, const int64_t** cigar_off);

/* Output options of the runs to come.
 * cigar_style: 0 = the reference's RLE "MXID" (cigar_sprint, quicked_utils/src/cigar.c:453-488; default),
 *              1 = SAM CIGAR with mismatches, "=XID", 2 = SAM CIGAR "MID" with X folded into M before
 *              runs are merged (cigar_compute_CIGAR + cigar_sprint_SAM_CIGAR, cigar.c:194-240, 504-529),
 *              byte-identical to that printer including its one quirk: an alignment that STARTS with a
 *              mismatch keeps it as "1X" (the first operation is read before the mapping step).
 * check != 0:  every CIGAR is validated on the device against the raw bytes of its pair, the same walk
 *              as cigar_check_alignment (cigar.c:363-434); verdicts via quicked_batch_check_results
 *              (1 valid, 0 not, -1 the pair has no alignment) after a sync != 0 run. */
quicked_status_t quicked_batch_configure(quicked_batch_t* batch, int cigar_style, int check);
quicked_status_t quicked_batch_check_results(quicked_batch_t* batch, int32_t* ok_out);
/* ---- alignment tags: what a consumer of alignments wants besides, or instead of, the CIGAR strings ----
 * Identity, gap counts and the longest exact stretch per pair cost 32 bytes of D2H per pair; the strings of a 10 kb pair
 * about 2 kB (at 5 % error).  Computed on the device from the traceback's runs.
 *   QUICKED_TAG_STATS     a quicked_pair_stats_t per pair
 *   QUICKED_TAG_MD        the SAM MD:Z string per pair.  (NM is the score: there is no getter of its own.)
 *   QUICKED_TAG_NO_CIGAR  the run aligns -- traceback and all -- but formats and downloads no CIGAR strings: cigar_off is -1
 *                         for every pair and quicked_batch_cigar_bytes 0, scores and statuses are those of the CIGAR run,
 *                         the in-run validator gives -1 for every pair
 * Which runs: those that produce alignments -- only_score == 0 -- through quicked_batch_run with every algo and through
 * quicked_batch_run_bounded.  The default is 0, and then nothing about a run changes: no extra launch, allocation or copy.
 * The per-pair ABI (quicked_align) and quicked_align_batch never set tags.
 * Where the results are: in the getters below after a sync != 0 run.  A sync == 0 run with only_score == 0 on a batch whose
 * tags are not 0 returns QUICKED_UNIMPLEMENTED and queues nothing (as a queued bounded CIGAR run); queued only_score != 0
 * runs ignore the tags.  After a run that produced no tag data (tags 0, or only_score != 0) the getters return
 * QUICKED_ERROR, as quicked_batch_check_results does; so do a NULL batch and unknown bits.
 * Packed batches: STATS and NO_CIGAR work (they need no bases); QUICKED_TAG_MD returns QUICKED_UNIMPLEMENTED from
 * quicked_batch_configure_tags, as the validator does.
 * Pairs without an alignment -- empty sequences, a run-buffer overflow (score -1, QUICKED_ERROR), "beyond" in a bounded run --
 * get statistics of all -1 and md_off -1.
 *
 * Both are functions of the alignment's operation sequence -- what the style-0 CIGAR expands to, whatever style is
 * configured; I consumes text, D consumes pattern -- with runs maximal (equal neighbours merged), and of the pattern's raw bytes.
 * Statistics: the M / X / I / D columns, the numbers of maximal I and D runs, the longest maximal M run, all columns; hence
 *   matches + mismatches + del_bases == pattern_len,  matches + mismatches + ins_bases == text_len,
 *   mismatches + ins_bases + del_bases == score.
 * MD is over the sequence D consumes: in the SAM styles this library prints I consumes the text, so the text is SAM's query
 * and the PATTERN is SAM's reference: MD names pattern bytes, raw as stored, no case folding.  A number of matches, then per
 * mismatch the pattern byte (neighbouring mismatches separated by "0"), per deletion run '^' and its pattern bytes; an
 * insertion emits nothing and does not reset the count, but separates two deletion runs ("^AC0^GT"); the count at the end.
 * quicked_batch_md_bytes / quicked_batch_md: pool and offsets laid out like the CIGAR getters' (NUL-terminated strings,
 * md_off[i] -1: none). */
enum { QUICKED_TAG_STATS = 1, QUICKED_TAG_MD = 2, QUICKED_TAG_NO_CIGAR = 4 };
typedef struct {            /* 32 bytes; all -1 for a pair without an alignment */
    int32_t matches, mismatches, ins_bases, del_bases, ins_runs, del_runs, longest_match, columns;
} quicked_pair_stats_t;
quicked_status_t quicked_batch_configure_tags(quicked_batch_t* batch, int tags);
quicked_status_t quicked_batch_pair_stats(quicked_batch_t* batch, quicked_pair_stats_t* stats_out /* n */);
int64_t          quicked_batch_md_bytes(quicked_batch_t* batch);
quicked_status_t quicked_batch_md(quicked_batch_t* batch, char* md_pool, int64_t* md_off);   /* md_off -1: none */

/* The same validator for CIGAR strings from anywhere ("<len><op>", op in MXID, '=' read as M): string i is
 * cigar_pool + cigar_off[i], NUL-terminated, against the batch's resident pair i; cigar_off[i] < 0 -> -1.
 * What `align_benchmark -c correct` does per pair on the host (benchmark_check.c), at batch scale.
 * A length is decimal, at least 1 and at most 2147483647 (leading zeros allowed); a longer number, a zero, digits without an
 * operation, an operation without digits and any other byte make the string invalid (0), as does the first operation that
 * would leave either sequence -- whatever its length: no string makes the walk read outside its pair, and no sum of lengths
 * wraps back into it.  The empty string is the alignment of two empty sequences.  An offset >= pool_bytes: QUICKED_ERROR,
 * ok_out untouched. */
quicked_status_t quicked_batch_validate(quicked_batch_t* batch, const char* cigar_pool, int64_t pool_bytes,
                                        const int64_t* cigar_off, int32_t* ok_out);

/* counters of the last run, for the measurement harness:
 *   [0] block-advances of score-only BandEd passes (a search run: the block steps of its search passes)   [1] of fills
 *   [2] WindowEd block steps   [3] traceback steps   [4] CIGAR ops
 *   [5] last kernel-only time in ns (HIP events on the batch's stream)
 *   [6] pairs that went past stage 1   [7] pairs that went past stage 2
 * BANDED with only_score: a large list takes a first pass at half the cutoff and the full band only for the tasks whose
 * first result proves nothing (same scores; QE_SCORE_NARROW=0: one pass): [0] counts both passes' block-advances, so
 * two identical runs may report different [0]; [7] = tasks the second pass ran */
quicked_status_t quicked_batch_counters(quicked_batch_t* batch, int64_t counters_out[8]);
/* QUICKED runs that queue stage 1 and the align step together (see quicked_batch_run) align the pairs that leave stage 1,
 * or whose bound exceeds the planned buffers, after the run (early-finish threads, or the fetch): how many pairs of the last
 * sync != 0 run / fetch that were (0 on data like BASELINE configs 2-3; a harness that times sync == 0 runs it never
 * fetches should check this, bench.py does) */
int64_t quicked_batch_deferred_pairs(quicked_batch_t* batch);

/* Early-finish threads, process-wide since load: [0] host-driven flows they ran, [1] batch objects those finished, [2] flows
 * that served the pairs of SEVERAL batch objects at once (the runs that were over when the thread got to work: the flow's
 * duration is launch latency, not pairs), [3] batch objects in such flows.  QE_FINISH_MERGE (default 4) caps the batch
 * objects per flow; 1 = never merge. */
quicked_status_t quicked_early_finish_stats(int64_t stats_out[4]);

/* The device-pool planner's view of the calling thread (replaces mm_allocator, quicked_utils/src/mm_allocator.c:141-426):
 *   [0] bytes its pools hold   [1] allocations that had to take memory from this thread's other pools or from other threads
 *   (process-wide; the planner is there to keep this 0)   [2] pool sets in rotation in the last run   [3] fill sub-batches of
 *   the last run   [4] bytes one pool may hold   [5] bytes all pools of the thread's device hold (every thread's)
 *   [6] contexts {streams, pools} in existence   [7] contexts on lease to a live thread */
quicked_status_t quicked_pool_stats(int64_t stats_out[8]);

/* Gives the calling thread's device pools back to the device (waits for its runs first), and those that ended threads left
 * behind.  The pools belong to a per-thread context and stay allocated between runs -- that is what makes a steady stream of
 * batches allocation-free -- so a thread that is done with large batches while others go on should call this.  A thread that
 * simply ends leaves its context, pools and all, to the next thread that needs one; an allocation that finds the device
 * full takes the pools of threads that have no call in progress (their next run allocates again). */
quicked_status_t quicked_pool_trim(void);

/* Sum of the HIP-event durations (ms) of the dominant kernel (BandEd score /
 * fill) over the runs of this thread since the previous call, and how many
 * launches that was; synchronises the batch's stream. */
quicked_status_t quicked_batch_kernel_time(quicked_batch_t* batch, double* ms_sum, int64_t* launches);
/* The same by kind of launch: [0] score-only BandEd passes (a BANDED run, QuickEd's stage 3; the passes of a search run), [1] fills, [2] the half passes of
 * Hirschberg's split levels (bpm_hirschberg.c:85-100; the dominant launches of long reads), [3] diagonal-word launches of bounded
 * runs (quicked_batch_run_bounded; 0 in every other run). */
quicked_status_t quicked_batch_kernel_times(quicked_batch_t* batch, double ms_sum[4], int64_t launches[4]);

#ifdef __cplusplus
}
#endif
#endif /* QUICKED_BATCH_H */
