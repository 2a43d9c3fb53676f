// qe_stages.hip -- included by qe_driver.hip (same translation unit as the kernels): how a stage gets onto the device.
// Launch shape of the lane-per-alignment kernels, task lists and per-group workspace layouts, and the stage runners --
// BandEd score-only in its three forms (one lane / G lanes / one wave per alignment), WindowEd, the CIGAR formatter, and
// the align step (bpm_compute_matrix_hirschberg, bpm_hirschberg.c:33-270) as a level-by-level work list.  Every runner
// returns with its kernels enqueued on C.stream.  Every k_* named here is the kernels header's: qe_kernels.hip, or, in the
// host-only test build, the stand-ins of tests/native/hip_stub/qe_kernels_stub.h.
#pragma once

namespace qe {

// ---------------------------------------------------------------------------
// Launch of a lane-per-alignment kernel: ngroups waves.  Such a kernel is bound by VALU issue per SIMD:
// one or two waves on a SIMD take the same time, three take 1.4 x as long (measured).  Left
// to the dispatcher, 1563 one-wave workgroups land three-deep on some SIMDs in a good share of the
// launches (27.4 vs 38.8 ms for the same kernel).  So the placement is made a matter of resources: a
// workgroup is 4 waves -- the CU spreads them one per SIMD -- and claims a third-plus of the CU's LDS, so
// at most two workgroups share a CU and no SIMD ever holds more than two of these waves, whichever
// kernels and streams they come from.  A second kernel on another stream then fills exactly the SIMD
// slots the first one left empty, at no cost to either.
// ---------------------------------------------------------------------------
// The cooperative forms are launches of few waves, each a serial chain; next to a chip-filling launch of another run a lone
// wave gets a third of its SIMD's issue slots.  s_setprio 3 in those kernels puts them first in line.
template <class Args> static Args with_prio(Args a) { a.prio = 1; return a; }

template <typename Kernel, typename Args>
static void launch_groups(Context& C, Kernel kernel, const Args& args, size_t ngroups, int max_waves, size_t lds_per_wave, bool chain = false,
                          size_t pin_override = 0) {
    if (ngroups == 0) return;
    const int wpb = std::min(4, max_waves);
    const unsigned blocks = (unsigned)((ngroups + wpb - 1) / wpb);
    // 54 KB: 3 x 54 KB > 160 KB >= 2 x 54 KB, two workgroups per CU.  When the launches in flight have fewer workgroups than
    // the chip has CUs, 84 KB (one per CU): the dispatcher packs the workgroups of CONCURRENT small kernels two to a CU
    // while other CUs idle (three 49-workgroup launches in flight: 16.5 ms each at 54 KB, 11.7 ms at 84 KB, 11.4 ms alone)
    const Chip& chp = chip(C.device);
    size_t pin = ((size_t)blocks * (size_t)std::max(1, C.in_flight) > (size_t)chp.cus) ? (size_t)54 * 1024 : (size_t)84 * 1024;
    // chain: a launch of few waves whose duration is one wave's serial chain (WindowEd on a few thousand long reads: 157
    // waves of 1563 windows each).  108 KB: no 54 KB workgroup fits beside it, so its waves have their SIMDs to themselves
    // instead of sharing them with the fill of the run before (config 4: the stage took 59 ms beside that fill, 36 alone)
    if (chain && (size_t)blocks * (size_t)std::max(1, C.in_flight) <= (size_t)chp.cus / 2) pin = (size_t)108 * 1024;
    if (pin_override) pin = pin_override;
    const size_t lds = std::max(pin, lds_per_wave * (size_t)wpb);
    static thread_local std::vector<std::pair<const void*, int>> configured;      // per host thread and device
    const void* fn = reinterpret_cast<const void*>(kernel);
    if (std::find(configured.begin(), configured.end(), std::make_pair(fn, tl_device)) == configured.end()) {
        HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        configured.emplace_back(fn, tl_device);
    }
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * wpb), lds, C.stream, args);
    HIP_CHECK(hipGetLastError());             // a rejected launch (block shape, LDS) must not pass for zeroed results
}

// The launches between the construction and end() are timed as one stretch of `kind` (Context::kernel_events,
// quicked_batch_kernel_times) on the stream current at the construction; kind < 0, or no event pair left: the launches alone
struct TimedLaunches {
    hipStream_t s; hipEvent_t last = nullptr;
    TimedLaunches(Context& C, int kind) : s(C.stream) {
        auto* ke = kind >= 0 ? C.kernel_events(kind) : nullptr;
        if (!ke) return;
        HIP_CHECK(hipEventRecord(ke->first, s));
        last = ke->second;
    }
    void end() { if (last) HIP_CHECK(hipEventRecord(last, s)); }
};

// flags_of_reversed: the reversed pack ORs the flags in as the forward one does (quicked_debug_pack; no run asks for it)
static void launch_pack(quicked_batch& B, Context& C, bool reversed, bool flags_of_reversed = false) {
    if (B.packed) {                       // forward planes are the input; reversed ones come from them
        if (!reversed) return;
        const int blocks = (int)((B.n + 3) / 4);
        RevArgs r;
        r.nseq = (int32_t)B.n;
        r.fwd = B.d_pl_p[0]; r.rev = B.d_pl_pr[0]; r.pl_off = B.d_plp_off; r.len = B.d_p_len;
        hipLaunchKernelGGL(k_reverse_planes, dim3(blocks), dim3(256), 0, C.stream, r);
        r.fwd = B.d_pl_t[0]; r.rev = B.d_pl_tr[0]; r.pl_off = B.d_plt_off; r.len = B.d_t_len;
        hipLaunchKernelGGL(k_reverse_planes, dim3(blocks), dim3(256), 0, C.stream, r);
        for (bool& h : B.have_rev) h = true;    // every set aliases the same buffers
        return;
    }
    // patterns and texts in ONE launch (PackArgs): two launches are two kernels that each wait for CUs next to the band walk
    PackArgs a;
    a.nseq = (int32_t)B.n;
    a.reverse = reversed ? 1 : 0;
    const int q = B.parity;
    a.flags = (reversed && !flags_of_reversed) ? nullptr : B.d_flags[q];
    const int blocks = (int)((B.n + 3) / 4);
    a.set[0] = PackSet{B.d_asc_p, B.d_p_off, B.d_p_len, reversed ? B.d_pl_pr[q] : B.d_pl_p[q], B.d_plp_off};
    a.set[1] = PackSet{B.d_asc_t, B.d_t_off, B.d_t_len, reversed ? B.d_pl_tr[q] : B.d_pl_t[q], B.d_plt_off};
    hipLaunchKernelGGL(k_pack, dim3(2 * blocks), dim3(256), 0, C.stream, a);
}

// the reversed planes of the run's plane set, packed once per parity
static void ensure_reversed(quicked_batch& B, Context& C) {
    if (B.have_rev[B.parity]) return;
    launch_pack(B, C, true);
    B.have_rev[B.parity] = true;
}

// ---------------------------------------------------------------------------
// One stage = one task list (subset of pairs) laid out as 64-lane groups
// ---------------------------------------------------------------------------
struct TaskList {
    std::vector<int32_t> pair, p0, m, t0, n, cutoff, tfin;   // padded to a multiple of 64, pair = -1 in the padding
    int ngroups() const { return (int)(pair.size() / 64); }
    void push(int32_t pr, int32_t p0_, int32_t m_, int32_t t0_, int32_t n_, int32_t cut, int32_t tf) {
        pair.push_back(pr); p0.push_back(p0_); m.push_back(m_); t0.push_back(t0_); n.push_back(n_);
        cutoff.push_back(cut); tfin.push_back(tf);
    }
    void pad() { while (pair.size() % 64) push(-1, 0, 1, 0, 1, 0, 0); }
};

struct DevTasks {
    TaskView v;
    int32_t *pair, *p0, *m, *t0, *n, *cutoff, *tfin;
};
// one upload of raw bytes through the pinned stage of the run (or a plain async copy when staging is off)
static void h2d_bytes(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return;
    Context* C = tl_ctx;
    if (C && C->staging && (s == C->sa() || s == C->sw() || s == C->stream_x)) {      // W-phase copies too: the run's A phase, whose end frees the stage, is behind them
        uint8_t* st = C->stage[C->si].take(bytes);
        memcpy(st, src, bytes);
        copy_kernel(dst, st, bytes, s);
        return;
    }
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
}
// the seven arrays of a task list in ONE device block and ONE copy (a copy costs ~5-10 us of host time whatever its size)
static DevTasks upload_tasks(const TaskList& L, Context& C) {
    DevTasks d;
    const size_t nt = L.pair.size();
    int32_t* blk = C.scratch_p->take<int32_t>(7 * nt);
    d.pair = blk; d.p0 = blk + nt; d.m = blk + 2 * nt; d.t0 = blk + 3 * nt; d.n = blk + 4 * nt; d.cutoff = blk + 5 * nt; d.tfin = blk + 6 * nt;
    static thread_local std::vector<int32_t> host;
    host.resize(7 * nt);
    const std::vector<int32_t>* src[7] = {&L.pair, &L.p0, &L.m, &L.t0, &L.n, &L.cutoff, &L.tfin};
    for (int q = 0; q < 7; ++q) memcpy(host.data() + q * nt, src[q]->data(), nt * sizeof(int32_t));
    h2d_bytes(blk, host.data(), 7 * nt * sizeof(int32_t), C.stream);
    d.v.ntasks = (int32_t)nt; d.v.pair = d.pair; d.v.p0 = d.p0; d.v.m = d.m; d.v.t0 = d.t0; d.v.n = d.n;
    d.v.cutoff = d.cutoff; d.v.tfin = d.tfin;
    return d;
}

// per-group workspace geometry of a BandEd launch
struct BandLayout {
    std::vector<int64_t> ws_off, mat_off, runs_off;
    std::vector<int32_t> nslots, nrows, nch, runs_cap;
    size_t ws_bytes = 0, mat_u4 = 0, runs_u32 = 0;
};
static BandLayout band_layout(const TaskList& L, bool fill, bool want_runs, bool tight_runs = false) {
    BandLayout B;
    const int ng = L.ngroups();
    B.ws_off.resize(ng); B.mat_off.resize(ng); B.runs_off.resize(ng);
    B.nslots.resize(ng); B.nrows.resize(ng); B.nch.resize(ng); B.runs_cap.resize(ng);
    for (int g = 0; g < ng; ++g) {
        int ns = 3, nr = 4, nch = 2, nmax = 1, cap = 2;
        for (int l = 0; l < 64; ++l) {
            const size_t t = (size_t)g * 64 + l;
            if (L.pair[t] < 0) continue;
            const HGeom G = host_geometry(L.m[t], L.n[t], L.cutoff[t]);
            const int nsl = fill ? G.ebb : G.ebb_local;
            const int nw = (L.m[t] + 63) / 64;
            ns = std::max(ns, nsl);
            nr = std::max(nr, nw + nsl + 4);
            nch = std::max(nch, L.n[t] / 64 + 3);
            nmax = std::max(nmax, L.n[t]);
            // an alignment with e edits has at most 2 e + 1 runs.  tight_runs: the cutoff is known to be >= the distance
            // (QuickEd's bound, Hirschberg's exact child distances), so e <= cutoff; k_traceback reports, instead of
            // storing, a path that has more.  A user-chosen bandwidth promises nothing (a 35 %-error pair aligns at
            // bandwidth 15 with 499 edits against a cutoff of 300): every op may be its own run
            const int64_t every = (int64_t)L.m[t] + L.n[t] + 2;
            cap = std::max(cap, (int)(tight_runs ? std::min<int64_t>(every, (int64_t)2 * G.cutoff + 8) : every));
        }
        // the fill records the band edges of every chunk as int16 (cf / cl): a band of more than 32 k blocks (a leaf of
        // ~14 Mb at 15 % bandwidth -- Hirschberg splits long before that) is refused, not silently truncated
        if (fill && ns > 32760) throw HipError{hipErrorInvalidValue, "band of more than 32760 blocks: not supported", __LINE__};
        B.nslots[g] = ns; B.nrows[g] = nr; B.nch[g] = nch; B.runs_cap[g] = cap;
        B.ws_off[g] = (int64_t)B.ws_bytes;
        size_t bytes = (size_t)2 * (ns + 1) * 64 * 8 + (size_t)nr * 64 * 4 + (size_t)2 * nch * 64 * 2;
        B.ws_bytes += (bytes + 255) & ~(size_t)255;
        B.mat_off[g] = (int64_t)B.mat_u4;
        if (fill) B.mat_u4 += (size_t)(QE_CPC + 1) * nch * ns * 64;        // checkpoints cp[QE_CPC nch][ns][64] + carry words hw[nch][ns][64]
        B.runs_off[g] = (int64_t)B.runs_u32;
        if (want_runs) B.runs_u32 += (size_t)cap * 64;
    }
    return B;
}

struct DevLayout {                  // all null: a launch without a group workspace
    uint8_t* ws = nullptr; int64_t *ws_off = nullptr, *mat_off = nullptr, *runs_off = nullptr;
    int32_t *nslots = nullptr, *nrows = nullptr, *nch = nullptr, *runs_cap = nullptr; uint4* mat = nullptr; u32* runs = nullptr;
};
static DevLayout upload_layout(const BandLayout& B, Context& C) {
    DevLayout d;
    const size_t ng = B.ws_off.size();
    d.ws = C.scratch_p->take<uint8_t>(B.ws_bytes);
    d.mat = C.scratch_p->take<uint4>(B.mat_u4);
    d.runs = C.scratch_p->take<u32>(B.runs_u32);
    // three int64 + four int32 arrays per group: one device block, one copy
    uint8_t* blk = C.scratch_p->take<uint8_t>(ng * 40);
    d.ws_off = (int64_t*)blk; d.mat_off = d.ws_off + ng; d.runs_off = d.mat_off + ng;
    d.nslots = (int32_t*)(d.runs_off + ng); d.nrows = d.nslots + ng; d.nch = d.nrows + ng; d.runs_cap = d.nch + ng;
    static thread_local std::vector<uint8_t> host;
    host.resize(ng * 40);
    if (ng) {
        uint8_t* h = host.data();
        memcpy(h, B.ws_off.data(), ng * 8); memcpy(h + ng * 8, B.mat_off.data(), ng * 8); memcpy(h + ng * 16, B.runs_off.data(), ng * 8);
        memcpy(h + ng * 24, B.nslots.data(), ng * 4); memcpy(h + ng * 28, B.nrows.data(), ng * 4);
        memcpy(h + ng * 32, B.nch.data(), ng * 4); memcpy(h + ng * 36, B.runs_cap.data(), ng * 4);
        h2d_bytes(blk, h, ng * 40, C.stream);
    }
    return d;
}

struct TaskOut {   // device arrays per task
    int32_t *score, *first, *last, *posv, *hew, *nruns, *nops, *edits, *len;
    u32 *adv, *steps;
    int64_t* str_off;
};
static TaskOut take_out(Context& C, size_t nt) {
    TaskOut o;
    o.score = C.scratch_p->take<int32_t>(nt); o.first = C.scratch_p->take<int32_t>(nt); o.last = C.scratch_p->take<int32_t>(nt);
    o.posv = C.scratch_p->take<int32_t>(nt); o.hew = C.scratch_p->take<int32_t>(nt); o.nruns = C.scratch_p->take<int32_t>(nt);
    o.nops = C.scratch_p->take<int32_t>(nt); o.edits = C.scratch_p->take<int32_t>(nt); o.len = C.scratch_p->take<int32_t>(nt);
    const size_t ntp = (nt + 63) & ~(size_t)63;
    o.adv = C.scratch_p->take<u32>(2 * ntp); o.steps = o.adv + ntp;         // one block: one memset
    o.str_off = C.scratch_p->take<int64_t>(nt + 1);
    // the work counters are summed over every slot of the list: padding slots (and tasks a kernel skips) count 0
    HIP_CHECK(hipMemsetAsync(o.adv, 0, 2 * ntp * sizeof(u32), C.stream));
    return o;
}

// The cutoffs are still being computed on the device (QuickEd's fast flow): the list's are the estimates the buffers are
// sized for; k_apply_cutoffs puts the real ones in and takes the tasks out that the host finishes afterwards.  `cleared`, an
// output per task, reads -1 for those.
static void apply_device_cutoffs(Context& C, const DevTasks& T, size_t nt, int32_t* cleared, const int32_t* d_cut, const int32_t* d_skip) {
    HIP_CHECK(hipMemsetAsync(cleared, 0xFF, nt * sizeof(int32_t), C.stream));
    hipLaunchKernelGGL(k_apply_cutoffs, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, C.stream, (int)nt, T.cutoff, T.pair, d_cut, d_skip);
}

// ---------------------------------------------------------------------------
// Stage runners.  Each returns with its kernels enqueued on C.stream.
// ---------------------------------------------------------------------------
struct StageResult {
    std::vector<int32_t> score, hew, first, last, posv, nruns, nops, edits, len;
    std::vector<u32> adv, steps;
    std::vector<unsigned long long> narrow;   // a two-pass BandEd score-only run's (or a probe's) NarrowArgs::stat
    bool narrow_probe = false;
};

static uint64_t sum_u32(const std::vector<u32>& v) { uint64_t s = 0; for (u32 x : v) s += x; return s; }

// BandEd score-only over a task list (bpm_banded.c:791-964); the launch's device state stays
// addressable (Hirschberg reads the stopped bands)
struct ScoreLaunch {
    DevTasks T; DevLayout D; TaskOut O; size_t nt = 0;
    int G = 1;                                                          // >= 2: cooperative launch + fallback pass
    uint8_t* cws = nullptr; int64_t* c_off = nullptr; int32_t *c_ns = nullptr, *c_nr = nullptr, *c_nch = nullptr;
    unsigned long long* narrow = nullptr; bool narrow_probe = false;   // launch_banded_narrow / launch_banded_probe: NarrowArgs::stat
};
static BandState coop_state(const ScoreLaunch& S) {
    BandState b;
    b.G = S.G; b.ws = S.cws; b.g_ws_off = S.c_off; b.g_nslots = S.c_ns; b.g_nrows = S.c_nr; b.g_nch = S.c_nch;
    b.first = S.O.first; b.last = S.O.last; b.posv = S.O.posv; b.maxrow = S.O.len; b.abort = S.O.hew;
    return b;
}

static BandState band_state(const ScoreLaunch& S) {
    BandState b;
    b.G = 1; b.abort = nullptr;
    b.ws = S.D.ws; b.g_ws_off = S.D.ws_off; b.g_nslots = S.D.nslots; b.g_nrows = S.D.nrows; b.g_nch = S.D.nch;
    b.first = S.O.first; b.last = S.O.last; b.posv = S.O.posv; b.maxrow = S.O.len;   // O.len doubles as maxrow here
    return b;
}

// What every BandEd score-only launch passes alike: the pairs, the list, its group workspace (null where it has none) and the
// outputs (O.len doubles as maxrow) and the pass rule of k_banded<false>.  Every other field keeps BandedArgs' default
// (fill_multi = lane_rel = 1) or is 0 / null.
static BandedArgs score_args(const quicked_batch& B, const ScoreLaunch& S, bool reversed) {
    BandedArgs a{};
    a.score_masked = sw(Sw::ScoreMasked);
    a.P = pair_view(B, reversed); a.T = S.T.v;
    a.ws = S.D.ws; a.g_ws_off = S.D.ws_off; a.g_nslots = S.D.nslots; a.g_nrows = S.D.nrows; a.g_nch = S.D.nch;
    a.g_mat_off = S.D.mat_off;
    a.o_score = S.O.score; a.o_first = S.O.first; a.o_last = S.O.last; a.o_posv = S.O.posv; a.o_adv = S.O.adv; a.o_maxrow = S.O.len;
    return a;
}

// d_cut / d_skip: the cutoffs are still on the device (apply_device_cutoffs)
static ScoreLaunch launch_banded_score(quicked_batch& B, Context& C, const TaskList& L, bool reversed, int timed, bool fill_geom = false,
                                       const int32_t* d_cut = nullptr, const int32_t* d_skip = nullptr) {
    ScoreLaunch S;
    S.nt = L.pair.size();
    BandLayout lay = band_layout(L, fill_geom, false);
    lay.mat_u4 = 0;                                   // (the fill's geometry, not its checkpoints)
    S.T = upload_tasks(L, C);
    S.D = upload_layout(lay, C);
    S.O = take_out(C, S.nt);
    if (d_cut) apply_device_cutoffs(C, S.T, S.nt, S.O.score, d_cut, d_skip);      // a task taken out of the list has no score (-1)
    BandedArgs a = score_args(B, S, reversed);
    a.lane_rel = sw(Sw::LaneRel);
    a.fill_geom = fill_geom ? 1 : 0;
    TimedLaunches tl(C, timed - 1);       // timed = kind + 1, 0 = not timed
    launch_groups(C, k_banded<false>, a, L.ngroups(), 8, 0);
    tl.end();
    return S;
}

// ---------------------------------------------------------------------------
// BandEd score-only in two passes: k_banded<false> over the list with every task's cutoff halved where
// that makes its band narrower, k_narrow packs the tasks whose result proves nothing (-1, or above the halved cutoff) into
// dense groups of 64, k_banded<false> again over those at their own cutoffs.  A result 0 .. C' of the first pass is the cost
// of a real path, so the distance is within C', and the pass at C >= C' returns the same value: the scores are the single
// pass's.  Nothing waits for the host: the second launch has the grid of the whole list, and the groups beyond the misses
// find pair = -1 and return.  Both launches share one group workspace, laid out for the list's largest geometry at the
// full cutoff -- the membership of the second launch's groups is decided on the device.
// ---------------------------------------------------------------------------
struct NarrowPlan { bool ok = false; int cls = 0; size_t live = 0, narrower = 0; int slots1 = 0; };      // slots1: see score_lds_slots
// whole-text passes only (a stopped band is exported from ONE pass: Hirschberg half passes keep the single pass)
static NarrowPlan narrow_plan(const TaskList& L) {
    NarrowPlan P;
    int n_max = 1;
    for (size_t t = 0; t < L.pair.size(); ++t) {
        if (L.pair[t] < 0) continue;
        if (L.tfin[t] != L.n[t]) return P;
        ++P.live;
        const int c1 = narrow_cutoff(L.m[t], L.n[t], L.cutoff[t]);
        P.narrower += c1 != L.cutoff[t];
        P.slots1 = std::max(P.slots1, narrow_slots(L.m[t], L.n[t], c1));
        n_max = std::max(n_max, L.n[t]);
    }
    while ((n_max >> (P.cls + 1)) != 0 && P.cls < 31) ++P.cls;
    P.ok = P.narrower > 0;
    return P;
}
// The verdict per context and length class: the first pass pays while the tasks it halved advance fewer block-columns in
// both passes together than the single pass costs them -- estimated from what the second pass advanced per task it ran,
// times their number.  It is taken when a run's counts reach the host: at the end of a synchronous run, in the fetch of a
// queued one (a queued run that is never fetched teaches nothing).  A run without misses has paid (its band is the
// narrower one); unknown data take the first pass; after a run that did not pay the class takes the single pass and probes
// every QE_NARROW_PROBE-th eligible run.  A probe is a single-pass run like its neighbours, plus a pass at the halved cutoffs
// over the tasks of every QE_NARROW_PROBE-th group on the side stream (launch_banded_probe): no result waits for it, and it
// is over before the run's own launch is.  (Two passes over a sample IN the run were measured first: the second launch's few
// waves walk a whole band at the full cutoff behind the first launch, the run holds its set of the rotation for two
// chains' time, and a stream of 10 kb pairs at 10 % ran 4.5-5 % behind the single pass: profiles/narrow_headline.md.)
enum : int { QE_NARROW_PROBE = 16 };
// -> 0: the single pass, 1: two passes, 2: the single pass and a probe
static int narrow_take(Context& C, int cls) {
    const int v = C.narrow_off[cls].load();
    if (v == 0) return 1;
    if (v >= QE_NARROW_PROBE) { C.narrow_off[cls] = 1; return sw(Sw::ScoreNarrow) == -2 ? 0 : 2; }      // -2: no probes (diagnosis)
    C.narrow_off[cls] = v + 1;
    return 0;
}
// The fit (qe_types.h: narrow_fit_lane): a class's q is the largest ratio of distance to cutoff that its last QE_NARROW_FIT_RUNS
// reported two-pass runs saw (NarrowArgs::stat[4]; 0 = unknown data: half the cutoff) -- the cadence the probes have.  A run
// whose fit caused misses reports the ratios of those too, so it has raised q for the next run; and its verdict is taken as
// if the fit's own misses (stat[5]) had been accepted: a stale fit never sends a class to the single pass where half the
// cutoff would have paid.  QE_NARROW_FIT = 0: never, k > 0: q = k for every list (tests).
enum : int { QE_NARROW_FIT_RUNS = 16 };
static int narrow_fit_q(Context& C, int cls, bool policy) {
    const int f = sw(Sw::NarrowFit);
    if (f >= 0) return f;
    if (!policy) return 0;
    int q = 0;
    for (auto& v : C.narrow_q[cls]) q = std::max(q, v.load());
    return q;
}
// The pruning threshold of a fitted first pass (qe_types.h: narrow_prune): the ratio qp = q + w, w = what the maxima in the
// ring varied by (q less its smallest reported ratio).  On repeated data w = 0 and the band edges prune at r_hat itself; on
// fresh batches of one distribution the threshold sits above r_hat by the spread the class has shown; after a shift the old
// entries make w large and the threshold is the fitted cutoff, i.e. none.  Only with two reported runs in the ring: one
// report says nothing about the spread.  QE_NARROW_PRUNE = 0: never, k > 0: qp = k for every fitted list, also under a
// forced QE_NARROW_FIT (tests); a forced fit alone has no threshold.
static int narrow_prune_q(Context& C, int cls, bool policy) {
    const int f = sw(Sw::NarrowPrune);
    if (f >= 0) return f;
    if (!policy || sw(Sw::NarrowFit) >= 0) return 0;
    int q = 0, lo = 0, reports = 0;
    for (auto& a : C.narrow_q[cls]) {
        const int v = a.load();
        if (v <= 0) continue;
        ++reports;
        q = std::max(q, v);
        lo = lo ? std::min(lo, v) : v;
    }
    return reports >= 2 ? q + (q - lo) : 0;
}
static void narrow_report(Context* C, int cls, const std::vector<unsigned long long>& st, bool probe) {
    static_assert(sizeof(C->narrow_q[0]) / sizeof(C->narrow_q[0][0]) == QE_NARROW_FIT_RUNS, "the ring holds the window");
    if (!C || st.size() < QE_NARROW_STAT) return;
    if (!probe) C->narrow_q[cls][C->narrow_qn[cls].fetch_add(1) % QE_NARROW_FIT_RUNS] = (int)st[4];
    const double misses = (double)(st[0] - st[5]), a1 = (double)st[1], halved = (double)st[3];
    const double a2 = st[0] ? (double)st[2] * misses / (double)st[0] : 0.0;
    const bool paid = st[0] == st[5] || (a1 + a2) * misses < a2 * halved;
    int unknown = 0;
    if (paid) C->narrow_off[cls] = 0; else C->narrow_off[cls].compare_exchange_strong(unknown, 1);
}

// every group: the tallest band, the most rows and the most chunks of the list
static BandLayout narrow_uniform(BandLayout lay) {
    int ns = 3, nr = 4, nch = 2;
    for (size_t g = 0; g < lay.nslots.size(); ++g) { ns = std::max(ns, (int)lay.nslots[g]); nr = std::max(nr, (int)lay.nrows[g]); nch = std::max(nch, (int)lay.nch[g]); }
    const size_t bytes = ((size_t)2 * (ns + 1) * 64 * 8 + (size_t)nr * 64 * 4 + (size_t)2 * nch * 64 * 2 + 255) & ~(size_t)255;
    for (size_t g = 0; g < lay.nslots.size(); ++g) { lay.nslots[g] = ns; lay.nrows[g] = nr; lay.nch[g] = nch; lay.ws_off[g] = (int64_t)(g * bytes); }
    lay.ws_bytes = bytes * lay.nslots.size();
    lay.mat_u4 = 0;
    return lay;
}

// A probe: the list's single pass as launch_banded_score queues it, and beside it, on the side stream, k_banded<false> at the
// halved cutoffs over the tasks of every QE_NARROW_PROBE-th group whose band is narrower there.  k_narrow phase 3 then counts
// what two passes would have cost that sample.  The sample's pass starts with the run's launch and walks half its band.
static ScoreLaunch launch_banded_probe(quicked_batch& B, Context& C, const TaskList& L, bool reversed, int timed) {
    ScoreLaunch S;
    S.nt = L.pair.size();
    TaskList Ls;
    for (size_t g = 0; g < S.nt / 64; g += QE_NARROW_PROBE)
        for (size_t t = g * 64; t < g * 64 + 64; ++t) {
            const int c1 = L.pair[t] >= 0 ? narrow_cutoff(L.m[t], L.n[t], L.cutoff[t]) : 0;
            if (L.pair[t] >= 0 && c1 != L.cutoff[t]) Ls.push(L.pair[t], L.p0[t], L.m[t], L.t0[t], L.n[t], c1, L.tfin[t]);
            else Ls.push(-1, 0, 1, 0, 1, 0, 0);
        }
    BandLayout lay = band_layout(L, false, false), lays = band_layout(Ls, false, false);
    lay.mat_u4 = 0; lays.mat_u4 = 0;
    S.T = upload_tasks(L, C);
    S.D = upload_layout(lay, C);
    S.O = take_out(C, S.nt);
    ScoreLaunch P;
    P.nt = Ls.pair.size();
    P.T = upload_tasks(Ls, C);
    P.D = upload_layout(lays, C);
    P.O = take_out(C, P.nt);
    S.narrow = C.scratch_p->take<unsigned long long>(QE_NARROW_STAT);
    S.narrow_probe = true;
    HIP_CHECK(hipMemsetAsync(S.narrow, 0, QE_NARROW_STAT * sizeof(unsigned long long), C.stream));
    hipStream_t main_s = C.stream, side = C.side_stream();
    HIP_CHECK(hipEventRecord(C.ev_fork, main_s)); HIP_CHECK(hipStreamWaitEvent(side, C.ev_fork, 0));
    BandedArgs a = score_args(B, S, reversed);
    a.lane_rel = sw(Sw::LaneRel);
    TimedLaunches tl(C, timed - 1);       // timed = kind + 1, 0 = not timed
    launch_groups(C, k_banded<false>, a, L.ngroups(), 8, 0);
    tl.end();
    C.stream = side;
    BandedArgs b = score_args(B, P, reversed);
    b.lane_rel = a.lane_rel;
    launch_groups(C, k_banded<false>, b, Ls.ngroups(), 8, 0);
    C.stream = main_s;
    HIP_CHECK(hipEventRecord(C.ev_join, side)); HIP_CHECK(hipStreamWaitEvent(main_s, C.ev_join, 0));
    NarrowArgs x{};
    x.phase = 3; x.stride = QE_NARROW_PROBE;
    x.T = P.T.v; x.score = S.O.score; x.adv = S.O.adv; x.q_score = P.O.score; x.q_adv = P.O.adv; x.main_cutoff = S.T.cutoff; x.stat = S.narrow;
    hipLaunchKernelGGL(k_narrow, dim3((unsigned)((P.nt + 255) / 256)), dim3(256), 0, main_s, x);
    HIP_CHECK(hipGetLastError());
    return S;
}

// Band state in LDS for the FIRST launch (k_banded<false, true>): the slot count its slices are sized for, or 0
// = the group workspace as ever.  The bound on a task's first-launch band is its slot count at narrow_cutoff -- the fit only
// ever takes fewer, a task that keeps its cutoff walks exactly that; narrow_plan takes the largest over the list in the scan it
// makes anyway (NarrowPlan::slots1) -- and the list takes the form when that fits the budget of qe_types.h.  At the cap a
// workgroup's four slices are 72 KB: two workgroups still share a CU (launch_groups).  QE_SCORE_LDS = 0: never, 1: whatever
// the list's size (by default a list of a group per SIMD, as the two passes themselves: smaller launches were not measured).
static int score_lds_slots(const Context& C, const TaskList& L, int bound) {
    if (!QE_K_BANDED_LDS) return 0;                  // the host-only build's kernels header declines the form
    const int mode = sw(Sw::ScoreLds);
    if (mode == 0 || (mode != 1 && (size_t)L.ngroups() < (size_t)chip(C.device).simds)) return 0;
    return score_lds_fits(bound) ? bound : 0;
}

// Eq from a table for the tall passes of the FIRST launch (k_banded<false, false, true>): the LDS then holds a
// wave's Eq table (peq_bytes(): 80 KB per workgroup) and the band state goes back to the group workspace.  QE_SCORE_PEQ = -1:
// wherever the launch would by default take the LDS form with tall passes (`tall_lds`); 0: never; 1: wherever a tall pass can
// run, whatever the list's size and its bands (tests).  A forced QE_SCORE_LDS = 1 asks for the band state in LDS and so for the
// form without the table, QE_SCORE_TALL = 0 leaves no pass that reads one.  The form needs two workgroups per CU like every
// launch_groups launch: where the runtime's occupancy query does not place two of 80 KB, it is declined.
static bool score_peq(const Context& C, const TaskList& L, bool tall_lds) {
    (void)C; (void)L;
#ifdef QE_K_BANDED_PEQ
    if (!QE_K_BANDED_LDS) return false;
    const int mode = sw(Sw::ScorePeq);
    if (mode == 0 || sw(Sw::ScoreLds) == 1 || sw(Sw::ScoreTall) == 0) return false;
    if (mode != 1 && !tall_lds) return false;
    static thread_local std::vector<std::pair<int, int>> per_cu;          // per host thread and device, as launch_groups' `configured`
    for (const auto& d : per_cu) if (d.first == tl_device) return d.second >= 2;
    const void* fn = reinterpret_cast<const void*>(k_banded<false, false, true>);
    int nb = 0;
    HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, (size_t)4 * (size_t)peq_bytes()) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
    if (trace_on()) fprintf(stderr, "[qe] table form: %d workgroups of %d B of LDS per CU\n", nb, 4 * peq_bytes());
    per_cu.emplace_back(tl_device, nb);
    return nb >= 2;
#else
    return false;
#endif
}

static ScoreLaunch launch_banded_narrow(quicked_batch& B, Context& C, const TaskList& L, bool reversed, int timed, const BandLayout& lay, int q, int qp, int slots1) {
    ScoreLaunch S;
    S.nt = L.pair.size();
    const size_t nt = S.nt;
    S.T = upload_tasks(L, C);
    S.D = upload_layout(lay, C);
    S.O = take_out(C, nt);
    ScoreLaunch S2 = S;                              // the packed list of the misses, its outputs; the same workspace
    S2.O = take_out(C, nt);
    int32_t* blk = C.scratch_p->take<int32_t>(10 * nt);
    S.narrow = C.scratch_p->take<unsigned long long>(QE_NARROW_STAT);
    NarrowArgs x{};
    x.T = S.T.v; x.cut1 = blk; x.score = S.O.score; x.adv = S.O.adv;
    x.q_pair = blk + nt; x.q_p0 = blk + 2 * nt; x.q_m = blk + 3 * nt; x.q_t0 = blk + 4 * nt; x.q_n = blk + 5 * nt;
    x.q_cutoff = blk + 6 * nt; x.q_tfin = blk + 7 * nt; x.q_src = blk + 8 * nt;
    x.q_score = S2.O.score; x.q_adv = S2.O.adv; x.stat = S.narrow; x.q = q;
    x.qp = q > 0 ? qp : 0; x.prune1 = blk + 9 * nt;      // the first launch's pruning thresholds, beside cut1
    S2.T.v.pair = x.q_pair; S2.T.v.p0 = x.q_p0; S2.T.v.m = x.q_m; S2.T.v.t0 = x.q_t0; S2.T.v.n = x.q_n;
    S2.T.v.cutoff = x.q_cutoff; S2.T.v.tfin = x.q_tfin;
    const dim3 grid((unsigned)((nt + 255) / 256)), block(256);
    TimedLaunches tl(C, timed - 1);       // timed = kind + 1, 0 = not timed
    x.phase = 0;
    hipLaunchKernelGGL(k_narrow, grid, block, 0, C.stream, x);
    BandedArgs a = score_args(B, S, reversed);
    a.T.cutoff = x.cut1;
    if (x.qp > 0) a.prune = x.prune1;                // (without a ratio prune1 = cut1: today's launch)
    a.lane_rel = sw(Sw::LaneRel);
    a.lds_slots = score_lds_slots(C, L, slots1);
    a.score_tall = (a.lds_slots && sw(Sw::ScoreTall) != 0) ? 1 : 0;      // tall passes: the LDS form only
    const bool peq = score_peq(C, L, a.lds_slots != 0 && a.score_tall != 0);
    if (peq) { a.lds_slots = 0; a.score_tall = 1; }                       // the table form: the LDS holds Eq, the state goes to the group workspace
    if (trace_on()) fprintf(stderr, "[qe] two-pass score: first launch of %d groups, band state in %s (%d slots), tall passes %s%s\n", L.ngroups(), a.lds_slots ? "LDS" : "the group workspace", a.lds_slots, a.score_tall ? "on" : "off", peq ? ", Eq from a table in LDS" : "");
#ifdef QE_K_BANDED_PEQ
    if (peq) launch_groups(C, k_banded<false, false, true>, a, L.ngroups(), 8, (size_t)peq_bytes());
    else
#endif
    if (a.lds_slots) launch_groups(C, k_banded<false, true>, a, L.ngroups(), 8, (size_t)score_lds_bytes(a.lds_slots));
    else launch_groups(C, k_banded<false>, a, L.ngroups(), 8, 0);
    x.phase = 1;
    hipLaunchKernelGGL(k_narrow, grid, block, 0, C.stream, x);
    BandedArgs b = score_args(B, S2, reversed);
    b.lane_rel = a.lane_rel;
    launch_groups(C, k_banded<false>, b, L.ngroups(), 8, 0);
    x.phase = 2;
    hipLaunchKernelGGL(k_narrow, grid, block, 0, C.stream, x);
    HIP_CHECK(hipGetLastError());
    tl.end();
    return S;
}

// lanes per alignment for the cooperative score-only kernel: enough waves to fill the chip
// (>= ~4 per SIMD) while every lane keeps >= 2 band slots; QE_COOP_G overrides (0 / 1 = off)
static int coop_lanes(const TaskList& L, int in_flight = 1, bool fill = false) {
    const Sw force = fill ? Sw::CoopFillG : Sw::CoopG;
    const bool e = sw_set(force);
    int min_nsl = 1 << 30, n_max = 1;
    size_t live = 0;
    for (size_t t = 0; t < L.pair.size(); ++t) {
        if (L.pair[t] < 0) continue;
        ++live;
        const HGeom hg = host_geometry(L.m[t], L.n[t], L.cutoff[t]);
        min_nsl = std::min(min_nsl, fill ? hg.ebb : hg.ebb_local);
        n_max = std::max(n_max, L.n[t]);
    }
    if (live == 0) return 1;
    int G = 1;
    // Waves to aim for: ~700 for 10 kb reads (measured with the multi-slot one-lane kernel and overlapped runs:
    // 8 k / 16 k pairs are best at G = 4, 32 k at G = 2, 50 k and up at G = 1), more for longer reads, whose one-lane
    // latency grows with their length (100 kb half passes: 526 -> 430 ms from G = 8 to 32)
    const Chip& chp = chip(tl_device);
    const size_t target = std::min<size_t>(2 * chp.slots2(), chp.frac2(0.34) * (size_t)std::max(1, n_max / 10000));      // ~700 waves of 2 048 slots per 10 kb of read
    if (e) G = sw(force);
    else
        while (G < 64 && ((live * G) / 64) * (size_t)std::max(1, in_flight) < target) G *= 2;      // runs in flight fill the chip together
    // the band-height test first + 2 < last must stay decidable G - 2 chunks early: a band of >= 3 G + 4 slots always is;
    // with 2 G + 4 a task whose band comes within G slots of its minimum height is flagged and recomputed by the one-lane
    // kernel -- rare, and worth it where the launch is short of waves anyway (4 000 pairs of 10 kb: 4.2 -> 2.8 ms with G = 8)
    while (G > 1 && min_nsl < 3 * G + 4) G /= 2;
    if (!e)
        while (G < 64 && min_nsl >= 2 * (2 * G) + 4 && ((live * G) / 64) * (size_t)std::max(1, in_flight) < chp.slots2() / 4) G *= 2;
    return G < 2 ? 1 : G;
}

// the band state of a wave's 64 / G tasks in LDS (k_banded_coop_lds): bytes per wave for bands of ns slots
static size_t coop_lds_bytes(int ns, int G) {
    const int NA = 64 / G, rr = ns + G + 4, cr = std::max(16, 4 * G);
    const size_t bytes = (size_t)2 * (ns + 1) * NA * 8 + (size_t)2 * rr * NA * 4 + (size_t)2 * cr * NA * 2 + (size_t)2 * NA * 4;
    return (bytes + 63) & ~(size_t)63;
}
// k_banded_coop(_lds) over the list, then k_banded<false> over the tasks it flagged
static ScoreLaunch launch_banded_coop(quicked_batch& B, Context& C, const TaskList& L, bool reversed, int G, int timed) {
    ScoreLaunch S;
    S.nt = L.pair.size();
    const int NA = 64 / G;
    const size_t nwaves = S.nt / NA;
    std::vector<int64_t> w_off(nwaves);
    std::vector<int32_t> w_ns(nwaves), w_nr(nwaves), w_nch(nwaves);
    size_t ws_bytes = 0;
    int ns_max = 3;
    for (size_t w = 0; w < nwaves; ++w) {
        int ns = 3, nr = 4, nch = 2;
        for (int q = 0; q < NA; ++q) {
            const size_t t = w * NA + q;
            if (L.pair[t] < 0) continue;
            const HGeom Gm = host_geometry(L.m[t], L.n[t], L.cutoff[t]);
            const int nsl = Gm.ebb_local;
            ns = std::max(ns, nsl);
            nr = std::max(nr, (L.m[t] + 63) / 64 + nsl + 4);
            nch = std::max(nch, L.n[t] / 64 + 3);
        }
        w_ns[w] = ns; w_nr[w] = nr; w_nch[w] = nch;
        ns_max = std::max(ns_max, ns);
        w_off[w] = (int64_t)ws_bytes;
        const size_t bytes = (size_t)2 * (ns + 1) * NA * 8 + (size_t)2 * nr * NA * 4 + (size_t)2 * nch * NA * 2 + (size_t)2 * NA * 4;
        ws_bytes += (bytes + 255) & ~(size_t)255;
    }
    S.T = upload_tasks(L, C);
    S.O = take_out(C, S.nt);
    uint8_t* ws = C.scratch_p->take<uint8_t>(ws_bytes + 256);
    int64_t* d_off = C.scratch_p->take<int64_t>(nwaves); int32_t* d_ns = C.scratch_p->take<int32_t>(nwaves);
    int32_t* d_nr = C.scratch_p->take<int32_t>(nwaves); int32_t* d_nch = C.scratch_p->take<int32_t>(nwaves);
    { CopyBatch cb(C.stream); h2d(d_off, w_off, C.stream); h2d(d_ns, w_ns, C.stream); h2d(d_nr, w_nr, C.stream); h2d(d_nch, w_nch, C.stream); }
    S.G = G; S.cws = ws; S.c_off = d_off; S.c_ns = d_ns; S.c_nr = d_nr; S.c_nch = d_nch;
    CoopArgs a;
    a.P = pair_view(B, reversed); a.T = S.T.v; a.G = G;
    a.ws = ws; a.w_ws_off = d_off; a.w_nslots = d_ns; a.w_nrows = d_nr; a.w_nch = d_nch;
    a.o_score = S.O.score; a.o_first = S.O.first; a.o_last = S.O.last; a.o_posv = S.O.posv; a.o_adv = S.O.adv;
    a.o_maxrow = S.O.len; a.o_abort = S.O.hew;
    HIP_CHECK(hipMemsetAsync(S.O.hew, 0, S.nt * sizeof(int32_t), C.stream));
    TimedLaunches tl(C, timed - 1);       // timed = kind + 1, 0 = not timed
    // band state on chip where a wave's tasks fit its share of the LDS (k_banded_coop_lds); QE_COOP_LDS = 0: never
    CoopLdsArgs x;
    memset(&x, 0, sizeof(x));
    x.A = a;
    x.lgG = 0; while ((1 << x.lgG) < G) ++x.lgG;
    x.ns = ns_max;
    x.rr = x.ns + G + 4;
    x.cr = std::max(16, 4 * G);
    x.lds_per_wave = (int32_t)coop_lds_bytes(x.ns, G);
    if (sw(Sw::CoopLds) != 0 && (size_t)x.lds_per_wave <= (size_t)38 * 1024)
        launch_groups(C, k_banded_coop_lds<false>, x, (size_t)nwaves, 8, (size_t)x.lds_per_wave);
    else
        launch_groups(C, k_banded_coop, a, (size_t)nwaves, 8, 0);
    // fallback pass: one lane per task, only where a band-edge decision could not be resolved in time
    BandLayout lay = band_layout(L, false, false);
    lay.mat_u4 = 0;
    S.D = upload_layout(lay, C);
    BandedArgs b = score_args(B, S, reversed);
    b.only_if = S.O.hew;
    b.lane_rel = sw(Sw::LaneRel);
    launch_groups(C, k_banded<false>, b, L.ngroups(), 8, 0);
    tl.end();
    return S;
}

// upper bound of one pair's RLE string incl. terminator: every op its own run
static size_t cigar_bound(int m, int n) { return (size_t)2 * ((size_t)m + (size_t)n) + 12; }
// the same for an alignment made of `leaves` BandEd leaves whose run buffers hold at most `runs` runs in total: a run is
// "<= 10 digits + op"; never more than the every-op-its-own-run bound
static size_t cigar_bound_runs(int m, int n, int64_t runs, int leaves) {
    return std::min(cigar_bound(m, n), (size_t)11 * (size_t)(runs + 2 * leaves + 2) + 12);
}

// ---------------------------------------------------------------------------
// CIGAR assembly: per list entry ("root" = one pair's alignment) an ordered list of segments
// ---------------------------------------------------------------------------
struct SegList {
    std::vector<int64_t> off;                 // [nroots + 1]
    std::vector<int32_t> kind, a, b;
    std::vector<int32_t> root_pair;           // pair index of every root
    std::vector<size_t> bound;                // string bound of every root
};

struct AlignOut {                             // device, per root
    int32_t *len = nullptr, *edits = nullptr, *nops = nullptr;
    int64_t *str_off = nullptr, *total = nullptr;
    char* pool = nullptr;
    int32_t* ok = nullptr;                    // validator verdicts (null unless the batch asks for them)
    size_t nroots = 0;
    size_t pool_bytes = 0;                    // what `pool` was sized for (the host-side bound of the strings)
    // alignment tags (null unless the run asks for them): statistics; MD lengths, offsets, total, overflow flag and pool
    TagStats* stats = nullptr;
    int32_t *md_len = nullptr, *md_bad = nullptr;
    int64_t *md_off = nullptr, *md_total = nullptr;
    char* md_pool = nullptr;
    size_t md_pool_bytes = 0;                 // sum of tag_md_bound over the roots
};
static_assert(sizeof(TagStats) == sizeof(quicked_pair_stats_t) && sizeof(TagStats) == 32, "TagStats is quicked_pair_stats_t");

// Results of a sync == 0 run, still on the device: what quicked_batch_fetch() copies once the run is over.  The device
// pointers are those of the batch's result arena (stash_results): valid until the batch's next run, reload or destroy.
struct PanelOut; struct HitsOut;              // (the panel runners', below)
struct PendingFetch {
    int kind = 0;                             // 1: one score per task (score-only BandEd / WindowEd); 2: alignments (segments);
                                              // 3: a panel run; 4: an all-occurrences panel run (below)
    quicked_status_t ok_status = QUICKED_WIP;
    bool want_strings = false;
    // kind 1
    std::vector<int32_t> task_pair;
    const int32_t* d_score = nullptr; const u32* d_adv = nullptr; const u32* d_steps = nullptr; const int32_t* d_abort = nullptr;
    int counter_slot = 0;                     // where sum(adv) / sum(steps) goes in counters[]
    // a two-pass BandEd score-only run (launch_banded_narrow): its counts, and whose verdict they feed (narrow_report)
    const unsigned long long* d_narrow = nullptr; Context* narrow_ctx = nullptr; int narrow_cls = 0; bool narrow_probe = false;
    // kind 2
    SegList SL; AlignOut AO; std::vector<int32_t> root_status;
    std::vector<int32_t> leaf_pair; const u32* d_leaf_adv = nullptr; const u32* d_leaf_steps = nullptr;
    int64_t counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // what the run's host-side stages already counted
    bool quicked = false;                     // run_quicked ignores the Hirschberg status (quicked.c:290-291)
    // QuickEd fast path (quicked_fast): what decides which pairs still need the classic flow
    bool fast = false;
    const int32_t* d_cut = nullptr; const int32_t* d_skip = nullptr; const u32* d_stage_steps = nullptr;
    quicked_params_t params; TaskList L; size_t matrix_budget = 0;
    int parity = 0;                           // the plane set / ev_done slot of the run
    std::vector<int32_t> beyond_pair;         // bounded runs: pairs that are beyond their bound by their lengths alone (no task): score -1, ok_status
    std::vector<int32_t> pair_bound;          // bounded runs: every pair's bound (the fetch thresholds the pairs it hands to the QuickEd flow)
    bool search = false;                      // a search run (kind 1): locations per task next to the scores
    const int32_t* d_start = nullptr; const int32_t* d_end = nullptr;
    // kind 3: a panel run (PO), kind 4: an all-occurrences panel run (HO), queued on a batch configured for it
    // (quicked_batch_configure_panel_queue).  The getters show the run, and what kind it was, only once it is fetched: the
    // kind travels here.  no_text: every text is empty, nothing was launched
    std::shared_ptr<PanelOut> PO; std::shared_ptr<HitsOut> HO; int32_t panel_members = 0; bool no_text = false;
};

// One wavefront per alignment (k_banded_wave) is for few, long alignments: up to ~1000 tasks every task gets a wave of its
// own at once and the run takes one alignment's latency (measured, 10 kb reads: 4.2 ms against 5.1 ms for the
// cooperative form; beyond ~2000 tasks, or for 1 kb reads, the other forms win: tools/small_n_probe.py).  Needs whole
// passes (tfin == n: no stopped band to export) and a band that fits the wave.  QE_WAVE = 0 / 1 switches the form off /
// forces it wherever it is eligible (tests).
static bool wave_form_wanted(const TaskList& L) {
    const int force = sw(Sw::Wave);
    if (force == 0) return false;
    size_t live = 0;
    int n_max = 0;
    for (size_t t = 0; t < L.pair.size(); ++t) {
        if (L.pair[t] < 0) continue;
        ++live;
        n_max = std::max(n_max, L.n[t]);
        if (L.tfin[t] != L.n[t] || host_geometry(L.m[t], L.n[t], L.cutoff[t]).ebb_local > 62) return false;
    }
    return live > 0 && (force == 1 || (live <= (size_t)chip(tl_device).simds && n_max >= 4096));      // at most a wave per SIMD
}

static ScoreLaunch launch_banded_wave(quicked_batch& B, Context& C, const TaskList& L, bool reversed, int timed) {
    ScoreLaunch S;
    S.nt = L.pair.size();
    S.T = upload_tasks(L, C);
    S.O = take_out(C, S.nt);
    BandedArgs a = score_args(B, S, reversed);       // no group workspace
    a.fill_multi = 0; a.lane_rel = 0;
    TimedLaunches tl(C, timed - 1);       // timed = kind + 1, 0 = not timed
    launch_groups(C, k_banded_wave, a, S.nt, 4, 0);                     // one wave per task
    tl.end();
    return S;
}

// k_banded_sys<.., false> over the list (16 lanes per task for bands of <= 15 slots, else a wave per task), then
// k_banded<false> over the tasks it flagged (N, a taller band)
static ScoreLaunch launch_banded_sys(quicked_batch& B, Context& C, const TaskList& L, bool reversed, int lg, int timed, bool fill_geom = false,
                                     const int32_t* d_cut = nullptr, const int32_t* d_skip = nullptr) {
    ScoreLaunch S;
    S.nt = L.pair.size();
    BandLayout lay = band_layout(L, fill_geom, false);
    lay.mat_u4 = 0;
    int max_nsl = 0;
    for (int32_t v : lay.nslots) max_nsl = std::max(max_nsl, (int)v);
    S.T = upload_tasks(L, C);
    S.D = upload_layout(lay, C);
    S.O = take_out(C, S.nt);
    if (d_cut) apply_device_cutoffs(C, S.T, S.nt, S.O.score, d_cut, d_skip);
    BandedArgs a = score_args(B, S, reversed);
    a.fill_geom = fill_geom ? 1 : 0;
    a.o_abort = S.O.hew;
    a.lane_rel = sw(Sw::LaneRel);
    TimedLaunches tl(C, timed - 1);       // timed = kind + 1, 0 = not timed
    if (lg == 4) launch_groups(C, k_banded_sys<4, false>, with_prio(a), S.nt / 4, 4, 0, false, (size_t)40 * 1024);
    else launch_groups(C, k_banded_sys<6, false>, with_prio(a), S.nt, 4, 0, false, (size_t)40 * 1024);
    a.only_if = S.O.hew;
    if (lg == 6 && max_nsl > 63) launch_groups(C, k_banded_sys2<false>, with_prio(a), S.nt, 4, 0, false, (size_t)40 * 1024);      // bands of 64 .. 127 slots
    launch_groups(C, k_banded<false>, a, L.ngroups(), 8, 0);
    tl.end();
    return S;
}
// whole-text passes on few tasks (QuickEd's stage-3 doubling rounds on the pairs a run left, a BandEd score-only call on one
// pair or a few hundred): 0 = no, else log2 of the lanes per task.  QE_SCORE_SYS = 0 / 1: never / wherever eligible (tests)
static int sys_score_lanes(const TaskList& L, int in_flight, bool fill_geom = false) {
    const int env = sw(Sw::ScoreSys);
    if (env == 0) return 0;
    size_t live = 0;
    int max_nsl = 0;
    for (size_t t = 0; t < L.pair.size(); ++t) {
        if (L.pair[t] < 0) continue;
        ++live;
        if (L.tfin[t] != L.n[t]) return 0;                  // a stopped band is exported in k_banded's layout (Hirschberg half passes)
        const HGeom hg = host_geometry(L.m[t], L.n[t], L.cutoff[t]);
        max_nsl = std::max(max_nsl, fill_geom ? hg.ebb : hg.ebb_local);
    }
    if (live == 0 || max_nsl > 127) return 0;
    const size_t nt = L.pair.size(), fl = (size_t)std::max(1, in_flight);
    const Chip& chp = chip(tl_device);
    // one round of waves; two for the pass over the fill's cells, as for the fill itself (run_align's sys_fill: 12.5 k tasks, 3 125 waves)
    if (max_nsl <= 15) return (env == 1 || nt / 4 * fl <= (fill_geom ? 2 : 1) * chp.slots2()) ? 4 : 0;
    return (env == 1 || nt * fl <= chp.frac2(0.54)) ? 6 : 0;                            // a wave per task: about a wave per SIMD
}

// QuickEd's stage 3 (quicked.c:248-278) in ONE launch: k_banded_sys<.., false> with the band doubling on the device.  Every
// task comes back either converged (score = the exact distance within its last cutoff) or flagged with the cutoff it was about
// to run (its band outgrew the group's lanes, N symbols): the host's rounds take those from there.  false: not tried
// (too many tasks for a wave each).  QE_STAGE3_DEVICE = 0 / 1: never / whenever the list is not empty (tests)
static bool stage3_on_device(quicked_batch& B, Context& C, const TaskList& L, std::vector<int32_t>& score, std::vector<u32>& adv,
                             std::vector<int32_t>& flagged, std::vector<int32_t>& cutoff) {
    const int env = sw(Sw::Stage3Device);
    if (env == 0) return false;
    size_t live = 0;
    for (int32_t pr : L.pair) live += pr >= 0;
    if (live == 0 || (env != 1 && L.pair.size() > chip(C.device).frac2(0.54))) return false;
    const size_t nt = L.pair.size();
    ScoreLaunch S;                                   // no group workspace
    S.nt = nt;
    S.T = upload_tasks(L, C);
    S.O = take_out(C, nt);
    int32_t* d_cut = C.scratch_p->take<int32_t>(nt);
    HIP_CHECK(hipMemsetAsync(S.O.hew, 0, nt * sizeof(int32_t), C.stream));
    BandedArgs a = score_args(B, S, false);
    a.o_abort = S.O.hew; a.doubling = 1; a.o_cutoff = d_cut;
    launch_groups(C, k_banded_sys<6, false>, with_prio(a), nt, 4, 0, false, (size_t)40 * 1024);
    d2h(score, S.O.score, nt, C.stream); d2h(adv, S.O.adv, nt, C.stream); d2h(flagged, S.O.hew, nt, C.stream); d2h(cutoff, d_cut, nt, C.stream);
    HIP_CHECK(hipStreamSynchronize(C.stream));
    return true;
}

static void run_banded_score(quicked_batch& B, Context& C, const TaskList& L, bool reversed, StageResult* R,
                             bool fetch, int32_t** d_score_out, PendingFetch* pf = nullptr, bool narrow_ok = false) {
    // one wavefront per alignment only where the cooperative on-chip form has no room (a band of fewer than 8 slots): with
    // G = 8 lanes per alignment and 4-slot passes that form does a 10 kb pair in 2.7 ms, the wave form in 4.3
    const bool forced = sw_set(Sw::CoopG) || sw(Sw::Wave) == 1;      // tests of the other forms
    const int lg = forced ? 0 : sys_score_lanes(L, fetch ? 1 : C.in_flight);
    const int G0 = lg ? 1 : coop_lanes(L, fetch ? 1 : C.in_flight);
    const bool wave = !lg && wave_form_wanted(L) && (G0 < 2 || sw(Sw::Wave) == 1);
    const int G = wave ? 1 : G0;
    // two passes (launch_banded_narrow).  QE_SCORE_NARROW = 1: wherever a task's band at half its cutoff is narrower, in the
    // one-lane form whatever the list's size (tests); by default only where the one-lane form is the choice anyway, the list
    // has a group per SIMD (smaller ones are one wave's serial chain, and the forms that serve them were measured at full band
    // height), at least half of its tasks have a narrower band there, the workspace of the uniform layout is at most twice
    // the list's own (one outlier among short reads would otherwise size every group for itself: such a list keeps the single
    // pass, whose workspace is the sum of what the groups need), and the first pass has been paying (narrow_take)
    const int nmode = narrow_ok ? sw(Sw::ScoreNarrow) : 0;
    NarrowPlan np;
    BandLayout ulay;
    bool narrow = false, policy = false, probe = false;
    auto fits = [&]() {
        const BandLayout own = band_layout(L, false, false);
        ulay = narrow_uniform(own);
        return ulay.ws_bytes <= 2 * own.ws_bytes;
    };
    if (nmode == 1) { np = narrow_plan(L); narrow = np.ok && fits(); }
    else if (nmode != 0 && !forced && !lg && !wave && G < 2 && (size_t)L.ngroups() >= (size_t)chip(C.device).simds) {
        np = narrow_plan(L);
        policy = np.ok && 2 * np.narrower >= np.live;
        const int take = policy ? narrow_take(C, np.cls) : 0;
        if (take == 1 && !fits()) policy = false;
        narrow = policy && take == 1;
        probe = policy && take == 2;
    }
    const ScoreLaunch S = narrow ? launch_banded_narrow(B, C, L, reversed, 1, ulay, narrow_fit_q(C, np.cls, policy), narrow_prune_q(C, np.cls, policy), np.slots1) :
                          probe ? launch_banded_probe(B, C, L, reversed, 1) :
                          lg ? launch_banded_sys(B, C, L, reversed, lg, 1) :
                          wave ? launch_banded_wave(B, C, L, reversed, 1)
                               : ((G >= 2) ? launch_banded_coop(B, C, L, reversed, G, 1) : launch_banded_score(B, C, L, reversed, 1));
    if (d_score_out) *d_score_out = S.O.score;
    if (pf && !fetch) {
        pf->kind = 1; pf->task_pair = L.pair; pf->d_score = S.O.score; pf->d_adv = S.O.adv; pf->counter_slot = 0;
        pf->d_abort = (!narrow && !probe && G >= 2) ? S.O.hew : nullptr;
        pf->d_narrow = S.narrow; pf->narrow_ctx = policy ? &C : nullptr; pf->narrow_cls = np.cls; pf->narrow_probe = probe;
    }
    if (fetch && R) {
        FetchBatch fb(C);
        if (!narrow && !probe && G >= 2) fb.add(R->hew, S.O.hew, S.nt);              // abort flags (diagnostics)
        fb.add(R->score, S.O.score, S.nt); fb.add(R->adv, S.O.adv, S.nt);
        if (S.narrow) fb.add(R->narrow, (const unsigned long long*)S.narrow, QE_NARROW_STAT);
        fb.sync();
        R->narrow_probe = probe;
        if (S.narrow && policy) narrow_report(&C, np.cls, R->narrow, probe);
    }
}

// QuickEd with only_score (quicked.c:283-294 aligns and extract_results counts the alignment's edits, quicked.c:34-56): the
// bound is an upper bound of the distance (it is the cost of a real path), so the banded alignment with that cutoff is an
// optimal one and its edit count is the value of the fill's end cell -- which a pass over the FILL's cells (its band
// geometry, its bookkeeping: BandedArgs::fill_geom) computes without storing a checkpoint, walking a path or formatting a
// run.  A read whose align step would split (bpm_hirschberg.c:63-65) keeps it -- the children's distances add up to the same
// end value, but the levels' half passes are the faster way through a band that long (quicked_classic).  One lane per alignment,
// or the systolic forms where the launch is short of waves (run_fill_score).
// Measured on 10 kb pairs (align step / score pass, profiles/r06_t_probe_score_pass*.txt): one run alone 1 pair 3.9 / 2.9 ms,
// 1 k pairs 4.7 / 3.2, 4 k 4.8 / 3.2, 8 k 6.1 / 3.8, 12.5 k 8.2 / 5.0, 25 k 13.5 / 8.6, 100 k 21.9 / 14.3; a stream of queued runs
// 1 k pairs 0.44 / 1.5 M alignments/s, 4 k 2.9 / 4.8, 12.5 k 5.6 / 9.1, 25 k 6.3 / 10.4, 100 k 7.05 / 11.5 -- every size of such reads (taller bands: quicked_score_pass_fits).
// In the fast flow the pass reads its cutoffs from the device like the align step does (k_apply_cutoffs); pairs with lower-case /
// IUPAC symbols leave the flow there (Stage1Args::flags) and in the host-driven flow keep the whole batch on the align step.
// QE_QUICKED_SCORE_PASS = 0: never (the align step: tests), 1: wherever the results allow it and no read splits.
static bool quicked_score_pass_wanted() { return sw(Sw::QuickedScorePass) != 0; }
// ... and for THIS list (cutoffs: the bounds, or the fast flow's estimates): a run the caller waits for, of a few thousand
// tasks whose bands are too tall for the systolic forms, is a handful of one-lane waves with one wave's chain each, and the
// align step's cooperative fill is ahead there (2 000 pairs of 20 kb at 5 %: 11 ms against 15; of 10 kb at 10 %: 7.8 / 7.8;
// from 8 000 pairs on the pass wins: 20 / 16 and 12.6 / 7.9 ms).  Queued runs fill the chip together: always.
static bool quicked_score_pass_fits(const TaskList& L, bool fetch) {
    if (sw(Sw::QuickedScorePass) == 1 || !fetch) return true;
    if (sys_score_lanes(L, 1, true) != 0) return true;
    size_t live = 0;
    for (int32_t pr : L.pair) live += pr >= 0;
    return live >= (size_t)chip(tl_device).simds * 4;
}
// fetch: the scores and block-advance counts to the host (R).  pf: a queued run's (kind 1; the fast flow's fields are the caller's)
static void run_fill_score(quicked_batch& B, Context& C, const TaskList& L, StageResult* R, bool fetch, int32_t** d_score_out,
                           PendingFetch* pf = nullptr, const int32_t* d_cut = nullptr, const int32_t* d_skip = nullptr) {
    // launches of few waves: the systolic forms (16 lanes or a wave per task), as the score-only passes and the fills take them
    // (a cooperative LDS form of the pass was tried in round 6 and lost to the one-lane kernel everywhere: 2 000 / 8 000 / 30 000
    // pairs of 20 kb alone 21 / 21 / 30 ms against 15 / 16 / 21, its bands of ~20 slots leave G = 8 lanes 2 G + 4 slots and
    // most tasks to the fallback pass: profiles/r06_y_probe_coop_form.txt)
    const int lg = sys_score_lanes(L, fetch ? 1 : C.in_flight, true);
    const ScoreLaunch S = lg ? launch_banded_sys(B, C, L, false, lg, 2 /* timed as a fill */, true, d_cut, d_skip)
                             : launch_banded_score(B, C, L, false, 2, true, d_cut, d_skip);
    if (d_score_out) *d_score_out = S.O.score;
    if (pf && !fetch) {
        pf->kind = 1; pf->task_pair = L.pair; pf->d_score = S.O.score; pf->d_adv = S.O.adv; pf->counter_slot = 1;
        pf->ok_status = QUICKED_WIP;
    }
    if (fetch && R) {
        FetchBatch fb(C);
        fb.add(R->score, S.O.score, S.nt); fb.add(R->adv, S.O.adv, S.nt);
        fb.sync();
    }
}

// ---------------------------------------------------------------------------
// Bounded runs (quicked_batch_run_bounded): per task "the distance if it is within the task's bound, else -1".
// ---------------------------------------------------------------------------

// Which form takes a task.  QE_BOUNDED_DIAG = 1: the diagonal word (k_bounded_diag) wherever its precondition holds --
// bounded_diag_takes: min(bound, max(m, n)) <= 63; 0: never.  Unset, the library's choice: the diagonal word for pairs of
// 2000 bases and more, the lengths at which it was measured ahead of both the general path and a BANDED run at bandwidth 1
// by more than their spread (ms per queued run, diagonal word / general / BANDED: 400 k x 2 kb 4.4 / 9.8 / 8.1, 200 k x 4 kb
// 2.4 / 4.4 / 3.7, 100 k x 10 kb 2.5 / 3.4 / 3.1).  On 800 k x 1 kb (16.1 / 22.8 / 16.5) and 1 M x 150 b (19.7 / 27.8 / 20.4) it
// ties with the BANDED run -- such runs spend their time on the task list and the pack, which all three do -- although it
// is well ahead of the general path: by the rule of DESIGN.md 4.9 that is not enough for a default.
// Everything else goes through the general path: the score-only pass over the FILL's band geometry with cutoff = the bound
// (run_fill_score), then k_bounded_threshold.  That geometry (bpm_banded.c:121-135) holds the diagonals -rel .. diff + rel,
// rel = ceil((cutoff - |diff|) / 2), of Ukkonen's band in whole blocks, and "cutoff >= distance => end cell = distance" is
// what QuickEd's only_score rests on.
enum : int { QE_BOUNDED_DIAG_DEFAULT_MIN_LEN = 2000 };
static bool bounded_diag_wanted(int bound, int m, int n) {
    const int force = sw(Sw::BoundedDiag);
    if (force == 0 || !bounded_diag_takes(bound, m, n)) return false;
    return force == 1 || std::max(m, n) >= QE_BOUNDED_DIAG_DEFAULT_MIN_LEN;
}

// Ld / Lg: the tasks of the diagonal word / of the general path (bounded_pairs: cutoff = the effective bound, padded).  Leaves
// one score and one column count per task of `task_pair` on the device; the diagonal-word launch is timed as kind 3
// (quicked_batch_kernel_times)
struct BoundedOut { std::vector<int32_t> task_pair; int32_t* d_score = nullptr; u32* d_adv = nullptr; };
static BoundedOut run_bounded_score(quicked_batch& B, Context& C, const TaskList& Ld, const TaskList& Lg) {
    BoundedOut O;
    const size_t nd = Ld.pair.size(), ng = Lg.pair.size();
    O.task_pair = Ld.pair;
    O.task_pair.insert(O.task_pair.end(), Lg.pair.begin(), Lg.pair.end());
    if (nd + ng == 0) return O;
    O.d_score = C.scratch_p->take<int32_t>(nd + ng);
    O.d_adv = C.scratch_p->take<u32>(nd + ng);
    HIP_CHECK(hipMemsetAsync(O.d_score, 0xFF, (nd + ng) * sizeof(int32_t), C.stream));
    HIP_CHECK(hipMemsetAsync(O.d_adv, 0, (nd + ng) * sizeof(u32), C.stream));
    if (nd) {
        const DevTasks T = upload_tasks(Ld, C);
        BoundedArgs a{};
        a.P = pair_view(B, false); a.T = T.v; a.o_score = O.d_score; a.o_adv = O.d_adv;
        TimedLaunches tl(C, 3);
        launch_groups(C, k_bounded_diag, a, (size_t)Ld.ngroups(), 4, 0);
        tl.end();
    }
    if (ng) {
        PendingFetch G;                                // where the pass leaves its scores and block-advance counts
        int32_t* d_pass = nullptr;
        run_fill_score(B, C, Lg, nullptr, false, &d_pass, &G);
        int32_t* d_bound = C.scratch_p->take<int32_t>(ng);
        h2d(d_bound, Lg.cutoff, C.stream);
        hipLaunchKernelGGL(k_bounded_threshold, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, C.stream, (int)ng, G.d_score, G.d_adv,
                           (const int32_t*)d_bound, O.d_score + nd, O.d_adv + nd);
        HIP_CHECK(hipGetLastError());
    }
    return O;
}

// ---------------------------------------------------------------------------
// Search runs (quicked_batch_run_search): per task {d, text_start, text_end}, or {-1, -1, -1} = beyond.
// ---------------------------------------------------------------------------

// Which form takes a pattern of nb blocks: the register form's instantiation (1, 2 or 4 blocks), or 0 = the workspace form.
// QE_SEARCH_FORM = 0: the workspace form always; 1: the register form wherever it applies (up to QE_SEARCH_REG_BLOCKS
// blocks = 256 bases).  Unset, the library's choice, by the rule of DESIGN.md 4.9 -- the register form only where its median
// beats the workspace form's by more than the larger of the two spreads -- is the workspace form at every block count: the
// register form's kernels are the faster ones (1 M pairs in 400-base texts, both passes, workspace / registers: 3.1 / 2.1 ms
// at 64 bases, 4.1 / 3.4 at 128, 3.9 / 3.6 at 150, 6.1 / 5.5 at 256), but a queued run of that size takes 14 - 20 ms, most of it
// the host's task lists and uploads, and there the register form was level (150 bases: 16.1 against 16.3 ms, spread 1.1) or
// behind (64 / 128 / 256 bases: 19.9 / 17.1 / 19.5 against 15.7 / 15.4 / 14.8 ms).  DESIGN.md 4.12, profiles/search.md.
static int search_reg_form(int nb) {
    if (sw(Sw::SearchForm) != 1 || nb > QE_SEARCH_REG_BLOCKS) return 0;
    return nb <= 1 ? 1 : (nb == 2 ? 2 : 4);
}
static_assert((int)QUICKED_SEARCH_PREFIX == (int)SEARCH_PREFIX && (int)QUICKED_SEARCH_INFIX == (int)SEARCH_INFIX, "quicked_search_mode_t is qe_search.h's mode");

// The lists of a search run: one per kernel form, so that a wave's lanes are of a kind ([0] the workspace form, [1] / [2] /
// [3] the register form of 1 / 2 / 4 blocks); a task's index in the run's outputs is its list's offset plus its index
// there.  Within a list the tasks keep the batch's order (sorted by length).
struct SearchLists { TaskList L[4]; };
static int search_bound(const SearchRun& sr, int pr) { return sr.max_dist ? sr.max_dist[pr] : sr.max_dist_all; }
static void search_pairs(const quicked_batch& B, const SearchRun& sr, SearchLists& S) {
    for (int64_t i = 0; i < B.n; ++i) {
        const int pr = B.order[(size_t)i];
        const int m = B.p_len[pr], n = B.t_len[pr];
        if (m == 0 || n == 0) continue;                             // QUICKED_EMPTY_SEQUENCE, as in every run
        const int f = search_reg_form(search_blocks(m));
        S.L[f == 0 ? 0 : (f == 1 ? 1 : (f == 2 ? 2 : 3))].push(pr, 0, m, 0, n, search_effective(search_bound(sr, pr), m), n);
    }
    for (TaskList& l : S.L) l.pad();
}

// the workspace form's groups: Pv | Mv | S of the group's tallest pattern
struct SearchWs { uint8_t* ws = nullptr; int64_t* d_ws_off = nullptr; int32_t* d_nb = nullptr; };
static size_t search_group_bytes(int nb) { return ((size_t)nb * 64 * (8 + 8 + 4) + 255) & ~(size_t)255; }
static SearchWs search_workspace(Context& C, const TaskList& Lw) {
    SearchWs W;
    const int ngw = Lw.ngroups();
    std::vector<int64_t> ws_off((size_t)ngw);
    std::vector<int32_t> g_nb((size_t)ngw);
    size_t ws_bytes = 0;
    for (int g = 0; g < ngw; ++g) {
        int nb = 1;
        for (int l = 0; l < 64; ++l) if (Lw.pair[(size_t)g * 64 + l] >= 0) nb = std::max(nb, search_blocks(Lw.m[(size_t)g * 64 + l]));
        g_nb[g] = nb; ws_off[g] = (int64_t)ws_bytes;
        ws_bytes += search_group_bytes(nb);
    }
    if (ngw) {
        W.ws = C.scratch_p->take<uint8_t>(ws_bytes + 256);
        W.d_ws_off = C.scratch_p->take<int64_t>((size_t)ngw); W.d_nb = C.scratch_p->take<int32_t>((size_t)ngw);
        CopyBatch cb(C.stream);
        h2d(W.d_ws_off, ws_off, C.stream); h2d(W.d_nb, g_nb, C.stream);
    }
    return W;
}

// The kernel of a form (0 the workspace form, 1 / 2 / 3 the register form of 1 / 2 / 4 blocks) under the run's equality
template <class Eq> static void launch_search_eq(Context& C, int f, const SearchArgs& a, size_t ng) {
    if (f == 0) launch_groups(C, k_search<0, Eq>, a, ng, 4, 0);
    else if (f == 1) launch_groups(C, k_search<1, Eq>, a, ng, 4, 0);
    else if (f == 2) launch_groups(C, k_search<2, Eq>, a, ng, 4, 0);
    else launch_groups(C, k_search<4, Eq>, a, ng, 4, 0);
}
static void launch_search(Context& C, int eq, int f, const SearchArgs& a, size_t ng) {
    if (eq) launch_search_eq<SearchEqIupac>(C, f, a, ng); else launch_search_eq<SearchEq3>(C, f, a, ng);
}
template <class Eq> static void launch_search_hits_eq(Context& C, int f, const SearchHitsArgs& x, size_t ng) {
    if (f == 0) launch_groups(C, k_search_hits<0, Eq>, x, ng, 4, 0);
    else if (f == 1) launch_groups(C, k_search_hits<1, Eq>, x, ng, 4, 0);
    else if (f == 2) launch_groups(C, k_search_hits<2, Eq>, x, ng, 4, 0);
    else launch_groups(C, k_search_hits<4, Eq>, x, ng, 4, 0);
}
static void launch_search_hits(Context& C, int eq, int f, const SearchHitsArgs& x, size_t ng) {
    if (eq) launch_search_hits_eq<SearchEqIupac>(C, f, x, ng); else launch_search_hits_eq<SearchEq3>(C, f, x, ng);
}

// The planes a search pass reads.  The library's equality: the batch's own (pair_view).  A flagged run (eq 1
// QUICKED_SEARCH_IUPAC, 2 QUICKED_SEARCH_IUPAC_PATTERN): four membership planes, packed into the run's pool
// when a pass first asks for them -- forward for the forward pass, reversed for the start pass -- from the resident ASCII
// (k_pack_iupac) or, packed batch, from its three planes (k_planes_iupac; the reversed ones from the reversed three).  They
// live as long as the run: no batch state, nothing a reload, the other flag or another plane set could leave stale.  The
// offsets stay the batch's three-plane ones (SearchEqIupac::offset).
static size_t search_iupac_bytes(const quicked_batch& B, int eq, int mode) {      // what a flagged run takes from its pool for them
    if (!eq) return 0;
    const size_t one = (iupac_offset((int64_t)B.pl_p_words) + iupac_offset((int64_t)B.pl_t_words) + 16) * sizeof(u64) + 512;
    return mode == SEARCH_INFIX ? 2 * one : one;
}
// one side's four planes: the patterns' or the texts'.  QUICKED_SEARCH_IUPAC_PATTERN (eq 2) narrows the texts alone: ACGT only
// (k_pack_iupac's acgt_only), N the empty set (k_planes_iupac's n_empty)
static u64* iupac_side_planes(quicked_batch& B, Context& C, int eq, bool reversed, bool text) {
    if (B.packed && reversed) ensure_reversed(B, C);
    const PairView v = pair_view(B, reversed);
    u64* pl = C.scratch_p->take<u64>((size_t)iupac_offset((int64_t)(text ? B.pl_t_words : B.pl_p_words)) + 8);
    const int blocks = (int)((B.n + 3) / 4), narrow = (text && eq == 2) ? 1 : 0;
    if (B.packed) {
        IupacPlanesArgs a;
        a.nseq = (int32_t)B.n; a.n_empty = narrow;
        a.src = text ? v.pl_t : v.pl_p; a.dst = pl; a.pl_off = text ? B.d_plt_off : B.d_plp_off; a.len = text ? B.d_t_len : B.d_p_len;
        hipLaunchKernelGGL(k_planes_iupac, dim3(blocks), dim3(256), 0, C.stream, a);
    } else {
        IupacPackArgs a;
        a.nseq = (int32_t)B.n; a.reverse = reversed ? 1 : 0; a.acgt_only = narrow;
        a.asc = text ? B.d_asc_t : B.d_asc_p; a.asc_off = text ? B.d_t_off : B.d_p_off; a.len = text ? B.d_t_len : B.d_p_len;
        a.planes = pl; a.pl_off = text ? B.d_plt_off : B.d_plp_off;
        hipLaunchKernelGGL(k_pack_iupac, dim3(blocks), dim3(256), 0, C.stream, a);
    }
    HIP_CHECK(hipGetLastError());
    return pl;
}
static PairView search_planes(quicked_batch& B, Context& C, int eq, bool reversed) {
    if (!eq) return pair_view(B, reversed);
    u64* const pl_p = iupac_side_planes(B, C, eq, reversed, false);
    u64* const pl_t = iupac_side_planes(B, C, eq, reversed, true);
    PairView v = pair_view(B, reversed);
    v.pl_p = pl_p; v.pl_t = pl_t;
    return v;
}

// Forward pass over whole pairs, then -- INFIX -- the start pass: the PREFIX form over the reversed planes on the stretch
// that ends at text_end, bound d, the largest end; it reads the forward pass's results on the device and runs only the
// tasks within their bound (no host round trip).  Leaves per task of `task_pair` score / start / end and the block steps
// of both passes on the device.  Both passes are timed as kind 0 (quicked_batch_kernel_times).
struct SearchOut { std::vector<int32_t> task_pair; int32_t *d_score = nullptr, *d_start = nullptr, *d_end = nullptr; u32* d_adv = nullptr; };
static SearchOut run_search(quicked_batch& B, Context& C, const SearchLists& S, int mode, int eq = 0) {
    SearchOut O;
    size_t off[5] = {0, 0, 0, 0, 0};
    for (int f = 0; f < 4; ++f) {
        O.task_pair.insert(O.task_pair.end(), S.L[f].pair.begin(), S.L[f].pair.end());
        off[f + 1] = O.task_pair.size();
    }
    const size_t nt = O.task_pair.size();
    if (nt == 0) return O;
    int32_t* blk = C.scratch_p->take<int32_t>(4 * nt);
    O.d_score = blk; O.d_start = blk + nt; O.d_end = blk + 2 * nt; O.d_adv = (u32*)(blk + 3 * nt);
    HIP_CHECK(hipMemsetAsync(blk, 0xFF, 3 * nt * sizeof(int32_t), C.stream));
    HIP_CHECK(hipMemsetAsync(O.d_adv, 0, nt * sizeof(u32), C.stream));
    const SearchWs Wk = search_workspace(C, S.L[0]);
    uint8_t* const ws = Wk.ws; int64_t* const d_ws_off = Wk.d_ws_off; int32_t* const d_nb = Wk.d_nb;
    DevTasks T[4];
    for (int f = 0; f < 4; ++f) if (!S.L[f].pair.empty()) T[f] = upload_tasks(S.L[f], C);
    auto pass = [&](bool start_pass) {
        const PairView PV = search_planes(B, C, eq, start_pass);
        TimedLaunches tl(C, 0);
        for (int f = 0; f < 4; ++f) {
            if (S.L[f].pair.empty()) continue;
            SearchArgs a{};
            a.P = PV; a.T = T[f].v;
            a.mode = start_pass ? SEARCH_PREFIX : mode; a.flags = start_pass ? SEARCH_LARGEST_END : 0;
            a.in_score = start_pass ? O.d_score + off[f] : nullptr; a.in_end = start_pass ? O.d_end + off[f] : nullptr;
            a.o_score = O.d_score + off[f]; a.o_end = O.d_end + off[f]; a.o_start = O.d_start + off[f]; a.o_adv = O.d_adv + off[f];
            const size_t ng = (size_t)S.L[f].ngroups();
            if (f == 0) { a.ws = ws; a.g_ws_off = d_ws_off; a.g_nb = d_nb; }
            launch_search(C, eq, f, a, ng);
        }
        tl.end();
    };
    pass(false);
    if (mode == SEARCH_INFIX) {
        if (!eq) ensure_reversed(B, C);
        pass(true);
    }
    return O;
}

// Every occurrence within the bound (quicked_batch_run_search_all): the forward pass in its all-occurrences form
// (k_search_hits: found / best score / stored per pair, up to max_hits {end, score} per task), the offset scan over the stored
// counts in the order of the pairs, and -- the one thing the host reads in between -- their total, which sizes the rest: the
// stored occurrences become a task list on the device (k_hits_expand) and, INFIX, the best search's start pass runs one lane
// per occurrence over its window of min(text_end, m + score) columns.  That list is in the order of the pairs, so its waves
// mix the kernel forms: every form that has tasks gets a pair array of its own (-1 where an occurrence is another form's) and
// a launch over the whole list; a wave without a lane of the form leaves at once.  The workspace form's groups are all as
// tall as the list's tallest pattern, and are run in slices that share one workspace of at most 256 MiB (QE_SEARCH_HITS_WS_KB).
// Both passes are timed as kind 0; d_adv / d_adv2 hold their block steps per task / per occurrence.
struct HitsOut {                                   // of both all-occurrences runs, pairs and panel
    std::vector<int32_t> task_pair;                // task (panel: slot) -> pair, -1 in the padding
    int32_t *d_found = nullptr, *d_best = nullptr, *d_hits = nullptr; int64_t* d_off = nullptr; u32 *d_adv = nullptr, *d_adv2 = nullptr;
    int64_t total = 0;
    // QUICKED_PANEL_CIGARS (run_panel_align): per stored occurrence where its string starts in the pool (-1: the aligner and the
    // sweeps disagree) and its block steps | operations; the pool's bytes
    bool cigars = false;
    int64_t* d_cig_off = nullptr; char* d_cig_pool = nullptr; int64_t cig_bytes = 0; u32* d_al_steps = nullptr;
    // QUICKED_PANEL_TAILS (run_panel_tails): every pair's quicked_panel_tail_t (-1 in every field: none) and the row steps of
    // the walk per slot (task_pair.size() of them)
    int32_t* d_tails = nullptr; u32* d_tail_rows = nullptr;
    // QUICKED_PANEL_HEADS (run_panel_heads): every pair's quicked_panel_head_t (-1 in every field: none) and, per slot, the
    // block steps of the head sweep | the row steps of its walk (2 x task_pair.size() of them)
    int32_t* d_heads = nullptr; u32* d_head_steps = nullptr;
    // a queued panel run (quicked_batch_configure_panel_queue): total = -1 -- the fetch takes it from the offsets --, the records'
    // room, and {W, the records' bytes, the step counts' bytes} on the device (k_panel_queue_clamp)
    int64_t cap = 0; int64_t* d_queue = nullptr;
};
// The per-pair arrays of an all-occurrences run -- found (0) | smallest score (-1) | stored - 1 (-1: the scan then counts 0) --,
// the offsets and `nadv` step counters.  -> the stored counts, for the forward pass to fill
static int32_t* hits_arrays(Context& C, HitsOut& O, size_t n, size_t nadv) {
    int32_t* blk = C.scratch_p->take<int32_t>(3 * n);
    O.d_found = blk; O.d_best = blk + n;
    HIP_CHECK(hipMemsetAsync(O.d_found, 0, n * sizeof(int32_t), C.stream));
    HIP_CHECK(hipMemsetAsync(O.d_best, 0xFF, 2 * n * sizeof(int32_t), C.stream));
    O.d_adv = C.scratch_p->take<u32>(nadv);
    HIP_CHECK(hipMemsetAsync(O.d_adv, 0, nadv * sizeof(u32), C.stream));
    O.d_off = C.scratch_p->take<int64_t>(n + 1);
    return blk + 2 * n;
}
// ... and behind the forward pass the offsets in the order of the pairs (every pair counts: d_seq_len, lengths that are never
// negative, stands in for the scan's list of tasks) with the total behind them -- the one thing the host reads in between
static void hits_offsets(const quicked_batch& B, Context& C, HitsOut& O, const int32_t* d_len, const int32_t* d_seq_len) {
    const size_t n = (size_t)B.n;
    hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(1024), 0, C.stream, d_len, d_seq_len, O.d_off, O.d_off + n, (int)n);
    HIP_CHECK(hipGetLastError());
}
static void hits_total(const quicked_batch& B, Context& C, HitsOut& O, const int32_t* d_len, const int32_t* d_seq_len) {
    const size_t n = (size_t)B.n;
    hits_offsets(B, C, O, d_len, d_seq_len);
    std::vector<int64_t> tot;
    FetchBatch fb(C);
    fb.add(tot, (const int64_t*)(O.d_off + n), 1);
    fb.sync();
    O.total = tot[0];
}
// The start pass of the panel runs: k_search<4, Eq> in its start-pass form (PREFIX, the largest end, bound and window from the
// forward pass's score / end on the device) over nt tasks laid out as arrays, one launch, timed as kind 0.
// Its arrays: {pair | m | n | score | end | start} in one take, the kernel before the pass writes the first five (into(): its
// argument block's o_* fields); start is preset to -1, which a lane that finds nothing leaves, and adv -- the block steps per
// task, a seventh stretch of the take or (adv_apart, the runs that fetch it: HitsOut / PanelOut::d_adv2) a take of its own -- to 0
struct StartTasks {
    size_t nt = 0;                                  // 0: a run without the pass
    int32_t *pair = nullptr, *m = nullptr, *n = nullptr, *score = nullptr, *end = nullptr, *start = nullptr;
    u32* adv = nullptr;
    template <class A> void into(A& a) const { a.o_pair = pair; a.o_m = m; a.o_n = n; a.o_score = score; a.o_end = end; }
};
static StartTasks take_start_tasks(Context& C, size_t nt, bool adv_apart) {
    StartTasks t;
    t.nt = nt;
    int32_t* q = C.scratch_p->take<int32_t>((adv_apart ? 6 : 7) * nt);
    t.pair = q; t.m = q + nt; t.n = q + 2 * nt; t.score = q + 3 * nt; t.end = q + 4 * nt; t.start = q + 5 * nt;
    t.adv = adv_apart ? C.scratch_p->take<u32>(nt) : (u32*)(q + 6 * nt);
    HIP_CHECK(hipMemsetAsync(t.start, 0xFF, nt * sizeof(int32_t), C.stream));
    HIP_CHECK(hipMemsetAsync(t.adv, 0, nt * sizeof(u32), C.stream));
    return t;
}
static void launch_start_pass(Context& C, int eq, const PairView& PV, const StartTasks& t) {
    SearchArgs s{};
    s.P = PV;
    s.T.ntasks = (int32_t)t.nt; s.T.pair = t.pair; s.T.m = t.m; s.T.n = t.n; s.T.cutoff = t.score;
    s.mode = SEARCH_PREFIX; s.flags = SEARCH_LARGEST_END;
    s.in_score = t.score; s.in_end = t.end; s.o_start = t.start; s.o_adv = t.adv;
    TimedLaunches tl(C, 0);
    launch_search(C, eq, 3, s, (t.nt + 63) / 64);
    tl.end();
}
static HitsOut run_search_hits(quicked_batch& B, Context& C, const SearchLists& S, int mode, int max_hits, int eq = 0) {
    HitsOut O;
    size_t off[5] = {0, 0, 0, 0, 0};
    for (int f = 0; f < 4; ++f) {
        O.task_pair.insert(O.task_pair.end(), S.L[f].pair.begin(), S.L[f].pair.end());
        off[f + 1] = O.task_pair.size();
    }
    const size_t nt = O.task_pair.size();
    if (nt == 0) return O;
    int32_t* const d_len = hits_arrays(C, O, (size_t)B.n, nt);
    int32_t* raw = C.scratch_p->take<int32_t>(2 * nt * (size_t)max_hits);
    const SearchWs Wk = search_workspace(C, S.L[0]);
    DevTasks T[4];
    for (int f = 0; f < 4; ++f) if (!S.L[f].pair.empty()) T[f] = upload_tasks(S.L[f], C);
    const PairView PF = search_planes(B, C, eq, false);
    TimedLaunches tl(C, 0);
    for (int f = 0; f < 4; ++f) {
        if (S.L[f].pair.empty()) continue;
        SearchHitsArgs x{};
        x.S.P = PF; x.S.T = T[f].v; x.S.mode = mode; x.S.o_adv = O.d_adv + off[f];
        x.max_hits = max_hits; x.raw = raw + 2 * off[f] * (size_t)max_hits;
        x.o_found = O.d_found; x.o_best = O.d_best; x.o_len = d_len;
        const size_t ng = (size_t)S.L[f].ngroups();
        if (f == 0) { x.S.ws = Wk.ws; x.S.g_ws_off = Wk.d_ws_off; x.S.g_nb = Wk.d_nb; }
        launch_search_hits(C, eq, f, x, ng);
    }
    tl.end();
    hits_total(B, C, O, d_len, B.d_p_len);                // (a pair without a task has 0 stored)
    if (O.total <= 0) return O;
    const size_t nh = (size_t)O.total;
    const bool infix = mode == SEARCH_INFIX;
    O.d_hits = C.scratch_p->take<int32_t>(3 * nh);
    int32_t *o_m = nullptr, *o_n = nullptr, *o_score = nullptr, *o_end = nullptr, *o_start = nullptr, *o_pair[4] = {nullptr, nullptr, nullptr, nullptr};
    if (infix) {
        int32_t* q = C.scratch_p->take<int32_t>(5 * nh);
        o_m = q; o_n = q + nh; o_score = q + 2 * nh; o_end = q + 3 * nh; o_start = q + 4 * nh;
        HIP_CHECK(hipMemsetAsync(o_start, 0xFF, nh * sizeof(int32_t), C.stream));
        for (int f = 0; f < 4; ++f) {
            if (S.L[f].pair.empty()) continue;
            o_pair[f] = C.scratch_p->take<int32_t>(nh);
            HIP_CHECK(hipMemsetAsync(o_pair[f], 0xFF, nh * sizeof(int32_t), C.stream));
        }
        O.d_adv2 = C.scratch_p->take<u32>(nh);
        HIP_CHECK(hipMemsetAsync(O.d_adv2, 0, nh * sizeof(u32), C.stream));
    }
    for (int f = 0; f < 4; ++f) {
        if (S.L[f].pair.empty()) continue;
        HitExpandArgs e{};
        e.T = T[f].v; e.max_hits = max_hits; e.infix = infix ? 1 : 0; e.raw = raw + 2 * off[f] * (size_t)max_hits;
        e.len = d_len; e.off = O.d_off; e.hits = O.d_hits;
        e.o_pair = o_pair[f]; e.o_m = o_m; e.o_n = o_n; e.o_score = o_score; e.o_end = o_end;
        hipLaunchKernelGGL(k_hits_expand, dim3((unsigned)((S.L[f].pair.size() + 255) / 256)), dim3(256), 0, C.stream, e);
        HIP_CHECK(hipGetLastError());
    }
    if (!infix) return O;
    if (!eq) ensure_reversed(B, C);
    const PairView PR = search_planes(B, C, eq, true);
    TimedLaunches tl2(C, 0);
    const size_t ngh = (nh + 63) / 64;
    for (int f = 0; f < 4; ++f) {
        if (S.L[f].pair.empty()) continue;
        SearchArgs a{};
        a.P = PR;
        a.mode = SEARCH_PREFIX; a.flags = SEARCH_LARGEST_END;
        size_t slice = ngh;                              // groups per launch
        if (f == 0) {
            int nb = 1;
            for (size_t t = 0; t < S.L[0].pair.size(); ++t) if (S.L[0].pair[t] >= 0) nb = std::max(nb, search_blocks(S.L[0].m[t]));
            const size_t gb = search_group_bytes(nb);
            slice = std::max<size_t>(1, std::min(ngh, ((size_t)std::max<long long>(1, sw_ll(Sw::SearchHitsWsKb)) << 10) / gb));
            std::vector<int64_t> ws_off(slice);
            std::vector<int32_t> g_nb(slice, nb);
            for (size_t g = 0; g < slice; ++g) ws_off[g] = (int64_t)(g * gb);
            a.ws = C.scratch_p->take<uint8_t>(slice * gb + 256);
            int64_t* d_ws_off = C.scratch_p->take<int64_t>(slice); int32_t* d_nb = C.scratch_p->take<int32_t>(slice);
            CopyBatch cb(C.stream);
            h2d(d_ws_off, ws_off, C.stream); h2d(d_nb, g_nb, C.stream);
            a.g_ws_off = d_ws_off; a.g_nb = d_nb;
        }
        for (size_t g0 = 0; g0 < ngh; g0 += slice) {
            const size_t j0 = g0 * 64, ng = std::min(slice, ngh - g0);
            a.T = TaskView{};
            a.T.ntasks = (int32_t)std::min(nh - j0, ng * 64);
            a.T.pair = o_pair[f] + j0; a.T.m = o_m + j0; a.T.n = o_n + j0; a.T.cutoff = o_score + j0;
            a.in_score = o_score + j0; a.in_end = o_end + j0; a.o_start = o_start + j0; a.o_adv = O.d_adv2 + j0;
            launch_search(C, eq, f, a, ng);
        }
    }
    tl2.end();
    hipLaunchKernelGGL(k_hits_finish, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, C.stream, (int64_t)nh, (const int32_t*)o_start, O.d_hits);
    HIP_CHECK(hipGetLastError());
    return O;
}

// ---------------------------------------------------------------------------
// Panel runs (quicked_batch_run_panel; qe_panel.h): every text of the batch against one shared set of patterns.
// ---------------------------------------------------------------------------

// Slices of the panel, chosen on the host: one while the text groups alone fill the chip (two waves on every SIMD); else enough
// that groups x slices reach about twice the resident wave slots -- the last waves of a launch then have company --, never more
// than the panel has members.  QE_PANEL_SLICES forces a count (clamped to 1 .. K).
static int panel_slices(const Context& C, size_t ngroups, int K) {
    if (sw_set(Sw::PanelSlices)) return (int)std::max<long long>(1, std::min<long long>(K, sw_ll(Sw::PanelSlices)));
    const size_t slots = chip(C.device).slots2();
    if (ngroups >= slots) return 1;
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)K, (2 * slots + ngroups - 1) / std::max<size_t>(1, ngroups)));
}
// the three-plane words of the panel's members, two rows of zeros behind each (k_pack's layout)
static size_t panel_plane_words(const PanelRun& pr) {
    size_t w = 0;
    for (int32_t p = 0; p < pr.n_patterns; ++p) w += 3 * ((size_t)(pr.len[p] + 63) / 64 + 2);
    return w;
}
// the non-empty texts of the batch: the ones a panel run gives a slot
static size_t panel_texts(const quicked_batch& B) {
    size_t texts = 0;
    for (int64_t i = 0; i < B.n; ++i) texts += B.t_len[(size_t)i] > 0;
    return texts;
}
// a panel of K members cut into `want` slices at the most: the members per slice, and the slices that makes
struct PanelCut { int per_slice, nslices; };
static PanelCut panel_cut(int K, int want) {
    const int per_slice = (K + want - 1) / want;
    return PanelCut{per_slice, (K + per_slice - 1) / per_slice};
}
// What the panel runs take from their pools alike (the planner's fixed needs): the panel's bytes, tables and planes (forward and,
// INFIX, reversed), a flagged run's four-plane words of the texts, the takes' padding.  -> nslots: the non-empty texts in whole
// waves, as panel_upload lays them out
static size_t panel_shared_bytes(const quicked_batch& B, const SearchRun& sr, size_t& nslots) {
    const PanelRun& pr = *sr.panel;
    size_t pool = 0;
    for (int32_t p = 0; p < pr.n_patterns; ++p) pool += (size_t)pr.len[p];
    nslots = (panel_texts(B) + 63) / 64 * 64;
    const size_t K = (size_t)pr.n_patterns, passes = sr.mode == SEARCH_INFIX ? 2 : 1;
    size_t b = pool + 64 + K * 32 + passes * (size_t)iupac_offset((int64_t)panel_plane_words(pr) + 24) * sizeof(u64);
    if (sr.eq) b += passes * ((size_t)iupac_offset((int64_t)B.pl_t_words) + 16) * sizeof(u64);
    return b + 16 * 512;
}
// ... and a panel run besides: the slice partials at the most slices the host would choose, the start-pass arrays, the matrix
static size_t panel_fixed_bytes(const quicked_batch& B, const Context& C, const SearchRun& sr) {
    const PanelRun& pr = *sr.panel;
    size_t nslots = 0, b = panel_shared_bytes(B, sr, nslots);
    const size_t n = (size_t)B.n, K = (size_t)pr.n_patterns;
    b += 6 * (size_t)panel_slices(C, nslots / 64, pr.n_patterns) * nslots * sizeof(int32_t);
    b += nslots * 4 + n * 24 + nslots * 8 * 4 + n * 8;
    if (pr.matrix) b += 2 * n * K * sizeof(int32_t);
    return b;
}
// The text planes a panel pass reads: the batch's own under the library's equality; a flagged run packs the four membership
// planes of the TEXTS into its pool, as search_planes does for both sides -- the batch's patterns play no part
static const u64* panel_text_planes(quicked_batch& B, Context& C, int eq, bool reversed) {
    return eq ? iupac_side_planes(B, C, eq, reversed, true) : pair_view(B, reversed).pl_t;
}

// The run: the panel's bytes and tables go up in one block and are packed on the device by the batch's own packers (k_pack
// with null flags, and k_panel_wire_codes behind it where the batch is a packed one; k_pack_iupac for a flagged run), forward
// and -- INFIX -- reversed; k_search_panel over text groups x slices
// leaves the partial keepers; k_panel_reduce merges them into the texts' results and, INFIX, the tasks of the start pass,
// which is the unchanged k_search<4, Eq> in its start-pass form (PREFIX, SEARCH_LARGEST_END, SearchArgs::in_score) over a
// PairView whose pattern side is the reversed panel planes with a per-text offset array: every member has at most four blocks
// and pattern_rows gives zero planes for the absent ones.  No per-pair task list: the one array that goes up per text is its
// slot's pair index.  Both passes are timed as kind 0.
struct PanelOut {
    std::vector<int32_t> text;                     // slot -> pair, -1 in the padding
    int32_t *d_hits = nullptr, *d_mscore = nullptr, *d_mend = nullptr; u32 *d_adv = nullptr, *d_adv2 = nullptr;
};
// The panel and the text slots on the device, shared by the panel runs: one host block {asc_off | pl_off | len | bound |
// bytes} in one upload, and slot -> pair in the batch's length order (the non-empty texts, padded to whole waves with -1)
struct PanelDev {
    std::vector<int32_t> text;                     // slot -> pair, -1 in the padding; empty: no text to search
    size_t nslots = 0, ngroups = 0, words3 = 0;
    const int64_t *d_asc_off = nullptr, *d_pl_off = nullptr;  const int32_t *d_len = nullptr, *d_bound = nullptr;  const uint8_t* d_pool = nullptr;
    int32_t* d_text = nullptr;
};
static PanelDev panel_upload(quicked_batch& B, Context& C, const SearchRun& sr) {
    const PanelRun& pr = *sr.panel;
    const int K = pr.n_patterns;
    PanelDev D;
    for (int64_t i = 0; i < B.n; ++i) { const int p = B.order[(size_t)i]; if (B.t_len[(size_t)p] > 0) D.text.push_back(p); }
    if (D.text.empty()) return D;
    while (D.text.size() % 64) D.text.push_back(-1);
    D.nslots = D.text.size(); D.ngroups = D.nslots / 64;
    D.words3 = panel_plane_words(pr);
    size_t pool_bytes = 0;
    for (int p = 0; p < K; ++p) pool_bytes += (size_t)pr.len[p];
    const size_t tab_bytes = (size_t)K * (8 + 8 + 4 + 4), blk_bytes = (tab_bytes + pool_bytes + 15) & ~(size_t)15;
    static thread_local std::vector<uint8_t> host;
    host.assign(blk_bytes, 0);
    int64_t* h_asc_off = (int64_t*)host.data();
    int64_t* h_pl_off = h_asc_off + K;
    int32_t* h_len = (int32_t*)(h_pl_off + K);
    int32_t* h_bound = h_len + K;
    uint8_t* h_pool = (uint8_t*)(h_bound + K);
    {
        int64_t at = 0, w = 0;
        for (int p = 0; p < K; ++p) {
            h_asc_off[p] = at; h_pl_off[p] = w; h_len[p] = pr.len[p];
            h_bound[p] = sr.max_dist ? sr.max_dist[p] : sr.max_dist_all;
            memcpy(h_pool + at, pr.pool + pr.off[p], (size_t)pr.len[p]);
            at += pr.len[p]; w += 3 * ((int64_t)(pr.len[p] + 63) / 64 + 2);
        }
    }
    uint8_t* d_blk = C.scratch_p->take<uint8_t>(blk_bytes + 16);
    h2d_bytes(d_blk, host.data(), blk_bytes, C.stream);
    D.d_asc_off = (const int64_t*)d_blk;
    D.d_pl_off = D.d_asc_off + K;
    D.d_len = (const int32_t*)(D.d_pl_off + K);
    D.d_bound = D.d_len + K;
    D.d_pool = (const uint8_t*)(D.d_bound + K);
    D.d_text = C.scratch_p->take<int32_t>(D.nslots);
    h2d(D.d_text, D.text, C.stream);
    return D;
}
// the panel's planes, packed on the device by the batch's own packers: forward, or reversed for a start pass
static const u64* panel_planes(quicked_batch& B, Context& C, const PanelDev& D, int K, int eq, bool reversed) {
    const size_t plane_words = (size_t)(eq ? iupac_offset((int64_t)D.words3) : (int64_t)D.words3) + 8;
    u64* pl = C.scratch_p->take<u64>(plane_words);
    const int blocks = (K + 3) / 4;
    if (eq) {
        IupacPackArgs a;
        a.nseq = K; a.reverse = reversed ? 1 : 0; a.acgt_only = 0;
        a.asc = D.d_pool; a.asc_off = D.d_asc_off; a.len = D.d_len; a.planes = pl; a.pl_off = D.d_pl_off;
        hipLaunchKernelGGL(k_pack_iupac, dim3(blocks), dim3(256), 0, C.stream, a);
    } else {
        PackArgs a;
        a.nseq = K; a.reverse = reversed ? 1 : 0; a.flags = nullptr;
        a.set[0] = PackSet{D.d_pool, D.d_asc_off, D.d_len, pl, D.d_pl_off};
        a.set[1] = a.set[0];                  // (one set's blocks: never read)
        hipLaunchKernelGGL(k_pack, dim3(blocks), dim3(256), 0, C.stream, a);
        // a packed batch's texts carry the wire formats' base codes, not k_pack's
        if (B.packed) hipLaunchKernelGGL(k_panel_wire_codes, dim3((unsigned)((D.words3 / 3 + 255) / 256)), dim3(256), 0, C.stream, pl, (int64_t)(D.words3 / 3));
    }
    HIP_CHECK(hipGetLastError());
    return (const u64*)pl;
}
// what every sweep kernel reads first (PanelSweepArgs): the panel cut into slices of per_slice members over the planes pl_m, the
// texts' planes pl_t, the text slots (run_search_panel_scan puts its window slots in their place)
static void panel_sweep_args(PanelSweepArgs& a, const quicked_batch& B, const PanelDev& D, int K, int per_slice, const u64* pl_m, const u64* pl_t) {
    a.pl_m = pl_m; a.m_off = D.d_pl_off; a.m_len = D.d_len; a.m_bound = D.d_bound;
    a.n_members = K; a.per_slice = per_slice;
    a.pl_t = pl_t; a.pl_t_off = B.d_plt_off; a.t_len = B.d_t_len;
    a.nslots = (int32_t)D.nslots; a.text = D.d_text;
}
// A sweep's launch, k3 / k4 the kernel under the library's equality / a flagged run's: slot groups x slices, four groups per
// workgroup, one per SIMD of its CU, and launch_groups' claim on the CU's LDS: at most two of these workgroups share a CU,
// whichever slices they belong to
template <class A>
static void launch_panel_sweep(Context& C, int eq, void (*k3)(A), void (*k4)(A), const A& a, size_t ngroups, int nslices) {
    const dim3 grid((unsigned)((ngroups + 3) / 4), (unsigned)nslices);
    if (eq) hipLaunchKernelGGL(k4, grid, dim3(256), 54 * 1024, C.stream, a);
    else hipLaunchKernelGGL(k3, grid, dim3(256), 54 * 1024, C.stream, a);
    HIP_CHECK(hipGetLastError());
}
static PanelOut run_search_panel(quicked_batch& B, Context& C, const SearchRun& sr) {
    const PanelRun& pr = *sr.panel;
    const int K = pr.n_patterns, eq = sr.eq;
    const bool infix = sr.mode == SEARCH_INFIX;
    PanelOut O;
    const PanelDev D = panel_upload(B, C, sr);
    O.text = D.text;
    // (QUICKED_PANEL_NO_INDELS: k_panel_ham in k_search_panel's place, the reduction in its PREFIX form -- no start-pass task --
    // and text_start = text_end - m behind it)
    const bool start_pass = infix && !sr.no_indels;
    if (O.text.empty()) return O;
    const size_t n = (size_t)B.n, nslots = D.nslots;
    // ---- the forward pass
    const PanelCut cut = panel_cut(K, panel_slices(C, D.ngroups, K));
    const int nslices = cut.nslices;
    PanelArgs a{};
    const u64* pl_m = panel_planes(B, C, D, K, eq, false);
    panel_sweep_args(a, B, D, K, cut.per_slice, pl_m, panel_text_planes(B, C, eq, false));
    a.mode = sr.mode;
    a.part = C.scratch_p->take<int32_t>(6 * (size_t)nslices * nslots);
    if (pr.matrix) {
        O.d_mscore = C.scratch_p->take<int32_t>(2 * n * (size_t)K);
        O.d_mend = O.d_mscore + n * (size_t)K;
        HIP_CHECK(hipMemsetAsync(O.d_mscore, 0xFF, 2 * n * (size_t)K * sizeof(int32_t), C.stream));
        a.m_score = O.d_mscore; a.m_end = O.d_mend;
    }
    O.d_hits = C.scratch_p->take<int32_t>(6 * n);
    HIP_CHECK(hipMemsetAsync(O.d_hits, 0xFF, 6 * n * sizeof(int32_t), C.stream));
    O.d_adv = C.scratch_p->take<u32>(nslots);
    HIP_CHECK(hipMemsetAsync(O.d_adv, 0, nslots * sizeof(u32), C.stream));
    TimedLaunches tl(C, 0);
    if (sr.no_indels) launch_panel_sweep(C, eq, k_panel_ham<SearchEq3>, k_panel_ham<SearchEqIupac>, a, D.ngroups, nslices);
    else launch_panel_sweep(C, eq, k_search_panel<SearchEq3>, k_search_panel<SearchEqIupac>, a, D.ngroups, nslices);
    tl.end();
    // ---- the reduction, and the start pass's tasks
    PanelReduceArgs r{};
    r.nslots = (int32_t)nslots; r.nslices = nslices; r.infix = start_pass ? 1 : 0;
    r.text = D.d_text; r.part = a.part; r.m_len = D.d_len; r.m_off = D.d_pl_off; r.t_len = B.d_t_len;
    r.hits = O.d_hits; r.o_adv = O.d_adv;
    StartTasks st;
    if (start_pass) {
        st = take_start_tasks(C, nslots, true);
        st.into(r);
        O.d_adv2 = st.adv;
        r.o_plp_off = C.scratch_p->take<int64_t>(n);
        HIP_CHECK(hipMemsetAsync(r.o_plp_off, 0, n * sizeof(int64_t), C.stream));
    }
    hipLaunchKernelGGL(k_panel_reduce, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, C.stream, r);
    HIP_CHECK(hipGetLastError());
    if (sr.no_indels && infix) {
        hipLaunchKernelGGL(k_panel_ham_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, C.stream, (int64_t)n, D.d_len, O.d_hits);
        HIP_CHECK(hipGetLastError());
    }
    if (!start_pass) return O;
    // ---- the start pass: one lane per text over the window that ends at its best member's text_end, reversed
    if (!eq) ensure_reversed(B, C);
    PairView PV = pair_view(B, true);
    PV.pl_p = panel_planes(B, C, D, K, eq, true); PV.pl_p_off = r.o_plp_off;
    PV.pl_t = panel_text_planes(B, C, eq, true); PV.pl_t_off = B.d_plt_off;
    launch_start_pass(C, eq, PV, st);
    hipLaunchKernelGGL(k_panel_finish, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, C.stream, (int)nslots, (const int32_t*)D.d_text,
                       (const int32_t*)st.pair, (const int32_t*)st.start, O.d_hits);
    HIP_CHECK(hipGetLastError());
    return O;
}

// The alignment pass of the all-occurrences panel runs (QUICKED_PANEL_CIGARS; qe_panel_align.h), behind
// k_panel_hits_finish: k_panel_align_sizes and k_scan_offsets lay the strings' slots out from the scores (4 (2 score + 1) + 1
// bytes hold any string with `score` edits), the host reads their total, and k_panel_occ_align<Eq> runs one lane per stored
// occurrence over the run's forward planes.  A wave's history is cols x blocks x 64 cells of 16 bytes -- cols the longest
// stretch a member can have (m + its effective bound), blocks the panel's tallest member --, and the launch is cut into
// sub-batches of as many waves as QE_PANEL_ALIGN_WS_KB holds (unset: 1 GiB; never fewer than one), which reuse one history in
// stream order.  Every launch is timed as kind 1.
static void panel_align_geometry(const SearchRun& sr, int& cols, int& blocks) {
    const PanelRun& pr = *sr.panel;
    cols = 1; blocks = 1;
    for (int32_t p = 0; p < pr.n_patterns; ++p) {
        const int m = pr.len[p];
        cols = std::max(cols, m + search_effective(sr.max_dist ? sr.max_dist[p] : sr.max_dist_all, m));
        blocks = std::max(blocks, search_blocks(m));
    }
}
static size_t panel_align_wave_bytes(const SearchRun& sr) {
    int cols, blocks;
    panel_align_geometry(sr, cols, blocks);
    return (size_t)cols * (size_t)blocks * 64 * sizeof(AlignCell);
}
static size_t panel_align_waves(const SearchRun& sr, size_t waves) {
    const size_t budget = (size_t)std::max<long long>(1, sw_ll(Sw::PanelAlignWsKb)) << 10;
    return std::max<size_t>(1, std::min(waves, budget / panel_align_wave_bytes(sr)));
}
// what is fixed of it before the total is known: the history at the most occurrences the run can store
static size_t panel_align_fixed_bytes(const quicked_batch& B, const SearchRun& sr) {
    if (!sr.cigars) return 0;
    return panel_align_waves(sr, (panel_texts(B) * (size_t)sr.max_hits + 63) / 64) * panel_align_wave_bytes(sr) + 1024;
}
static void run_panel_align(quicked_batch& B, Context& C, const SearchRun& sr, const PanelDev& D, const u64* pl_m, const u64* pl_t, HitsOut& O) {
    const size_t nh = (size_t)O.total;
    O.cigars = true;
    int32_t* d_len = C.scratch_p->take<int32_t>(nh);
    int64_t* d_str_off = C.scratch_p->take<int64_t>(nh + 1);
    hipLaunchKernelGGL(k_panel_align_sizes, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, C.stream, (int64_t)nh, (const int32_t*)O.d_hits, d_len);
    hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(1024), 0, C.stream, (const int32_t*)d_len, (const int32_t*)d_len, d_str_off, d_str_off + nh, (int)nh);
    HIP_CHECK(hipGetLastError());
    {
        std::vector<int64_t> tot;
        FetchBatch fb(C);
        fb.add(tot, (const int64_t*)(d_str_off + nh), 1);
        fb.sync();
        O.cig_bytes = tot[0];
    }
    O.d_cig_pool = C.scratch_p->take<char>(((size_t)O.cig_bytes + 127) & ~(size_t)63);
    O.d_cig_off = C.scratch_p->take<int64_t>(nh);
    O.d_al_steps = C.scratch_p->take<u32>(2 * nh);
    int cols, blocks;
    panel_align_geometry(sr, cols, blocks);
    const size_t waves = (nh + 63) / 64, per = panel_align_waves(sr, waves), wave_cells = (size_t)cols * (size_t)blocks * 64;
    PanelAlignArgs a{};
    a.pl_m = pl_m; a.m_off = D.d_pl_off; a.m_len = D.d_len; a.n_members = sr.panel->n_patterns;
    a.pl_t = pl_t; a.t_off = B.d_plt_off; a.t_len = B.d_t_len;
    a.occ_off = O.d_off; a.npairs = (int32_t)B.n;
    a.hits = O.d_hits; a.total = (int64_t)nh;
    a.hist = C.scratch_p->take<AlignCell>(per * wave_cells); a.hist_cols = cols; a.hist_blocks = blocks;
    a.style = B.cigar_style;
    a.str_off = d_str_off; a.pool = O.d_cig_pool;
    a.o_off = O.d_cig_off; a.o_steps = O.d_al_steps; a.o_ops = O.d_al_steps + nh;
    for (size_t w0 = 0; w0 < waves; w0 += per) {
        a.first = (int64_t)(64 * w0); a.count = (int64_t)std::min(nh - 64 * w0, 64 * per);
        TimedLaunches tl(C, 1);
        const dim3 grid((unsigned)((a.count + 255) / 256));
        if (sr.eq) hipLaunchKernelGGL(k_panel_occ_align<SearchEqIupac>, grid, dim3(256), 0, C.stream, a);
        else hipLaunchKernelGGL(k_panel_occ_align<SearchEq3>, grid, dim3(256), 0, C.stream, a);
        HIP_CHECK(hipGetLastError());
        tl.end();
    }
}

// The tails of an all-occurrences panel run (QUICKED_PANEL_TAILS; qe_panel.h), behind k_panel_tails, which
// left one keeper per (slice, slot): k_panel_tails_merge merges them per text and writes the start-pass task of every text that
// has a tail; k_panel_tail_planes<Eq> lays the task's pattern -- the member's first `overlap` bases, reversed -- out in a
// scratch pool of one stretch per slot (the panel's tallest member and two rows of zeros); the start pass is the unchanged
// k_search<4, Eq> in its start-pass form over those planes and the texts' reversed planes, one lane per slot, timed as kind 0;
// k_panel_tails_finish adds its o_start.  Nothing here waits for the host or depends on the occurrences' total: a batch
// without a single full occurrence gets its tails all the same.  The pass's block steps are not the unflagged run's and stay
// out of counter 0.
static int panel_tallest_rows(const PanelRun& pr) {
    int nb = 1;
    for (int32_t p = 0; p < pr.n_patterns; ++p) nb = std::max(nb, search_blocks(pr.len[p]));
    return nb + 2;
}
static size_t panel_tails_fixed_bytes(const quicked_batch& B, const SearchRun& sr, size_t nslots, size_t nslices) {
    if (!sr.tails) return 0;
    const size_t n = (size_t)B.n, plane_words = (size_t)iupac_offset(3 * (int64_t)panel_tallest_rows(*sr.panel)) * nslots + 8;
    return 4 * nslices * nslots * sizeof(int32_t) + 4 * n * sizeof(int32_t) + 8 * nslots * sizeof(int32_t) + n * sizeof(int64_t) + plane_words * sizeof(u64) + 8 * 512;
}
static void run_panel_tails(quicked_batch& B, Context& C, const SearchRun& sr, const PanelDev& D, const PanelTailsArgs& ta, int nslices, const u64* pl_t_rev, HitsOut& O) {
    const size_t n = (size_t)B.n, nslots = D.nslots;
    const int eq = sr.eq;
    O.d_tails = C.scratch_p->take<int32_t>(4 * n);
    HIP_CHECK(hipMemsetAsync(O.d_tails, 0xFF, 4 * n * sizeof(int32_t), C.stream));
    O.d_tail_rows = C.scratch_p->take<u32>(nslots);
    HIP_CHECK(hipMemsetAsync(O.d_tail_rows, 0, nslots * sizeof(u32), C.stream));
    PanelTailsMergeArgs g{};
    g.nslots = (int32_t)nslots; g.nslices = nslices; g.text = D.d_text; g.tpart = ta.tpart; g.t_len = B.d_t_len;
    g.plane_stride = 3 * (int64_t)panel_tallest_rows(*sr.panel);
    g.tails = O.d_tails; g.o_rows = O.d_tail_rows;
    const StartTasks st = take_start_tasks(C, nslots, false);
    st.into(g);
    g.o_plp_off = C.scratch_p->take<int64_t>(n);
    HIP_CHECK(hipMemsetAsync(g.o_plp_off, 0, n * sizeof(int64_t), C.stream));
    const dim3 grid((unsigned)((nslots + 255) / 256));
    hipLaunchKernelGGL(k_panel_tails_merge, grid, dim3(256), 0, C.stream, g);
    PanelTailPlanesArgs w{};
    w.nslots = (int32_t)nslots; w.o_pair = g.o_pair; w.tails = O.d_tails;
    w.pl_m = ta.H.pl_m; w.m_off = D.d_pl_off; w.o_plp_off = g.o_plp_off;
    w.pool = C.scratch_p->take<u64>((size_t)(eq ? iupac_offset(g.plane_stride) : g.plane_stride) * nslots + 8);
    if (eq) hipLaunchKernelGGL(k_panel_tail_planes<SearchEqIupac>, grid, dim3(256), 0, C.stream, w);
    else hipLaunchKernelGGL(k_panel_tail_planes<SearchEq3>, grid, dim3(256), 0, C.stream, w);
    HIP_CHECK(hipGetLastError());
    PairView PV = pair_view(B, true);
    PV.pl_p = w.pool; PV.pl_p_off = g.o_plp_off;
    PV.pl_t = pl_t_rev; PV.pl_t_off = B.d_plt_off;
    launch_start_pass(C, eq, PV, st);
    hipLaunchKernelGGL(k_panel_tails_finish, grid, dim3(256), 0, C.stream, (int)nslots, (const int32_t*)st.pair, (const int32_t*)st.start, O.d_tails);
    HIP_CHECK(hipGetLastError());
}

// The heads of an all-occurrences panel run (QUICKED_PANEL_HEADS; qe_panel.h): k_panel_heads<Eq> in
// k_panel_hits' launch shape over the members' reversed planes and the texts' forward planes leaves one keeper per (slice,
// slot); k_panel_heads_merge merges them per text and writes the end-pass task of every text that has a head;
// k_panel_head_planes<Eq> lays the task's pattern -- the member's last `overlap` bases, forwards -- out in a scratch pool of one
// stretch per slot (the panel's tallest member and two rows of zeros); the end pass is the unchanged k_search<4, Eq> in its
// start-pass form over those planes and the texts' FORWARD planes, from column 0: its largest end is text_end, so it wants no
// reversed copy of the texts; k_panel_heads_finish writes it into the record.  The kernels are timed as kind 0.  Nothing here
// waits for the host, depends on the occurrences' total or reads what the occurrence kernel wrote.  The steps go to counters
// 6 and 7, never into counter 0.
static size_t panel_heads_fixed_bytes(const quicked_batch& B, const SearchRun& sr, size_t nslots, size_t nslices) {
    if (!sr.heads) return 0;
    const size_t n = (size_t)B.n, plane_words = (size_t)iupac_offset(3 * (int64_t)panel_tallest_rows(*sr.panel)) * nslots + 8;
    // (a PREFIX run packs no reversed panel planes of its own)
    const size_t rev = sr.mode == SEARCH_INFIX ? 0 : (size_t)iupac_offset((int64_t)panel_plane_words(*sr.panel) + 24) * sizeof(u64);
    return rev + 5 * nslices * nslots * sizeof(int32_t) + 4 * n * sizeof(int32_t) + 9 * nslots * sizeof(int32_t) + n * sizeof(int64_t) + plane_words * sizeof(u64) + 8 * 512;
}
static void run_panel_heads(quicked_batch& B, Context& C, const SearchRun& sr, const PanelDev& D, const PanelHitsArgs& a, int nslices, const u64* pl_m_rev, HitsOut& O) {
    const size_t n = (size_t)B.n, nslots = D.nslots;
    const int eq = sr.eq;
    PanelHeadsArgs h{a};                            // the occurrence kernel's panel, slices and slots ...
    h.pl_m = pl_m_rev;                              // ... over the members' reversed planes
    h.min_overlap = B.head_min_overlap;
    h.hpart = C.scratch_p->take<int32_t>(5 * (size_t)nslices * nslots);
    {
        TimedLaunches tl(C, 0);
        launch_panel_sweep(C, eq, k_panel_heads<SearchEq3>, k_panel_heads<SearchEqIupac>, h, D.ngroups, nslices);
        tl.end();
    }
    O.d_heads = C.scratch_p->take<int32_t>(4 * n);
    HIP_CHECK(hipMemsetAsync(O.d_heads, 0xFF, 4 * n * sizeof(int32_t), C.stream));
    O.d_head_steps = C.scratch_p->take<u32>(2 * nslots);
    HIP_CHECK(hipMemsetAsync(O.d_head_steps, 0, 2 * nslots * sizeof(u32), C.stream));
    PanelHeadsMergeArgs g{};
    g.nslots = (int32_t)nslots; g.nslices = nslices; g.text = D.d_text; g.hpart = h.hpart; g.t_len = B.d_t_len;
    g.plane_stride = 3 * (int64_t)panel_tallest_rows(*sr.panel);
    g.heads = O.d_heads; g.o_steps = O.d_head_steps; g.o_rows = O.d_head_steps + nslots;
    const StartTasks st = take_start_tasks(C, nslots, false);
    st.into(g);
    g.o_plp_off = C.scratch_p->take<int64_t>(n);
    HIP_CHECK(hipMemsetAsync(g.o_plp_off, 0, n * sizeof(int64_t), C.stream));
    const dim3 grid((unsigned)((nslots + 255) / 256));
    hipLaunchKernelGGL(k_panel_heads_merge, grid, dim3(256), 0, C.stream, g);
    PanelHeadPlanesArgs w{};
    w.nslots = (int32_t)nslots; w.o_pair = g.o_pair; w.heads = O.d_heads;
    w.pl_m = a.pl_m; w.m_off = D.d_pl_off; w.m_len = D.d_len; w.o_plp_off = g.o_plp_off;
    w.pool = C.scratch_p->take<u64>((size_t)(eq ? iupac_offset(g.plane_stride) : g.plane_stride) * nslots + 8);
    if (eq) hipLaunchKernelGGL(k_panel_head_planes<SearchEqIupac>, grid, dim3(256), 0, C.stream, w);
    else hipLaunchKernelGGL(k_panel_head_planes<SearchEq3>, grid, dim3(256), 0, C.stream, w);
    HIP_CHECK(hipGetLastError());
    PairView PV = pair_view(B, false);
    PV.pl_p = w.pool; PV.pl_p_off = g.o_plp_off;
    PV.pl_t = a.pl_t; PV.pl_t_off = B.d_plt_off;
    launch_start_pass(C, eq, PV, st);
    hipLaunchKernelGGL(k_panel_heads_finish, grid, dim3(256), 0, C.stream, (int)nslots, (const int32_t*)st.pair, (const int32_t*)st.start, O.d_heads);
    HIP_CHECK(hipGetLastError());
}

// Every occurrence of every member (quicked_batch_run_panel_all): the panel upload and pack of a panel run,
// k_panel_hits over text groups x slices -- per (slice, slot) its counts and up to max_hits raw records --, k_panel_hits_count
// (found / smallest score / stored per pair), the offset scan over the stored counts in the order of the pairs and -- the one
// thing the host reads in between -- their total, which sizes the rest: k_panel_hits_expand puts the stored occurrences in
// their places and, INFIX, writes one start-pass task per occurrence; the pass is the unchanged k_search<4, Eq> in its
// start-pass form with task j's pair = j and two arrays of `total` plane offsets (the member's into the reversed panel planes,
// the text's); k_panel_hits_finish adds its o_start.  Both passes are timed as kind 0.
// A queued run (SearchRun::queue_total) reads nothing in between: the total stays at d_off[n], the arrays it
// sizes are taken at panel_queue_cap, k_panel_queue_expand writes below that cap only, the start pass runs over cap task slots
// whose pair was preset to -1, k_panel_queue_finish takes min(total, cap) from the device and k_panel_queue_clamp clamps the
// offsets, with the total the run wanted beside them.
//
// The raw buffer is nslices x nslots x max_hits records of 12 bytes: the slice count is lowered until that fits
// QE_PANEL_HITS_RAW_KB (1 GiB unset; one slice always fits it under the 2^26 rule of the entry point).
static int panel_hits_slices(const Context& C, size_t nslots, int K, int max_hits) {
    const size_t budget = (size_t)std::max<long long>(1, sw_ll(Sw::PanelHitsRawKb)) << 10;
    const size_t per_slice_bytes = nslots * (size_t)max_hits * sizeof(PanelRawHit);
    const size_t fit = std::max<size_t>(1, budget / std::max<size_t>(1, per_slice_bytes));
    return (int)std::min<size_t>((size_t)panel_slices(C, nslots / 64, K), fit);
}
// the room a queued run takes for its records: min(max_total, non-empty texts x max_hits) -- no run stores more than the latter
static int64_t panel_queue_cap(const quicked_batch& B, const SearchRun& sr) {
    return std::min<int64_t>(sr.queue_total, (int64_t)panel_texts(B) * (int64_t)sr.max_hits);
}
// what such a run takes from its pool before the total is known (the planner's fixed needs): panel_shared_bytes, the slice
// partials and the raw buffer at the slices the host would choose, the per-pair arrays.  The arrays sized by the total (16
// bytes per stored occurrence, 60 with the start pass) are not known before the run and are not planned, as in an
// all-occurrences search run; a queued run takes them at its cap, which is known, and they are planned
static size_t panel_hits_fixed_bytes(const quicked_batch& B, const Context& C, const SearchRun& sr) {
    size_t nslots = 0, b = panel_shared_bytes(B, sr, nslots);
    const size_t n = (size_t)B.n, nslices = (size_t)panel_hits_slices(C, nslots, sr.panel->n_patterns, sr.max_hits);
    b += nslices * nslots * (4 * sizeof(int32_t) + (size_t)sr.max_hits * sizeof(PanelRawHit));
    b += nslots * 8 + n * 12 + (n + 1) * 8;
    // (a queued run takes them at its cap, which is known: panel_queue_cap)
    if (sr.queue_total > 0) b += (size_t)panel_queue_cap(B, sr) * (sr.mode == SEARCH_INFIX ? 60 : 16) + 8 * 512;
    return b + panel_align_fixed_bytes(B, sr) + panel_tails_fixed_bytes(B, sr, nslots, nslices) + panel_heads_fixed_bytes(B, sr, nslots, nslices);
}
// the reversed planes of a panel run, packed when a pass first asks for them: the panel's for the occurrences' start pass and
// the heads' sweep, the texts' for the start passes
struct PanelReversed {
    quicked_batch& B; Context& C; const PanelDev& D; int K, eq;
    const u64 *pl_m = nullptr, *pl_t = nullptr;
    const u64* members() { if (!pl_m) pl_m = panel_planes(B, C, D, K, eq, true); return pl_m; }
    const u64* texts() {
        if (!pl_t) { if (!eq) ensure_reversed(B, C); pl_t = panel_text_planes(B, C, eq, true); }
        return pl_t;
    }
};
// Behind the offsets, for both all-occurrences panel runs: the records' array at O.total (queued: O.cap) places, the run's own
// expand kernel -- expand(e), over its argument block e, whose fields both blocks have alike are filled here --, INFIX the
// start pass with one task per place and the finish step, the mismatch-only run's finish step in their stead, a queued run's
// clamp, the strings.  a: the forward pass's planes
template <class E, class Expand>
static void panel_occ_records(quicked_batch& B, Context& C, const SearchRun& sr, const PanelDev& D, const PanelSweepArgs& a, PanelReversed& R,
                              bool infix, E& e, Expand expand, HitsOut& O) {
    const bool queued = O.cap > 0;
    const size_t nh = (size_t)(queued ? O.cap : O.total);
    const int eq = sr.eq;
    O.d_hits = C.scratch_p->take<int32_t>(4 * nh);
    e.off = O.d_off; e.m_len = D.d_len; e.m_off = D.d_pl_off; e.t_len = B.d_t_len; e.t_off = B.d_plt_off; e.hits = O.d_hits;
    StartTasks st;
    if (infix) {
        st = take_start_tasks(C, nh, true);
        st.into(e);
        O.d_adv2 = st.adv;
        if (queued) HIP_CHECK(hipMemsetAsync(st.pair, 0xFF, nh * sizeof(int32_t), C.stream));      // the task slots past the total: no pair, so no lane
        e.o_plp_off = C.scratch_p->take<int64_t>(2 * nh);
        e.o_plt_off = e.o_plp_off + nh;
    }
    expand(e);
    HIP_CHECK(hipGetLastError());
    const dim3 grid((unsigned)((nh + 255) / 256));
    if (sr.no_indels && sr.mode == SEARCH_INFIX) {
        hipLaunchKernelGGL(k_panel_ham_hits_finish, grid, dim3(256), 0, C.stream, (int64_t)nh, D.d_len, O.d_hits);
        HIP_CHECK(hipGetLastError());
    }
    if (infix) {
        // ---- the start pass: one lane per stored occurrence over its window, reversed
        PairView PV = pair_view(B, true);
        PV.pl_p = R.members(); PV.pl_p_off = e.o_plp_off;
        PV.pl_t = R.texts(); PV.pl_t_off = e.o_plt_off;
        launch_start_pass(C, eq, PV, st);
        if (queued) hipLaunchKernelGGL(k_panel_queue_finish, grid, dim3(256), 0, C.stream, (const int64_t*)(O.d_off + (size_t)B.n), (int64_t)O.cap, (const int32_t*)st.start, O.d_hits);
        else hipLaunchKernelGGL(k_panel_hits_finish, grid, dim3(256), 0, C.stream, (int64_t)nh, (const int32_t*)st.start, O.d_hits);
        HIP_CHECK(hipGetLastError());
    }
    if (queued) {
        // ---- the offsets clamped to the cap, W and the real lengths of the records and their step counts beside them
        O.d_queue = C.scratch_p->take<int64_t>(4);
        hipLaunchKernelGGL(k_panel_queue_clamp, dim3((unsigned)(((size_t)B.n + 256) / 256)), dim3(256), 0, C.stream, (int64_t)B.n, (int64_t)O.cap, O.d_off, O.d_queue);
        HIP_CHECK(hipGetLastError());
    }
    if (sr.cigars) run_panel_align(B, C, sr, D, a.pl_m, a.pl_t, O);
}
static HitsOut run_search_panel_hits(quicked_batch& B, Context& C, const SearchRun& sr) {
    const PanelRun& pr = *sr.panel;
    const int K = pr.n_patterns, eq = sr.eq, max_hits = sr.max_hits;
    // (QUICKED_PANEL_NO_INDELS: k_panel_ham_hits in k_panel_hits' place, the expand step in its PREFIX form -- no start-pass task
    // -- and text_start = text_end - m behind it; never queued, never with strings, tails or heads)
    const bool infix = sr.mode == SEARCH_INFIX && !sr.no_indels;
    HitsOut O;
    const PanelDev D = panel_upload(B, C, sr);
    O.task_pair = D.text;
    if (O.task_pair.empty()) return O;
    const size_t nslots = D.nslots;
    // ---- the forward pass
    const PanelCut cut = panel_cut(K, panel_hits_slices(C, nslots, K, max_hits));
    const int nslices = cut.nslices;
    PanelHitsArgs a{};
    const u64* pl_m = panel_planes(B, C, D, K, eq, false);
    panel_sweep_args(a, B, D, K, cut.per_slice, pl_m, panel_text_planes(B, C, eq, false));
    a.mode = sr.mode; a.max_hits = max_hits;
    a.part = C.scratch_p->take<int32_t>(4 * (size_t)nslices * nslots);
    a.raw = C.scratch_p->take<PanelRawHit>((size_t)nslices * nslots * (size_t)max_hits);
    int32_t* const d_plen = hits_arrays(C, O, (size_t)B.n, nslots);
    // (QUICKED_PANEL_TAILS: k_panel_tails is k_panel_hits with the walk down the last column, and one keeper per (slice, slot) more)
    PanelTailsArgs ta{};
    if (sr.tails) { ta.H = a; ta.min_overlap = B.tail_min_overlap; ta.tpart = C.scratch_p->take<int32_t>(4 * (size_t)nslices * nslots); }
    TimedLaunches tl(C, 0);
    if (sr.tails) launch_panel_sweep(C, eq, k_panel_tails<SearchEq3>, k_panel_tails<SearchEqIupac>, ta, D.ngroups, nslices);
    else if (sr.no_indels) launch_panel_sweep(C, eq, k_panel_ham_hits<SearchEq3>, k_panel_ham_hits<SearchEqIupac>, a, D.ngroups, nslices);
    else launch_panel_sweep(C, eq, k_panel_hits<SearchEq3>, k_panel_hits<SearchEqIupac>, a, D.ngroups, nslices);
    tl.end();
    PanelReversed R{B, C, D, K, eq};
    // ---- counts per pair, offsets in the order of the pairs (a pair without a slot has -1 + 1 = 0 stored), the total
    PanelHitsCountArgs c{};
    c.nslots = (int32_t)nslots; c.nslices = nslices; c.max_hits = max_hits; c.text = D.d_text; c.part = a.part;
    c.found = O.d_found; c.best = O.d_best; c.len = d_plen; c.o_adv = O.d_adv;
    hipLaunchKernelGGL(k_panel_hits_count, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, C.stream, c);
    if (sr.tails) run_panel_tails(B, C, sr, D, ta, nslices, R.texts(), O);        // (before the total: it needs none)
    if (sr.heads) run_panel_heads(B, C, sr, D, a, nslices, R.members(), O);       // (likewise; no reversed text planes)
    // (a queued run: the total stays on the device and the arrays it sizes are taken at the run's cap instead)
    const bool queued = sr.queue_total > 0;
    if (queued) { hits_offsets(B, C, O, d_plen, B.d_t_len); O.total = -1; O.cap = panel_queue_cap(B, sr); }
    else hits_total(B, C, O, d_plen, B.d_t_len);
    if (!queued && O.total <= 0) return O;
    PanelHitsExpandArgs e{};
    e.nslots = (int32_t)nslots; e.nslices = nslices; e.max_hits = max_hits; e.infix = infix ? 1 : 0;
    e.text = D.d_text; e.part = a.part; e.raw = a.raw;
    panel_occ_records(B, C, sr, D, a, R, infix, e, [&](const PanelHitsExpandArgs& x) {
        if (queued) hipLaunchKernelGGL(k_panel_queue_expand, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, C.stream, x, (int64_t)O.cap);
        else hipLaunchKernelGGL(k_panel_hits_expand, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, C.stream, x);
    }, O);
    return O;
}

// Every occurrence of every member, long texts split across lanes (quicked_batch_run_panel_scan): the run
// above with a window slot {pair, c0, c1} per lane.  The slot table is built on the host -- the texts in the batch's length
// order, a text's windows contiguous and ascending, padded to whole waves -- and goes up in one block with the per-pair
// {first_slot, nwin}; k_panel_scan over window groups x slices leaves counts and raw records per (slice, slot);
// k_panel_scan_sums (one thread per slice and text) and k_panel_scan_count (one per text) merge the counts and leave every
// slice's rank base; k_scan_offsets and the total
// as above; k_panel_scan_expand (one thread per lane) ranks the records among their text's and writes them and their
// start-pass tasks; the start pass and k_panel_hits_finish are the run's above (panel_occ_records).
//
// The library's window (window == 0).  A multiple of 64; enough window groups that groups x slices reach about twice the
// resident wave slots with the panel cut as finely as it can be (slices cost no warm-up, windows do): groups = ceil(2 slots2
// / K) rounded down to whole workgroups of four, window = the batch's text columns / (64 groups) rounded up; never below max(1024, 8 x the longest warm-up), so that a lane's
// warm-up is at most an eighth of what it owns; then doubled until the window slots x max_hits fit 2^26 (one window per text
// does, or the entry point has refused the run).  The 1024 and the eighth rest on the sweep in profiles/panel_scan.md as
// far as it reaches; 2 slots2 is panel_slices' figure and was not swept again.
static int32_t panel_scan_window(const quicked_batch& B, const Context& C, const SearchRun& sr) {
    if (sr.window > 0) return sr.window;
    const PanelRun& pr = *sr.panel;
    int64_t columns = 0, longest = 0, warm = 64;
    for (int64_t i = 0; i < B.n; ++i) { columns += B.t_len[(size_t)i]; longest = std::max<int64_t>(longest, B.t_len[(size_t)i]); }
    // (the mismatch-only scan has no warm-up: the term stays at its floor)
    for (int32_t p = 0; p < pr.n_patterns && !sr.no_indels; ++p) warm = std::max<int64_t>(warm, panel_window_warmup(pr.len[p], sr.max_dist ? sr.max_dist[p] : sr.max_dist_all));
    const int64_t whole = std::min<int64_t>(std::max<int64_t>(64, (longest + 63) / 64 * 64), 0x7FFFFFC0);      // one window per text
    // (whole workgroups of four groups, rounded down, and the window rounded up: one group over two rounds of the chip is a third)
    const int64_t groups = std::max<int64_t>(4, (2 * (int64_t)chip(C.device).slots2() + pr.n_patterns - 1) / pr.n_patterns / 4 * 4);
    int64_t w = (columns + 64 * groups - 1) / (64 * groups);
    w = (w + 63) / 64 * 64;
    w = std::min(whole, std::max<int64_t>(w, std::max<int64_t>(1024, 8 * warm)));
    while (w < whole && panel_scan_slots(B, w) * sr.max_hits > ((int64_t)1 << 26)) w = std::min(whole, 2 * w);
    return (int32_t)w;
}
struct PanelScanTable {                            // window slot -> {pair (-1 in the padding), text slot, c0, c1}; pair -> {first_slot, nwin}
    std::vector<int32_t> w_pair, w_text, w_c0, w_c1, first_slot, nwin;
};
static void panel_scan_table(const quicked_batch& B, const std::vector<int32_t>& text, int32_t window, PanelScanTable& T) {
    T.first_slot.assign((size_t)B.n, 0); T.nwin.assign((size_t)B.n, 0);
    for (size_t t = 0; t < text.size(); ++t) {
        const int32_t pair = text[t];
        if (pair < 0) continue;
        const int64_t n = B.t_len[(size_t)pair];
        T.first_slot[(size_t)pair] = (int32_t)T.w_pair.size();
        for (int64_t c0 = 0; c0 < n; c0 += window) {
            T.w_pair.push_back(pair); T.w_text.push_back((int32_t)t);
            T.w_c0.push_back((int32_t)c0); T.w_c1.push_back((int32_t)std::min<int64_t>(n, c0 + window));
            ++T.nwin[(size_t)pair];
        }
    }
    while (T.w_pair.size() % 64) { T.w_pair.push_back(-1); T.w_text.push_back(-1); T.w_c0.push_back(0); T.w_c1.push_back(0); }
}
static int panel_scan_slices(const Context& C, size_t wslots, int K, int max_hits) { return panel_hits_slices(C, wslots, K, max_hits); }
// the planner's fixed needs: panel_shared_bytes, the slot table, the partials, rank bases and the raw buffer at the slices the
// host would choose, the per-pair arrays; what is sized by the total is not planned, as in run_search_panel_hits
static size_t panel_scan_fixed_bytes(const quicked_batch& B, const Context& C, const SearchRun& sr) {
    size_t ntext = 0, b = panel_shared_bytes(B, sr, ntext);
    const size_t n = (size_t)B.n, wslots = ((size_t)panel_scan_slots(B, panel_scan_window(B, C, sr)) + 63) / 64 * 64;
    const size_t nslices = (size_t)panel_scan_slices(C, wslots, sr.panel->n_patterns, sr.max_hits);
    b += nslices * wslots * (4 * sizeof(int32_t) + (size_t)sr.max_hits * sizeof(PanelRawHit)) + 5 * nslices * ntext * sizeof(int32_t);
    b += wslots * 16 + n * 8 + ntext * 8 + n * 12 + (n + 1) * 8 + 16 * 512;
    return b + panel_align_fixed_bytes(B, sr);
}
// (quicked_batch_run_panel_scan_no_indels, sr.no_indels; DESIGN.md 4.14.8: k_panel_ham_scan in k_panel_scan's place, the
// ranking step without start-pass tasks and text_start = text_end - m behind it; never with strings)
static HitsOut run_search_panel_scan(quicked_batch& B, Context& C, const SearchRun& sr) {
    const PanelRun& pr = *sr.panel;
    const int K = pr.n_patterns, eq = sr.eq, max_hits = sr.max_hits;
    const bool infix = !sr.no_indels;                 // (the run's mode is INFIX always: whether a start pass follows)
    HitsOut O;
    const PanelDev D = panel_upload(B, C, sr);
    O.task_pair = D.text;
    if (O.task_pair.empty()) return O;
    const size_t n = (size_t)B.n, ntext = D.nslots;
    // ---- the window slots
    PanelScanTable T;
    panel_scan_table(B, D.text, panel_scan_window(B, C, sr), T);
    const size_t nslots = T.w_pair.size();
    // one block, one copy: {w_pair | w_text | w_c0 | w_c1 | first_slot | nwin}, every array on a 16-byte boundary (the copy kernel
    // moves whole uint4 and rounds a copy's end up)
    const size_t n4 = (n + 3) & ~(size_t)3;
    static thread_local std::vector<int32_t> tab;
    tab.assign(4 * nslots + 2 * n4, 0);
    const std::vector<int32_t>* src[6] = {&T.w_pair, &T.w_text, &T.w_c0, &T.w_c1, &T.first_slot, &T.nwin};
    for (int q = 0; q < 6; ++q) memcpy(tab.data() + (q < 4 ? (size_t)q * nslots : 4 * nslots + (size_t)(q - 4) * n4), src[q]->data(), src[q]->size() * sizeof(int32_t));
    int32_t* d_tab = C.scratch_p->take<int32_t>(tab.size());
    h2d(d_tab, tab, C.stream);
    int32_t *d_w_pair = d_tab, *d_w_text = d_tab + nslots, *d_w_c0 = d_tab + 2 * nslots, *d_w_c1 = d_tab + 3 * nslots;
    int32_t *d_first = d_tab + 4 * nslots, *d_nwin = d_first + n4;
    // ---- the forward pass
    const PanelCut cut = panel_cut(K, panel_scan_slices(C, nslots, K, max_hits));
    const int nslices = cut.nslices;
    PanelScanArgs a{};
    const u64* pl_m = panel_planes(B, C, D, K, eq, false);
    panel_sweep_args(a, B, D, K, cut.per_slice, pl_m, panel_text_planes(B, C, eq, false));
    a.nslots = (int32_t)nslots; a.text = d_w_pair; a.w_c0 = d_w_c0; a.w_c1 = d_w_c1; a.max_hits = max_hits;      // window slots for text slots
    a.part = C.scratch_p->take<int32_t>(4 * (size_t)nslices * nslots);
    a.raw = C.scratch_p->take<PanelRawHit>((size_t)nslices * nslots * (size_t)max_hits);
    int32_t* const d_base = C.scratch_p->take<int32_t>((size_t)nslices * ntext);
    int32_t* const d_plen = hits_arrays(C, O, n, ntext);
    TimedLaunches tl(C, 0);
    if (sr.no_indels) launch_panel_sweep(C, eq, k_panel_ham_scan<SearchEq3>, k_panel_ham_scan<SearchEqIupac>, a, nslots / 64, nslices);
    else launch_panel_sweep(C, eq, k_panel_scan<SearchEq3>, k_panel_scan<SearchEqIupac>, a, nslots / 64, nslices);
    tl.end();
    // ---- counts per pair and rank bases per (slice, text), offsets in the order of the pairs, the total
    PanelScanCountArgs c{};
    c.ntext = (int32_t)ntext; c.nslots = (int32_t)nslots; c.nslices = nslices; c.max_hits = max_hits;
    c.text = D.d_text; c.first_slot = d_first; c.nwin = d_nwin; c.part = a.part;
    c.sums = C.scratch_p->take<int32_t>(4 * (size_t)nslices * ntext);
    c.found = O.d_found; c.best = O.d_best; c.len = d_plen; c.base = d_base; c.o_adv = O.d_adv;
    hipLaunchKernelGGL(k_panel_scan_sums, dim3((unsigned)((ntext + 255) / 256), (unsigned)nslices), dim3(256), 0, C.stream, c);
    hipLaunchKernelGGL(k_panel_scan_count, dim3((unsigned)((ntext + 255) / 256)), dim3(256), 0, C.stream, c);
    hits_total(B, C, O, d_plen, B.d_t_len);
    if (O.total <= 0) return O;
    PanelScanExpandArgs e{};
    e.ntext = (int32_t)ntext; e.nslots = (int32_t)nslots; e.nslices = nslices; e.max_hits = max_hits;
    e.w_pair = d_w_pair; e.w_text = d_w_text; e.first_slot = d_first; e.nwin = d_nwin;
    e.part = a.part; e.raw = a.raw; e.base = d_base;
    PanelReversed R{B, C, D, K, eq};
    panel_occ_records(B, C, sr, D, a, R, infix, e, [&](const PanelScanExpandArgs& x) {
        const dim3 grid((unsigned)((nslots + 255) / 256), (unsigned)nslices);
        if (infix) hipLaunchKernelGGL(k_panel_scan_expand, grid, dim3(256), 0, C.stream, x);
        else hipLaunchKernelGGL(k_panel_ham_scan_expand, grid, dim3(256), 0, C.stream, x);
    }, O);
    return O;
}

// One wave per alignment wherever the strings are more than a few runs long, else one lane per alignment.  Decided before the
// traceback runs: the wave form wants every task's runs in a stretch of their own (TraceArgs::runs_by_task).  Round 5: the
// wave form used to be kept for few alignments or very long reads; measured per read length and batch size
// (tools/probe_format_wave.sh) it is never behind -- streams of 12.5 k pairs of 10 kb 5.1 -> 5.8 M alignments/s, one such
// batch alone 9.8 -> 8.8 ms, 100 k pairs 6.7 -> 6.95 M, 100 k pairs of 3 kb 19.1 -> 21.9 M, of 300 bases 20.2 -> 21.8 M
static bool wave_formatter_wanted(const quicked_batch& B, const SegList& SL, bool want_strings) {
    const size_t nr = SL.root_pair.size(), nseg = SL.kind.size();
    size_t pool_bytes = 0;
    // QUICKED_TAG_NO_CIGAR: the run lays its runs out, and picks the tag kernels' form, as the CIGAR run of the same pairs would
    if (want_strings || (B.run_tags & QUICKED_TAG_NO_CIGAR)) for (size_t b : SL.bound) pool_bytes += b;
    const int wave_env = sw(Sw::FormatWave);      // tests force either form
    return B.cigar_style != 2 && nr > 0 && (wave_env >= 0 ? wave_env != 0 : (nseg > 0 && pool_bytes / nr >= 512));
}

// Which form of the tag kernels a stage takes: the wave form where the CIGAR formatter takes its wave form (runs laid out by
// task: 256-byte rows), else the lane form; QE_TAGS_WAVE = 0 / 1 forces one (tests).  Both read either run layout.
static std::atomic<int64_t> g_tag_launches[2];      // count passes launched, process-wide: [0] lane form, [1] wave form (tests)
int64_t tag_launches(int form) { return g_tag_launches[form ? 1 : 0].load(std::memory_order_relaxed); }
static bool tags_wave_wanted(bool format_wave) {
    const int force = sw(Sw::TagsWave);
    return force >= 0 ? force != 0 : format_wave;
}

// what format_segments takes from the pool for the tags of these roots: statistics, MD lengths and offsets, the MD pool
static size_t tag_scratch_bytes(const quicked_batch& B, const SegList& SL) {
    size_t bytes = 0;
    const size_t nr = SL.root_pair.size();
    if (B.run_tags & QUICKED_TAG_STATS) bytes += (nr + 1) * sizeof(TagStats) + 256;
    if (B.run_tags & QUICKED_TAG_MD) {
        bytes += (nr + 1) * 12 + 1024;
        for (int32_t pr : SL.root_pair) bytes += (size_t)tag_md_bound(B.p_len[(size_t)pr]);
    }
    return bytes;
}

static AlignOut format_segments(const quicked_batch& B, Context& C, const SegList& SL, const u32* runs, const int64_t* g_runs_off,
                                const int32_t* nruns, bool want_strings, bool wave = false, const int32_t* g_runs_cap = nullptr, bool runs_by_task = false) {
    AlignOut A;
    A.nroots = SL.root_pair.size();
    const size_t nr = A.nroots, nseg = SL.kind.size();
    int64_t* d_off = C.scratch_p->take<int64_t>(nr + 1);
    int32_t* d_kind = C.scratch_p->take<int32_t>(nseg + 1); int32_t* d_a = C.scratch_p->take<int32_t>(nseg + 1);
    int32_t* d_b = C.scratch_p->take<int32_t>(nseg + 1);
    int32_t* d_rootpair = C.scratch_p->take<int32_t>(nr + 1);
    {
        CopyBatch cb(C.stream);
        h2d(d_off, SL.off, C.stream); h2d(d_kind, SL.kind, C.stream); h2d(d_a, SL.a, C.stream); h2d(d_b, SL.b, C.stream);
        h2d(d_rootpair, SL.root_pair, C.stream);
    }
    A.len = C.scratch_p->take<int32_t>(nr + 1); A.edits = C.scratch_p->take<int32_t>(nr + 1); A.nops = C.scratch_p->take<int32_t>(nr + 1);
    A.str_off = C.scratch_p->take<int64_t>(nr + 1); A.total = C.scratch_p->take<int64_t>(1);
    size_t pool_bytes = 0;
    if (want_strings) for (size_t b : SL.bound) pool_bytes += b;
    A.pool = C.scratch_p->take<char>(pool_bytes + 16);
    A.pool_bytes = pool_bytes + 16;
    SegFormatArgs f;
    f.npairs = (int32_t)nr; f.seg_off = d_off; f.seg_kind = d_kind; f.seg_a = d_a; f.seg_b = d_b;
    f.runs = runs; f.g_runs_off = g_runs_off; f.nruns = nruns;
    f.g_runs_cap = g_runs_cap; f.runs_by_task = runs_by_task ? 1 : 0;
    f.o_len = A.len; f.o_edits = A.edits; f.o_nops = A.nops; f.str_off = A.str_off; f.pool = A.pool;
    f.style = B.cigar_style;
    const int blocks = (int)((nr + 63) / 64);
    if (B.check && want_strings) {
        A.ok = C.scratch_p->take<int32_t>(nr + 1);
        SegCheckArgs ck;
        ck.F = f; ck.P = pair_view(B, false); ck.root_pair = d_rootpair; ck.o_ok = A.ok;
        hipLaunchKernelGGL(k_check_segs, dim3(blocks), dim3(64), 0, C.stream, ck);
    }
    (void)nseg;
    if (wave) hipLaunchKernelGGL(k_format_segs_wave<false>, dim3((unsigned)nr), dim3(64), 0, C.stream, f);
    else hipLaunchKernelGGL(k_format_segs<false>, dim3(blocks), dim3(64), 0, C.stream, f);
    if (want_strings) {
        hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(1024), 0, C.stream, A.len, d_rootpair, A.str_off, A.total, (int)nr);
        if (wave) hipLaunchKernelGGL(k_format_segs_wave<true>, dim3((unsigned)nr), dim3(64), 0, C.stream, f);
        else hipLaunchKernelGGL(k_format_segs<true>, dim3(blocks), dim3(64), 0, C.stream, f);
    }
    const bool want_stats = (B.run_tags & QUICKED_TAG_STATS) != 0, want_md = (B.run_tags & QUICKED_TAG_MD) != 0;
    if ((want_stats || want_md) && nr > 0) {
        // alignment tags: the count pass leaves the statistics and every MD string's length, the scan its offset, the write
        // pass the strings.  The MD pool is taken before the lengths are known: tag_md_bound per root (qe_tags.h)
        SegTagArgs tg;
        tg.F = f; tg.P = pair_view(B, false); tg.root_pair = d_rootpair;
        tg.want_stats = want_stats ? 1 : 0; tg.want_md = want_md ? 1 : 0;
        tg.o_stats = nullptr; tg.o_md_len = nullptr; tg.o_md_bad = nullptr; tg.md_off = nullptr; tg.md_pool = nullptr;
        if (want_stats) tg.o_stats = A.stats = C.scratch_p->take<TagStats>(nr + 1);
        if (want_md) {
            for (int32_t pr : SL.root_pair) A.md_pool_bytes += (size_t)tag_md_bound(B.p_len[(size_t)pr]);
            tg.o_md_len = A.md_len = C.scratch_p->take<int32_t>(nr + 1);
            tg.md_off = A.md_off = C.scratch_p->take<int64_t>(nr + 1);
            A.md_total = C.scratch_p->take<int64_t>(1);
            tg.o_md_bad = A.md_bad = C.scratch_p->take<int32_t>(4);
            A.md_pool_bytes += 16;
            tg.md_pool = A.md_pool = C.scratch_p->take<char>(A.md_pool_bytes);
            HIP_CHECK(hipMemsetAsync(A.md_bad, 0, sizeof(int32_t), C.stream));
        }
        const bool tw = tags_wave_wanted(wave);
        g_tag_launches[tw ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
        if (tw) hipLaunchKernelGGL(k_tags_segs_wave<false>, dim3((unsigned)nr), dim3(64), 0, C.stream, tg);
        else hipLaunchKernelGGL(k_tags_segs<false>, dim3(blocks), dim3(64), 0, C.stream, tg);
        if (want_md) {
            hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(1024), 0, C.stream, A.md_len, d_rootpair, A.md_off, A.md_total, (int)nr);
            if (tw) hipLaunchKernelGGL(k_tags_segs_wave<true>, dim3((unsigned)nr), dim3(64), 0, C.stream, tg);
            else hipLaunchKernelGGL(k_tags_segs<true>, dim3(blocks), dim3(64), 0, C.stream, tg);
        }
    }
    return A;
}

// D2H of a formatted stage into the batch's host-side result arrays
static void fetch_alignments(quicked_batch& B, Context& C, const SegList& SL, const AlignOut& A, bool want_strings,
                             int32_t ok_status, const std::vector<int32_t>* root_status) {
    std::vector<int32_t> len, edits, nops; std::vector<int64_t> off;
    std::vector<int32_t> okv;
    std::vector<quicked_pair_stats_t> tstats; std::vector<int32_t> md_len; std::vector<int64_t> md_off;      // alignment tags
    int32_t md_bad = 0;
    const size_t nr = A.nroots;
    const bool strings = want_strings && A.pool != nullptr && A.pool_bytes > 0;
    const size_t tag_bytes = (A.stats ? ((nr * 32 + 63) & ~(size_t)63) : 0) + (A.md_len ? 2 * ((nr * 8 + 63) & ~(size_t)63) + 64 + A.md_pool_bytes + 64 : 0);
    const size_t small_bytes = 6 * (((nr * 8) + 63) & ~(size_t)63) + (strings ? A.pool_bytes + 64 : 0) + tag_bytes;
    const size_t base = B.wr->cigar_pool.size;
    const size_t md_base = B.wr->md_pool.size;
    // the MD strings of this stage: their lengths give the total (offsets are a scan of length + 1, as the CIGARs')
    auto md_total_of = [&]() {
        int64_t total = 0;
        for (size_t i = 0; i < nr; ++i) total = std::max<int64_t>(total, md_off[i] + md_len[i] + 1);
        if (md_bad || (size_t)total > A.md_pool_bytes) throw HipError{hipErrorUnknown, "MD strings beyond their pool's bound", __LINE__};
        return total;
    };
    if (small_bytes <= ((size_t)256 << 10)) {
        // few alignments (a single quicked_align call): the per-root arrays and the string pool up to its bound arrive in the
        // context's pinned block through ONE copy launch and ONE synchronisation (five copies, the strings' own round trip
        // and two synchronisations otherwise: ~0.1 ms of a call)
        uint8_t* st = C.small_pinned(small_bytes + 256);
        size_t top = 0;
        auto get = [&](const void* src, size_t bytes) { uint8_t* p = st + top; copy_kernel(p, src, bytes, C.stream); top += (bytes + 63) & ~(size_t)63; return p; };
        const uint8_t *h_len, *h_edits, *h_nops, *h_off = nullptr, *h_ok = nullptr, *h_pool = nullptr;
        const uint8_t *h_stats = nullptr, *h_mdlen = nullptr, *h_mdoff = nullptr, *h_mdbad = nullptr, *h_mdpool = nullptr;
        {
            CopyBatch cb(C.stream);
            h_len = get(A.len, nr * 4); h_edits = get(A.edits, nr * 4); h_nops = get(A.nops, nr * 4);
            if (want_strings) h_off = get(A.str_off, nr * 8);
            if (A.ok) h_ok = get(A.ok, nr * 4);
            if (strings) h_pool = get(A.pool, A.pool_bytes);
            if (A.stats) h_stats = get(A.stats, nr * 32);
            if (A.md_len) { h_mdlen = get(A.md_len, nr * 4); h_mdoff = get(A.md_off, nr * 8); h_mdbad = get(A.md_bad, 4); h_mdpool = get(A.md_pool, A.md_pool_bytes); }
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(C.stream));
        len.assign((const int32_t*)h_len, (const int32_t*)h_len + nr); edits.assign((const int32_t*)h_edits, (const int32_t*)h_edits + nr);
        nops.assign((const int32_t*)h_nops, (const int32_t*)h_nops + nr);
        if (h_off) off.assign((const int64_t*)h_off, (const int64_t*)h_off + nr);
        if (h_ok) okv.assign((const int32_t*)h_ok, (const int32_t*)h_ok + nr);
        int64_t total = 0;
        if (want_strings) for (size_t i = 0; i < nr; ++i) total = std::max<int64_t>(total, off[i] + len[i] + 1);
        if (total && h_pool) {
            if ((size_t)total > A.pool_bytes) throw HipError{hipErrorUnknown, "CIGAR strings beyond their pool's bound", __LINE__};
            B.wr->cigar_pool.reserve(base + (size_t)total);
            memcpy(B.wr->cigar_pool.p + base, h_pool, (size_t)total);
            B.wr->cigar_pool.size = base + (size_t)total;
        }
        if (h_stats) tstats.assign((const quicked_pair_stats_t*)h_stats, (const quicked_pair_stats_t*)h_stats + nr);
        if (h_mdlen) {
            md_len.assign((const int32_t*)h_mdlen, (const int32_t*)h_mdlen + nr); md_off.assign((const int64_t*)h_mdoff, (const int64_t*)h_mdoff + nr);
            md_bad = *(const int32_t*)h_mdbad;
            const int64_t md_total = md_total_of();
            if (md_total) {
                B.wr->md_pool.reserve(md_base + (size_t)md_total);
                memcpy(B.wr->md_pool.p + md_base, h_mdpool, (size_t)md_total);
                B.wr->md_pool.size = md_base + (size_t)md_total;
            }
        }
    } else {
        d2h(len, A.len, A.nroots, C.stream); d2h(edits, A.edits, A.nroots, C.stream); d2h(nops, A.nops, A.nroots, C.stream);
        if (want_strings) d2h(off, A.str_off, A.nroots, C.stream);
        if (A.ok) d2h(okv, A.ok, A.nroots, C.stream);
        std::vector<int32_t> bad1;
        if (A.stats) d2h(tstats, (const quicked_pair_stats_t*)A.stats, A.nroots, C.stream);
        if (A.md_len) { d2h(md_len, A.md_len, A.nroots, C.stream); d2h(md_off, A.md_off, A.nroots, C.stream); d2h(bad1, A.md_bad, 1, C.stream); }
        HIP_CHECK(hipStreamSynchronize(C.stream));
        if (A.md_len) {
            md_bad = bad1[0];
            const int64_t md_total = md_total_of();
            if (md_total) {
                B.wr->md_pool.reserve(md_base + (size_t)md_total);
                HIP_CHECK(hipMemcpyAsync(B.wr->md_pool.p + md_base, A.md_pool, (size_t)md_total, hipMemcpyDeviceToHost, C.stream));
                B.wr->md_pool.size = md_base + (size_t)md_total;      // (the stream is synchronised below, or with the CIGARs' copy)
            }
        }
        int64_t total = 0;
        if (want_strings) for (size_t i = 0; i < A.nroots; ++i) total = std::max<int64_t>(total, off[i] + len[i] + 1);
        if (total) {
            B.wr->cigar_pool.reserve(base + (size_t)total);
            HIP_CHECK(hipMemcpyAsync(B.wr->cigar_pool.p + base, A.pool, (size_t)total, hipMemcpyDeviceToHost, C.stream));
            HIP_CHECK(hipStreamSynchronize(C.stream));
            B.wr->cigar_pool.size = base + (size_t)total;
        } else if (A.md_len) HIP_CHECK(hipStreamSynchronize(C.stream));
    }
    for (size_t i = 0; i < A.nroots; ++i) {
        const int pr = SL.root_pair[i];
        B.wr->score[pr] = edits[i];
        B.wr->status[pr] = root_status ? (*root_status)[i] : ok_status;
        if (edits[i] < 0) { B.wr->score[pr] = -1; B.wr->status[pr] = QUICKED_ERROR; }      // run-buffer overflow: cutoff below the distance
        B.counters[4] += nops[i];
        B.note_pair(pr, 4, nops[i]);
        if (A.ok) B.wr->check_ok[pr] = okv[i];
        if (want_strings && len[i] > 0) B.wr->cigar_off[pr] = (int64_t)base + off[i];      // NUL-terminated in the pool
        if (A.stats && !B.wr->stats.empty()) B.wr->stats[pr] = tstats[i];
        if (A.md_len && !B.wr->md_off.empty()) B.wr->md_off[pr] = md_len[i] > 0 ? (int64_t)md_base + md_off[i] : -1;
    }
}

// WindowEd over a task list (bpm_windowed.c:563-628)
static void run_windowed(quicked_batch& B, Context& C, const TaskList& L, bool reversed, int W, int O_, int hew_threshold,
                         bool score_only, bool sse, StageResult* R, bool fetch, bool want_cigar, int32_t** d_score_out,
                         PendingFetch* pf = nullptr, TaskOut* dev_out = nullptr, DevTasks* dev_tasks = nullptr) {
    const size_t nt = L.pair.size();
    const int ng = L.ngroups();
    // per group: Pv/Mv [W][64] u64 + tiled history of (64W+3) columns x W blocks
    const size_t g_bytes = ((size_t)2 * W * 64 * 8 + (size_t)(8 * W + 2) * W * 512 * 16 + 255) & ~(size_t)255;
    BandLayout lay;
    lay.ws_off.resize(ng); lay.mat_off.assign(ng, 0); lay.runs_off.resize(ng);
    lay.nslots.assign(ng, W); lay.nrows.assign(ng, 0); lay.nch.assign(ng, 0); lay.runs_cap.resize(ng);
    for (int g = 0; g < ng; ++g) {
        int cap = 2;
        for (int l = 0; l < 64; ++l) {
            const size_t t = (size_t)g * 64 + l;
            if (L.pair[t] >= 0) cap = std::max(cap, L.m[t] + L.n[t] + 2);
        }
        lay.ws_off[g] = (int64_t)lay.ws_bytes; lay.ws_bytes += g_bytes;
        lay.runs_cap[g] = cap; lay.runs_off[g] = (int64_t)lay.runs_u32;
        if (!score_only) lay.runs_u32 += (size_t)cap * 64;
    }
    const DevTasks T = upload_tasks(L, C);
    const DevLayout D = upload_layout(lay, C);
    const TaskOut O = take_out(C, nt);
    WindowArgs a;
    a.P = pair_view(B, reversed); a.T = T.v;
    a.W = W; a.O = O_; a.hew_threshold = hew_threshold; a.score_only = score_only ? 1 : 0; a.sse = sse ? 1 : 0; a.reversed = reversed ? 1 : 0;
    a.ws = D.ws; a.g_ws_off = D.ws_off; a.runs = D.runs; a.g_runs_off = D.runs_off; a.g_runs_cap = D.runs_cap;
    a.o_score = O.score; a.o_hew = O.hew; a.o_nruns = O.nruns; a.o_nops = O.nops; a.o_edits = O.edits; a.o_steps = O.steps;
    // (2, 1) windows stay on chip (k_windowed); every other shape runs the checkpointed general path
    a.cp_path = sw(Sw::WindowedCp);
    if (W == 2 && O_ == 1) {
        // few waves: four lanes per alignment run the chain of full windows first (k_windowed_quad, a third of the one-lane
        // chain's latency for 1.9 x its instructions), the one-lane kernel then only has every task's clamped last windows
        // left.  Worth it while the launches in flight leave SIMDs idle; QE_WINDOWED_QUAD = 0 / 1: never / always (tests)
        const int quad = sw(Sw::WindowedQuad);
        const size_t waves = (size_t)ng * 4 * (size_t)std::max(1, fetch ? 1 : C.in_flight);
        if (score_only && (quad == 1 || (quad != 0 && waves <= chip(C.device).slots2()))) {
            a.state = C.scratch_p->take<int32_t>(5 * nt);
            launch_groups(C, k_windowed_quad, with_prio(a), nt / 16, 4, (size_t)QE_WQ_LDS_PER_WAVE, /* chain */ true);
        }
        launch_groups(C, k_windowed, a, (size_t)ng, 8, 8192, /* chain */ true);
    } else {
        // few waves: sixteen lanes per alignment (k_windowed_sys: the window's block rows as a systolic array, sixteen traceback
        // tiles rebuilt at a time); what it flags (N, non-canonical symbols) stays with the one-lane kernel.
        // QE_WINDOWED_SYS = 0 / 1: never / wherever eligible (tests)
        const int wsys = sw(Sw::WindowedSys);
        const size_t waves = (size_t)ng * 16 * (size_t)std::max(1, fetch ? 1 : C.in_flight);
        // not for W == 2 with the x86 SSE semantics (bpm_windowed.c:577: the SSE window kernel runs whenever window_size == 2
        // and force_scalar is off, whatever the overlap): k_windowed_sys computes the scalar kernel's windows, the one-lane
        // kernel's history path has the SSE boundary pattern
        if (score_only && W <= 15 && !(sse && W == 2) && a.cp_path != 0 && (wsys == 1 || (wsys != 0 && waves <= 2 * chip(C.device).slots2()))) {
            a.o_abort = C.scratch_p->take<int32_t>(nt);
            launch_groups(C, k_windowed_sys, with_prio(a), nt / 4, 4, 0, /* chain */ false, (size_t)40 * 1024);
            a.only_if = a.o_abort;
        }
        launch_groups(C, k_windowed_cp, a, (size_t)ng, 8, 8192, /* chain */ true);
    }
    if (d_score_out) *d_score_out = O.score;
    if (dev_out) *dev_out = O;
    if (dev_tasks) *dev_tasks = T;
    SegList SL; AlignOut AO;
    if (!score_only) {
        SL.off.push_back(0);
        for (size_t t = 0; t < nt; ++t) {
            if (L.pair[t] < 0) continue;
            SL.kind.push_back(0); SL.a.push_back((int32_t)t); SL.b.push_back(0);
            SL.off.push_back((int64_t)SL.kind.size());
            SL.root_pair.push_back(L.pair[t]); SL.bound.push_back(cigar_bound(L.m[t], L.n[t]));
        }
        AO = format_segments(B, C, SL, D.runs, D.runs_off, O.nruns, want_cigar, wave_formatter_wanted(B, SL, want_cigar), D.runs_cap, false);
        if (d_score_out) *d_score_out = AO.edits;
    }
    if (pf && !fetch) {
        pf->task_pair = L.pair; pf->d_score = O.score; pf->d_steps = O.steps; pf->counter_slot = 2;
        pf->kind = score_only ? 1 : 2;
        if (!score_only) { pf->SL = std::move(SL); pf->AO = AO; pf->want_strings = want_cigar; pf->ok_status = QUICKED_WIP; }
        return;
    }
    if (fetch && R) {
        { FetchBatch fb(C); fb.add(R->score, O.score, nt); fb.add(R->hew, O.hew, nt); fb.add(R->steps, O.steps, nt); fb.sync(); }
        if (!score_only) fetch_alignments(B, C, SL, AO, want_cigar, QUICKED_WIP, nullptr);
    }
}

// ---------------------------------------------------------------------------
// The align step (bpm_compute_matrix_hirschberg, bpm_hirschberg.c:33-270) over a list of
// roots = (pair, cutoff).  The recursion becomes a level-by-level work list: every level is
// one batch of forward + reverse score-only half passes and one join kernel; the leaves of
// all levels are then filled and traced back in sub-batches that fit the pool, and every
// pair's leaves are stitched into one CIGAR in text order.
// ---------------------------------------------------------------------------
// BUFFER_SIZE_16M of bpm_hirschberg.c:65; QE_SPLIT_BYTES lowers it so tests can force many split levels on small inputs
static uint64_t split_threshold() {
    return (uint64_t)sw_ll(Sw::SplitBytes);
}
static void reset_host_results(quicked_batch& B) {
    B.wr->score.assign((size_t)B.n, -1);
    B.wr->status.assign((size_t)B.n, QUICKED_EMPTY_SEQUENCE);
    B.wr->cigar_off.assign((size_t)B.n, -1);
    B.wr->cigar_pool.size = 0;
    B.wr->check_ok.assign((size_t)B.n, -1);
    // alignment tags: arrays only where this run produces them (the getters refuse the others)
    static const quicked_pair_stats_t no_stats = {-1, -1, -1, -1, -1, -1, -1, -1};
    if (B.run_tags & QUICKED_TAG_STATS) B.wr->stats.assign((size_t)B.n, no_stats); else B.wr->stats.clear();
    if (B.run_tags & QUICKED_TAG_MD) B.wr->md_off.assign((size_t)B.n, -1); else B.wr->md_off.clear();
    B.wr->md_pool.size = 0;
    using Kind = quicked_batch::SearchKind;
    if (B.search_kind == Kind::Best) { B.wr->text_start.assign((size_t)B.n, -1); B.wr->text_end.assign((size_t)B.n, -1); }
    else { B.wr->text_start.clear(); B.wr->text_end.clear(); }
    if (B.search_kind == Kind::All) { B.wr->found.assign((size_t)B.n, 0); B.wr->hit_off.assign((size_t)B.n + 1, 0); }
    else { B.wr->found.clear(); B.wr->hit_off.clear(); }
    B.wr->hits.clear();
    static const quicked_panel_hit_t no_panel_hit = {-1, -1, -1, -1, -1, -1};
    const bool panel = B.search_kind == Kind::Panel;
    if (panel) B.wr->panel_hits.assign((size_t)B.n, no_panel_hit); else B.wr->panel_hits.clear();
    B.wr->panel_members = panel ? B.panel_members : 0;
    if (panel && B.panel_matrix) { B.wr->panel_score.assign((size_t)B.n * (size_t)B.panel_members, -1); B.wr->panel_end.assign((size_t)B.n * (size_t)B.panel_members, -1); }
    else { B.wr->panel_score.clear(); B.wr->panel_end.clear(); }
    if (B.search_kind == Kind::PanelAll) { B.wr->panel_found.assign((size_t)B.n, 0); B.wr->panel_occ_off.assign((size_t)B.n + 1, 0); }
    else { B.wr->panel_found.clear(); B.wr->panel_occ_off.clear(); }
    B.wr->panel_occ.clear();
    B.wr->panel_cigars = false; B.wr->panel_cig_off.clear(); B.wr->panel_cig_pool.clear();
    B.wr->panel_tails.clear();
    B.wr->panel_heads.clear();
    B.wr->panel_queue_wanted = -1;
    B.wr->deferred_pairs = 0;
}

struct HNode { int32_t pair, p0, m, t0, n, cutoff, left, right, leaf_task; };

struct AlignStats { uint64_t fill_adv = 0, tb_steps = 0, score_adv = 0, splits = 0, leaves = 0; };

static void run_align(quicked_batch& B, Context& C, const TaskList& roots, bool fetch, bool want_cigar,
                      size_t matrix_budget, uint64_t split_bytes, int32_t ok_status, int32_t** d_score_out, AlignStats* stats,
                      PendingFetch* pf = nullptr, bool tight_runs = false, const int32_t* d_cut = nullptr, const int32_t* d_skip = nullptr) {
    double tr_last = now_ms();
    std::vector<HNode> nodes;
    std::vector<int32_t> root_node, root_status;
    for (size_t t = 0; t < roots.pair.size(); ++t) {
        if (roots.pair[t] < 0) continue;
        root_node.push_back((int32_t)nodes.size());
        root_status.push_back(ok_status);
        nodes.push_back(HNode{roots.pair[t], roots.p0[t], roots.m[t], roots.t0[t], roots.n[t], roots.cutoff[t], -1, -1, -1});
    }
    std::vector<int32_t> node_root(nodes.size());
    for (size_t i = 0; i < root_node.size(); ++i) node_root[root_node[i]] = (int32_t)i;
    // ---- split levels
    std::vector<int32_t> frontier(root_node);
    while (true) {
        std::vector<int32_t> split;
        for (int32_t id : frontier) {
            const HNode& nd = nodes[id];
            if (nd.m == 0 || nd.n == 0) continue;
            const HGeom G = host_geometry(nd.m, nd.n, nd.cutoff);
            if ((uint64_t)G.ebb * (uint64_t)nd.n * 16u > split_bytes) split.push_back(id);     // bpm_hirschberg.c:63-65
        }
        if (split.empty()) break;
        const DevicePool::Mark mark = C.scratch_p->mark();
        TaskList F, V;
        std::vector<int32_t> hm, hn1, hn2;
        for (int32_t id : split) {
            const HNode& nd = nodes[id];
            const int n1 = (nd.n + 1) / 2, n2 = nd.n - n1;                                      // bpm_hirschberg.c:68-69
            // both half passes use the FULL (m, n, cutoff) geometry and stop at their half (85-100)
            F.push(nd.pair, nd.p0, nd.m, nd.t0, nd.n, nd.cutoff, n1);
            V.push(nd.pair, B.p_len[nd.pair] - (nd.p0 + nd.m), nd.m, B.t_len[nd.pair] - (nd.t0 + nd.n), nd.n, nd.cutoff, n2);
            hm.push_back(nd.m); hn1.push_back(n1); hn2.push_back(n2);
        }
        F.pad(); V.pad();
        if (!B.have_rev[B.parity]) {
            hipStream_t cur = C.stream; C.stream = C.sw();
            launch_pack(B, C, true);
            HIP_CHECK(hipStreamSynchronize(C.sw()));
            C.stream = cur; B.have_rev[B.parity] = true;
        }
        const int Gf = coop_lanes(F);
        // forward half passes on the run's stream, reverse ones beside them on the side stream, joined before k_join
        hipStream_t main_s = C.stream, side = C.side_stream();
        if (side != main_s) { HIP_CHECK(hipEventRecord(C.ev_fork, main_s)); HIP_CHECK(hipStreamWaitEvent(side, C.ev_fork, 0)); }
        const ScoreLaunch SF = (Gf >= 2) ? launch_banded_coop(B, C, F, false, Gf, 3) : launch_banded_score(B, C, F, false, 3);
        C.stream = side;
        const ScoreLaunch SV = (Gf >= 2) ? launch_banded_coop(B, C, V, true, Gf, 3) : launch_banded_score(B, C, V, true, 3);
        C.stream = main_s;
        if (side != main_s) { HIP_CHECK(hipEventRecord(C.ev_join, side)); HIP_CHECK(hipStreamWaitEvent(main_s, C.ev_join, 0)); }
        const size_t ns = split.size();
        JoinArgs J;
        J.nnodes = (int32_t)ns;
        int32_t* dm = C.scratch_p->take<int32_t>(ns); int32_t* dn1 = C.scratch_p->take<int32_t>(ns); int32_t* dn2 = C.scratch_p->take<int32_t>(ns);
        { CopyBatch cb(C.stream); h2d(dm, hm, C.stream); h2d(dn1, hn1, C.stream); h2d(dn2, hn2, C.stream); }
        J.m = dm; J.n1 = dn1; J.n2 = dn2;
        J.Ffb = band_state(SF); J.Rfb = band_state(SV);
        J.F = (Gf >= 2) ? coop_state(SF) : J.Ffb; J.R = (Gf >= 2) ? coop_state(SV) : J.Rfb;
        J.o_best = C.scratch_p->take<int32_t>(ns); J.o_score_l = C.scratch_p->take<int32_t>(ns);
        J.o_score_r = C.scratch_p->take<int32_t>(ns); J.o_ok = C.scratch_p->take<int32_t>(ns);
        hipLaunchKernelGGL(k_join, dim3((unsigned)ns), dim3(64), 0, C.stream, J);       // one wave per node
        std::vector<int32_t> best, sl, sr, ok; std::vector<u32> advf, advv;
        d2h(best, J.o_best, ns, C.stream); d2h(sl, J.o_score_l, ns, C.stream); d2h(sr, J.o_score_r, ns, C.stream);
        d2h(ok, J.o_ok, ns, C.stream); d2h(advf, SF.O.adv, ns, C.stream); d2h(advv, SV.O.adv, ns, C.stream);
        QE_TRACE_POINT("  level: queued");
        HIP_CHECK(hipStreamSynchronize(C.stream));
        QE_TRACE_POINT("  level: half passes+join");
        C.scratch_p->release(mark);
        if (stats) { stats->score_adv += sum_u32(advf) + sum_u32(advv); stats->splits += ns; }
        for (size_t k = 0; k < ns; ++k) B.note_pair(nodes[split[k]].pair, 0, (int64_t)advf[k] + (int64_t)advv[k]);
        frontier.clear();
        for (size_t k = 0; k < ns; ++k) {
            const int32_t id = split[k];
            const HNode nd = nodes[id];
            if (!ok[k]) {                                                                       // bpm_hirschberg.c:116-122
                root_status[node_root[id]] = QUICKED_FAIL_NON_CONVERGENCE;
                nodes[id].m = 0; nodes[id].n = 0;                                               // contributes nothing
                continue;
            }
            const int n1 = (nd.n + 1) / 2;
            const int32_t l = (int32_t)nodes.size(), r = l + 1;
            nodes.push_back(HNode{nd.pair, nd.p0, best[k], nd.t0, n1, sl[k], -1, -1, -1});
            nodes.push_back(HNode{nd.pair, nd.p0 + best[k], nd.m - best[k], nd.t0 + n1, nd.n - n1, sr[k], -1, -1, -1});
            node_root.push_back(node_root[id]); node_root.push_back(node_root[id]);
            nodes[id].left = l; nodes[id].right = r;
            frontier.push_back(l); frontier.push_back(r);
        }
    }
    // ---- leaves in text order, per root
    TaskList LL;
    SegList SL;
    SL.off.push_back(0);
    std::vector<int32_t> stack;
    for (size_t i = 0; i < root_node.size(); ++i) {
        stack.clear();
        stack.push_back(root_node[i]);
        int64_t root_runs = 0; int root_segs = 0;
        while (!stack.empty()) {
            const int32_t id = stack.back(); stack.pop_back();
            HNode& nd = nodes[id];
            if (nd.left >= 0) { stack.push_back(nd.right); stack.push_back(nd.left); continue; }
            if (nd.m == 0 && nd.n == 0) continue;
            ++root_segs;
            if (nd.m == 0) { SL.kind.push_back(1); SL.a.push_back((int32_t)OP_I); SL.b.push_back(nd.n); continue; }
            if (nd.n == 0) { SL.kind.push_back(1); SL.a.push_back((int32_t)OP_D); SL.b.push_back(nd.m); continue; }
            nd.leaf_task = (int32_t)LL.pair.size();
            LL.push(nd.pair, nd.p0, nd.m, nd.t0, nd.n, nd.cutoff, nd.n);
            SL.kind.push_back(0); SL.a.push_back(nd.leaf_task); SL.b.push_back(0);
            root_runs += tight_runs ? std::min<int64_t>((int64_t)nd.m + nd.n + 2, (int64_t)2 * host_geometry(nd.m, nd.n, nd.cutoff).cutoff + 8)
                                    : (int64_t)nd.m + nd.n + 2;                                                        // band_layout's cap
        }
        SL.off.push_back((int64_t)SL.kind.size());
        const HNode& rt = nodes[root_node[i]];
        SL.root_pair.push_back(rt.pair);
        SL.bound.push_back(cigar_bound_runs(rt.m, rt.n, root_runs, root_segs));
    }
    const size_t n_leaves = LL.pair.size();
    LL.pad();
    QE_TRACE_POINT("  leaves listed");
    if (stats) stats->leaves += LL.pair.size();
    // ---- leaves: fill + traceback in sub-batches; runs and per-leaf outputs persist
    const size_t nt = LL.pair.size();
    const int ng = LL.ngroups();
    const BandLayout lay = band_layout(LL, true, true, tight_runs);
    B.last_mat_bytes = lay.mat_u4 * 16;
    // what the stage takes from the pool besides the matrices: run buffers, string pool, per-task arrays, segment lists
    size_t fixed_bytes = lay.runs_u32 * 4 + (size_t)nt * 160 + SL.kind.size() * 16 + ((size_t)4 << 20);
    if (want_cigar) for (size_t b : SL.bound) fixed_bytes += b;
    fixed_bytes += tag_scratch_bytes(B, SL);
    B.last_fixed_bytes = fixed_bytes + lay.ws_bytes;
    B.last_groups = ng;
    // partition the groups so that each sub-batch's matrices (and workspaces) fit what is left of the pool's budget
    // (matrix_budget = the pool's whole budget, plan_pools in run_batch); sub-batches are made equal so that none is a
    // sliver; offsets restart per sub-batch
    std::vector<int> sub_start{0};
    std::vector<int64_t> ws_off(ng), mat_off(ng);
    {
        const size_t room = matrix_budget > fixed_bytes + ((size_t)64 << 20) ? matrix_budget - fixed_bytes : (size_t)64 << 20;
        const size_t total = lay.mat_u4 * 16 + lay.ws_bytes;
        const size_t nsub = std::max<size_t>(1, (total + room - 1) / room);
        const size_t target = (total + nsub - 1) / nsub;                  // bytes per sub-batch when split evenly
        size_t ws = 0, mat = 0;
        for (int g = 0; g < ng; ++g) {
            const size_t gws = (size_t)((g + 1 < ng ? lay.ws_off[g + 1] : (int64_t)lay.ws_bytes) - lay.ws_off[g]);
            const size_t gmat = (size_t)((g + 1 < ng ? lay.mat_off[g + 1] : (int64_t)lay.mat_u4) - lay.mat_off[g]);
            const size_t after = (mat + gmat) * 16 + ws + gws;
            if (g > sub_start.back() && (after > room || (nsub > 1 && after > target + target / 16))) { sub_start.push_back(g); ws = 0; mat = 0; }
            ws_off[g] = (int64_t)ws; mat_off[g] = (int64_t)mat;
            ws += gws; mat += gmat;
        }
        sub_start.push_back(ng);
    }
    C.last_sub_batches = (int)sub_start.size() - 1;
    {   // what is still to be taken from the pool: per-task arrays, run buffers, strings, one sub-batch of matrices
        size_t sub_max = 0;
        for (size_t sb = 0; sb + 1 < sub_start.size(); ++sb) {
            size_t b = 0;
            for (int g = sub_start[sb]; g < sub_start[sb + 1]; ++g)
                b += (size_t)((g + 1 < ng ? lay.ws_off[g + 1] : (int64_t)lay.ws_bytes) - lay.ws_off[g]) +
                     16 * (size_t)((g + 1 < ng ? lay.mat_off[g + 1] : (int64_t)lay.mat_u4) - lay.mat_off[g]);
            sub_max = std::max(sub_max, b);
        }
        if (fixed_bytes + sub_max > ((size_t)1 << 30)) C.scratch_p->reserve(fixed_bytes + sub_max);
    }
    const DevTasks T = upload_tasks(LL, C);
    const TaskOut O = take_out(C, nt);
    if (d_cut) {
        // the roots' cutoffs are still being computed on the device (quicked_fast): the host sized everything for the
        // estimates in roots.cutoff; no root may have split or vanished, so leaf k is root k
        if (n_leaves != root_node.size() || nodes.size() != root_node.size())
            throw HipError{hipErrorInvalidValue, "device-side cutoffs need one leaf per root", __LINE__};
        apply_device_cutoffs(C, T, nt, O.nruns, d_cut, d_skip);      // a task taken out of the list has no runs (-1)
    }
    int64_t* d_ws_off = C.scratch_p->take<int64_t>(ng + 1); int64_t* d_mat_off = C.scratch_p->take<int64_t>(ng + 1);
    int64_t* d_runs_off = C.scratch_p->take<int64_t>(ng + 1);
    int32_t* d_nslots = C.scratch_p->take<int32_t>(ng + 1); int32_t* d_nrows = C.scratch_p->take<int32_t>(ng + 1);
    int32_t* d_nch = C.scratch_p->take<int32_t>(ng + 1); int32_t* d_runs_cap = C.scratch_p->take<int32_t>(ng + 1);
    {
        CopyBatch cb(C.stream);
        h2d(d_ws_off, ws_off, C.stream); h2d(d_mat_off, mat_off, C.stream); h2d(d_runs_off, lay.runs_off, C.stream);
        h2d(d_nslots, lay.nslots, C.stream); h2d(d_nrows, lay.nrows, C.stream); h2d(d_nch, lay.nch, C.stream);
        h2d(d_runs_cap, lay.runs_cap, C.stream);
    }
    u32* d_runs = C.scratch_p->take<u32>(lay.runs_u32 + 64);
    const bool wave_fmt = wave_formatter_wanted(B, SL, want_cigar);       // also the layout the traceback leaves its runs in
    // Lanes per leaf for the fill: 1 where the leaves fill the chip -- and wherever the cutoff is a tight bound of the distance
    // (QuickEd's bound, Hirschberg's exact child distances): such a band is pruned down to a few slots, its height test
    // (first + 2 < last) cannot be decided chunks ahead, and the cooperative protocol hands most leaves back to the
    // one-lane kernel (config 4's leaves: both kernels ran, 45 + 36 ms instead of 38).  A user bandwidth leaves the band
    // tall: few long BandEd alignments with CIGAR fill with G lanes each.  QE_COOP_FILL_G forces a width (tests).
    const bool fill_forced = sw_set(Sw::CoopFillG);
    int Gfill = (sw(Sw::CoopLds) == 0 || (tight_runs && !fill_forced)) ? 1 : coop_lanes(LL, fetch ? 1 : C.in_flight, true);
    // Round 4: ... except where the bound is LARGE.  A pair with large indels has a bound of thousands, its band is 40-60
    // slots tall for most of its length (the edge pruning only bites as the score nears the cutoff), and a launch of such
    // leaves is a few waves of one lane's chain each (the pairs a QuickEd run left for the host-driven flow: 25-35 ms for
    // thirteen waves).  There the leaves whose bands are tall enough for G >= 4 lanes (>= 3 G + 4 slots) fill cooperatively
    // and the others arrive flagged and stay with the one-lane kernel -- one list may hold both kinds.  Not where the
    // cutoffs are still on the device (the fast flow's chip-filling runs), and only for launches of at most 64 one-lane
    // waves: 20 k such pairs (313 waves one-lane, 3 750 cooperative) fill faster one lane each (76 against 85 ms per run),
    // the 813 pairs a 100 k-pair run leaves gain (50 -> 47 ms per batch of the mixed stream).
    // tight bounds in a launch of few waves: the systolic fill (k_banded_sys, below) -- 16 lanes per leaf for bands of <= 15
    // slots, a wave per leaf for bands of <= 63 (the bounds of pairs with large indels), the one-lane kernel for what is left.
    // QE_FILL_SYS = 0 / 1: never / wherever the bound is tight (tests)
    const int sys_env = sw(Sw::FillSys);
    const size_t in_fl = (size_t)std::max(1, fetch ? 1 : C.in_flight);
    const Chip& chp = chip(C.device);
    const bool sys_fill = Gfill < 2 && tight_runs && (sys_env == 1 || (sys_env != 0 && (size_t)ng * 16 * in_fl <= 2 * chp.slots2()));
    std::vector<int32_t> hew_init;
    if (!sys_fill && Gfill < 2 && tight_runs && !fill_forced && !d_cut && sw(Sw::CoopLds) != 0 && sw(Sw::CoopTallFill) != 0 &&
        (size_t)ng * (size_t)std::max(1, fetch ? 1 : C.in_flight) <= 64) {
        size_t live = 0;
        std::vector<int> ebb(nt, 0);
        for (size_t t = 0; t < nt; ++t) if (LL.pair[t] >= 0) { ebb[t] = host_geometry(LL.m[t], LL.n[t], LL.cutoff[t]).ebb; ++live; }
        for (int G : {16, 8, 4}) {
            size_t ok = 0;
            for (size_t t = 0; t < nt; ++t) ok += LL.pair[t] >= 0 && ebb[t] >= 3 * G + 4;
            if (ok >= 16 && ok * 4 >= live) {              // a quarter of the leaves or more: the launch's duration is theirs
                Gfill = G;
                hew_init.assign(nt, 1);
                for (size_t t = 0; t < nt; ++t) if (LL.pair[t] >= 0 && ebb[t] >= 3 * G + 4) hew_init[t] = 0;
                break;
            }
        }
    }
    int32_t* d_hew_init = nullptr;
    if (!hew_init.empty()) { d_hew_init = C.scratch_p->take<int32_t>(nt); h2d(d_hew_init, hew_init, C.stream); }
    for (size_t sb = 0; sb + 1 < sub_start.size(); ++sb) {
        const int g0 = sub_start[sb], g1 = sub_start[sb + 1];
        if (g1 <= g0) continue;
        size_t ws_bytes = 0, mat_u4 = 0;
        for (int g = g0; g < g1; ++g) {
            ws_bytes = std::max(ws_bytes, (size_t)ws_off[g] + (size_t)((g + 1 < ng ? lay.ws_off[g + 1] : (int64_t)lay.ws_bytes) - lay.ws_off[g]));
            mat_u4 = std::max(mat_u4, (size_t)mat_off[g] + (size_t)((g + 1 < ng ? lay.mat_off[g + 1] : (int64_t)lay.mat_u4) - lay.mat_off[g]));
        }
        const DevicePool::Mark mark = C.scratch_p->mark();
        uint8_t* ws = C.scratch_p->take<uint8_t>(ws_bytes + 256);
        uint4* mat = C.scratch_p->take<uint4>(mat_u4 + 16);
        const size_t o = (size_t)g0 * 64;
        BandedArgs a;
        a.P = pair_view(B, false);
        a.T = T.v;
        a.T.ntasks = (int32_t)((size_t)(g1 - g0) * 64);
        a.T.pair = T.pair + o; a.T.p0 = T.p0 + o; a.T.m = T.m + o; a.T.t0 = T.t0 + o; a.T.n = T.n + o;
        a.T.cutoff = T.cutoff + o; a.T.tfin = T.tfin + o;
        a.ws = ws; a.g_ws_off = d_ws_off + g0; a.g_nslots = d_nslots + g0; a.g_nrows = d_nrows + g0; a.g_nch = d_nch + g0;
        a.mat = mat; a.g_mat_off = d_mat_off + g0;
        a.o_score = O.score + o; a.o_first = O.first + o; a.o_last = O.last + o; a.o_posv = O.posv + o; a.o_adv = O.adv + o;
        a.o_maxrow = O.len + o;
        a.only_if = nullptr;
        TimedLaunches tl(C, 1);
        if (Gfill >= 2) {
            // few leaves: G lanes per leaf, band state on chip, the same checkpoints / carry words / band edges in the
            // traceback's layout (k_banded_coop_lds<true>); leaves it flags are refilled by the one-lane kernel
            const int NAf = 64 / Gfill;
            CoopLdsArgs x;
            memset(&x, 0, sizeof(x));
            x.A.P = a.P; x.A.T = a.T; x.A.G = Gfill;
            x.A.o_score = a.o_score; x.A.o_first = a.o_first; x.A.o_last = a.o_last; x.A.o_posv = a.o_posv; x.A.o_adv = a.o_adv;
            x.A.o_maxrow = a.o_maxrow; x.A.o_abort = O.hew + o;
            x.lgG = 0; while ((1 << x.lgG) < Gfill) ++x.lgG;
            x.ns = 3; for (int g = g0; g < g1; ++g) x.ns = std::max(x.ns, lay.nslots[g]);
            x.rr = x.ns + Gfill + 4;
            x.cr = std::max(16, 4 * Gfill);
            x.lds_per_wave = (int32_t)coop_lds_bytes(x.ns, Gfill);
            x.mat = mat; x.g_mat_off = a.g_mat_off; x.gws = ws; x.g_ws_off = a.g_ws_off;
            x.g_nslots = a.g_nslots; x.g_nrows = a.g_nrows; x.g_nch = a.g_nch;
            if ((size_t)x.lds_per_wave <= (size_t)38 * 1024) {
                if (d_hew_init) copy_kernel(O.hew + o, d_hew_init + o, (size_t)(g1 - g0) * 64 * sizeof(int32_t), C.stream);
                else HIP_CHECK(hipMemsetAsync(O.hew + o, 0, (size_t)(g1 - g0) * 64 * sizeof(int32_t), C.stream));
                launch_groups(C, k_banded_coop_lds<true>, x, (size_t)(g1 - g0) * 64 / NAf, 8, (size_t)x.lds_per_wave);
                a.only_if = O.hew + o;
            }
        }
        // the cooperative kernels need few registers and no LDS: four workgroups per CU (40 KB each), so that a launch of up
        // to 4 096 waves is resident at once instead of running in two rounds of 2 048 (12.5 k leaves x 16 lanes = 3 125 waves)
        const size_t sys_pin = (size_t)40 * 1024;
        if (sys_fill && a.only_if == nullptr) {
            int maxns = 0;
            for (int g = g0; g < g1; ++g) maxns = std::max(maxns, (int)lay.nslots[g]);
            a.o_abort = O.hew + o;
            launch_groups(C, k_banded_sys<4, true>, with_prio(a), (size_t)(g1 - g0) * 16, 4, 0, false, sys_pin);
            a.only_if = O.hew + o;
            // what it flagged for its height: one wave per leaf while the sub-batch is small enough for that
            if (maxns > 15 && (sys_env == 1 || (size_t)(g1 - g0) * 64 * in_fl <= 2 * chp.slots2())) {
                launch_groups(C, k_banded_sys<6, true>, with_prio(a), (size_t)(g1 - g0) * 64, 4, 0, false, sys_pin);
                // ... and what THAT flagged for its height (64 .. 127 slots): two rows per lane, two sweeps per chunk
                if (maxns > 63) launch_groups(C, k_banded_sys2<true>, with_prio(a), (size_t)(g1 - g0) * 64, 4, 0, false, sys_pin);
            }
        }
        a.fill_multi = sw(Sw::FillMulti);
        a.lane_rel = sw(Sw::LaneRel);
        launch_groups(C, k_banded<true>, a, (size_t)(g1 - g0), 8, 0);     // everything, or what the cooperative fill flagged
        tl.end();
        TraceArgs tr;
        tr.P = a.P; tr.T = a.T;
        tr.ws = ws; tr.g_ws_off = a.g_ws_off; tr.g_nslots = a.g_nslots; tr.g_nrows = a.g_nrows; tr.g_nch = a.g_nch;
        tr.mat = mat; tr.g_mat_off = a.g_mat_off;
        tr.runs = d_runs; tr.g_runs_off = d_runs_off + g0; tr.g_runs_cap = d_runs_cap + g0;
        tr.o_nruns = O.nruns + o; tr.o_nops = O.nops + o; tr.o_edits = O.edits + o; tr.o_steps = O.steps + o;
        tr.runs_by_task = wave_fmt ? 1 : 0;
        // a launch of few waves: sixteen lanes per leaf rebuild the tiles along the path's diagonal together and hand the
        // walk from tile to tile (k_traceback_sys); what it flags (N, non-canonical symbols) stays with the one-lane kernel.
        // QE_TRACE_SYS = 0 / 1: never / always (tests)
        // lanes per leaf: 16 while the launch is one round of waves (two per SIMD at 246 VGPRs: ~8 k leaves), 8 up to ~3 300
        // waves (the walk runs in all lanes of a group at once in both: one batch of 12.5 k leaves alone 8.1 ms with 8 lanes,
        // 8.6 with 16, 10.3 with the tile-by-tile walk of the round's first half), 4 up to ~1 700 waves
        const int tsys = sw(Sw::TraceSys);
        const size_t gw = (size_t)(g1 - g0) * (size_t)std::max(1, fetch ? 1 : C.in_flight);      // one-lane waves in flight
        int tlg = 0;
        if (tsys > 1) tlg = tsys == 4 ? 2 : (tsys == 8 ? 3 : 4);
        // (2 100 / 3 300 / 1 700 waves on the 1 024 SIMDs of an MI355X: one round at two waves per SIMD, 1.6 rounds, 0.8)
        else if (tsys != 0) tlg = (gw * 16 <= chp.frac2(1.03) || tsys == 1) ? 4 : (gw * 8 <= chp.frac2(1.61) ? 3 : (gw * 4 <= chp.frac2(0.83) ? 2 : 0));
        if (tlg) {
            tr.o_abort = C.scratch_p->take<int32_t>((size_t)(g1 - g0) * 64);
            const size_t nwv = (size_t)(g1 - g0) << tlg;
            if (tlg == 4) launch_groups(C, k_traceback_sys<4>, with_prio(tr), nwv, 4, 0, false, sys_pin);
            else if (tlg == 3) launch_groups(C, k_traceback_sys<3>, with_prio(tr), nwv, 4, 0, false, sys_pin);
            else launch_groups(C, k_traceback_sys<2>, with_prio(tr), nwv, 4, 0, false, sys_pin);
            tr.only_if = tr.o_abort;
        }
        launch_groups(C, k_traceback, tr, (size_t)(g1 - g0), 8, 0);
        // the next sub-batch reuses this scratch: its kernels are behind this sub-batch's in the stream, no host wait
        if (sb + 2 < sub_start.size()) C.scratch_p->release(mark);
    }
    QE_TRACE_POINT("  fill+traceback queued");
    const AlignOut AO = format_segments(B, C, SL, d_runs, d_runs_off, O.nruns, want_cigar, wave_fmt, d_runs_cap, wave_fmt);
    QE_TRACE_POINT("  format queued");
    if (d_score_out) *d_score_out = AO.edits;
    if (pf && !fetch) {
        pf->kind = 2; pf->SL = std::move(SL); pf->AO = AO; pf->want_strings = want_cigar;
        pf->ok_status = (quicked_status_t)ok_status; pf->root_status = std::move(root_status);
        pf->leaf_pair = LL.pair; pf->d_leaf_adv = O.adv; pf->d_leaf_steps = O.steps;
        return;
    }
    if (fetch) {
        if (stats) {
            std::vector<u32> adv, steps;
            { FetchBatch fb(C); fb.add(adv, O.adv, nt); fb.add(steps, O.steps, nt); fb.sync(); }
            for (size_t t = 0; t < nt; ++t) if (LL.pair[t] >= 0) { stats->fill_adv += adv[t]; stats->tb_steps += steps[t]; B.note_pair(LL.pair[t], 1, adv[t]); B.note_pair(LL.pair[t], 3, steps[t]); }
        }
        fetch_alignments(B, C, SL, AO, want_cigar, ok_status, &root_status);
    }
}

}  // namespace qe
