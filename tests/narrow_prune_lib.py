"""The pruning threshold of a fitted first pass (QE_NARROW_PRUNE), modelled: narrow_fit_lib's run with the
first pass of every lane that has a threshold below its cutoff walked by tests/native/narrow_prune_cpu.cpp -- the oracle's
own pass cannot prune below the cutoff its geometry is made from.  What the CPU tests and the GPU tests of the threshold
compare with.  Test infrastructure only."""
import os
import re
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import narrow_fit_lib as FL
import narrow_lib as NL
import native_build


def prune_of(m, n, cutoff, c1, qp):
    """qe_types.h: narrow_prune -- the threshold of a lane whose first pass runs at c1"""
    if qp <= 0 or c1 == cutoff or c1 == NL.narrow_cutoff(m, n, cutoff):
        return c1
    if NL.slots(m, n, c1) <= 3:                            # no band edge moves in three slots
        return c1
    return min(FL.rhat(qp, cutoff), c1)


def accepts_pruned(m, n, c1, cutoff, p, r):
    return NL.accepts(m, n, c1, cutoff, r) and r <= p


def policy_qp(ring):
    """qe_stages.hip: narrow_prune_q over the ratios a class's last runs reported (0: not reported)"""
    seen = [v for v in ring[-16:] if v > 0]
    return 2 * max(seen) - min(seen) if len(seen) >= 2 else 0


def write_launch(path, pairs, launch):
    """launch = [(pair index, c1, p, C)] in the order of the task list"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(launch)))
        for i, c1, p, c in launch:
            pt, tx = pairs[i]
            f.write(struct.pack("<iiiii", len(pt), len(tx), c1, p, c) + pt + tx)


def build_walk(out_dir, sanitize=False):
    return native_build.build_walk("narrow_prune_cpu", out_dir, sanitize)


def walk(exe, path, lane_rel=1, masked=1):
    """-> the program's counts, its lines per pair as [(score, adv, accepted)], its exit code and the rest of its output"""
    r = subprocess.run([exe, path, str(lane_rel), str(masked)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    per_pair, rest = {}, []
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "pair":
            per_pair[int(w[1])] = (int(w[3]), int(w[5]), int(w[7]))
        else:
            rest.append(line)
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)(?= |$)", rest[0])} if rest else {}
    return counts, [per_pair[k] for k in sorted(per_pair)], r.returncode, "\n".join(rest) + r.stderr


def walk_many(exe, tmp_dir, pairs, launch, name="launch", lane_rel=1, masked=1, groups_per_file=32):
    """the walk over a long launch, split at group borders into files walked in parallel -> per-pair lines, summed counts"""
    step = 64 * groups_per_file
    parts = [launch[k:k + step] for k in range(0, len(launch), step)]

    def one(a):
        k, part = a
        path = os.path.join(tmp_dir, f"{name}_{k}.bin")
        write_launch(path, pairs, part)
        counts, rows, code, out = walk(exe, path, lane_rel, masked)
        os.remove(path)
        assert code == 0 and len(rows) == len(part), out[-3000:]
        return counts, rows

    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        res = list(ex.map(one, enumerate(parts)))
    total = {}
    for counts, _ in res:
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    return [r for _, rows in res for r in rows], total


def prune_model(pairs, q, qp, exe, tmp_dir, bandwidth=15, cutoffs=None, memo=None, name="model"):
    """narrow_fit_lib.fit_model's run with the threshold of the ratio qp on the lanes that took the fit -> the same records
    (plus prune = the lane's threshold), and the walk's counts over the lanes that have one below their cutoff"""
    fit = FL.fit_model(pairs, q, bandwidth=bandwidth, cutoffs=cutoffs, memo=memo)
    if cutoffs is None:
        cutoffs = [NL.max_cutoff(len(p), len(t), bandwidth) for p, t in pairs]
    out = [dict(r, prune=r["cut1"]) for r in fit]
    launch = []
    for i in NL.library_order(pairs):
        m, n = len(pairs[i][0]), len(pairs[i][1])
        p = prune_of(m, n, cutoffs[i], fit[i]["cut1"], qp)
        out[i]["prune"] = p
        if p < fit[i]["cut1"]:
            launch.append((i, fit[i]["cut1"], p, cutoffs[i]))
    counts = {}
    if launch:
        rows, counts = walk_many(exe, tmp_dir, pairs, launch, name=name)
        assert counts["diffs"] == 0 and counts["rule_diffs"] == 0, counts
        for (i, c1, p, c), (s1, a1, ok) in zip(launch, rows):
            m, n = len(pairs[i][0]), len(pairs[i][1])
            r = out[i]
            assert ok == accepts_pruned(m, n, c1, c, p, s1)
            rt = FL.ratio(m, n, c, s1 if ok else r["score"])
            r.update(score1=s1, adv1=a1, miss=not ok, fit_miss=(not ok) and rt >= 0, adv2p=a1 + (0 if ok else r["adv"]), ratio=rt)
    return out, counts


def native_rule(tmp_dir):
    """qe_types.h's narrow_prune / narrow_accepts_pruned compiled for the host"""
    return native_build.host_lib(tmp_dir, "narrow_prune_rule",
                                 'extern "C" int np_prune(int m, int n, int c, int c1, int qp) { return qe::narrow_prune(m, n, c, c1, qp); }\n'
                                 'extern "C" int np_accepts(int m, int n, int c1, int c, int p, int r) { return qe::narrow_accepts_pruned(m, n, c1, c, p, r) ? 1 : 0; }\n')
