"""Masked multi-slot passes of k_banded<false> on the CPU: tests/native/pass_plan_cpu.cpp walks groups of 64
pairs in library order with the pass plan the kernel uses (qe_types.h: pass_plan), computes every pass slot by slot with
the oracle's block step -- dead slots on zeros, scores by the backward rule -- and compares every pair's score, first /
last / pos_v and block advances with the oracle's own pass.  Run on the inputs of tests/test_gpu_masked_passes.py and on
256 pairs of the headline at the full cutoff, half of it and ten slots; `pytest -s` prints the passes per chunk."""
import os
import shutil

import pytest

import masked_lib as ML


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    return ML.build_walk(str(tmp_path_factory.mktemp("pass_plan")))


def launch_files(tmp_path, name):
    pairs, env, _, launches = ML.case(name)
    out = []
    for k, launch in enumerate(launches):
        path = os.path.join(str(tmp_path), f"{name}_{k}.bin")
        ML.write_launch(path, pairs, launch)
        out.append(path)
    return out, int(env.get("QE_LANE_REL", "1"))


@pytest.mark.parametrize("name", list(ML.CASES))
def test_gpu_cases_walk_to_the_oracles_results(exe, tmp_path, name):
    files, lane_rel = launch_files(tmp_path, name)
    for path in files:
        partial = {}
        for masked in (0, 1):
            counts, code, out = ML.walk(exe, path, lane_rel, masked)
            print(name, os.path.basename(path), out.strip())
            assert code == 0 and counts["diffs"] == 0 and counts["rule_diffs"] == 0, out[-2000:]
            partial[masked] = counts["partial_passes"]
        assert partial[0] == 0
        # the GPU test of this case cannot pass by never masking: lanes with 0 < nl < K take part in passes of every launch --
        # except in the first launch of a fitted run of these reads, whose bands are three slots in every lane of every wave
        # (the fit gives a group one slot count, and no band edge moves in a band that low): that is asserted instead
        if name in ML.UNIFORM_FIRST and path == files[0]:
            assert partial[1] == 0, (name, partial)
        else:
            assert partial[1] > 0, (name, partial)


def test_union_walk_refuses_dead_slots_on_top(exe, tmp_path):
    """QE_LANE_REL = 0 on bands that have drifted apart: the masked rule takes fewer multi-slot passes than the lane-relative
    walk of the same pairs (a lane whose band starts inside a pass sends the wave to the single-slot form), never a wrong one"""
    files, _ = launch_files(tmp_path, "indels_union_walk")
    union, _, _ = ML.walk(exe, files[0], 0, 1)
    rel, _, _ = ML.walk(exe, files[0], 1, 1)
    assert union["diffs"] == 0 and rel["diffs"] == 0
    assert union["passes1"] > rel["passes1"]


@pytest.mark.parametrize("cutoff", [1500, 750, 576])
def test_headline_pairs(exe, tmp_path, cutoff):
    pairs, launches = ML.headline_launches()
    path = os.path.join(str(tmp_path), f"headline_{cutoff}.bin")
    ML.write_launch(path, pairs, launches[cutoff])
    seen = {}
    for masked in (0, 1):
        counts, code, out = ML.walk(exe, path, 1, masked)
        print("headline", cutoff, out.strip())
        assert code == 0 and counts["diffs"] == 0 and counts["rule_diffs"] == 0, out[-2000:]
        seen[masked] = counts
    # masking turns single-slot passes into multi-slot ones and never adds a pass
    total = lambda c: c["passes4"] + c["passes2"] + c["passes1"]
    assert seen[1]["passes1"] < seen[0]["passes1"] and total(seen[1]) < total(seen[0])
    assert seen[1]["partial_passes"] > 0


def test_walk_under_sanitizers(tmp_path):
    """the program is host code with its own main: built once with ASan + UBSan and run on the two smallest cases"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the walk for the host")
    exe = ML.build_walk(str(tmp_path), sanitize=True)
    for name in ("last_row", "ragged_symbols"):
        files, lane_rel = launch_files(tmp_path, name)
        for masked in (0, 1):
            counts, code, out = ML.walk(exe, files[0], lane_rel, masked)
            assert code == 0 and counts["diffs"] == 0, out[-4000:]
            assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
