"""scripts/dp_worklist_stats.py on the smoke seed: its worklist is the set of pairs
the decision rule sends to the DP, and its row counts are the kernel model's."""
import importlib.util
import os

import pytest

import kernel_model
from gfalign_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mod():
    spec = importlib.util.spec_from_file_location("dp_worklist_stats",
                                                  os.path.join(ROOT, "scripts", "dp_worklist_stats.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def case(mod):
    t = synth.make("smoke")
    return mod.split(t.path_off, t.path_steps), mod.split(t.aln_off, t.aln_steps)


def brute_worklist(paths, alns):
    out = []
    for p, A in enumerate(paths):
        nodes = {s >> 1 for s in A}
        for k, B in enumerate(alns):
            n, m = len(A), len(B)
            if m == 0 or m > n or any((s >> 1) not in nodes for s in B):
                continue
            R = kernel_model.rc(list(B))
            if any(list(A[i:i + m]) in (list(B), R) for i in range(n - m + 1)):
                continue
            fw, rc = kernel_model.has_overhang(list(A), list(B)), kernel_model.has_overhang(list(A), R)
            if fw or rc:
                out.append((p, k, fw, rc))
    return out


def test_worklist_is_the_decision_rule(mod, case):
    paths, alns = case
    got = mod.worklist(paths, alns)
    assert got == brute_worklist(paths, alns)
    assert len(got) > 20


def test_rows_are_the_kernel_models(mod, case):
    paths, alns = case
    for p, k, fw, rc in mod.worklist(paths, alns):
        A, B = paths[p], alns[k]
        occ = mod.occurrences(A)
        rows = mod.rows_of(A, B, occ)
        for Bo in ([list(B)] if fw else []) + ([kernel_model.rc(list(B))] if rc else []):
            score, n_rows = kernel_model.traceback_score_skip(list(A), Bo)
            assert len(rows) == n_rows
            assert score == kernel_model.traceback_score(list(A), Bo)
        every, masked = mod.loop_turns(A, B, occ, rows)
        assert len(rows) < masked <= every


def test_wave_figures_are_consistent(mod, case):
    paths, alns = case
    out = mod.stats(paths, alns)
    assert out["pairs"] == len(mod.worklist(paths, alns))
    assert sum(r["entries"] for r in out["classes"].values()) == out["pairs"]
    for r in out["classes"].values():
        assert r["waves"] == (r["entries"] + 63) // 64
        assert r["max_lane"] <= r["wave_union"] <= r["run_union"]
        assert r["turns_mask"] <= r["turns_all"]
        assert sum(r["paths_per_wave"].values()) == r["waves"]
