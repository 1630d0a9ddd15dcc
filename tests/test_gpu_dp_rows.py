"""The throughput DP's row loop on long paths with repeated nodes: a lane goes from
one 32-row block with rows straight to the next (mark_match_rows' block mask), so
the cases put matched rows in scattered blocks, dilations across block edges, and
batches of at least 2 048 paths (the big-batch launches)."""
import importlib.util
import os
import random

import numpy as np
import pytest

import oracle
import verdict_model
from gfalign_amd.scorer import GFAL_STEP_OTHER, Scorer
from helpers import csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worklist_stats():
    spec = importlib.util.spec_from_file_location("dp_worklist_stats",
                                                  os.path.join(ROOT, "scripts", "dp_worklist_stats.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def overhang_batch(seed, n_paths=2048, n_nodes=80):
    """Paths: prefixes of one 1000-step walk on few nodes (every node repeats many
    times), a few with GFAL_STEP_OTHER steps.  Alignments: m = 1..16 pieces that
    end (or, reversed, start) with a prefix of the walk -- overhang pairs in one or
    both orientations -- and plain subwalks."""
    rnd = random.Random(seed)
    walk = [(rnd.randrange(n_nodes) << 1) | rnd.randrange(2) for _ in range(1000)]
    alns = []
    for m in range(1, 17):
        for _ in range(12):
            ov = rnd.randint(1, max(1, m - 1))
            s = rnd.randrange(0, 1000 - m)
            a = walk[s:s + m - ov] + walk[:ov]
            alns.append(a[:m])
            alns.append([x ^ 1 for x in reversed(a[:m])])
            # both orientations flagged: a palindromic tail around the prefix
            alns.append([walk[0] ^ 1] + walk[:m - 1] if m > 1 else [walk[0]])
        alns.append(walk[rnd.randrange(0, 1000 - m):][:m])
    # n = m for every m, the block edges, the longest paths
    lens = list(range(1, 17)) + [1000, 999, 512, 513, 33, 32, 31]
    lens += [rnd.randint(1, 1000) for _ in range(n_paths - len(lens))]
    paths = []
    for n in lens:
        p = list(walk[:n])
        if rnd.random() < 0.05 and n > 2:
            p[rnd.randrange(1, n)] = GFAL_STEP_OTHER | (p[rnd.randrange(n)] & ~1)
        paths.append(p)
    return alns, paths


@pytest.mark.parametrize("limit", ["0", "4000000000"])
def test_big_batch_both_families(gpu, monkeypatch, limit):
    alns, paths = overhang_batch(11)
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    monkeypatch.setenv("GFAL_DP_SYS_LIMIT", limit)
    exp = [oracle.fast_evaluate_paths(aoff, ast, poff, pst, flt) for flt in (True, False)]
    with Scorer(aoff, ast, 80) as sc, Scorer(aoff, ast, 80, dedup=True) as dd:
        for flt, e in zip((True, False), exp):
            for s in (sc, dd):
                got = s.evaluate_paths(poff, pst, flt)
                for g, x in zip(got, e):
                    assert np.array_equal(g, x)
        assert sc.info()["dp_pairs"] > 10000


def test_big_batch_verdicts(gpu, monkeypatch):
    alns, paths = overhang_batch(12)
    paths = paths[:2048]
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    monkeypatch.setenv("GFAL_DP_SYS_LIMIT", "0")
    with Scorer(aoff, ast, 80) as sc:
        got = sc.verdicts(poff, pst, True)
    sel = list(range(0, 2048, 97))           # the model runs a full DP per pair: a sample of paths
    sub_off, sub_st = csr([paths[p] for p in sel])
    exp = verdict_model.verdicts(aoff, ast, sub_off, sub_st, True)
    assert np.array_equal(got[:, sel], exp)


def sparse_batch(seed, n_paths=2048, n_nodes=400):
    """Paths that start at many offsets of a walk, so each has only a few overhang
    pairs: the waves of the sorted worklist span many paths."""
    rnd = random.Random(seed)
    walk = [(rnd.randrange(n_nodes) << 1) | rnd.randrange(2) for _ in range(1200)]
    alns = []
    for _ in range(600):
        m = rnd.randint(2, 16)
        s0 = rnd.randrange(0, 150)
        ov = rnd.randint(1, m - 1)
        a = walk[s0 + 200:s0 + 200 + m - ov] + walk[s0:s0 + ov]
        alns.append(a if rnd.random() < 0.5 else [x ^ 1 for x in reversed(a)])
    paths = []
    for _ in range(n_paths):
        s0 = rnd.randrange(0, 150)
        paths.append(walk[s0:s0 + rnd.randint(16, 1000)])
    return alns, paths


def tup(xs):
    return [tuple(x) for x in xs]


def test_batches_cover_the_cases(gpu):
    """What the batches hold, from the CPU model of the worklist (in the device's
    sort order): pairs with both orientations flagged and n = m for every m that
    can reach the DP (overhang_batch), waves over more than 4 paths (sparse_batch)."""
    ws = worklist_stats()
    alns, paths = overhang_batch(11, n_paths=64)
    wl = ws.worklist(tup(paths), tup(alns))
    assert any(fw and rc for _, _, fw, rc in wl)
    assert {len(alns[k]) for p, k, _, _ in wl if len(paths[p]) == len(alns[k])} >= set(range(2, 17))
    alns, paths = sparse_batch(14)
    out = ws.stats(tup(paths), tup(alns))
    assert max(w for r in out["classes"].values() for w in r["paths_per_wave"]) > 4


@pytest.mark.parametrize("limit", ["0", "4000000000"])
def test_big_sparse_batch(gpu, monkeypatch, limit):
    alns, paths = sparse_batch(14)
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    monkeypatch.setenv("GFAL_DP_SYS_LIMIT", limit)
    exp = oracle.fast_evaluate_paths(aoff, ast, poff, pst, True)
    with Scorer(aoff, ast, 400) as sc:
        got = sc.evaluate_paths(poff, pst, True)
        assert sc.info()["dp_pairs"] > 2048
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)


def test_big_batch_worklist_overflow(gpu, monkeypatch):
    """More pairs than the worklist holds: the throughput kernels return at once on
    the overflowed pass, the call grows the list and runs the batch again."""
    alns, paths = overhang_batch(13)
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    exp = oracle.fast_evaluate_paths(aoff, ast, poff, pst, True)
    monkeypatch.setenv("GFAL_DP_SYS_LIMIT", "0")
    monkeypatch.setenv("GFAL_DEBUG_WL_CAPACITY", "1")      # capacity = max(n_aln, 1)
    with Scorer(aoff, ast, 80) as sc:
        got = sc.evaluate_paths(poff, pst, True)
        info = sc.info()
        assert info["dp_pairs"] > len(alns) and info["n_overflow_reruns"] == 1
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)
