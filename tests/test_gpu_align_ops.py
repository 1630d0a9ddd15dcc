"""GPU: evalPath's printed alignment from the device (gfal_scorer_pair_alignment_
lengths / _ops, Scorer.pair_alignments) equals the oracle's traceback op for op."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import align_ops
from gfalign_amd import synth
from gfalign_amd.scorer import GFAL_STEP_OTHER, Scorer, ScorerError
from helpers import GOLDEN, csr, walk_case

pytestmark = pytest.mark.gpu


def expect(aoff, ast, path):
    return align_ops.pair_alignments(np.asarray(aoff), np.asarray(ast), path)


def same(got, exp):
    for g, e, what in zip(got, exp, ("fw", "rc", "ops_off", "ops")):
        assert np.array_equal(np.asarray(g), np.asarray(e)), what


def check(alns, path, n_nodes, **kw):
    aoff, ast = csr(alns)
    exp = expect(aoff, ast, path)
    with Scorer(aoff, ast, n_nodes, **kw) as sc:
        got = sc.pair_alignments(path)
        same(got, exp)
        fw, rc = sc.pair_scores(path)          # the scores are pair_scores'
        assert np.array_equal(fw, exp[0]) and np.array_equal(rc, exp[1])
    return exp


def test_committed_kernel_cases(gpu):
    with open(os.path.join(GOLDEN, "kernel_cases.json")) as f:
        cases = json.load(f)
    for c in cases:
        off = c["path_off"]
        for q in range(min(3, len(off) - 1)):
            path = c["path_steps"][off[q]:off[q + 1]]
            exp = expect(c["aln_off"], c["aln_steps"], path)
            with Scorer(c["aln_off"], c["aln_steps"], c["n_nodes"]) as sc:
                same(sc.pair_alignments(path), exp)
            if q == 0:
                assert exp[0].tolist() == c["pair_scores_path0"]["fw"]


def test_config2_sample(gpu):
    t = synth.make("config2")
    rng = np.random.default_rng(4)
    pick = np.sort(rng.choice(t.N, 4000, replace=False))
    alns = [t.aln_steps[t.aln_off[k]:t.aln_off[k + 1]].tolist() for k in pick]
    for q in (0, 1):
        check(alns, t.path_steps[t.path_off[q]:t.path_off[q + 1]].tolist(), t.V)


@pytest.mark.parametrize("scratch_mb", [None, "1", "40"])
def test_maximum_sizes(gpu, scratch_mb, monkeypatch):
    """n = m = 1000: the move scratch of long alignments in HBM, at the default
    budget and at budgets of one and of two waves in flight."""
    if scratch_mb:
        monkeypatch.setenv("GFAL_TRACE_SCRATCH_MB", scratch_mb)
    rnd = random.Random(7)
    walk = [(rnd.randrange(300) << 1) | rnd.randrange(2) for _ in range(1000)]
    alns = [walk, [s ^ 1 for s in reversed(walk)], walk[1:], walk[:999],
            walk[:500] + [walk[500] ^ 1] + walk[501:], [walk[-1]] + walk[:-1]]
    alns += [walk[s:s + rnd.randint(1, 30)] for s in (rnd.randrange(0, 970) for _ in range(120))]
    alns += [[(rnd.randrange(300) << 1) | rnd.randrange(2) for _ in range(1000)] for _ in range(3)]
    for path in (walk, walk[:2]):
        check(alns, path, 300)


def test_zero_step_alignments_and_other_steps(gpu):
    O = GFAL_STEP_OTHER
    alns = [[], [0], [1], [0, 2], [2, 0], [3, 1], [], [4], [0, 2, 4], [4, 2, 0, 2, 4, 6, 8]]
    for path in ([O | 0, 2], [0, O | 2, 4], [O | 0], [O | 4, 2, 0], [0, 2, O | 4], [6, 4, 2, 0]):
        exp = check(alns, path, 8)
        assert exp[3][exp[2][0]:exp[2][1]].tolist() == [2] * len(path)
    check([[], [], []], [0, 2], 4)          # a shard of zero-step alignments only


def test_dedup_scorer(gpu):
    rnd = random.Random(31)
    alns, paths = walk_case(rnd, 20, 150, 600, 2, 25)
    alns += [list(a) for a in alns[:200]] + [[]] * 5
    rnd.shuffle(alns)
    for path in paths:
        check(alns, path, 40, dedup=True)


@pytest.mark.parametrize("n_shards", [2, 3])
@pytest.mark.parametrize("dedup", [False, True])
def test_shards_fill_one_result(gpu, n_shards, dedup):
    rnd = random.Random(52 + n_shards)
    alns, paths = walk_case(rnd, 30, 200, 900, 2, 40)
    alns[5] = []
    alns[77] = []
    alns += [list(a) for a in alns[:100]]
    aoff, ast = csr(alns)
    exp = expect(aoff, ast, paths[0])
    res = None
    for k in range(n_shards):
        with Scorer(aoff, ast, 64, shard=(k, n_shards), dedup=dedup) as sc:
            res = sc.pair_alignments(paths[0], out=res)
    same(res, exp)


def test_sub_ranges(gpu):
    """[k0, k1) ranges that cut items apart, written straight into one buffer."""
    rnd = random.Random(9)
    alns, paths = walk_case(rnd, 25, 300, 1000, 1, 60)
    aoff, ast = csr(alns)
    fw, rc, ops_off, ops = expect(aoff, ast, paths[0])
    with Scorer(aoff, ast, 50) as sc:
        _, _, ops_len = sc.pair_alignment_lengths(paths[0])
        assert np.array_equal(ops_len, np.diff(ops_off))
        got = np.full(len(ops), 99, np.uint8)
        cuts = sorted({0, len(alns)} | {rnd.randrange(len(alns)) for _ in range(12)})
        for k0, k1 in zip(cuts, cuts[1:]):
            sc.pair_alignment_ops(paths[0], ops_off, got, k0, k1)
        assert np.array_equal(got, ops)
        # one range alone writes its own slots only
        part = np.full(len(ops), 99, np.uint8)
        sc.pair_alignment_ops(paths[0], ops_off, part, 100, 357)
        lo, hi = ops_off[100], ops_off[357]
        assert np.array_equal(part[lo:hi], ops[lo:hi])
        assert (part[:lo] == 99).all() and (part[hi:] == 99).all()


def test_argument_checks(gpu):
    alns = [[0, 2], [2, 4, 6], []]
    aoff, ast = csr(alns)
    with Scorer(aoff, ast, 8) as sc:
        path = [0, 2, 4]
        _, _, ops_off, ops = sc.pair_alignments(path)
        bad_off = ops_off.copy()
        bad_off[1:] += 1                            # alignment 0 given one op too many
        with pytest.raises(ScorerError) as e:
            sc.pair_alignment_ops(path, bad_off, np.zeros(len(ops) + 1, np.uint8))
        assert e.value.code == -1
        lib, p3 = sc._lib, np.asarray(path, np.int32)
        pp = p3.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        po = ops_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        pb = ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        assert lib.gfal_scorer_pair_alignment_ops(sc._h, None, 3, 0, 1, po, pb) == -1
        assert lib.gfal_scorer_pair_alignment_ops(sc._h, pp, 3, 0, 4, po, pb) == -1    # k1 > n_aln
        assert lib.gfal_scorer_pair_alignment_ops(sc._h, pp, 3, 2, 1, po, pb) == -1    # k1 < k0
        assert lib.gfal_scorer_pair_alignment_ops(sc._h, pp, 3, 0, 1, None, pb) == -1
        assert lib.gfal_scorer_pair_alignment_ops(sc._h, pp, 3, 1, 1, None, None) == 0  # empty range
        assert lib.gfal_scorer_pair_alignment_lengths(sc._h, pp, 3, None, None, None) == -1
        for p in ([], [8 << 1], [0] * 1001, [-1]):
            with pytest.raises(ScorerError) as e:
                sc.pair_alignment_lengths(p)
            assert e.value.code == -2
