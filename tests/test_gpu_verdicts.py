"""GPU: gfal_scorer_verdicts / gfal_scorer_discordance (Scorer.verdicts /
Scorer.discordance) against the test-side model (tests/verdict_model.py), the
counters of gfal_scorer_score, and each other."""
import ctypes
import random

import numpy as np
import pytest

import verdict_model
from gfalign_amd import synth
from gfalign_amd.scorer import GFAL_STEP_OTHER as O, Scorer, ScorerError
from helpers import csr, random_case, walk_case

pytestmark = pytest.mark.gpu


def check(alns, paths, n_nodes, flt, **kw):
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    exp = verdict_model.verdicts(aoff, ast, poff, pst, flt)
    with Scorer(aoff, ast, n_nodes, **kw) as sc:
        got = sc.verdicts(poff, pst, flt)
        assert np.array_equal(got, exp)
        d = sc.discordance(poff, pst, flt)
        assert np.array_equal(d, verdict_model.discordance(exp))
        bad, good, _ = sc.evaluate_paths(poff, pst, flt)
        b2, g2, _ = verdict_model.column_sums(got)
        assert np.array_equal(bad, b2) and np.array_equal(good, g2)
    return exp


@pytest.mark.parametrize("flt", [True, False])
def test_random_cases(gpu, flt):
    rnd = random.Random(11)
    alns, paths = random_case(rnd, 6, 700, 20, 8, 14)
    check(alns, paths, 6, flt)
    alns, paths = walk_case(rnd, 30, 400, 3000, 40, 70)      # long alignments: k_dp_long
    check(alns + [[], []], paths, 30, flt)


@pytest.mark.parametrize("flt", [True, False])
def test_other_steps_and_zero_step_alignments(gpu, flt):
    alns = [[], [0], [1], [0, 2], [2, 0], [3, 1], [], [4], [0, 2, 4], [4, 2, 0, 2, 4, 6, 8]]
    paths = [[O | 0, 2], [0, O | 2, 4], [O | 0], [O | 4, 2, 0], [0, 2, O | 4], [6, 4, 2, 0]]
    exp = check(alns, paths, 8, flt)
    assert (exp[0] == 0).all() and (exp[6] == 0).all()
    check([[], [], []], paths, 8, flt)                       # zero-step alignments only


def test_maximum_sizes(gpu):
    rnd = random.Random(7)
    walk = [(rnd.randrange(300) << 1) | rnd.randrange(2) for _ in range(1000)]
    alns = [walk, [s ^ 1 for s in reversed(walk)], walk[1:], walk[:999],
            walk[:500] + [walk[500] ^ 1] + walk[501:], [walk[-1]] + walk[:-1]]
    alns += [walk[s:s + rnd.randint(1, 30)] for s in (rnd.randrange(0, 970) for _ in range(120))]
    for flt in (True, False):
        check(alns, [walk, walk[:2], walk[3:]], 300, flt)


def test_config2_sample(gpu):
    t = synth.make("config2")
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(t.N, 4000, replace=False))
    alns = [t.aln_steps[t.aln_off[k]:t.aln_off[k + 1]].tolist() for k in pick]
    paths = [t.path_steps[t.path_off[q]:t.path_off[q + 1]].tolist() for q in range(8)]
    for flt in (True, False):
        check(alns, paths, t.V, flt)


def test_million_alignments_in_slabs(gpu, monkeypatch):
    """>= 1 M alignments x 64 paths: codes and matrix with a scratch budget of several
    slabs equal the ones of one slab; the column sums equal the counters of
    gfal_scorer_score (k_scan3 there, k_scan here); a sample of rows equals the model."""
    t = synth.make("config3")
    P = 64
    poff = t.path_off[:P + 1].copy()
    pst = t.path_steps[:poff[-1]].copy()
    with Scorer(t.aln_off, t.aln_steps, t.V) as sc:
        n_items = (sc.info()["n_lanes"] + 63) // 64
        one = sc.verdicts(poff, pst, True)
        d_one = sc.discordance(poff, pst, True)
        # verdicts: 2 P * 8 + 64 P + 256 bytes per item; discordance: 2 P * 8
        mb_v = max(1, (n_items * (16 * P + 64 * P + 256)) >> 20) // 5
        mb_d = max(1, (n_items * 16 * P) >> 20) // 5
        assert mb_v >= 1 and mb_d >= 1
        monkeypatch.setenv("GFAL_VERDICT_SCRATCH_MB", str(mb_v))
        assert np.array_equal(sc.verdicts(poff, pst, True), one)
        monkeypatch.setenv("GFAL_VERDICT_SCRATCH_MB", str(mb_d))
        assert np.array_equal(sc.discordance(poff, pst, True), d_one)
        bad, good, _ = sc.evaluate_paths(poff, pst, True)
    assert t.N >= 1_000_000
    b2, g2, _ = verdict_model.column_sums(one)
    assert np.array_equal(bad, b2) and np.array_equal(good, g2)
    assert np.array_equal(d_one, verdict_model.discordance(one))
    pick = np.sort(np.random.default_rng(3).choice(t.N, 3000, replace=False))
    sub = [t.aln_steps[t.aln_off[k]:t.aln_off[k + 1]] for k in pick]
    soff, sst = csr(sub)
    assert np.array_equal(one[pick], verdict_model.verdicts(soff, sst, poff, pst, True))


def test_sub_ranges(gpu):
    rnd = random.Random(9)
    alns, paths = walk_case(rnd, 25, 300, 1500, 6, 60)
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    with Scorer(aoff, ast, 50) as sc:
        full = sc.verdicts(poff, pst, True)
        cuts = sorted({0, len(alns)} | {rnd.randrange(len(alns)) for _ in range(10)})
        parts = [sc.verdicts(poff, pst, True, k0, k1) for k0, k1 in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts), full)
        assert sc.verdicts(poff, pst, True, 17, 17).shape == (0, len(paths))


@pytest.mark.parametrize("flt", [True, False])
def test_dedup_scorer(gpu, flt):
    rnd = random.Random(31)
    alns, paths = walk_case(rnd, 20, 150, 600, 9, 25)
    alns += [list(a) for a in alns[:200]] + [list(a) for a in alns[:50]] * 7 + [[]] * 5
    rnd.shuffle(alns)
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    with Scorer(aoff, ast, 40) as plain, Scorer(aoff, ast, 40, dedup=True) as dd:
        assert dd.info()["n_lanes"] < plain.info()["n_lanes"]
        codes = plain.verdicts(poff, pst, flt)
        assert np.array_equal(dd.verdicts(poff, pst, flt), codes)
        assert np.array_equal(dd.discordance(poff, pst, flt), plain.discordance(poff, pst, flt))
    assert np.array_equal(codes, verdict_model.verdicts(aoff, ast, poff, pst, flt))


@pytest.mark.parametrize("n_shards", [2, 3])
@pytest.mark.parametrize("dedup", [False, True])
def test_shards(gpu, n_shards, dedup):
    rnd = random.Random(52 + n_shards)
    alns, paths = walk_case(rnd, 30, 200, 900, 7, 40)
    alns[5] = []
    alns[77] = []
    alns += [list(a) for a in alns[:100]]
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    with Scorer(aoff, ast, 64) as sc:
        full, d_full = sc.verdicts(poff, pst, True), sc.discordance(poff, pst, True)
    sentinel = 7
    res = np.full(full.shape, sentinel, np.uint8)
    d_sum = np.zeros_like(d_full)
    written = np.zeros(len(alns), np.int32)
    for k in range(n_shards):
        with Scorer(aoff, ast, 64, shard=(k, n_shards), dedup=dedup) as sc:
            mine = sc.verdicts(poff, pst, True, out=np.full(full.shape, sentinel, np.uint8))
            rows = (mine != sentinel).all(axis=1)
            assert ((mine == sentinel).all(axis=1) | rows).all()
            written += rows
            res[rows] = mine[rows]
            d_sum += sc.discordance(poff, pst, True)
    assert (written == 1).all()                   # disjoint, and together every alignment
    assert np.array_equal(res, full)
    assert np.array_equal(d_sum, d_full)


def test_discordance_identity_without_filter(gpu):
    rnd = random.Random(13)
    alns, paths = walk_case(rnd, 20, 200, 2000, 70, 40)      # 70 paths: two tiles of k_discord
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    with Scorer(aoff, ast, 40) as sc:
        d = sc.discordance(poff, pst, False).astype(np.int64)
        _, good, _ = sc.evaluate_paths(poff, pst, False)
    good = good.astype(np.int64)
    assert np.array_equal(d - d.T, good[:, None] - good[None, :])
    assert (np.diag(d) == 0).all()


def test_argument_checks(gpu):
    aoff, ast = csr([[0, 2], [2, 4, 6], []])
    poff, pst = csr([[0, 2, 4], [2]])
    with Scorer(aoff, ast, 8) as sc:
        lib = sc._lib
        po = poff.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        ps = pst.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        codes = np.zeros(3 * 2, np.uint8)
        pc = codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        d = np.zeros(4, np.uint32)
        pd = d.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        assert lib.gfal_scorer_verdicts(sc._h, po, ps, 2, 1, 0, 3, pc) == 0
        assert lib.gfal_scorer_verdicts(None, po, ps, 2, 1, 0, 3, pc) == -1
        assert lib.gfal_scorer_verdicts(sc._h, None, ps, 2, 1, 0, 3, pc) == -1
        assert lib.gfal_scorer_verdicts(sc._h, po, ps, -1, 1, 0, 3, pc) == -1
        assert lib.gfal_scorer_verdicts(sc._h, po, ps, 2, 1, -1, 3, pc) == -1     # k0 < 0
        assert lib.gfal_scorer_verdicts(sc._h, po, ps, 2, 1, 0, 4, pc) == -1      # k1 > n_aln
        assert lib.gfal_scorer_verdicts(sc._h, po, ps, 2, 1, 2, 1, pc) == -1      # k0 > k1
        assert lib.gfal_scorer_verdicts(sc._h, po, ps, 2, 1, 0, 3, None) == -1
        assert lib.gfal_scorer_verdicts(sc._h, po, ps, 2, 1, 1, 1, None) == 0     # empty range
        assert lib.gfal_scorer_discordance(sc._h, po, ps, 2, 1, pd) == 0
        assert lib.gfal_scorer_discordance(sc._h, po, ps, 2, 1, None) == -1
        assert lib.gfal_scorer_discordance(None, po, ps, 2, 1, pd) == -1
        for bad_paths in ([[]], [[8 << 1]], [[0] * 1001], [[-1]]):
            boff, bst = csr(bad_paths)
            for call in (lambda: sc.verdicts(boff, bst), lambda: sc.discordance(boff, bst)):
                with pytest.raises(ScorerError) as e:
                    call()
                assert e.value.code == -2
        many_off, many_st = csr([[0, 2]] * 4097)
        with pytest.raises(ScorerError) as e:
            sc.discordance(many_off, many_st)
        assert e.value.code == -1
        assert sc.discordance(many_off[:4097], many_st[:4096 * 2]).shape == (4096, 4096)


def test_discordance_in_slabs_with_equal_length_paths(gpu, monkeypatch):
    """256 paths of one length: the length sort places them with atomics from several
    waves, and every slab's pass sorts them again.  With slabs of 1 MB (16 k lanes) the
    matrix of a plain and of a dedup scorer must still equal the model's."""
    rnd = random.Random(5)
    walk = [(rnd.randrange(60) << 1) | rnd.randrange(2) for _ in range(6000)]
    alns = []
    for _ in range(50_000):
        m = rnd.randint(1, 10)
        s0 = rnd.randrange(0, 6000 - m)
        b = walk[s0:s0 + m]
        if rnd.random() < 0.2:
            b[rnd.randrange(m)] = (rnd.randrange(60) << 1) | rnd.randrange(2)
        if rnd.random() < 0.5:
            b = [x ^ 1 for x in reversed(b)]
        alns.append(b)
    alns += [list(alns[rnd.randrange(len(alns))]) for _ in range(10_000)] + [[]] * 3
    paths = [walk[s:s + 24] for s in range(0, 256 * 7, 7)]
    assert len(paths) == 256 and {len(p) for p in paths} == {24}
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    exp = verdict_model.verdicts(aoff, ast, poff, pst, True)
    d_exp = verdict_model.discordance(exp)
    assert d_exp.sum() > 0
    monkeypatch.setenv("GFAL_VERDICT_SCRATCH_MB", "1")       # 4 KB per item at 256 paths: 256 items a slab
    for dedup in (False, True):
        with Scorer(aoff, ast, 120, dedup=dedup) as sc:
            assert (sc.info()["n_lanes"] + 63) // 64 > 2 * 256    # at least three slabs
            for _ in range(2):
                assert np.array_equal(sc.discordance(poff, pst, True), d_exp)
            assert np.array_equal(sc.verdicts(poff, pst, True), exp)
            d0 = sc.discordance(poff, pst, False).astype(np.int64)
            _, good, _ = sc.evaluate_paths(poff, pst, False)
        good = good.astype(np.int64)
        assert np.array_equal(d0 - d0.T, good[:, None] - good[None, :])
