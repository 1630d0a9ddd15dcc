"""CPU: evalPath's printed alignment as op codes (gfal_scorer_pair_alignment_ops'
encoding), derived from the oracle's traceback rows, renders the same row text
and the same score as the rows themselves -- the contract the device ops and
the CLI's default rendering are held to on the GPU."""
import random

import numpy as np

from align_ops import (STEP_OTHER, align, b_row_from_ops, b_row_from_rows, ops_from_rows,
                       pair_alignments, reverse_complement, unpack, winner)
from helpers import load_appendix_c, parse_gaf_path, parse_path_string


def name(i):
    return "n%d" % i if i % 3 else "node_%d" % i    # headers of two widths


def check_pair(a, b):
    fw, rc, ob, (score, ra, rb) = winner(a, b)
    assert score == max(fw, rc)
    ops = ops_from_rows(ra, rb)
    assert ops.count(0) + ops.count(1) + ops.count(2) == len(a)
    assert ops.count(0) + ops.count(1) + ops.count(3) == len(b)
    text, got = b_row_from_ops(a, ob, ops, name)
    assert text == b_row_from_rows(ra, rb, name)
    assert got == score
    return fw, rc


def random_steps(rnd, n, n_nodes, other=0.0):
    out = []
    for _ in range(n):
        s = (rnd.randrange(n_nodes) << 1) | rnd.randrange(2)
        if rnd.random() < other:
            s = STEP_OTHER | (s & ~1)
        out.append(unpack(s))
    return out


def test_random_pairs_render_identically():
    rnd = random.Random(11)
    ties = 0
    for t in range(1500):
        n = rnd.randint(1, 40)
        m = rnd.randint(0, 60) if t % 3 else rnd.randint(n, n + 30)   # m > n on a third
        a = random_steps(rnd, n, 6, other=0.15 if t % 2 else 0.0)
        if rnd.random() < 0.5 and m:                                  # overlapping content
            b = [a[(k + rnd.randrange(3)) % n] for k in range(m)]
            b = b if rnd.random() < 0.5 else reverse_complement(b)
            b = [(i, "+" if o == "0" else o) for i, o in b]          # alignment steps are +/-
        else:
            b = random_steps(rnd, m, 6)
        fw, rc = check_pair(a, b)
        ties += fw == rc
    assert ties > 100


def test_zero_step_alignment_is_n_up_moves():
    a = [(0, "+"), (1, "-"), (2, "0")]
    score, ra, rb = align(a, [])
    assert score == 0 and ops_from_rows(ra, rb) == [2, 2, 2]
    fw, rc, ops_off, ops = pair_alignments([0, 0], [], [0, 3, STEP_OTHER | 4])
    assert (fw[0], rc[0]) == (0, 0) and ops.tolist() == [2, 2, 2] and ops_off.tolist() == [0, 3]


def test_tie_goes_to_rc():
    # B == its own reverse complement's mirror: fw == rc, rc's orientation is printed
    a = [(0, "+"), (1, "+")]
    b = [(0, "+"), (0, "-")]
    fw, rc, ob, _ = winner(a, b)
    assert fw == rc and ob == reverse_complement(b)


def test_maximum_size_pairs():
    rnd = random.Random(5)
    walk = random_steps(rnd, 1000, 300)
    walk = [(i, "+" if o == "0" else o) for i, o in walk]
    for b in (walk, reverse_complement(walk), walk[1:], walk[:500] + [(walk[500][0], "-")] + walk[501:],
              random_steps(rnd, 1000, 300)):
        check_pair(walk, b)


def test_appendix_c2_rows_from_ops():
    gold = load_appendix_c()
    ids = gold["node_ids"]
    header = {v: k for k, v in ids.items()}
    ev = gold["eval_path"]
    path = parse_path_string(ev["path"], ids)
    alns = [parse_gaf_path(t, ids) for t in gold["alignments"]]
    off = np.zeros(len(alns) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in alns])
    fw, rc, ops_off, ops = pair_alignments(off, np.concatenate(alns).astype(np.int32), path)
    a = [unpack(s) for s in path]
    rows = []
    for k, aln in enumerate(alns):
        b = [unpack(s) for s in aln]
        ob = b if fw[k] > rc[k] else reverse_complement(b)
        text, score = b_row_from_ops(a, ob, ops[ops_off[k]:ops_off[k + 1]].tolist(), header.get)
        assert score == max(fw[k], rc[k]) == ev["best_scores"][k]
        rows.append(text)
    assert rows == [line.split("\t")[0] for line in ev["stdout"][1:5]]


def test_scores_are_the_oracles_pair_scores():
    """Every path of the committed kernel cases, long and short ones in turn: the
    helper's scores are oracle.pair_scores' (a fresh table per path, as the
    reference zeroes it once per evaluatePath)."""
    import json
    import os

    import oracle
    from helpers import GOLDEN
    with open(os.path.join(GOLDEN, "kernel_cases.json")) as f:
        cases = json.load(f)
    for c in cases:
        off = c["path_off"]
        for q in range(len(off) - 1):
            path = c["path_steps"][off[q]:off[q + 1]]
            fw, rc, ops_off, ops = pair_alignments(np.asarray(c["aln_off"]), np.asarray(c["aln_steps"]), path)
            efw, erc = oracle.pair_scores(c["aln_off"], c["aln_steps"], path)
            assert np.array_equal(fw, efw) and np.array_equal(rc, erc), (c["name"], q)
            assert len(ops) == ops_off[-1]
