"""Test-side model of the per-alignment verdicts (gfal_scorer_verdicts): what
src/eval.cpp:80-98 decides for every (alignment, path) pair, built from the
oracle's traceback scores alone.

    unaligned (2)  filter on and a node of the alignment is not on the path
    bad (1)        otherwise, max(fw, rc) < 0
    good (0)       otherwise
"""
import numpy as np

import oracle

GFAL_STEP_OTHER = 0x40000000
GOOD, BAD, UNALIGNED = 0, 1, 2


def path_nodes(steps):
    return np.unique((np.asarray(steps, np.int64) & ~GFAL_STEP_OTHER) >> 1)


def verdicts(aln_off, aln_steps, path_off, path_steps, filter):
    """uint8[n_aln, n_paths]."""
    aln_off, aln_steps = np.asarray(aln_off, np.int64), np.asarray(aln_steps, np.int64)
    path_off, path_steps = np.asarray(path_off, np.int64), np.asarray(path_steps, np.int64)
    n, P = len(aln_off) - 1, len(path_off) - 1
    owner = np.repeat(np.arange(n), np.diff(aln_off))
    codes = np.zeros((n, P), np.uint8)
    for p in range(P):
        steps = path_steps[path_off[p]:path_off[p + 1]]
        fw, rc = oracle.pair_scores(aln_off, aln_steps, steps)
        col = np.where(np.maximum(fw, rc) < 0, BAD, GOOD).astype(np.uint8)
        if filter:
            off_path = ~np.isin(aln_steps >> 1, path_nodes(steps))
            missing = np.bincount(owner[off_path], minlength=n) > 0
            col[missing] = UNALIGNED
        codes[:, p] = col
    return codes


def column_sums(codes):
    """(bad, good, unaligned alignments) per path.  bad and good are gfal_scorer_score's
    counters; its `unaligned` (src/eval.cpp:86) counts the off-path steps instead."""
    return tuple((codes == c).sum(axis=0).astype(np.uint32) for c in (BAD, GOOD, UNALIGNED))


def discordance(codes, weight=None):
    """d[i, j] = alignments good for path i and bad for path j."""
    g = (codes == GOOD).astype(np.int64)
    b = (codes == BAD).astype(np.int64)
    if weight is not None:
        g = g * np.asarray(weight, np.int64)[:, None]
    return (g.T @ b).astype(np.uint32)


def parse_path_line(line):
    """What `gfalign comparePaths -P` takes from a line: the path text, or None for a
    line it skips (blank, '#...', the search's step-cap notice)."""
    line = line.rstrip("\r\n")
    if not line or line.startswith("#") or line.startswith("Reached maximum number of steps"):
        return None
    return line.rsplit("\t", 1)[-1]
