"""The printed alignment of evalPath as op codes, derived from the CPU oracle.

gfal_scorer_pair_alignment_ops returns the traceback of the winning orientation
as one op per column (0 diagonal with equal steps, 1 diagonal with different
ones, 2 up, 3 left).  Here the same codes come from the rows of the oracle's
own traceback (gfo_align_paths, a literal restatement of reference
src/alignments.cpp:499-554), and the evalPath row text is rendered both from
those rows (the way include/alignments.h:113-121 does) and from ops alone (the
way the CLI does by default), so the tests can hold all three against each other.
"""
import ctypes

import numpy as np

import oracle

STEP_OTHER = 0x40000000


class GfoStep(ctypes.Structure):
    _fields_ = [("id", ctypes.c_int32), ("orient", ctypes.c_char)]


_lib = None
_dp = None
_dirty_n = 0   # row 0 of the table holds -j up to this column (see align)


def _oracle():
    global _lib, _dp
    if _lib is None:
        L = oracle.lib()
        sp = ctypes.POINTER(GfoStep)
        L.gfo_align_paths.restype = ctypes.c_int32
        L.gfo_align_paths.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, sp, ctypes.c_uint32,
                                      sp, ctypes.c_uint32, ctypes.c_void_p, sp, sp,
                                      ctypes.POINTER(ctypes.c_uint32)]
        L.gfo_dp_new.restype = ctypes.c_void_p
        L.gfo_dp_zero.argtypes = [ctypes.c_void_p]
        _dp = L.gfo_dp_new()
        _lib = L
    return _lib


def unpack(s):
    """packed step -> (id, orientation char)"""
    s = int(s)
    if s & STEP_OTHER:
        return ((s & ~STEP_OTHER) >> 1, "0")
    return (s >> 1, "-" if s & 1 else "+")


def reverse_complement(steps):
    """include/alignments.h:64-70 on (id, orient) tuples."""
    return [(i, "-" if o == "+" else "+") for i, o in reversed(steps)]


def align(a, b):
    """gfo_align_paths(0, -1, -1, a, b) -> (score, row_a, row_b); gaps are (-1, '0')."""
    global _dirty_n
    L = _oracle()
    # the table is zeroed once per evaluatePath (src/eval.cpp:79) and row 0 is filled
    # up to column n only: after a longer path, its row-0 cells beyond n must be 0 again
    if len(a) < _dirty_n:
        L.gfo_dp_zero(_dp)
    _dirty_n = len(a)
    arr_a = (GfoStep * max(len(a), 1))(*[GfoStep(i, o.encode()) for i, o in a])
    arr_b = (GfoStep * max(len(b), 1))(*[GfoStep(i, o.encode()) for i, o in b])
    cap = len(a) + len(b) + 1
    row_a, row_b = (GfoStep * cap)(), (GfoStep * cap)()
    n_row = ctypes.c_uint32()
    score = L.gfo_align_paths(0, -1, -1, arr_a, len(a), arr_b, len(b), _dp, row_a, row_b,
                              ctypes.byref(n_row))
    ra = [(row_a[t].id, row_a[t].orient.decode()) for t in range(n_row.value)]
    rb = [(row_b[t].id, row_b[t].orient.decode()) for t in range(n_row.value)]
    return score, ra, rb


def ops_from_rows(row_a, row_b):
    ops = []
    for x, y in zip(row_a, row_b):
        if y[0] == -1:
            ops.append(2)
        elif x[0] == -1:
            ops.append(3)
        else:
            ops.append(0 if x == y else 1)
    return ops


def winner(a, b):
    """src/eval.cpp:92-101: (fw, rc, oriented B of the winner, score, row_a, row_b)."""
    fw = align(a, b)
    rb = reverse_complement(b)
    rc = align(a, rb)
    if fw[0] > rc[0]:
        return fw[0], rc[0], b, fw
    return fw[0], rc[0], rb, rc


def pair_alignments(aln_off, aln_steps, path_steps):
    """Expected result of Scorer.pair_alignments: (fw, rc, ops_off, ops)."""
    a = [unpack(s) for s in path_steps]
    n_aln = len(aln_off) - 1
    fw = np.zeros(n_aln, np.int32)
    rc = np.zeros(n_aln, np.int32)
    chunks = []
    for k in range(n_aln):
        b = [unpack(s) for s in aln_steps[aln_off[k]:aln_off[k + 1]]]
        fw[k], rc[k], _, (_, ra, rb) = winner(a, b)
        chunks.append(np.asarray(ops_from_rows(ra, rb), np.uint8))
    ops_off = np.zeros(n_aln + 1, np.int64)
    ops_off[1:] = np.cumsum([len(c) for c in chunks])
    ops = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    return fw, rc, ops_off, ops.astype(np.uint8)


def b_row_from_rows(row_a, row_b, name):
    """include/alignments.h:113-121 (what the CLI's traceback_rows path prints)."""
    out = []
    for x, y in zip(row_a, row_b):
        if y[0] == -1:
            out.append("-" * (len(name(x[0])) + 1) + ",")
        elif x != y:
            out.append(name(y[0]) + y[1] + ",")
        else:
            out.append("." * (len(name(y[0])) + 1) + ",")
    return "".join(out)


def b_row_from_ops(a, b, ops, name):
    """The same text from the ops alone, with the score the reference's traceback
    charges (src/alignments.cpp:516-550, walked last column first for b_taken)."""
    out, i, j = [], 0, 0
    for op in ops:
        if op == 2:
            out.append("-" * (len(name(a[i][0])) + 1) + ",")
            i += 1
        else:
            y = b[j]
            out.append(("." * (len(name(y[0])) + 1) if op == 0 else name(y[0]) + y[1]) + ",")
            i += op != 3
            j += 1
    assert (i, j) == (len(a), len(b))
    score, taken = 0, 0
    for op in reversed(ops):
        if i == 0 or j == 0:                 # :517-524 free
            i, j = i - (op == 2), j - (op == 3)
            continue
        if op in (0, 1):
            score -= op
            taken += 1
            i, j = i - 1, j - 1
        elif op == 2:
            score -= taken > 0
            i -= 1
        else:
            score -= 1
            taken += 1
            j -= 1
    return "".join(out), score
