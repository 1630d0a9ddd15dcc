"""Row counts of the exact-DP worklist of a synthetic batch, built on the CPU.

usage: dp_worklist_stats.py [config] [--json]      (config: a synth.CONFIGS name, default config3)

The worklist holds the pairs that reach the DP: the filter
passes, B is not a subpath of A on either strand, m <= n, and a proper suffix of
B (fw) or of rc(B) (rc) equals a prefix of A.  For every pair it derives the
rows that row skipping selects (the first m rows and the rows r .. r + m after
every row r whose node occurs in B), forms the waves of 64
entries as the device's counting sort does (by length class, then by path in the
order k_wl_offsets lays the bins out), and reports per class:

  max_lane    sum over waves of the busiest lane's rows (per-lane row loops)
  max_sorted  the same with each (class, path) run sorted by row count
  run_union   sum over waves of the row union of each path run of the wave
  wave_union  sum over waves of the row union over all lanes of the wave
  paths/wave  how many paths a wave spans
  turns_all   sum over waves of the busiest lane's turns of the row loop when
              a lane visits every 32-row block of its path (an empty block
              costs a turn)
  turns_mask  the same when a lane visits only the blocks of its block mask
              (the blocks of its marked rows r and of r + m)

A pair with both orientations flagged runs a second fill over the same rows;
every figure counts both fills.  Counts, not times.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kernel_model  # noqa: E402
from gfalign_amd import synth  # noqa: E402

WAVE = 64
N_CLASSES = 5
MC = (4, 8, 16, 32, None)


def length_class(m):
    return 0 if m <= 4 else 1 if m <= 8 else 2 if m <= 16 else 3 if m <= 32 else 4


def split(off, steps):
    return [tuple(int(s) for s in steps[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def worklist(paths, alns):
    """[(path index, alignment index, has_fw, has_rc)] in path-major order."""
    # distinct prefixes of the paths, up to the longest proper suffix of an alignment
    max_m = max((len(b) for b in alns), default=0)
    by_prefix = {}                    # prefix -> paths that start with it
    for p, A in enumerate(paths):
        for ln in range(1, min(max_m - 1, len(A)) + 1):
            by_prefix.setdefault(A[:ln], []).append(p)
    flags = {}                        # (p, k) -> [fw, rc]
    for k, B in enumerate(alns):
        m = len(B)
        for o, Bo in enumerate((B, tuple(kernel_model.rc(B)))):
            for ln in range(1, m):
                for p in by_prefix.get(Bo[m - ln:], ()):
                    flags.setdefault((p, k), [False, False])[o] = True
    out = []
    occ = {}
    for (p, k), (fw, rc) in sorted(flags.items()):
        A, B = paths[p], alns[k]
        n, m = len(A), len(B)
        if m > n:
            continue
        if p not in occ:
            occ = {p: occurrences(A)}
        o = occ[p]
        if any((s >> 1) not in o for s in B):
            continue
        if is_subpath(A, B, o) or is_subpath(A, tuple(kernel_model.rc(B)), o):
            continue
        out.append((p, k, fw, rc))
    return out


def occurrences(A):
    """node -> positions of the path's steps on that node"""
    o = {}
    for i, s in enumerate(A):
        o.setdefault(s >> 1, []).append(i)
    return o


def is_subpath(A, B, occ):
    m = len(B)
    return any(A[i:i + m] == B for i in occ.get(B[0] >> 1, ()))


def rows_of(A, B, occ):
    """Path positions (0-based) whose rows row skipping computes."""
    n, m = len(A), len(B)
    rows = set(range(min(m, n)))
    for v in {s >> 1 for s in B}:
        for r in occ.get(v, ()):
            rows.update(range(r, min(r + m + 1, n)))
    return frozenset(rows)


def loop_turns(A, B, occ, rows):
    """(turns visiting every block, turns visiting the masked blocks) of one fill:
    a visited block costs max(1, its rows) turns, and the loop one more to end."""
    n, m = len(A), len(B)
    per_block = {}
    for r in rows:
        per_block[r >> 5] = per_block.get(r >> 5, 0) + 1
    every = sum(max(1, per_block.get(b, 0)) for b in range((n + 31) // 32)) + 1
    mask = {0}
    for v in {s >> 1 for s in B}:
        for r in occ.get(v, ()):
            mask.update((r >> 5, min((r + m) >> 5, 31)))
    masked = sum(max(1, per_block.get(b, 0)) for b in mask if b * 32 < n) + 1
    return every, masked


def device_order(paths, wl):
    """The sorted list as k_wl_scatter lays it out: class, then the bins of the
    paths in slot order (longest path first), thread-strided over 1024 threads."""
    n_paths = len(paths)
    slot = np.empty(n_paths, np.int64)
    slot[sorted(range(n_paths), key=lambda p: (-len(paths[p]), p))] = np.arange(n_paths)
    def key(e):
        p, k = e[0], e[1]
        s = int(slot[p])
        return (e[4], s % 1024, s // 1024, k)
    return sorted(wl, key=key)


def stats(paths, alns):
    wl = worklist(paths, alns)
    ents, occ = [], {}
    for p, k, fw, rc in wl:
        if p not in occ:
            occ = {p: occurrences(paths[p])}
        rows = rows_of(paths[p], alns[k], occ[p])
        turns = loop_turns(paths[p], alns[k], occ[p], rows)
        ents.append((p, k, fw, rc, length_class(len(alns[k])), rows, turns))
    ents = device_order(paths, ents)
    out = {"pairs": len(ents), "classes": {}}
    for c in range(N_CLASSES):
        cl = [e for e in ents if e[4] == c]
        if not cl:
            continue
        # (b): each (class, path) run sorted by row count, longest first
        runs, srt = {}, []
        for e in cl:
            runs.setdefault(e[0], []).append(e)
        seen = set()
        for e in cl:
            if e[0] not in seen:
                seen.add(e[0])
                srt.extend(sorted(runs[e[0]], key=lambda x: -len(x[5])))
        r = dict(entries=len(cl), waves=0, max_lane=0, max_sorted=0, run_union=0, wave_union=0,
                 turns_all=0, turns_mask=0,
                 both=sum(1 for e in cl if e[2] and e[3]), lane_rows=0, paths_per_wave={})
        for w0 in range(0, len(cl), WAVE):
            wave, wave_s = cl[w0:w0 + WAVE], srt[w0:w0 + WAVE]
            r["waves"] += 1
            for fill in (0, 1):
                pick = (lambda e: True) if fill == 0 else (lambda e: e[2] and e[3])
                lanes = [e for e in wave if pick(e)]
                if not lanes:
                    continue
                r["lane_rows"] += sum(len(e[5]) for e in lanes)
                r["max_lane"] += max(len(e[5]) for e in lanes)
                r["turns_all"] += max(e[6][0] for e in lanes)
                r["turns_mask"] += max(e[6][1] for e in lanes)
                lanes_s = [e for e in wave_s if pick(e)]
                r["max_sorted"] += max(len(e[5]) for e in lanes_s) if lanes_s else 0
                by_path = {}
                for e in lanes:
                    by_path.setdefault(e[0], set()).update(e[5])
                r["run_union"] += sum(len(u) for u in by_path.values())
                r["wave_union"] += len(set().union(*(e[5] for e in lanes)))
            np_ = len({e[0] for e in wave})
            r["paths_per_wave"][np_] = r["paths_per_wave"].get(np_, 0) + 1
        r["paths_per_wave"] = dict(sorted(r["paths_per_wave"].items()))
        out["classes"][c] = r
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    name = args[0] if args else "config3"
    t = synth.make(name)
    paths = split(t.path_off, t.path_steps)
    alns = split(t.aln_off, t.aln_steps)
    out = stats(paths, alns)
    out["config"] = name
    if "--json" in sys.argv:
        print(json.dumps(out))
        return
    print("%s: %d DP pairs" % (name, out["pairs"]))
    print("%-5s %8s %6s %6s %11s %11s %11s %11s %11s %11s  %s" % (
        "class", "entries", "both", "waves", "max_lane", "max_sorted", "run_union", "wave_union",
        "turns_all", "turns_mask", "paths per wave: waves"))
    for c, r in out["classes"].items():
        print("%-5d %8d %6d %6d %11d %11d %11d %11d %11d %11d  %s" % (
            c, r["entries"], r["both"], r["waves"], r["max_lane"], r["max_sorted"], r["run_union"],
            r["wave_union"], r["turns_all"], r["turns_mask"],
            " ".join("%d:%d" % kv for kv in r["paths_per_wave"].items())))


if __name__ == "__main__":
    main()
