"""Time of the verdict calls on a synthetic alignment set (default: config3's 1 M
alignments) for batches of its first P candidates: Scorer.verdicts + Scorer.discordance
against P calls of pair_scores (the per-path route evalPath offers; timed on the first
min(P, PAIR_SAMPLE) paths and scaled to P), and discordance against gfal_scorer_score of
the same batch with k_scan (GFAL_SCAN=1); and discordance on a gfal_scorer_create_dedup
scorer (what `gfalign comparePaths` uses by default: k_discord weighs lanes by weight bits).  Median of `reps` calls each, after one warm-up.
usage: compare_time.py [config] [reps] [P ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gfalign_amd import scorer as gscorer, synth

cfg = sys.argv[1] if len(sys.argv) > 1 else "config3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
Ps = [int(x) for x in sys.argv[3:]] or [64, 256, 1024]
PAIR_SAMPLE = 16
t = synth.make(cfg)
lib = gscorer.load_library()
print("%s: %d alignments; build %s" % (cfg, t.N, lib.gfal_build_id().decode()), flush=True)


def med(fn):
    fn()
    v = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        v.append(time.perf_counter() - t0)
    return sorted(v)[len(v) // 2] * 1e3


os.environ["GFAL_SCAN"] = "1"
sc = gscorer.Scorer(t.aln_off, t.aln_steps, t.V)
dd = gscorer.Scorer(t.aln_off, t.aln_steps, t.V, dedup=True)
print("dedup scorer: %d resident lanes" % dd.info()["n_lanes"],
      flush=True)
for P in Ps:
    off = t.path_off[:P + 1].copy()
    st = t.path_steps[:off[-1]].copy()
    ms_v = med(lambda: sc.verdicts(off, st, True))
    ms_d = med(lambda: sc.discordance(off, st, True))
    ms_s = med(lambda: sc.evaluate_paths(off, st, True))
    ms_dd = med(lambda: dd.discordance(off, st, True))
    ms_dds = med(lambda: dd.evaluate_paths(off, st, True))
    k = min(P, PAIR_SAMPLE)
    ms_pair = med(lambda: [sc.pair_scores(st[off[q]:off[q + 1]]) for q in range(k)]) * P / k
    print("P=%5d  verdicts %9.2f ms  discordance %8.2f ms  score(k_scan) %7.2f ms  "
          "P x pair_scores %10.1f ms (from %d)  | discord/score %.2fx  pair/(verdicts+discord) %.1fx  "
          "| dedup: discordance %7.2f ms  score %7.2f ms"
          % (P, ms_v, ms_d, ms_s, ms_pair, k, ms_d / ms_s, ms_pair / (ms_v + ms_d), ms_dd, ms_dds), flush=True)
sc.close()
dd.close()
