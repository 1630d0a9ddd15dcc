"""Wall time of `gfalign evalPath` with stdout to /dev/null: rows rendered from the
device's traceback ops (the default) against the host refill (GFALIGN_HOST_TRACEBACK=1),
alternated, on a synthetic GAF (default: config5's 10 M alignments) and a path of the
first L steps of its truth walk.  usage: evalpath_traceback_time.py [config] [L] [reps]"""
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gfalign_amd import build, synth

cfg = sys.argv[1] if len(sys.argv) > 1 else "config5"
L = int(sys.argv[2]) if len(sys.argv) > 2 else 100
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
t = synth.make(cfg)
d = "/tmp/evalpath_" + cfg
os.makedirs(d, exist_ok=True)
t.write_gfa(d + "/g.gfa")
t.write_gaf(d + "/a.gaf")
path = ",".join("utig4-%d%s" % (int(s) >> 1, "-" if int(s) & 1 else "+") for s in t.T[:L])
cli = build.build_cli()
args = [cli, "evalPath", "-f", d + "/g.gfa", "-g", d + "/a.gaf", "-p", path]
print("%s: %d alignments, path of %d steps, %d cores" % (cfg, t.N, L, os.cpu_count()), flush=True)
times = {"device ops": [], "host traceback": []}
for r in range(reps):
    for name, env in (("device ops", {}), ("host traceback", {"GFALIGN_HOST_TRACEBACK": "1"})):
        t0 = time.time()
        p = subprocess.run(args, env=dict(os.environ, **env), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        times[name].append(time.time() - t0)
        assert p.returncode == 0, p.stderr[-2000:]
        print("  rep %d %-15s %.2f s" % (r, name, times[name][-1]), flush=True)
for name, v in times.items():
    print("%-15s min %.2f s  median %.2f s" % (name, min(v), sorted(v)[len(v) // 2]))
