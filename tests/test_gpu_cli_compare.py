"""GPU: `gfalign comparePaths` on a synthetic tangle -- fed the rows of
`gfalign search --return-all-paths` -- against the oracle and the verdict model;
stdout and the --alignments rows do not depend on sharding or on the code blocks."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import verdict_model
from gfalign_amd import build as gbuild
from gfalign_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    return gbuild.build_cli()


def run(cli, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([cli] + args, env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def packed(text):
    return [(int(c[:-1].split("-")[1]) << 1) | int(c[-1] == "-") for c in text.split(",")]


def test_search_rows_into_compare_paths(cli, gpu, tmp_path):
    t = synth.Tangle(V=30, n_T=24, N=400, P=1, seed=22)
    gfa, nodes, gaf = (str(tmp_path / n) for n in ("g.gfa", "nodes.tsv", "a.gaf"))
    t.write_gfa(gfa)
    t.write_nodelist(nodes)
    t.write_gaf(gaf)
    rows = run(cli, ["search", "-f", gfa, "-g", gaf, "-n", nodes, "-s", "utig4-0", "-d", "utig4-29",
                     "-m", "150", "--return-all-paths"])
    (tmp_path / "rows.txt").write_text("# search output\n" + rows)
    found = [r.split("\t") for r in rows.splitlines() if "\t" in r]
    assert len(found) >= 2
    texts = [r[-1] for r in found]
    poff = np.zeros(len(texts) + 1, np.int32)
    poff[1:] = np.cumsum([len(packed(x)) for x in texts])
    pst = np.concatenate([packed(x) for x in texts]).astype(np.int32)
    names = ["read%d" % k for k in range(t.N)]

    for flt in (True, False):
        base = ["comparePaths", "-f", gfa, "-g", gaf, "-P", str(tmp_path / "rows.txt")] + (["--filter"] if flt else [])
        outs, tables = [], []
        for env, extra in (({}, []), ({"GFALIGN_COMPARE_BLOCK": "37"}, []),
                           ({"GFALIGN_SHARE_DEVICE": "1"}, ["--devices", "2"]),
                           ({"GFALIGN_SHARE_DEVICE": "1", "GFALIGN_COMPARE_BLOCK": "101"}, ["--devices", "3"]),
                           ({"GFALIGN_DEDUP": "0"}, [])):
            tsv = tmp_path / ("aln%d.tsv" % len(outs))
            outs.append(run(cli, base + extra + ["--alignments", str(tsv)], env))
            tables.append(tsv.read_text())
        assert all(o == outs[0] for o in outs) and all(x == tables[0] for x in tables)

        lines = outs[0].splitlines()
        P = len(texts)
        assert lines[0] == "#path\tbad\tgood\tunaligned\tpath" and lines[P + 1].startswith("#pair")
        bad, good, _ = oracle.evaluate_paths(t.aln_off, t.aln_steps, poff, pst, flt)
        codes = verdict_model.verdicts(t.aln_off, t.aln_steps, poff, pst, flt)
        for p in range(P):
            f = lines[1 + p].split("\t")
            assert f == [str(p + 1), str(bad[p]), str(good[p]), str(t.N - bad[p] - good[p]), texts[p]]
            if flt:     # search prints the filtered counters
                assert f[1:3] == found[p][1:3]
        d = verdict_model.discordance(codes)
        pairs = [l.split("\t") for l in lines[P + 2:]]
        assert pairs == [[str(i + 1), str(j + 1), str(d[i, j]), str(d[j, i])]
                         for i in range(P) for j in range(i + 1, P)]
        exp_rows = "".join("%s\t%s\n" % (names[k], "".join("GBU"[c] for c in codes[k]))
                           for k in range(t.N) if (codes[k] != codes[k, 0]).any())
        assert tables[0] == exp_rows
        assert exp_rows                               # the paths do differ somewhere
