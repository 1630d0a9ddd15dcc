"""GPU: `gfalign evalPath` renders its rows from the device's traceback ops by
default; GFALIGN_HOST_TRACEBACK=1 fills the table again on the host.  Stdout must
be byte-identical either way, and equal to the rows the oracle's own traceback
renders."""
import os
import subprocess

import numpy as np
import pytest

import align_ops
from gfalign_amd import build as gbuild
from gfalign_amd import synth
from helpers import REF_FILES, load_appendix_c

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


def both(cli, args, env=None):
    dev = run(cli, args, env)
    host = run(cli, args, dict(env or {}, GFALIGN_HOST_TRACEBACK="1"))
    assert dev == host
    return dev


def oracle_rows(t, path_text):
    ids = {"utig4-%d" % k: k for k in range(t.V)}
    a = [(ids[c[:-1]], c[-1]) for c in path_text.split(",")]
    rows = []
    for k in range(t.N):
        b = [align_ops.unpack(s) for s in t.aln_steps[t.aln_off[k]:t.aln_off[k + 1]]]
        fw, rc, _, (score, ra, rb) = align_ops.winner(a, b)
        rows.append((align_ops.b_row_from_rows(ra, rb, lambda i: "utig4-%d" % i), score))
    return rows


def test_appendix_c2(cli, gpu):
    gold = load_appendix_c()["eval_path"]
    args = ["evalPath", "-f", REF_FILES + "/random3.gfa", "-g", REF_FILES + "/random3.gaf", "-p", gold["path"]]
    assert both(cli, args).splitlines() == gold["stdout"]
    out = both(cli, args + ["--devices", "2"], {"GFALIGN_SHARE_DEVICE": "1"})
    assert out.splitlines() == gold["stdout"]


def test_config5_flow_two_devices(cli, gpu, tmp_path):
    """test_cli.py::test_config5_flow_search_then_eval_path's flow: search over two
    scorers, then evalPath on the best path, rows checked against the oracle."""
    t = synth.Tangle(V=20, n_T=16, N=1500, P=1, seed=25)
    d = str(tmp_path)
    t.write_gfa(d + "/g.gfa")
    t.write_nodelist(d + "/nodes.tsv")
    t.write_gaf(d + "/a.gaf")
    env = {"GFALIGN_SHARE_DEVICE": "1"}
    out = run(cli, ["search", "-f", d + "/g.gfa", "-g", d + "/a.gaf", "-n", d + "/nodes.tsv", "-s", "utig4-0",
                    "-d", "utig4-19", "-m", "1000000000", "--devices", "2"], env)
    path_text = out.splitlines()[-1].split("\t")[7]
    out = both(cli, ["evalPath", "-f", d + "/g.gfa", "-g", d + "/a.gaf", "-p", path_text, "--devices", "2"], env)
    lines = out.splitlines()
    assert lines[0] == path_text and len(lines) == t.N + 2
    got = [(l.split("\t")[0], int(l.rsplit("\t", 1)[1])) for l in lines[1:-1]]
    assert got == oracle_rows(t, path_text)


def test_many_render_blocks(cli, gpu, tmp_path):
    """More than four 2048-alignment blocks: rendered on several threads, ops fetched
    per block; three scorers, and one lane per alignment."""
    t = synth.Tangle(V=30, n_T=40, N=9000, P=1, seed=41)
    d = str(tmp_path)
    t.write_gfa(d + "/g.gfa")
    t.write_gaf(d + "/a.gaf")
    path_text = ",".join("utig4-%d%s" % (int(s) >> 1, "-" if int(s) & 1 else "+") for s in t.T[:25])
    args = ["evalPath", "-f", d + "/g.gfa", "-g", d + "/a.gaf", "-p", path_text]
    out = both(cli, args)
    assert both(cli, args + ["--devices", "3"], {"GFALIGN_SHARE_DEVICE": "1", "GFALIGN_DEDUP": "0"}) == out
    lines = out.splitlines()
    got = [(l.split("\t")[0], int(l.rsplit("\t", 1)[1])) for l in lines[1:-1]]
    assert got == oracle_rows(t, path_text)


def test_several_ops_chunks(cli, gpu, tmp_path):
    """140 000 alignments: 69 render blocks, more than the 64 a renderer may run
    ahead of the writer, and three chunks of device ops (32 blocks each)."""
    import oracle
    t = synth.Tangle(V=40, n_T=60, N=140000, P=1, seed=43)
    d = str(tmp_path)
    t.write_gfa(d + "/g.gfa")
    t.write_gaf(d + "/a.gaf")
    path_text = ",".join("utig4-%d%s" % (int(s) >> 1, "-" if int(s) & 1 else "+") for s in t.T[:30])
    out = both(cli, ["evalPath", "-f", d + "/g.gfa", "-g", d + "/a.gaf", "-p", path_text, "--devices", "2"],
               {"GFALIGN_SHARE_DEVICE": "1"})
    lines = out.splitlines()
    assert len(lines) == t.N + 2
    path = [(int(c[6:-1]) << 1) | int(c[-1] == "-") for c in path_text.split(",")]
    fw, rc = oracle.pair_scores(t.aln_off, t.aln_steps, path)
    assert [int(l.rsplit("\t", 1)[1]) for l in lines[1:-1]] == np.maximum(fw, rc).tolist()
