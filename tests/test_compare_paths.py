"""CPU: the verdict model behind gfal_scorer_verdicts / `gfalign comparePaths`
agrees with the oracle's counters; the path-file rules; comparePaths without
alignments runs without a GPU; its argument errors."""
import os
import random
import subprocess

import numpy as np
import pytest

import oracle
import verdict_model
from gfalign_amd import build as gbuild
from helpers import REF_FILES, csr, random_case, walk_case

O = verdict_model.GFAL_STEP_OTHER


@pytest.fixture(scope="module")
def cli():
    path = gbuild.build_cli()
    assert path and os.path.exists(path)
    return path


def run(cli, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([cli] + args, env=e, capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("flt", [True, False])
def test_model_column_sums_equal_the_oracle(seed, flt):
    rnd = random.Random(seed)
    if seed == 1:
        alns, paths = random_case(rnd, 6, 300, 12, 6, 12)
    else:
        alns, paths = walk_case(rnd, 12, 80, 400, 10, 20)
    alns += [[], []]
    paths.append([O | paths[0][0]] + paths[0][1:])         # a step that equals nothing
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    codes = verdict_model.verdicts(aoff, ast, poff, pst, flt)
    exp = oracle.evaluate_paths(aoff, ast, poff, pst, flt)
    bad, good, una = verdict_model.column_sums(codes)
    assert np.array_equal(bad, exp[0]) and np.array_equal(good, exp[1])
    # (the reference's own `unaligned` counts the off-path steps of those alignments)
    assert np.array_equal(una, len(alns) - exp[0] - exp[1])
    assert (una <= exp[2]).all()
    assert (codes[-2:] == 0).all()                          # zero-step: good for every path
    if not flt:
        assert (codes != 2).all()


def test_model_discordance_identity():
    """filter off: d[i, j] - d[j, i] = good_i - good_j."""
    rnd = random.Random(8)
    alns, paths = walk_case(rnd, 10, 60, 300, 8, 15)
    aoff, ast = csr(alns)
    poff, pst = csr(paths)
    codes = verdict_model.verdicts(aoff, ast, poff, pst, False)
    d = verdict_model.discordance(codes).astype(np.int64)
    good = (codes == 0).sum(axis=0)
    assert np.array_equal(d - d.T, good[:, None] - good[None, :])
    assert (np.diag(d) == 0).all()


def test_path_file_lines():
    p = verdict_model.parse_path_line
    assert p("1+,2-,3+\n") == "1+,2-,3+"
    assert p("7\t3\t5\t-6\t3\t3\tT\tutig4-0+,utig4-1-\n") == "utig4-0+,utig4-1-"
    for skipped in ("", "\n", "# a comment\n", "Reached maximum number of steps (400)\n"):
        assert p(skipped) is None


def _paths_file(tmp_path, text):
    f = tmp_path / ("paths%d.txt" % len(list(tmp_path.glob("paths*.txt"))))
    f.write_text(text)
    return str(f)


def test_without_alignments_prints_the_zero_table(cli, tmp_path):
    """A GAF without alignments needs no GPU: every counter 0, every pair 0 0; search
    rows and bare paths are read alike, the other lines skipped."""
    gaf = tmp_path / "empty.gaf"
    gaf.write_text("")
    paths = _paths_file(tmp_path, "# candidates\n1+,4+\n\n"
                                  "1\t0\t0\t-2\t2\t2\tF\t1+,2+,3+,4+\n"
                                  "Reached maximum number of steps (3)\n2-,1-\n")
    for extra in ([], ["--filter"], ["--devices", "2"]):
        rc, out, err = run(cli, ["comparePaths", "-f", REF_FILES + "/random3.gfa", "-g", str(gaf),
                                 "-P", paths] + extra)
        assert rc == 0, err
        assert out == ("#path\tbad\tgood\tunaligned\tpath\n"
                       "1\t0\t0\t0\t1+,4+\n"
                       "2\t0\t0\t0\t1+,2+,3+,4+\n"
                       "3\t0\t0\t0\t2-,1-\n"
                       "#pair\tgood_first_bad_second\tgood_second_bad_first\n"
                       "1\t2\t0\t0\n1\t3\t0\t0\n2\t3\t0\t0\n")
    rows = tmp_path / "rows.tsv"
    rc, _, err = run(cli, ["comparePaths", "-f", REF_FILES + "/random3.gfa", "-g", str(gaf), "-P", paths,
                           "--alignments", str(rows)])
    assert rc == 0, err
    assert rows.read_text() == ""


def test_argument_errors(cli, tmp_path):
    gfa, gaf = REF_FILES + "/random3.gfa", REF_FILES + "/random3.gaf"
    empty = tmp_path / "empty.gaf"
    empty.write_text("")
    cases = [
        (["comparePaths", "-f", gfa, "-g", str(empty)], "path file"),
        (["comparePaths", "-f", gfa, "-g", str(empty), "-P", str(tmp_path / "missing.txt")], "does not exist"),
        (["comparePaths", "-f", gfa, "-g", str(empty), "-P", _paths_file(tmp_path, "1+,9+\n")],
         "cannot find node (9)"),
        (["comparePaths", "-f", gfa, "-g", str(empty), "-P", _paths_file(tmp_path, "# nothing\n\n")], "no paths"),
        (["comparePaths", "-f", gfa, "-g", str(empty), "-P", _paths_file(tmp_path, "1+,2+\n" * 4097)],
         "at most 4096"),
        (["comparePaths", "-f", gfa, "-g", str(empty), "-P", _paths_file(tmp_path, "1+\n"),
          "--alignments", str(tmp_path / "no" / "such" / "dir.tsv")], "cannot write"),
    ]
    for args, msg in cases:
        rc, out, err = run(cli, args)
        assert rc != 0 and msg in err and out == "", (args, err)


def test_needs_a_gpu_when_there_are_alignments(cli, tmp_path):
    from gfalign_amd import scorer
    if scorer.device_count() > 0:
        pytest.skip("a GPU is visible here")
    rc, out, err = run(cli, ["comparePaths", "-f", REF_FILES + "/random3.gfa", "-g", REF_FILES + "/random3.gaf",
                             "-P", _paths_file(tmp_path, "1+,4+\n")])
    assert rc != 0 and "no usable HIP device" in err and out == ""


def test_help_lists_the_tool(cli):
    rc, out, _ = run(cli, ["-h"])
    assert rc == 0 and "comparePaths" in out.split()
