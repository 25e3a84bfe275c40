"""The CPU oracle against the reference solver itself.

`make -C oracle ref` compiles the reference's solver where it lies into oracle/_ref/ref_cli
(plain -O2, no contraction, the machine's libm: as oracle_cli_libm is built).  On every input
below the two programs must end with the same status and leave the same files with the same
bytes: _segments.bed, _loss.tsv and the .db of stored cost functions.  Nothing here is a
tolerance: same algorithm, same arithmetic, same libm."""
import os

import pytest

import reference_live as rl
from conftest import GOLDEN, _build_oracle

if not os.path.isfile(rl.REF_CLI) and not rl.reference_sources_present():
    pytest.skip("oracle/_ref/ref_cli is absent and REFERENCE_SRC (%s) does not exist" % rl.REFERENCE_SRC,
                allow_module_level=True)


@pytest.fixture(scope="module")
def ref_cli():
    _build_oracle()
    cli = rl.build_reference()
    assert cli is not None, "the reference's sources are present but oracle/_ref/ref_cli was not built"
    return cli


def _same(ref_cli, tmp_path, name, text, pen, block=None):
    """both programs on one problem -> the reference's result, after asserting equality"""
    ref = rl.run_cli(ref_cli, str(tmp_path / (name + "_ref")), text, pen, block)
    libm = rl.run_cli(rl.ORACLE_CLI_LIBM, str(tmp_path / (name + "_libm")), text, pen, block)
    assert not rl.differences(ref, libm), (name, pen, rl.differences(ref, libm), ref["status"],
                                           libm["status"])
    return ref


def test_mono27ac_at_the_search_penalties(ref_cli, tmp_path):
    import test_gpu_parity as gp
    text = open(os.path.join(GOLDEN, "Mono27ac.bedGraph")).read()
    for i, pen in enumerate(gp.MONO_PENALTIES):
        ref = _same(ref_cli, tmp_path, "m%d" % i, text, pen)
        # (no store at penalty Inf: both programs answer that one without the dynamic programme)
        assert ref["status"] == 0 and (ref[".db"] is not None or pen == "Inf")


def test_fuzz_tiny_problems(ref_cli, tmp_path):
    import test_gpu_parity as gp
    for c, (cnt, wid, start, end, pen) in enumerate(gp.fuzz_cases(300, 5)):
        assert _same(ref_cli, tmp_path, "f%d" % c, rl.bedgraph_text(start, end, cnt), pen)["status"] == 0


def test_varied_data_shapes(ref_cli, tmp_path):
    import test_gpu_parity as gp
    n = 0
    for c, (cnt, w, cs, ce, pens) in enumerate(gp.varied_shape_cases(*gp.VARIED_SHAPES_RUN)):
        text = rl.bedgraph_text(cs, ce, cnt)
        for i, pen in enumerate(pens):
            assert _same(ref_cli, tmp_path, "v%d_%d" % (c, i), text, pen)["status"] == 0
            n += 1
    assert n == 54


def test_increasing_and_poisson_coverage(ref_cli, tmp_path):
    from peaksegdisk_amd import synthetic
    cs, ce, cnt = synthetic.increasing_coverage(600)
    for pen in ("100", "10000", "0"):
        assert _same(ref_cli, tmp_path, "inc" + pen, rl.bedgraph_text(cs, ce, cnt), pen)["status"] == 0
    cs, ce, cnt = synthetic.poisson_coverage(5000, seed=11)
    text = rl.bedgraph_text(cs, ce, cnt)
    for i, pen in enumerate(synthetic.penalty_grid(16)[::3]):
        assert _same(ref_cli, tmp_path, "p%d" % i, text, pen)["status"] == 0


def test_known_answers_solve_cases(ref_cli, known_answers, tmp_path):
    for case in known_answers["solve_cases"]:
        ref = _same(ref_cli, tmp_path, case["name"], case["bedGraph"], case["penalty"])
        assert ref["status"] == case["status"], case["name"]
        if "loss_row" in case:
            assert ref["_loss.tsv"].decode().rstrip("\n") == case["loss_row"], case["name"]
        if "db_bytes" in case:
            assert len(ref[".db"]) == case["db_bytes"], case["name"]


def test_known_answers_error_cases(ref_cli, known_answers, tmp_path):
    """statuses, and which files an error leaves behind: the cases that put a directory where an
    output file belongs included"""
    for case in known_answers["error_cases"]:
        ref = _same(ref_cli, tmp_path, case["name"], case["bedGraph"], case["penalty"], case.get("block"))
        assert ref["status"] == case["status"], case["name"]


def test_branch_fixture_is_what_the_reference_writes(ref_cli, tmp_path):
    """tests/golden/reference_branches.json (tools/reference_branches.py): the recorded outputs
    are the reference's, the libm oracle reproduces them byte for byte, and the deterministic
    oracle writes the same segments wherever the fixture says so -- and only there."""
    doc = rl.load_branch_fixture()
    assert doc["cases"]
    for case in doc["cases"]:
        assert 2 <= len(case["count"]) <= 40
        ref = _same(ref_cli, tmp_path, case["name"], rl.case_text(case), case["penalty"])
        assert ref["status"] == 0, case["name"]
        assert ref["_segments.bed"].decode() == case["segments"], case["name"]
        assert ref["_loss.tsv"].decode() == case["loss_row"], case["name"]
        assert len(ref[".db"]) == case["db_size"], case["name"]
        assert rl.sha256(ref[".db"]) == case["db_sha256"], case["name"]
        det = rl.run_cli(rl.ORACLE_CLI_DET, str(tmp_path / (case["name"] + "_det")),
                         rl.case_text(case), case["penalty"])
        assert det["status"] == 0
        assert (det["_segments.bed"] == ref["_segments.bed"]) == case["det_segments_equal_reference"], \
            case["name"]


def test_branch_fixture_table(ref_cli):
    """every decision of the table names a fixture case that exists, or says how many problems
    did not reach it: at least the 200 000 of the search's budget"""
    doc = rl.load_branch_fixture()
    names = {c["name"] for c in doc["cases"]}
    assert len(names) == len(doc["cases"])
    assert doc["search"]["oracle_libm_disagreements"] == []
    for row in doc["table"]:
        if "fixture" in row:
            assert row["fixture"] in names
        else:
            assert row["not_reached_in"] >= 200000, row
    listed = {(o["reference_line"], o["branch"]) for c in doc["cases"] for o in c["outcomes"]}
    assert listed <= {(r["reference_line"], r["branch"]) for r in doc["table"]}
