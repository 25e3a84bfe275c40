"""Helpers of the tests that run the reference solver itself (test infrastructure).

`make -C oracle ref` compiles the reference's two solver files where they lie into
oracle/_ref/ref_cli; nothing of the reference enters this tree.  The helpers here run a
command-line solver (that binary or one of the oracle's) on a problem in a scratch directory
and return everything it left behind, so that two solvers can be compared file by file."""
import hashlib
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
REFERENCE_SRC = os.environ.get("REFERENCE_SRC", "/root/reference/src")
REF_CLI = os.path.join(ORACLE_DIR, "_ref", "ref_cli")
REF_COV = os.path.join(ORACLE_DIR, "_ref", "ref_cov")
ORACLE_CLI_LIBM = os.path.join(ORACLE_DIR, "_build", "oracle_cli_libm")
ORACLE_CLI_DET = os.path.join(ORACLE_DIR, "_build", "oracle_cli_det")
ORACLE_COV_LIBM = os.path.join(ORACLE_DIR, "_build", "oracle_cov_libm")
ORACLE_COV_DET = os.path.join(ORACLE_DIR, "_build", "oracle_cov_det")
BRANCH_FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_branches.json")
SUFFIXES = ("_segments.bed", "_loss.tsv", ".db")


def reference_sources_present():
    return os.path.isfile(os.path.join(REFERENCE_SRC, "funPieceListLog.cpp"))


def build_reference(goals=("ref",)):
    """-> path of ref_cli, or None where neither the binary nor the sources exist"""
    if reference_sources_present():
        subprocess.run(["make", "-s", "-C", ORACLE_DIR, "REFERENCE_SRC=" + REFERENCE_SRC]
                       + list(goals), check=True)
    return REF_CLI if os.path.isfile(REF_CLI) else None


def bedgraph_text(chrom_start, chrom_end, count, chrom="chrT"):
    return "".join("%s\t%d\t%d\t%d\n" % (chrom, s, e, c)
                   for s, e, c in zip(chrom_start, chrom_end, count))


def case_text(case):
    return bedgraph_text(case["chromStart"], case["chromEnd"], case["count"])


def run_cli(cli, workdir, text, penalty, block=None, env=None):
    """Run `cli coverage.bedGraph penalty db` in workdir (created; must not exist).  text None:
    the input file is missing.  block in (None, "segments", "loss", "db"): that output path is
    a directory.  -> {"status": exit status, suffix: bytes, or None where no file was left}"""
    os.makedirs(workdir)
    bg = os.path.join(workdir, "coverage.bedGraph")
    if text is not None:
        with open(bg, "w") as f:
            f.write(text)
    pre = "%s_penalty=%s" % (bg, penalty)
    if block is not None:
        os.mkdir(pre + {"segments": "_segments.bed", "loss": "_loss.tsv", "db": ".db"}[block])
    proc = subprocess.run([cli, bg, penalty, pre + ".db"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL, env=env)
    out = {"status": proc.returncode}
    for suffix in SUFFIXES:
        path = pre + suffix
        if os.path.isfile(path):
            with open(path, "rb") as f:
                out[suffix] = f.read()
        else:
            out[suffix] = None
    return out


def differences(a, b):
    """names of the fields (status, the three files) in which two run_cli results differ"""
    return [k for k in ("status",) + SUFFIXES if a[k] != b[k]]


def sha256(data):
    return hashlib.sha256(data).hexdigest()


def load_branch_fixture():
    with open(BRANCH_FIXTURE) as f:
        return json.load(f)
