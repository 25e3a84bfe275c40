#!/usr/bin/env python3
"""Search for tiny problems that take the outcomes of the reference's piece algebra which the
suite's inputs never take, and write them to tests/golden/reference_branches.json.

    make -C oracle ref cov                      # ref_cov, oracle_cov_det, oracle_cov_libm
    tools/reference_branches.py --search        # baseline + >= 200 000 problems, writes the fixture
    tools/reference_branches.py --report        # the decision table, from the fixture alone
    tools/reference_branches.py --report --markdown   # the same as a table for the README

Every decision of the reference's funPieceListLog.cpp (lines 206-1270) is listed in DECISIONS
with the line of its mirror in oracle/peakseg_oracle.c.  `gcov -b` numbers a decision's branches
in source order: branch 2k is "test k holds", branch 2k+1 "test k does not hold".  An outcome
counts as taken by a problem when the reference takes it AND the deterministic-math oracle
takes the mirrored one on that same problem (the kernels are compared with that oracle, whose
arithmetic may go the other way at a near tie).  Every problem is also solved by the libm oracle,
and its three output files and exit status are compared with the reference's: a difference is a
bug in the oracle and is reported.

Coverage counters and listings stay in a temporary directory: listings hold the reference's
source text and never enter the tree.  The fixture holds data only."""
import argparse
import json
import multiprocessing
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_live as rl  # noqa: E402

ML, MM, ENV, PMP = "set_to_min_less_of", "set_to_min_more_of", "set_to_min_env_of", "push_min_pieces"
# (function, reference line, first branch used there, oracle line, tests in source order)
DECISIONS = [
    ("getCost", 211, 0, 111, ["cost asked at log-mean -inf"]),
    ("getCost", 216, 0, 116, ["piece has no log term"]),
    ("getDeriv", 228, 0, 127, ["derivative asked at log-mean -inf"]),
    (ML, 244, 0, 275, ["pieces left to walk"]),
    (ML, 247, 0, 279, ["no constant piece is open"]),
    (ML, 256, 0, 283, ["piece has no log term"]),
    (ML, 271, 0, 288, ["it is the last piece"]),
    (ML, 288, 0, 295, ["next piece starts numerically higher", "the piece's two ends differ numerically"]),
    (ML, 313, 0, 307, ["it is the last piece"]),
    (ML, 327, 0, 313, ["right end numerically above the minimum", "next piece numerically above the minimum"]),
    (ML, 328, 0, 314, ["minimum at or before the left end", "the costs confirm the minimum"]),
    (ML, 337, 0, 318, ["minimum before the right end", "the costs confirm the minimum"]),
    (ML, 347, 0, 320, ["the decreasing part is not empty"]),
    (ML, 376, 0, 335, ["piece has no log term"]),
    (ML, 378, 0, 336, ["its linear coefficient is negative"]),
    (ML, 389, 1, 341, ["piece meets the constant twice"]),
    (ML, 397, 0, 343, ["smaller root right of the left end", "smaller root left of the right end"]),
    (ML, 410, 0, 351, ["right end numerically at or below the constant", "a constant piece is still open"]),
    (ML, 429, 0, 362, ["the walk ends on an open constant piece"]),
    (MM, 450, 0, 407, ["pieces left to walk"]),
    (MM, 452, 0, 410, ["no constant piece is open"]),
    (MM, 458, 0, 411, ["piece has no log term"]),
    (MM, 475, 0, 420, ["it is the first piece"]),
    (MM, 484, 0, 428, ["minimum at or after the right end"]),
    (MM, 500, 0, 431, ["piece numerically decreasing"]),
    (MM, 524, 0, 441, ["minimum right of the left end", "left end numerically above the minimum",
                       "previous piece numerically above the minimum"]),
    (MM, 530, 0, 444, ["the increasing part is not empty"]),
    (MM, 561, 0, 461, ["piece has no log term"]),
    (MM, 569, 1, 465, ["piece meets the constant twice"]),
    (MM, 578, 0, 469, ["crossing right of the left end", "crossing left of the right end"]),
    (MM, 591, 0, 475, ["left end numerically at or below the constant"]),
    (MM, 608, 0, 485, ["the walk ends on an open constant piece"]),
    ("findMean", 646, 0, 521, ["pieces left to search"]),
    ("findMean", 647, 0, 523, ["left end at or below the mean", "right end at or above the mean"]),
    ("Minimize", 697, 0, 536, ["pieces left"]),
    ("Minimize", 699, 0, 539, ["argmin left of the piece"]),
    ("Minimize", 701, 0, 541, ["argmin right of the piece"]),
    ("Minimize", 705, 0, 545, ["candidate is cheaper"]),
    (ENV, 845, 0, 849, ["pieces of the first function left", "pieces of the second function left"]),
    (ENV, 853, 0, 858, ["the first function's piece ends here"]),
    (ENV, 856, 0, 862, ["the second function's piece ends here"]),
    (ENV, 866, 0, 556, ["same-function test: linear coefficients equal", "log coefficients equal"]),
    (PMP, 882, 0, 595, ["first piece starts left of the second"]),
    (PMP, 889, 0, 600, ["second piece starts left of the first"]),
    (PMP, 894, 0, 603, ["first function at its first piece", "second function at its first piece"]),
    (PMP, 908, 0, 612, ["first piece ends before the second"]),
    (PMP, 914, 0, 617, ["second piece ends before the first"]),
    (PMP, 919, 0, 620, ["first function at its last piece", "second function at its last piece"]),
    (PMP, 933, 0, 628, ["the overlap is empty"]),
    (PMP, 945, 0, 631, ["same function on the whole overlap"]),
    (PMP, 963, 0, 646, ["same function at the left", "same function at the right"]),
    (PMP, 965, 0, 647, ["same on both sides: first lower at the middle"]),
    (PMP, 973, 0, 654, ["difference has no log term"]),
    (PMP, 976, 0, 655, ["nor a linear term"]),
    (PMP, 978, 0, 656, ["constant difference negative"]),
    (PMP, 986, 0, 663, ["constant difference zero"]),
    (PMP, 988, 0, 664, ["linear difference negative"]),
    (PMP, 997, 0, 672, ["linear crossing right of the left end", "linear crossing left of the right end"]),
    (PMP, 1000, 0, 674, ["linear difference positive"]),
    (PMP, 1012, 0, 683, ["linear crossing outside: first lower at the middle"]),
    (PMP, 1024, 0, 694, ["difference has two roots"]),
    (PMP, 1029, 0, 698, ["same function at the right"]),
    (PMP, 1032, 0, 699, ["equal on the right: two roots"]),
    (PMP, 1047, 0, 703, ["equal on the right: smaller root right of the left end", "smaller root left of the optimum"]),
    (PMP, 1048, 0, 704, ["equal on the right: optimum left of the right end"]),
    (PMP, 1050, 0, 706, ["equal on the right, crossing inside: first lower at the left end"]),
    (PMP, 1067, 0, 716, ["equal on the right: crossing before the overlap"]),
    (PMP, 1069, 0, 717, ["equal on the right, crossing before the overlap: first lower at mean 0"]),
    (PMP, 1076, 0, 723, ["equal on the right, no crossing before the overlap: first lower at mean 0"]),
    (PMP, 1087, 0, 731, ["equal on the right, no roots: first lower at the middle"]),
    (PMP, 1094, 0, 738, ["same function at the left"]),
    (PMP, 1096, 0, 739, ["equal on the left: two roots"]),
    (PMP, 1101, 0, 742, ["equal on the left: optimum right of the left end", "optimum left of the larger root"]),
    (PMP, 1102, 0, 743, ["equal on the left: larger root left of the right end"]),
    (PMP, 1105, 0, 745, ["equal on the left, crossing inside: first lower at the right end"]),
    (PMP, 1116, 0, 755, ["equal on the left, no crossing: first lower at the middle"]),
    (PMP, 1128, 0, 764, ["equal on neither side: two roots"]),
    (PMP, 1130, 0, 766, ["larger root right of the left end", "larger root left of the right end"]),
    (PMP, 1136, 0, 768, ["smaller root right of the left end", "smaller root at a positive mean",
                         "smaller root left of the right end"]),
    (PMP, 1138, 0, 769, ["larger root inside"]),
    (PMP, 1139, 0, 770, ["larger root inside: smaller root inside too", "smaller root below the larger"]),
    (PMP, 1160, 0, 777, ["larger root outside: smaller root inside"]),
    (PMP, 1171, 0, 782, ["two crossings inside"]),
    (PMP, 1174, 0, 784, ["two crossings: gap before the first wider than between them"]),
    (PMP, 1180, 0, 787, ["two crossings: first function lower before the first crossing"]),
    (PMP, 1190, 0, 795, ["two crossings: first function lower between them"]),
    (PMP, 1196, 0, 801, ["two crossings: first function is the outer one"]),
    (PMP, 1206, 0, 810, ["one crossing inside"]),
    (PMP, 1219, 0, 815, ["one crossing: first lower before it"]),
    (PMP, 1220, 0, 816, ["one crossing, first lower before: first lower after too"]),
    (PMP, 1228, 0, 823, ["one crossing, second lower before: first lower after"]),
    (PMP, 1248, 0, 832, ["no crossing: middle difference negative", "no crossing: middle difference numerically zero"]),
    (PMP, 1253, 0, 837, ["no crossing: first lower"]),
    ("push_piece", 1263, 0, 563, ["the interval is empty"]),
]
# outcomes that no input can take, with the reason read off the code
UNREACHABLE = {
    (347, 1): "the walk's left bound is the piece's own left end or a smaller root on its decreasing side: "
              "both lie left of a minimum found inside the piece",
    (378, 0): "the solver would throw: every piece's linear coefficient is a sum of non-negative weights",
    (530, 1): "the walk's right bound is the piece's own right end or a larger root on its increasing side: "
              "both lie right of a minimum found inside the piece",
    (845, 3): "both functions cover the same range of means, so the first runs out no later than the second",
    (894, 3): "both functions start at the same smallest mean: pieces that start together there are both first",
    (919, 3): "both functions end at the same largest mean: pieces that end together there are both last",
}
# the deterministic build's exp is an inline function: gcov files the test around it under the
# line before, so that decision's det branches are listed one by one as (oracle line, branch)
DET_BRANCHES = {1136: [(768, 0), (768, 1), (767, 0), (767, 1), (768, 2), (768, 3)]}
# Two outcomes leave no trace where the constant piece would have ended at the function's end
# anyway.  For these a candidate is preferred when it matters: a det oracle compiled from a
# temporary copy of oracle/peakseg_oracle.c with that ending switched off (old text, new text)
# must write another .db.
MUTANTS = {
    (410, 2): ("if (right_cost <= prev_min_cost + NEWTON_EPSILON && prev_min_cost < INFINITY) {", "if (0) {"),
    (591, 0): ("} else if (left_cost <= prev_min_cost + NEWTON_EPSILON) {", "} else if (0) {"),
}
MUTANT_CLI = {}   # outcome -> path, set by build_mutants() before the workers start
COV = {"ref": (rl.REF_COV, os.path.join(rl.ORACLE_DIR, "_ref", "cov"), "funPieceListLog", "funPieceListLog.cpp"),
       "det": (rl.ORACLE_COV_DET, os.path.join(rl.ORACLE_DIR, "_build", "cov_det"), "peakseg_oracle", "peakseg_oracle.c"),
       "libm": (rl.ORACLE_COV_LIBM, os.path.join(rl.ORACLE_DIR, "_build", "cov_libm"), "peakseg_oracle", "peakseg_oracle.c")}


def outcome_words(key):
    line, k = key
    for fun, ref_line, _, _, tests in DECISIONS:
        if ref_line == line:
            return fun, "%s: %s" % (tests[k // 2], "no" if k % 2 else "yes")
    raise KeyError(key)


def all_outcomes():
    return [(d[1], k) for d in DECISIONS for k in range(2 * len(d[4]))]


# ---- running problems under the coverage builds ------------------------------------------

def problem_text(p):
    if "text" in p:
        return p["text"]
    end = np.cumsum(np.asarray(p["width"], dtype=np.int64))
    return rl.bedgraph_text(end - np.asarray(p["width"]), end, p["count"])


class Runner:
    def __init__(self, base):
        self.base = base
        self.serial = 0
        self.env = {k: dict(os.environ, GCOV_PREFIX=os.path.join(base, "cov_" + k)) for k in COV}
        self.reset()

    def gcda_dir(self, kind):
        return os.path.join(self.base, "cov_" + kind) + COV[kind][1]

    def reset(self):
        for kind in COV:
            shutil.rmtree(os.path.join(self.base, "cov_" + kind), ignore_errors=True)
            os.makedirs(self.gcda_dir(kind))
            shutil.copy(os.path.join(COV[kind][1], COV[kind][2] + ".gcno"), self.gcda_dir(kind))

    def run(self, p, kinds=("ref", "libm", "det")):
        self.serial += 1
        text = problem_text(p)
        out = {}
        for kind in kinds:
            d = os.path.join(self.base, "w%d_%s" % (self.serial, kind))
            out[kind] = rl.run_cli(COV[kind][0], d, text, p["penalty"], env=self.env[kind])
            shutil.rmtree(d)
        return out

    def branches(self, kind):
        """{line: [counts of the branches that are not exception edges]}"""
        d = self.gcda_dir(kind)
        gcda = os.path.join(d, COV[kind][2] + ".gcda")
        if not os.path.exists(gcda):
            return {}
        text = subprocess.run(["gcov", "-b", "--json-format", "--stdout", gcda], cwd=d,
                              capture_output=True, check=True).stdout
        for f in json.loads(text)["files"]:
            if f["file"].endswith(COV[kind][3]):
                return {ln["line_number"]: [b["count"] for b in ln["branches"] if not b["throw"]]
                        for ln in f["lines"] if ln["branches"]}
        return {}

    def counts(self, kinds=("ref", "det")):
        """{(reference line, branch): {kind: count}} for the decisions of the table"""
        br = {k: self.branches(k) for k in kinds}
        out = {}
        for _, ref_line, off, ora_line, tests in DECISIONS:
            for k in range(2 * len(tests)):
                c = {}
                for kind in kinds:
                    line, i = (ref_line, k + off) if kind == "ref" else (ora_line, k)
                    if kind == "det" and ref_line in DET_BRANCHES:
                        line, i = DET_BRANCHES[ref_line][k]
                    v = br[kind].get(line, [])
                    c[kind] = v[i] if i < len(v) else 0
                out[(ref_line, k)] = c
        return out

    def taken(self):
        return {key for key, c in self.counts().items() if c["ref"] > 0 and c["det"] > 0}


def build_mutants(base):
    src = open(os.path.join(rl.ORACLE_DIR, "peakseg_oracle.c")).read()
    for key, (old, new) in MUTANTS.items():
        assert src.count(old) == 1, key
        c = os.path.join(base, "mutant_%d_%d.c" % key)
        with open(c, "w") as f:
            f.write(src.replace(old, new))
        MUTANT_CLI[key] = c[:-2]
        subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-w", "-I" + rl.ORACLE_DIR,
                        "-I" + os.path.join(ROOT, "include"), "-o", MUTANT_CLI[key],
                        os.path.join(rl.ORACLE_DIR, "oracle_cli.c"), c, "-lm"], check=True)


def matters(runner, p, key, det_db):
    """True where no mutant exists for the outcome, or the mutant's store differs"""
    if key not in MUTANT_CLI:
        return True
    runner.serial += 1
    d = os.path.join(runner.base, "w%d_mut" % runner.serial)
    r = rl.run_cli(MUTANT_CLI[key], d, problem_text(p), p["penalty"])
    shutil.rmtree(d)
    return r[".db"] != det_db


def usable(p):
    """the device solves constant data in closed form on the host: keep problems that reach the
    dynamic programme"""
    return len(p["count"]) >= 2 and len(set(p["count"])) > 1 and min(p["width"]) >= 1


def takes(runner, p, key, need_equal_segments, need_matters=False):
    runner.reset()
    r = runner.run(p, ("ref", "det"))
    if r["ref"]["status"] != 0 or r["det"]["status"] != 0:
        return False
    if need_equal_segments and r["ref"]["_segments.bed"] != r["det"]["_segments.bed"]:
        return False
    c = runner.counts()[key]
    if not (c["ref"] > 0 and c["det"] > 0):
        return False
    return not need_matters or matters(runner, p, key, r["det"][".db"])


def shrink(runner, p, key, equal, need_matters=False):
    """drop points, then make widths 1 or halve them, while the outcome stays taken"""
    p = {"count": list(p["count"]), "width": list(p["width"]), "penalty": p["penalty"]}
    changed = True
    while changed:
        changed = False
        i = 0
        while i < len(p["count"]) and len(p["count"]) > 2:
            q = dict(p, count=p["count"][:i] + p["count"][i + 1:], width=p["width"][:i] + p["width"][i + 1:])
            if usable(q) and takes(runner, q, key, equal, need_matters):
                p, changed = q, True
            else:
                i += 1
    for i in range(len(p["width"])):
        for w in (1, p["width"][i] // 2):
            if 1 <= w < p["width"][i]:
                q = dict(p, width=p["width"][:i] + [w] + p["width"][i + 1:])
                if takes(runner, q, key, equal, need_matters):
                    p = q
                    break
    return p


# ---- inputs ------------------------------------------------------------------------------

def baseline_tasks():
    """the inputs the suite's parity tests use, and the ten further fuzz seeds"""
    tasks = [("mono", i) for i in range(13)] + [("fuzz", 5)] + [("varied", i) for i in range(3)]
    tasks += [("increasing", 0)] + [("poisson", i) for i in range(6)] + [("fuzz", s) for s in range(100, 110)]
    return tasks


def baseline_problems(kind, arg):
    import test_gpu_parity as gp
    from peaksegdisk_amd import synthetic
    if kind == "mono":
        text = open(os.path.join(ROOT, "tests", "golden", "Mono27ac.bedGraph")).read()
        yield {"text": text, "penalty": gp.MONO_PENALTIES[arg]}
    elif kind == "fuzz":
        for cnt, wid, _, _, pen in gp.fuzz_cases(300, arg):
            yield {"count": cnt.tolist(), "width": wid.tolist(), "penalty": pen}
    elif kind == "varied":
        for c, (cnt, w, _, _, pens) in enumerate(gp.varied_shape_cases(*gp.VARIED_SHAPES_RUN)):
            if c % 3 == arg:
                for pen in pens:
                    yield {"count": cnt.tolist(), "width": w.tolist(), "penalty": pen}
    elif kind == "increasing":
        cs, ce, cnt = synthetic.increasing_coverage(600)
        for pen in ("100", "10000", "0"):
            yield {"count": cnt.tolist(), "width": (ce - cs).tolist(), "penalty": pen}
    elif kind == "poisson":
        cs, ce, cnt = synthetic.poisson_coverage(20000, seed=11)
        yield {"count": cnt.tolist(), "width": (ce - cs).tolist(),
               "penalty": synthetic.penalty_grid(16)[::3][arg]}


GENERATORS = ["fuzz", "few", "runs", "plateau", "huge", "wide", "zeros", "symmetric", "mixed"]


def merge_cost(a, b, wa, wb):
    """Poisson cost of giving two bins one mean instead of their own"""
    def part(z, w, m):
        return w * (m - (z * np.log(m) if z > 0 else 0.0))
    m = (a * wa + b * wb) / (wa + wb)
    if m <= 0:
        return 0.0
    return float(part(a, wa, m) + part(b, wb, m) - part(a, wa, max(a, 1e-300)) - part(b, wb, max(b, 1e-300)))


def generate(kind, seed, n_problems):
    rng = np.random.default_rng([GENERATORS.index(kind), seed])
    if kind == "fuzz":
        import test_gpu_parity as gp
        for cnt, wid, _, _, pen in gp.fuzz_cases(n_problems, 1000 + seed):
            yield {"count": cnt.tolist(), "width": wid.tolist(), "penalty": pen}
        return
    for _ in range(n_problems):
        small = [0, 1, 2, 3, 5, 8]
        if kind == "few":        # two to twelve points
            n = int(rng.integers(2, 13))
            cnt = rng.choice([rng.integers(0, 4, n), rng.integers(0, 60, n), rng.choice(small, n)])
            wid = rng.choice([np.ones(n, dtype=np.int64), rng.integers(1, 30, n)])
        elif kind == "runs":     # long runs of one count with unequal widths
            k = int(rng.integers(2, 5))
            vals = rng.integers(0, int(rng.choice([3, 10, 1000])), k)
            cnt = np.concatenate([np.full(int(rng.integers(1, 14)), v) for v in vals])[:40]
            wid = rng.integers(1, int(rng.choice([3, 50, 5000])), len(cnt))
        elif kind == "plateau":  # plateaus, then a single step
            a, b = rng.integers(0, 40, 2)
            n = int(rng.integers(3, 30))
            cnt = np.full(n, a)
            cnt[int(rng.integers(1, n)):] = b
            if rng.random() < 0.5:
                cnt[int(rng.integers(0, n))] += int(rng.integers(1, 3))
            wid = rng.choice([np.ones(n, dtype=np.int64), rng.integers(1, 20, n)])
        elif kind == "huge":     # counts up to 2e6 next to 0 and 1
            n = int(rng.integers(2, 25))
            cnt = np.where(rng.random(n) < 0.5, rng.integers(0, 2, n), rng.integers(0, 2000001, n))
            wid = rng.integers(1, 30, n)
        elif kind == "wide":     # widths up to 1e6
            n = int(rng.integers(2, 30))
            cnt = rng.integers(0, int(rng.choice([3, 30, 3000])), n)
            wid = np.where(rng.random(n) < 0.5, rng.integers(1, 1000001, n), rng.integers(1, 4, n))
        elif kind == "zeros":    # leading and trailing zeros
            n = int(rng.integers(1, 20))
            mid = rng.integers(0, int(rng.choice([2, 5, 50])), n)
            cnt = np.concatenate([np.zeros(int(rng.integers(0, 8)), dtype=np.int64), mid,
                                  np.zeros(int(rng.integers(0, 8)), dtype=np.int64)])
            wid = rng.integers(1, int(rng.choice([2, 30])) + 1, len(cnt))
        elif kind == "symmetric":  # a b a and longer palindromes
            h = int(rng.integers(1, 8))
            half = rng.integers(0, int(rng.choice([4, 30, 500])), h + 1)
            cnt = np.concatenate([half, half[-2::-1]])
            w = rng.integers(1, int(rng.choice([2, 20])) + 1, h + 1)
            wid = np.concatenate([w, w[-2::-1]])
            if rng.random() < 0.3:
                cnt = np.tile(cnt, 2)[:40]
                wid = np.tile(wid, 2)[:40]
        else:                    # mixed: small alphabets, repeated blocks, occasional spikes
            n = int(rng.integers(2, 41))
            cnt = rng.choice(small[:int(rng.integers(2, 7))], n)
            if rng.random() < 0.3:
                cnt[int(rng.integers(0, n))] = int(rng.integers(100, 100000))
            wid = rng.choice([np.ones(n, dtype=np.int64), rng.integers(1, 4, n), rng.integers(1, 300, n)])
        cnt = np.asarray(cnt, dtype=np.int64)
        wid = np.asarray(wid, dtype=np.int64)
        u = rng.random()
        if u < 0.2:
            pen = "0"
        elif u < 0.45:
            i = int(rng.integers(0, len(cnt) - 1)) if len(cnt) > 1 else 0
            j = min(i + 1, len(cnt) - 1)
            pen = "%.15g" % abs(int(rng.integers(1, 4)) * merge_cost(float(cnt[i]), float(cnt[j]),
                                                                  float(wid[i]), float(wid[j])))
        elif u < 0.6:
            pen = str(int(rng.integers(1, 20)))
        else:
            pen = "%.15g" % (10.0 ** rng.uniform(-3, 7))
        p = {"count": cnt.tolist(), "width": wid.tolist(), "penalty": pen}
        if usable(p) and np.isfinite(float(pen)):
            yield p


# ---- worker tasks ------------------------------------------------------------------------

def check_against_libm(p, r, bad):
    diff = rl.differences(r["ref"], r["libm"])
    if diff and len(bad) < 20:
        bad.append({"problem": {k: v for k, v in p.items() if k != "text"}, "differs": diff})


def run_baseline(task):
    base = tempfile.mkdtemp(prefix="refbr_")
    try:
        runner = Runner(base)
        bad, n = [], 0
        for p in baseline_problems(*task):
            check_against_libm(p, runner.run(p), bad)
            n += 1
        return n, runner.counts(("ref", "det", "libm")), bad
    finally:
        shutil.rmtree(base, ignore_errors=True)


def run_search(task):
    kind, seed, n_problems, wanted, mutant_cli = task
    wanted = set(map(tuple, wanted))
    MUTANT_CLI.update(mutant_cli)
    base = tempfile.mkdtemp(prefix="refbr_")
    try:
        runner = Runner(base)
        bad, problems = [], []
        for p in generate(kind, seed, n_problems):
            check_against_libm(p, runner.run(p), bad)
            problems.append(p)
        found = {}
        new = runner.taken() & wanted
        if new:  # which problem takes it?  one at a time, with fresh counters
            candidates = {}
            for p in problems:
                runner.reset()
                r = runner.run(p, ("ref", "det"))
                if r["ref"]["status"] != 0 or r["det"]["status"] != 0:
                    continue
                equal = r["ref"]["_segments.bed"] == r["det"]["_segments.bed"]
                for key in runner.taken() & new:
                    best = candidates.get(key)
                    m = matters(runner, p, key, r["det"][".db"])
                    rank = (not m, not equal, len(p["count"]))
                    if best is None or rank < best[0]:
                        candidates[key] = (rank, p, equal, m)
            for key, (_, p, equal, m) in candidates.items():
                found[key] = (shrink(runner, p, key, equal, m), equal, kind, m)
        return len(problems), found, bad
    finally:
        shutil.rmtree(base, ignore_errors=True)


# ---- search ------------------------------------------------------------------------------

def record_case(name, p, keys, work):
    text = problem_text(p)
    ref = rl.run_cli(rl.REF_CLI, os.path.join(work, name + "_ref"), text, p["penalty"])
    det = rl.run_cli(rl.ORACLE_CLI_DET, os.path.join(work, name + "_det"), text, p["penalty"])
    assert ref["status"] == 0 and det["status"] == 0
    end = np.cumsum(p["width"])
    outcomes = []
    for key in sorted(keys):
        fun, words = outcome_words(key)
        outcomes.append({"function": fun, "reference_line": key[0], "branch": key[1], "outcome": words})
    return {"name": name, "outcomes": outcomes,
            "chromStart": (end - np.asarray(p["width"])).tolist(), "chromEnd": end.tolist(),
            "count": list(p["count"]), "penalty": p["penalty"],
            "segments": ref["_segments.bed"].decode(), "loss_row": ref["_loss.tsv"].decode(),
            "db_size": len(ref[".db"]), "db_sha256": rl.sha256(ref[".db"]),
            "det_segments_equal_reference": ref["_segments.bed"] == det["_segments.bed"]}


def search(args):
    rl.build_reference(("ref", "cov"))
    subprocess.run(["make", "-s", "-C", rl.ORACLE_DIR], check=True)
    t0 = time.time()
    mutant_dir = tempfile.mkdtemp(prefix="refbr_mut_")
    build_mutants(mutant_dir)
    pool = multiprocessing.Pool(min(16, args.procs))
    total = {key: {"ref": 0, "det": 0, "libm": 0} for key in all_outcomes()}
    n_baseline, bad = 0, []
    for n, counts, b in pool.imap_unordered(run_baseline, baseline_tasks()):
        n_baseline += n
        bad += b
        for key, c in counts.items():
            for kind in c:
                total[key][kind] += c[kind]
    # same algorithm, same inputs, same arithmetic: the libm oracle must take every mirrored
    # branch exactly as often as the reference, or DECISIONS pairs the wrong lines.  (getCost is
    # called more often by the reference, which also evaluates what only its verbose mode prints.)
    mapping_errors = [key for key, c in total.items()
                      if c["ref"] != c["libm"] and outcome_words(key)[0] != "getCost"]
    if mapping_errors:
        print("reference and libm oracle counts differ at", mapping_errors, file=sys.stderr)
    wanted = {key for key, c in total.items() if not (c["ref"] > 0 and c["det"] > 0)}
    table = sorted(wanted)
    print("baseline: %d problems, %d of %d outcomes untaken (%.0f s)"
          % (n_baseline, len(wanted), len(total), time.time() - t0), flush=True)
    found, n_search, rnd = {}, 0, 0
    while n_search < args.problems and (wanted - set(UNREACHABLE)):
        tasks = [(GENERATORS[(rnd * args.procs + i) % len(GENERATORS)], rnd * args.procs + i,
                  args.batch, sorted(wanted), dict(MUTANT_CLI)) for i in range(args.procs)]
        rnd += 1
        for n, f, b in pool.imap_unordered(run_search, tasks):
            n_search += n
            bad += b
            for key, (p, equal, kind, m) in f.items():
                old = found.get(key)
                rank = (not m, not equal, len(p["count"]))
                if old is None or rank < old[0]:
                    found[key] = (rank, p, equal, kind)
                    if equal and m:
                        wanted.discard(key)
                    print("  %s line %d branch %d: %d points, penalty %s, %s generator%s%s"
                          % (outcome_words(key)[0], key[0], key[1], len(p["count"]), p["penalty"], kind,
                             "" if equal else " (det segments differ)",
                             "" if m else " (leaves the store unchanged)"), flush=True)
        print("searched %d problems, %d outcomes left (%.0f s)" % (n_search, len(wanted), time.time() - t0),
              flush=True)
    pool.close()
    inert = sorted(key for key, v in found.items() if v[0][0])
    shutil.rmtree(mutant_dir, ignore_errors=True)
    # one fixture case per distinct problem
    by_problem = {}
    for key, (_, p, equal, kind) in found.items():
        by_problem.setdefault(json.dumps(p, sort_keys=True), (p, []))[1].append(key)
    work = tempfile.mkdtemp(prefix="refbr_rec_")
    cases = []
    for p, keys in sorted(by_problem.values(), key=lambda v: min(v[1])):
        fun = outcome_words(min(keys))[0]
        cases.append(record_case("%s_%d_%d" % (fun, min(keys)[0], min(keys)[1]), p, keys, work))
    shutil.rmtree(work, ignore_errors=True)
    rows = []
    for key in table:
        fun, words = outcome_words(key)
        row = {"function": fun, "reference_line": key[0], "branch": key[1], "outcome": words}
        names = [c["name"] for c in cases if any((o["reference_line"], o["branch"]) == key for o in c["outcomes"])]
        if names:
            row["fixture"] = names[0]
        else:
            row["not_reached_in"] = n_search + n_baseline
        rows.append(row)
    doc = {"about": "inputs that take outcomes of the reference's piece algebra which the suite's other "
                    "inputs never take; written by tools/reference_branches.py --search; data only",
           "search": {"date": args.date, "baseline_problems": n_baseline, "search_problems": n_search,
                      "oracle_libm_disagreements": bad,
                      "taken_without_changing_the_store": [list(k) for k in inert]},
           "table": rows, "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s: %d cases, %d of %d outcomes reached, %d libm disagreements"
          % (args.out, len(cases), sum("fixture" in r for r in rows), len(rows), len(bad)))
    return 1 if bad or mapping_errors else 0


def report(args):
    doc = rl.load_branch_fixture() if args.out == rl.BRANCH_FIXTURE else json.load(open(args.out))
    s = doc["search"]
    n = s["baseline_problems"] + s["search_problems"]
    if args.markdown:
        print("| Function | Reference line | Outcome that the other inputs never take | Fixture |")
        print("|---|---|---|---|")
    for r in doc["table"]:
        if "fixture" in r:
            what = "`%s`" % r["fixture"] if args.markdown else r["fixture"]
        else:
            what = "not reached in %d problems (%s)" % (r["not_reached_in"], s["date"])
            if (r["reference_line"], r["branch"]) in UNREACHABLE:
                what += ": " + UNREACHABLE[(r["reference_line"], r["branch"])]
        if args.markdown:
            print("| `%s` | %d | %s | %s |" % (r["function"], r["reference_line"], r["outcome"], what))
        else:
            print("%-20s %5d  %-75s %s" % (r["function"], r["reference_line"], r["outcome"], what))
    print()
    print("%d problems (%d baseline + %d searched, %s); %d outcomes in the table, %d reached by a fixture; "
          "%d cases whose det segments differ from the reference; %d disagreements of the libm oracle"
          % (n, s["baseline_problems"], s["search_problems"], s["date"], len(doc["table"]),
             sum("fixture" in r for r in doc["table"]),
             sum(not c["det_segments_equal_reference"] for c in doc["cases"]),
             len(s["oracle_libm_disagreements"])))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--problems", type=int, default=200000)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--procs", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--date", default=time.strftime("%Y-%m-%d"))
    ap.add_argument("--out", default=rl.BRANCH_FIXTURE)
    args = ap.parse_args()
    if args.search:
        return search(args)
    if args.report:
        return report(args)
    ap.print_help()
    return 2


if __name__ == "__main__":
    sys.exit(main())
