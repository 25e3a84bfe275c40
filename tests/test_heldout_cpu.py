"""Host-only logic of the penalty selection (peaksegdisk_amd/heldout.py): HeldoutSelection on
hand-made tables -- ties, a +Inf fold, all +Inf, the 1se rule, the K / (K - 1) factor --, the pairs
and the layout indices of the definition, the argument checks that need no device, and the
yardsticks of tests/heldout_ref.py against closed forms."""
import math

import numpy as np
import pytest

from heldout_ref import (dense_folds_ref, heldout_pair_ref, n_add, pileup_ref, read_folds_ref)

INF = float("inf")


@pytest.fixture(scope="module")
def heldout():
    import __graft_entry__ as entry
    entry.build_hip()  # the package refuses to import without its HIP library
    from peaksegdisk_amd import heldout
    return heldout


def selection(heldout, penalties, loss, rule="min"):
    loss = np.asarray(loss, dtype=np.float64)          # [folds, penalties]
    folds = loss.shape[0]
    peaks = np.tile(np.arange(len(penalties), 0, -1), (folds, 1))
    return heldout.HeldoutSelection(penalties, folds, peaks, 2 * peaks + 1, loss,
                                    ~np.isfinite(loss), rule)


def test_min_rule_and_factor(heldout):
    pens = [0.0, 1.0, 10.0, 100.0]
    sel = selection(heldout, pens, [[9.0, 5.0, 3.0, 8.0], [9.0, 6.0, 2.5, 8.0], [8.0, 5.0, 3.5, 9.0]])
    assert sel.train_index == 2 and sel.train_penalty == 10.0 and sel.folds == 3
    assert sel.penalty == 10.0 * 3 / 2
    assert sel.summary["heldout_loss"].tolist() == [26.0, 16.0, 9.0, 25.0]
    assert sel.summary["peaks"].tolist() == [4.0, 3.0, 2.0, 1.0]
    se = np.std([3.0, 2.5, 3.5], ddof=1) * math.sqrt(3)
    assert sel.summary["se"][2] == pytest.approx(se, rel=1e-15)
    assert list(sel.table.columns) == ["penalty", "fold", "peaks", "segments", "heldout_loss",
                                       "zero_mean_rows"]
    assert sel.table["fold"].tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert sel.table["penalty"].tolist() == pens * 3
    assert sel.table["segments"].tolist() == [9, 7, 5, 3] * 3
    for folds in (2, 4, 8):
        loss = np.tile([5.0, 1.0, 7.0], (folds, 1))
        assert selection(heldout, [1.0, 3.0, 9.0], loss).penalty == 3.0 * folds / (folds - 1)


def test_ties_take_the_larger_penalty(heldout):
    pens = [1.0, 100.0, 10.0, 1000.0]
    sel = selection(heldout, pens, [[2.0, 1.0, 1.0, 3.0], [2.0, 1.5, 1.5, 3.0]])
    assert sel.train_index == 1 and sel.train_penalty == 100.0
    sel = selection(heldout, pens, [[1.0] * 4, [2.0] * 4])
    assert sel.train_penalty == 1000.0


def test_an_infinite_fold_never_wins(heldout):
    pens = [0.0, 5.0, 50.0]
    sel = selection(heldout, pens, [[-100.0, 4.0, 6.0], [INF, 4.0, 6.0]])
    assert sel.summary["heldout_loss"].tolist() == [INF, 8.0, 12.0]
    assert sel.summary["se"][0] == INF and sel.train_penalty == 5.0
    assert sel.table["zero_mean_rows"].tolist() == [0, 0, 0, 1, 0, 0]
    assert selection(heldout, pens, [[-100.0, 4.0, 6.0], [INF, 4.0, 6.0]], "1se").train_penalty >= 5.0


def test_all_infinite(heldout):
    pens = [0.0, 50.0, 5.0]
    for rule in ("min", "1se"):
        sel = selection(heldout, pens, [[INF, 1.0, INF], [2.0, INF, INF]], rule)
        assert sel.train_penalty == 50.0 and sel.penalty == 100.0


def test_one_standard_error(heldout):
    pens = [1.0, 10.0, 100.0, 1000.0]
    loss = [[10.0, 8.0, 8.5, 20.0], [12.0, 10.0, 10.5, 22.0], [11.0, 9.0, 9.5, 21.0]]
    assert selection(heldout, pens, loss).train_penalty == 10.0
    sel = selection(heldout, pens, loss, "1se")     # sums 33, 27, 28.5, 63; se of 27: sqrt(3)
    assert sel.summary["se"][1] == pytest.approx(math.sqrt(3.0), rel=1e-15)
    assert sel.train_penalty == 100.0 and sel.rule == "1se"
    tight = [[10.0, 8.0, 8.5, 20.0], [10.0, 8.0, 8.5, 20.0]]      # no spread: nothing is within it
    assert selection(heldout, pens, tight, "1se").train_penalty == 10.0
    with pytest.raises(ValueError, match="rule"):
        selection(heldout, pens, loss, "2se")


def test_pairs_and_layout(heldout):
    from peaksegdisk_amd import ProblemSet
    n, folds, pens = 3, 4, [0.0, 2.0, 7.0, 9.0, 11.0]
    problem, contig, scale = heldout.selection_pairs(n, folds, len(pens))
    assert problem.dtype == np.int32 and contig.dtype == np.int32 and scale.dtype == np.float64
    assert len(problem) == n * folds * len(pens) and (scale == 1.0 / 3.0).all()
    pset = ProblemSet.__new__(ProblemSet)
    pset._h = None
    pset._fold_layout(n, pens, folds, "test")
    at = 0
    for i in range(n):
        for f in range(folds):
            assert pset.fold_contig(i, f) == (i * folds + f) * 2
            assert pset.fold_contig(i, f, test=True) == (i * folds + f) * 2 + 1
            for j in range(len(pens)):
                assert pset.fold_problem(i, f, j) == at == problem[at]
                assert pset.problems[at] == (pset.fold_contig(i, f), pens[j])
                assert contig[at] == pset.fold_contig(i, f, test=True)
                at += 1
    with pytest.raises(IndexError):
        pset.fold_contig(3, 0)
    with pytest.raises(IndexError):
        pset.fold_problem(0, 4, 0)


def test_arguments_checked_before_the_device():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    v = np.arange(10, dtype=np.int32)
    with pytest.raises(ValueError, match="rule"):
        psd.select_penalty_dense(v, [1.0], rule="best")
    with pytest.raises(ValueError, match="penalties"):
        psd.select_penalty_dense(v, [])
    with pytest.raises(ValueError, match="penalties"):
        psd.select_penalty_dense(v, None)
    with pytest.raises(ValueError, match="non-negative"):
        psd.select_penalty_reads((v, v + 5), [-1.0])
    with pytest.raises(TypeError):
        psd.select_penalty_dense(v)                     # penalties is required


def test_loss_yardstick_closed_forms():
    vector = np.array([0, 0, 4, 4, 4, 4, 0, 1], dtype=np.int32)
    cols = (np.array([6, 2, 0]), np.array([8, 6, 2]), np.array([0.5, 4.0, 0.0]))
    ref = heldout_pair_ref(cols, vector, 0.5)
    want = [0.25 * 2 - 1 * math.log(0.25), 2.0 * 4 - 16 * math.log(2.0), 0.0]
    assert ref["loss"] == math.fsum(want) and ref["zero_mean_rows"] == 0
    assert (ref["rows"], ref["bases"], ref["sum"]) == (3, 8, 17)
    weight = 0.5 + 1 * (abs(math.log(0.25)) + 1) + 8.0 + 16 * (math.log(2.0) + 1)
    assert ref["tol"] == pytest.approx((n_add(3) + 6) * 2.0 ** -52 * weight, rel=1e-14)
    assert [n_add(r) for r in (1, 256, 257, 512, 513)] == [10, 10, 11, 11, 12]
    loud = vector.copy()
    loud[1] = 2
    ref = heldout_pair_ref(cols, loud, 1.0)
    assert ref["loss"] == INF and ref["zero_mean_rows"] == 1 and ref["sum"] == 19


def test_fold_yardsticks():
    v = np.array([0, 1, 64, 65, 21, 22, 1000], dtype=np.int32)
    for folds in (2, 4, 8):
        t = dense_folds_ref(v, 0, folds, 1)
        assert t.shape == (folds, len(v)) and np.array_equal(t.sum(axis=0), v) and (t >= 0).all()
        assert not np.array_equal(t, dense_folds_ref(v, 1, folds, 1))
        assert not np.array_equal(t, dense_folds_ref(v, 0, folds, 2))
        fold = read_folds_ref(500, 0, folds, 1)
        assert fold.min() == 0 and fold.max() == folds - 1
        assert np.bincount(fold, minlength=folds).min() > 500 / folds / 2
    # the K = 2 count of fold 1 is a popcount of the word's low bits
    from peaksegdisk_amd.synthetic import splitmix64
    from heldout_ref import contig_seed
    h = splitmix64(contig_seed(1, 0), np.arange(7, dtype=np.uint64))
    word = int(splitmix64(h[2], np.zeros(1, dtype=np.uint64))[0])
    assert dense_folds_ref(v, 0, 2, 1)[1, 2] == bin(word).count("1")
    word = int(splitmix64(h[4], np.zeros(1, dtype=np.uint64))[0])
    assert dense_folds_ref(v, 0, 2, 1)[1, 4] == bin(word & ((1 << 21) - 1)).count("1")
    cov = pileup_ref(np.array([5, 0, 18]), np.array([12, 3, 30]), np.array([1, 2, 3]), 2, 20)
    assert cov.tolist() == [2] + [0] * 2 + [1] * 7 + [0] * 6 + [3] * 2
    cov = pileup_ref(np.array([5, 0, 18]), np.array([12, 3, 30]), np.array([1, 2, 3]), 2, 20, "end")
    assert cov.tolist() == [2] + [0] * 8 + [1] + [0] * 8
