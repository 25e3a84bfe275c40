"""The host side of the coverage features, without any device: features_from_stats (the 36
columns from integers), predict_penalties (the arithmetic, paste, the refusals), and the argument
check of PeakSegFPOP_dense / PeakSegFPOP_reads that precedes all device work."""
import math

import numpy as np
import pandas as pd
import pytest


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    return peaksegdisk_amd


BASE = ["quartile.0%", "quartile.25%", "quartile.50%", "quartile.75%", "quartile.100%", "mean", "sd",
        "bases", "data"]
NAMES = BASE + ["log+1." + n for n in BASE] + ["log." + n for n in BASE] + ["log.log." + n for n in BASE]


def same(got, want):
    """equal bit for bit, NaN where NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def test_feature_names_and_order(psd):
    from peaksegdisk_amd import grid
    assert len(NAMES) == 36 and len(grid.BASE_FEATURES) == 9
    # nine base features -- the five quartiles, mean, sd, bases, data -- under four transforms
    assert list(grid.BASE_FEATURES) == BASE
    assert list(grid.FEATURE_NAMES) == NAMES
    assert psd.features_from_stats is grid.features_from_stats


def test_worked_example(psd):
    x = np.array([1, 3, 0, 4, 2])
    srt = np.sort(x)
    lo, hi, g = [0, 1, 2, 3, 4], [1, 2, 3, 4, 4], [0.0] * 5
    from peaksegdisk_amd.grid import quartile_ranks
    assert quartile_ranks(5) == (lo, hi, g)
    f = psd.features_from_stats(srt[lo], srt[hi], 5, 5, int(x.sum()), int((x ** 2).sum()))
    assert f.dtype == np.float64 and f.shape == (len(NAMES),)
    base = np.array([0, 1, 2, 3, 4, 2, math.sqrt(2.5), 5, 5], dtype=np.float64)
    assert same(f[:9], base)
    with np.errstate(all="ignore"):
        assert same(f[9:18], np.log(base + 1))
        assert same(f[18:27], np.log(base))
        assert same(f[27:], np.log(np.log(base)))
    # minimum 0: log.quartile.0% is -inf, log.log.quartile.0% is NaN; log.log.quartile.25% is -inf
    at = dict(zip(NAMES, f.tolist()))
    assert at["log.quartile.0%"] == -math.inf and math.isnan(at["log.log.quartile.0%"])
    assert at["log+1.quartile.0%"] == 0.0 and at["log.log.quartile.25%"] == -math.inf
    assert f[6] == np.std(x, ddof=1)


def test_interpolated_quartiles_and_one_base(psd):
    from peaksegdisk_amd.grid import quartile_ranks
    x = np.array([7, 0, 2 ** 31 - 1, 5, 5, 9, 1, 1], dtype=np.int64)   # B - 1 = 7: g = 0, .75, .5, .25, 0
    srt = np.sort(x)
    lo, hi, g = quartile_ranks(len(x))
    assert lo == [0, 1, 3, 5, 7] and hi == [1, 2, 4, 6, 7] and g == [0.0, 0.75, 0.5, 0.25, 0.0]
    s1, s2 = sum(int(v) for v in x), sum(int(v) ** 2 for v in x)
    f = psd.features_from_stats(srt[lo], srt[hi], len(x), 7, s1, s2)
    assert same(f[:5], np.quantile(x, [0, .25, .5, .75, 1]))
    assert f[5] == s1 / len(x) and f[7] == 8.0 and f[8] == 7.0
    assert abs(f[6] - np.std(x.astype(np.float64), ddof=1)) <= 1e-9 * f[6]
    one = psd.features_from_stats([4] * 5, [4] * 5, 1, 1, 4, 16)     # B = 1
    assert same(one[:9], [4, 4, 4, 4, 4, 4, math.nan, 1, 1])
    assert math.isnan(one[NAMES.index("log.sd")]) and one[NAMES.index("log.bases")] == 0.0
    assert one[NAMES.index("log.log.bases")] == -math.inf


def frame(rows):
    return pd.DataFrame(np.array(rows, dtype=np.float64), columns=NAMES)


def test_predict_penalties(psd):
    x = np.array([1, 3, 0, 4, 2])
    srt = np.sort(x)
    f0 = psd.features_from_stats(srt[[0, 1, 2, 3, 4]], srt[[1, 2, 3, 4, 4]], 5, 5, 10, 30)
    f1 = psd.features_from_stats([2, 2, 3, 3, 9], [2, 3, 3, 9, 9], 5, 3, 19, 107)
    table = frame([f0, f1])
    model = {"intercept": 0.25, "weights": {"log.bases": 1.5, "log+1.quartile.75%": -0.5, "mean": 0.125,
                                            "log.quartile.0%": 0.0}}
    got = psd.predict_penalties(table, model)
    assert got.dtype == np.float64 and got.shape == (2,)
    for row, f in enumerate((f0, f1)):
        log_pen = 0.25
        for name, w in model["weights"].items():
            if w != 0.0:
                log_pen += w * f[NAMES.index(name)]
        want = float(np.exp(np.float64(log_pen)))
        assert got[row] == float(psd.paste(want))           # 15 significant digits
        assert abs(got[row] - want) <= 1e-14 * want
        assert psd.paste(float(got[row])) == psd.paste(want)    # the round trip is stable
        assert float(psd.paste(float(got[row]))) == got[row]
    # a weight on a feature that is not finite for contig 0
    for name in ("log.quartile.0%", "log.log.quartile.0%"):
        with pytest.raises(ValueError) as ei:
            psd.predict_penalties(table, {"intercept": 0.0, "weights": {name: 1.0}})
        assert "contig 0" in str(ei.value) and name in str(ei.value)
    with pytest.raises(ValueError, match="no.such.feature"):
        psd.predict_penalties(table, {"intercept": 0.0, "weights": {"no.such.feature": 1.0}})
    with pytest.raises(ValueError, match="no.such.feature"):     # (even with weight zero)
        psd.predict_penalties(table, {"intercept": 0.0, "weights": {"no.such.feature": 0.0}})
    assert psd.predict_penalties(table, {"intercept": 0.0, "weights": {}}).tolist() == [1.0, 1.0]


def test_exactly_one_of_penalties_and_model(psd, monkeypatch):
    """both, or neither, is refused before any device work: the set constructors are never reached"""
    from peaksegdisk_amd import grid

    def never(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(grid.ProblemSet, "from_dense", classmethod(never))
    monkeypatch.setattr(grid.ProblemSet, "from_reads", classmethod(never))
    v = np.array([1, 1, 5, 5, 0], np.int32)
    reads = (np.array([0, 2], np.int32), np.array([3, 5], np.int32))
    model = {"intercept": 1.0, "weights": {"log.bases": 1.0}}
    for call, data in ((psd.PeakSegFPOP_dense, v), (psd.PeakSegFPOP_reads, reads)):
        with pytest.raises(ValueError, match="exactly one"):
            call(data)
        with pytest.raises(ValueError, match="exactly one"):
            call(data, [1.0], penalty_model=model)
        with pytest.raises(ValueError, match="exactly one"):
            call(data, penalties=None, penalty_model=None)
        with pytest.raises(ValueError, match="unknown feature"):
            call(data, penalty_model={"intercept": 1.0, "weights": {"log.base": 1.0}})
