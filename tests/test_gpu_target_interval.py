"""targetInterval_dense / targetInterval_reads: the interval of log(penalty) with the fewest label
errors, found with several models per round on a resident problem set.

The scenario functions are shared with the emulator rehearsal (tests/test_target_interval_emu.py).
What a search reports is checked against models solved afresh and the brute-force yardstick of
tests/test_gpu_label_errors.py: every row's errors on that row's own segments table, and the
claims an interval makes -- just inside an exact limit the errors are min_errors, just outside
they are more, and in the middle they are min_errors."""
import math

import numpy as np
import pytest

from test_gpu_dense import as_numpy, mono27ac_dense
from test_gpu_label_errors import brute_force, golden_labels, random_labels

GPU = pytest.mark.gpu
MAX_ROUNDS = 20


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    from peaksegdisk_amd import _native
    assert _native.lib.peakseg_hip_device_count() >= 1, "no HIP device: GPU tests need an MI355X"
    return peaksegdisk_amd


def yardstick_errors(psd, dense, labels, first, penalties):
    """[errors, fp, fn] of the models of `penalties`, each solved afresh and counted by brute force"""
    pset = psd.ProblemSet.from_dense([as_numpy(dense)], [(0, float(p)) for p in penalties])
    try:
        pset.solve()
        columns = pset.segment_columns(first_chromStart=[first])
    finally:
        pset.close()
    return [brute_force(c, labels)[3][:3] for c in columns]


def check_interval(psd, dense, labels, first, width, middle=True):
    """scenario 1 on one labelled contig; -> the TargetInterval.  middle: also solve a penalty
    well inside the interval.  The search proves the two ends of the interval, not that no model
    of more errors hides between two neighbouring models of the run, so
    that check belongs to data where the run is known: Mono27ac."""
    res = psd.targetInterval_dense(as_numpy(dense), labels, width=width, max_rounds=MAX_ROUNDS,
                                   chrom_starts=[first])
    models = res.models
    print("width %d: %r\n%s" % (width, res, models.sort_values("penalty").to_string()))
    assert list(models.columns) == ["penalty", "peaks", "total.loss", "errors", "fp", "fn", "round"]
    assert res.rounds < MAX_ROUNDS and res.rounds == int(models["round"].max())
    assert models["penalty"].is_unique and set(models["penalty"][models["round"] == 1]) == {0.0, math.inf}
    assert int(models["errors"].min()) == res.min_errors           # no model has fewer
    assert res.min_log_lambda < res.max_log_lambda
    for limit, exact in ((res.min_log_lambda, res.lower_exact), (res.max_log_lambda, res.upper_exact)):
        assert exact, "the search ended before max_rounds: both limits are exact"
    # what to solve afresh: every row's penalty, the neighbours of the finite limits, the middle
    lo, hi = res.min_log_lambda, res.max_log_lambda
    extra = []
    if math.isfinite(lo):
        extra += [("outside", math.exp(lo) * (1 - 1e-6)), ("inside", math.exp(lo) * (1 + 1e-6))]
    if math.isfinite(hi):
        extra += [("inside", math.exp(hi) * (1 - 1e-6)), ("outside", math.exp(hi) * (1 + 1e-6))]
    if not middle:
        pass
    elif math.isfinite(lo) and math.isfinite(hi):
        extra.append(("inside", math.exp((lo + hi) / 2)))
    elif math.isfinite(lo):
        extra.append(("inside", math.exp(lo) * 4))
    elif math.isfinite(hi):
        extra.append(("inside", math.exp(hi) / 4))
    else:
        extra.append(("inside", 1.0))
    pens = models["penalty"].tolist()
    want = yardstick_errors(psd, dense, labels, first, pens + [p for _, p in extra])
    got = models[["errors", "fp", "fn"]].values.tolist()
    assert got == want[:len(pens)]
    for (side, pen), (errors, _, _) in zip(extra, want[len(pens):]):
        if side == "inside":
            assert errors == res.min_errors, (side, pen, errors, res.min_errors)
        else:
            assert errors > res.min_errors, (side, pen, errors, res.min_errors)
    return res


def small_contig(seed, n=1500):
    from peaksegdisk_amd import synthetic
    return synthetic.poisson_coverage(n, seed=seed)[2].astype(np.int32)


def small_labels(seed, n_bases, first):
    return random_labels(np.random.default_rng(seed), 12, first, first + n_bases - 60, 120)


# ---- the scenarios ---------------------------------------------------------------------------

def scenario_mono27ac_width8(psd):
    res = check_interval(psd, mono27ac_dense(), golden_labels()[0], 60000, 8)
    assert res.min_errors == 0 and math.isfinite(res.min_log_lambda + res.max_log_lambda)


def scenario_mono27ac_width1(psd):
    res = check_interval(psd, mono27ac_dense(), golden_labels()[0], 60000, 1)
    assert res.min_errors == 0 and math.isfinite(res.min_log_lambda + res.max_log_lambda)
    assert (res.models["round"].value_counts().drop(1) == 1).all()    # one model per round


def scenario_small_contig_widths(psd):
    dense = small_contig(31)
    labels = small_labels(32, len(dense), 500)
    found = [check_interval(psd, dense, labels, 500, width, middle=False) for width in (1, 3, 8)]
    # (The widths need not agree on the interval: each reports the widest run among the models
    # it met, and a wider round steps over models a narrower one lands on.  DESIGN.md section 12.)
    assert len(found) == 3


def scenario_no_labels(psd):
    dense = small_contig(33)
    for labels in (None, ()):
        res = psd.targetInterval_dense(as_numpy(dense), labels, width=4)
        assert (res.min_log_lambda, res.max_log_lambda) == (-math.inf, math.inf)
        assert res.lower_exact and res.upper_exact and res.min_errors == 0 and res.rounds == 1
        assert res.models["penalty"].tolist() == [0.0, math.inf]
        assert res.models[["errors", "fp", "fn"]].values.tolist() == [[0, 0, 0]] * 2
        assert res.models["peaks"].iloc[0] > 0 and res.models["peaks"].iloc[1] == 0


def scenario_lockstep(psd):
    vectors = [small_contig(34), small_contig(35, 900)]
    firsts = [0, 7000]
    labels = [small_labels(36, len(vectors[0]), 0), small_labels(37, len(vectors[1]), 7000)]
    both = psd.targetInterval_dense([as_numpy(v) for v in vectors], labels, width=4,
                                    chrom_starts=firsts)
    assert len(both) == 2
    for c in range(2):
        alone = psd.targetInterval_dense(as_numpy(vectors[c]), labels[c], width=4,
                                         chrom_starts=[firsts[c]])
        for name in ("min_log_lambda", "max_log_lambda", "lower_exact", "upper_exact", "min_errors",
                     "rounds"):
            assert getattr(both[c], name) == getattr(alone, name), (c, name)
        assert both[c].models.equals(alone.models), c
    assert both[0].rounds > 1 or both[1].rounds > 1


def scenario_constant(psd):
    dense = np.full(1000, 3, np.int32)
    labels = (np.array([10, 500], np.int32), np.array([90, 600], np.int32), ["peaks", "noPeaks"])
    res = psd.targetInterval_dense(dense, labels, width=8)
    assert (res.min_log_lambda, res.max_log_lambda) == (-math.inf, math.inf)
    assert res.rounds == 1 and res.min_errors == 1 and res.lower_exact and res.upper_exact
    assert res.models["peaks"].tolist() == [0, 0]
    assert res.models[["errors", "fp", "fn"]].values.tolist() == [[1, 0, 1]] * 2


def scenario_reads(psd):
    """targetInterval_reads is targetInterval_dense on the piled-up coverage"""
    from peaksegdisk_amd import synthetic
    start, end, extent = synthetic.poisson_reads(120, seed=3)
    cover = psd.coverage_from_reads(start, end, extent=extent)
    dense = np.repeat(cover["count"].to_numpy(), (cover["chromEnd"] - cover["chromStart"]).to_numpy())
    labels = small_labels(38, len(dense), extent[0])
    a = psd.targetInterval_reads((start, end), labels, width=4, extents=extent)
    b = psd.targetInterval_dense(dense.astype(np.int32), labels, width=4, chrom_starts=[extent[0]])
    assert (a.min_log_lambda, a.max_log_lambda, a.min_errors) == \
        (b.min_log_lambda, b.max_log_lambda, b.min_errors)
    assert a.models.equals(b.models)


def scenario_arguments(psd):
    dense = small_contig(33, 400)
    with pytest.raises(ValueError, match="width"):
        psd.targetInterval_dense(dense, None, width=257)
    with pytest.raises(ValueError, match="max_rounds"):
        psd.targetInterval_dense(dense, None, max_rounds=0)
    with pytest.raises(ValueError, match="one entry per contig"):
        psd.targetInterval_dense([dense, dense], [None])
    with pytest.raises(psd.PeakSegError) as ei:
        psd.targetInterval_dense(-dense - 1, None)
    assert ei.value.status == 17


SCENARIOS = [scenario_mono27ac_width8, scenario_mono27ac_width1, scenario_small_contig_widths,
             scenario_no_labels, scenario_lockstep, scenario_constant, scenario_reads,
             scenario_arguments]


@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_target_interval(psd, scenario):
    scenario(psd)
