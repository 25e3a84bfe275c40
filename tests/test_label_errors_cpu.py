"""The yardstick of the label-error tests, pinned on cases written out by hand (no device, no
emulator), and read_labels_bed on the golden labels.  brute_force() of
tests/test_gpu_label_errors.py is what the device's counts are compared with; here each of its
answers is spelled out.  The model has one peak, [10, 20), on a contig [0, 30)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_label_errors import NO_PEAKS, PEAK_END, PEAK_START, PEAKS, brute_force

# segment_columns() of the model background [0, 10), peak [10, 20), background [20, 30): last first
ONE_PEAK = (np.array([20, 10, 0], np.int32), np.array([30, 20, 10], np.int32))
TWO_PEAKS = (np.array([40, 30, 20, 10, 0], np.int32), np.array([50, 40, 30, 20, 10], np.int32))
NO_PEAK = (np.array([0], np.int32), np.array([30], np.int32))

CORRECT, FALSE_POSITIVE, FALSE_NEGATIVE = (0, 0), (1, 0), (0, 1)

CASES = [   # (model, annotation, chromStart, chromEnd, count, (fp, fn))
    (ONE_PEAK, PEAK_START, 10, 15, 1, CORRECT),          # the start is the label's first base
    (ONE_PEAK, PEAK_START, 5, 10, 0, FALSE_NEGATIVE),    # the label ends where the peak starts
    (ONE_PEAK, PEAK_END, 15, 20, 1, CORRECT),            # the peak's last base, 19, is in the label
    (ONE_PEAK, PEAK_END, 20, 25, 0, FALSE_NEGATIVE),     # base 19 is not
    (ONE_PEAK, NO_PEAKS, 20, 25, 0, CORRECT),            # no overlap: the peak ends at 20
    (ONE_PEAK, NO_PEAKS, 19, 25, 1, FALSE_POSITIVE),     # base 19 is shared
    (ONE_PEAK, PEAKS, 12, 13, 1, CORRECT),               # a peak that spans the whole label
    (ONE_PEAK, PEAKS, 0, 10, 0, FALSE_NEGATIVE),
    (ONE_PEAK, PEAKS, 20, 30, 0, FALSE_NEGATIVE),
    (TWO_PEAKS, PEAK_START, 5, 35, 2, FALSE_POSITIVE),   # over two starts, 10 and 30
    (TWO_PEAKS, PEAK_END, 15, 45, 2, FALSE_POSITIVE),    # over two ends, 20 and 40
    (TWO_PEAKS, PEAK_START, 11, 30, 0, FALSE_NEGATIVE),  # between the starts
    (TWO_PEAKS, NO_PEAKS, 0, 50, 2, FALSE_POSITIVE),
    (TWO_PEAKS, PEAKS, 19, 31, 2, CORRECT),
    (TWO_PEAKS, NO_PEAKS, 20, 30, 0, CORRECT),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-%d-%d" % (c[1], c[2], c[3]))
def test_yardstick_on_hand_written_cases(case):
    model, annotation, ls, le, count, (fp, fn) = case
    got = brute_force(model, ([ls], [le], [annotation]))
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == ([count], [fp], [fn])
    assert got[3] == [fp + fn, fp, fn, int(annotation != PEAKS), int(annotation != NO_PEAKS)]


@pytest.mark.parametrize("annotation", [NO_PEAKS, PEAK_START, PEAK_END, PEAKS])
def test_yardstick_model_without_peaks(annotation):
    got = brute_force(NO_PEAK, ([3], [17], [annotation]))
    assert got[0].tolist() == [0] and got[1].tolist() == [0]
    assert got[2].tolist() == [int(annotation != NO_PEAKS)]


def test_yardstick_sums_over_labels():
    starts, ends, codes = zip(*[(c[2], c[3], c[1]) for c in CASES if c[0] is ONE_PEAK])
    got = brute_force(ONE_PEAK, (starts, ends, codes))
    assert got[3] == [5, 1, 4, 6, 7]


def test_read_labels_bed_on_the_golden_file(tmp_path):
    from peaksegdisk_amd import read_labels_bed
    (start, end, codes), chrom = read_labels_bed(os.path.join(GOLDEN, "Mono27ac.labels.bed"))
    assert chrom == ["chr11"] * 6
    assert [a.dtype for a in (start, end, codes)] == [np.int32] * 3
    assert codes.tolist() == [NO_PEAKS, PEAK_START, PEAK_END, NO_PEAKS, NO_PEAKS, NO_PEAKS]
    assert start.tolist() == [321778, 325498, 326803, 329213, 345554, 357739]
    assert end.tolist() == [325306, 326736, 327796, 342182, 354431, 372331]
    assert int(np.sum(codes != PEAKS)) == 6 and int(np.sum(codes != NO_PEAKS)) == 2
    bad = tmp_path / "labels.bed"
    bad.write_text("chr1\t5\t9\tnoPeaks\nchr1\t10\t20\tpeak\n")
    with pytest.raises(ValueError, match="line 2"):
        read_labels_bed(str(bad))
