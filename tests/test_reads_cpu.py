"""What the tests of the path from aligned reads stand on, checked without a device or the
emulator: the recorded facts of the fixture tests/golden/ChIPreads_H3K4me3.npz, and the numpy
pile-up that tests/test_gpu_reads.py and tests/test_reads_emu.py compare the library with, against a
base-by-base loop."""
import numpy as np

import test_gpu_dense as gd
import test_gpu_reads as gr


def test_fixture_facts():
    s, e, k = gr.fixture_reads()
    assert s.dtype == e.dtype == k.dtype == np.int32
    assert len(s) == len(e) == len(k) == 12028
    assert (int(s.min()), int(e.max())) == (gr.FIXTURE_LO, gr.FIXTURE_HI) == (175434087, 175507002)
    assert gr.FIXTURE_HI - gr.FIXTURE_LO == 72915
    length = e - s
    assert (int(length.min()), int(length.max())) == (20, 107)
    assert int(k.min()) >= 1 and int(k.max()) == 11 and int(k.sum()) == 15757
    assert not (np.diff(s) >= 0).all()            # file order is not sorted by chromStart
    cov = gr.numpy_pileup(s, e, None, gr.FIXTURE_LO, gr.FIXTURE_HI)
    assert len(cov) == 72915 and len(gd.rle(cov)[0]) == 12051
    assert int(cov.max()) == 203 and int(cov.astype(np.int64).sum()) == 1147017
    assert int(cov.astype(np.int64).sum()) == int(length.astype(np.int64).sum())
    lo, hi = gr.WINDOW                            # the window clips reads at both of its edges
    assert ((s < lo) & (e > lo)).any() and ((s < hi) & (e > hi)).any()


def test_numpy_pileup_against_a_loop_over_bases():
    rng = np.random.default_rng(42)
    for case in range(50):
        lo = int(rng.integers(0, 50))
        n_bases = int(rng.integers(1, 60))
        hi = lo + n_bases
        n = int(rng.integers(0, 40))
        s = rng.integers(lo - 30, hi + 10, n)
        e = s + rng.integers(1, 40, n)
        k = rng.integers(0, 5, n)
        for mode in ("each", "end"):
            for count in (None, k):
                want = np.zeros(n_bases, np.int64)
                for i in range(n):
                    first = e[i] - 1 if mode == "end" else s[i]
                    for base in range(first, e[i]):
                        if lo <= base < hi:
                            want[base - lo] += 1 if count is None else count[i]
                got = gr.numpy_pileup(s, e, count, lo, hi, mode)
                assert got.dtype == np.int32 and np.array_equal(got, want), (case, mode)
