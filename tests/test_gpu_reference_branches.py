"""The kernels on tests/golden/reference_branches.json: tiny problems found by
tools/reference_branches.py, each of which takes an outcome of the reference's piece algebra
(a "numerically equal" ending of a constant piece, the second function coming first at two
crossings, ...) that no other input of the suite takes.  Every stored function must equal the
deterministic oracle's, on all three kernel builds; the files must equal the oracle's, and the
segments the reference itself wrote wherever the deterministic arithmetic does not change them
(det_segments_equal_reference).  Reads only tests/golden/ and oracle/_build/."""
import ctypes
import os

import numpy as np
import pytest

import reference_live as rl
from test_gpu_parity import psd, _files, REL_TOL  # noqa: F401  (psd: the module's fixture)

GPU = pytest.mark.gpu
LOSS_INTEGER_FIELDS = (0, 1, 2, 3, 4, 7)  # penalty, segments, peaks, bases, bedGraph.lines, equality.constraints
LOSS_FLOAT_FIELDS = (5, 6)                # mean.pen.cost, total.loss


@GPU
def test_reference_branch_fixture(psd, oracle_det, tmp_path, monkeypatch):
    from peaksegdisk_amd import ProblemSet, _native
    cases = rl.load_branch_fixture()["cases"]
    n = len(cases)
    assert n > 0
    want, gpu_bg = [], []
    for c, case in enumerate(cases):
        for side in ("o", "g"):
            d = tmp_path / ("%s%d" % (side, c))
            d.mkdir()
            (d / "coverage.bedGraph").write_text(rl.case_text(case))
        obg = str(tmp_path / ("o%d" % c) / "coverage.bedGraph")
        gpu_bg.append(str(tmp_path / ("g%d" % c) / "coverage.bedGraph"))
        assert oracle_det.solve(obg, case["penalty"]) == 0, case["name"]
        want.append((open("%s_penalty=%s.db" % (obg, case["penalty"]), "rb").read(),
                     _files(obg, case["penalty"])))
    contigs = [(np.array(case["count"], dtype=np.int32),
                (np.array(case["chromEnd"]) - np.array(case["chromStart"])).astype(np.int32))
               for case in cases]
    problems = [(c, float(case["penalty"])) for c, case in enumerate(cases)]
    # every stored function, on each kernel build
    for build in ("lat", "thr", "pk"):
        monkeypatch.setenv("PEAKSEG_HIP_VARIANT", build)
        pset = ProblemSet(contigs, problems)
        pset.solve()
        assert pset.kernel_build == build
        for c, case in enumerate(cases):
            assert pset.result(c).status == 0, (case["name"], build)
            db = str(tmp_path / "g.db")
            pset.export_db(c, np.array(case["chromEnd"], dtype=np.int32), db)
            assert open(db, "rb").read() == want[c][0], (case["name"], build)
        pset.close()
    monkeypatch.delenv("PEAKSEG_HIP_VARIANT")
    # the files, through the file API, once, in the default build
    arr = lambda xs: (ctypes.c_char_p * n)(*[x.encode() for x in xs])
    status = (ctypes.c_int * n)()
    pens = [case["penalty"] for case in cases]
    st = _native.lib.PeakSegFPOP_disk_batch(
        n, arr(gpu_bg), arr(pens), arr(["%s_penalty=%s.db" % (b, p) for b, p in zip(gpu_bg, pens)]),
        status)
    assert st == 0 and list(status) == [0] * n, _native.last_error()
    for c, case in enumerate(cases):
        seg, loss = _files(gpu_bg[c], case["penalty"])
        assert (seg, loss) == want[c][1], case["name"]
        # (the file API's db is sparse: it has the size of the reference's store, not its bytes)
        assert os.path.getsize("%s_penalty=%s.db" % (gpu_bg[c], case["penalty"])) == len(want[c][0]) \
            == case["db_size"], case["name"]
        if case["det_segments_equal_reference"]:
            assert seg.decode() == case["segments"], case["name"]
            got = loss.decode().rstrip("\n").split("\t")
            rec = case["loss_row"].rstrip("\n").split("\t")
            assert len(got) == len(rec) == 10
            for i in LOSS_INTEGER_FIELDS:
                assert got[i] == rec[i], (case["name"], i)
            for i in LOSS_FLOAT_FIELDS:
                assert float(got[i]) == pytest.approx(float(rec[i]), rel=REL_TOL), (case["name"], i)
