#!/usr/bin/env python3
"""Decode the reference's bundled data set data/ChIPreads.RData (gzip-compressed R serialization,
format RDX2/XDR) into the aligned-reads fixture of the tests.

A fixture is data: this script only reads the reference's *data file* and writes
tests/golden/ChIPreads_H3K4me3.npz (numpy.savez_compressed; int32 arrays chromStart, chromEnd,
count): the rows of the data.table ChIPreads whose experiment is H3K4me3 (all on chr2), in file
order.  The rows are not sorted by chromStart.

usage: python tools/decode_chipreads.py /root/reference/data/ChIPreads.RData tests/golden
"""
import gzip
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_mono27ac import Reader  # noqa: E402


def column(v):
    """a column of the data.table as a plain list (factors as their level strings)"""
    if not isinstance(v, dict):
        return v
    if "levels" in v["a"]:
        lev = v["a"]["levels"]
        lev = lev if isinstance(lev, list) else lev["v"]
        return [lev[i - 1] for i in v["v"]]
    return v["v"]


def main():
    src, outdir = sys.argv[1], sys.argv[2]
    raw = gzip.decompress(open(src, "rb").read())
    assert raw[:5] == b"RDX2\n", raw[:5]
    r = Reader(raw[5:])
    assert r.bytes(2) == b"X\n"
    r.int(); r.int(); r.int()          # format version, writer version, min reader version
    top = dict(r.item())               # pairlist: name -> object
    assert list(top) == ["ChIPreads"], list(top)
    reads = top["ChIPreads"]
    names = reads["a"]["names"]
    names = names if isinstance(names, list) else names["v"]
    assert names == ["experiment", "chrom", "chromStart", "chromEnd", "count"], names
    cols = {n: column(v) for n, v in zip(names, reads["v"])}
    keep = np.array([e == "H3K4me3" for e in cols["experiment"]])
    assert {c for c, k in zip(cols["chrom"], keep) if k} == {"chr2"}
    out = {n: np.asarray(cols[n], dtype=np.int64)[keep] for n in ("chromStart", "chromEnd", "count")}
    for n, v in out.items():
        assert v.min() >= 0 and v.max() < 2 ** 31, n
        out[n] = v.astype(np.int32)
    path = os.path.join(outdir, "ChIPreads_H3K4me3.npz")
    np.savez_compressed(path, **out)
    print("rows", len(keep), "kept", int(keep.sum()), "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
