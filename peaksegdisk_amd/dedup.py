"""Duplicate removal of aligned reads: the step in front of every *_reads entry
point that keeps the first `keep` units of every key -- (chromStart, chromEnd, strand) by fragment,
(5' base, strand) by 5' end -- in input order.  The marking (peakseg_hip_reads_dedup: a stable radix
sort of the keys on the device) and the compaction (peakseg_hip_reads_compact) are the library's; the
definitions are in include/peaksegdisk_hip.h.  Everything is integer."""
import ctypes

import numpy as np

from . import _native

BY = {"fragment": 0, "five_prime": 1}
SUMMARY_COLUMNS = ("reads", "kept", "rows_kept", "distinct")


class DuplicateRemoval:
    """What remove_duplicates returns: reads -- per contig (chromStart, chromEnd, count), the tuple
    itself for a single contig --, strands (alike, or None) and summary, a data frame with one row
    per contig and the int64 columns reads, kept, rows_kept, distinct."""

    def __init__(self, reads, strands, summary):
        self.reads = reads
        self.strands = strands
        self.summary = summary

    def __repr__(self):
        return "DuplicateRemoval(contigs=%d, reads=%d, kept=%d)" % (
            len(self.summary), int(self.summary["reads"].sum()), int(self.summary["kept"].sum()))


def _status_error(who, status, lib):
    err = RuntimeError("%s: status %d: %s" % (who, status, lib.peakseg_hip_last_error().decode()))
    err.status = status
    return err


def _like(v, n):
    """(a new int32 / int8 vector of n entries in the kind of memory of v -- at least one entry is
    allocated, so that it has an address --, that address)"""
    if isinstance(v, np.ndarray):
        new = np.empty(max(n, 1), dtype=v.dtype)
        return new[:n], new.ctypes.data
    import torch
    new = torch.empty(max(n, 1), dtype=v.dtype, device=v.device)
    return new[:n], new.data_ptr()


def _pointers(values):
    return (ctypes.c_void_p * len(values))(*values)


def _arguments(reads, strands, device, who):
    from .grid import reads_arguments
    from .strand import _strand_pointers
    placeholder = [(0, 1)] * len(reads)          # (no extent is needed here)
    args, keep, _ = reads_arguments(reads, placeholder, "each", device, who)
    strand_ptrs = None if strands is None else _strand_pointers(strands, args, keep, device, who)
    return args, keep, strand_ptrs


def mark(reads, strands=None, keep=1, by=None, device=0, lib=None, who="remove_duplicates"):
    """peakseg_hip_reads_dedup: (out_count per contig, in the kind of memory of the reads; the
    summary as an int64 array of (contigs, 4)).  reads as ProblemSet.from_reads takes them, strands
    one int8 array or tensor per contig or None."""
    lib = lib or _native.lib
    if by is None:
        by = "fragment" if strands is None else "five_prime"
    if by not in BY:
        raise ValueError('%s: by is %r, neither "fragment" nor "five_prime"' % (who, by))
    if isinstance(keep, bool) or not isinstance(keep, (int, np.integer)) or not -2 ** 31 <= keep < 2 ** 31:
        raise ValueError("%s: keep is %r, not an integer of 1 .. 2^31 - 1" % (who, keep))
    args, alive, strand_ptrs = _arguments(reads, strands, device, who)
    nc = args[0]
    out, ptrs = [], []
    for k, entry in enumerate(reads):
        new, ptr = _like(entry[0], int(args[1][k]))
        out.append(new)
        ptrs.append(ptr if args[1][k] else 0)
    summary = np.zeros((nc, len(SUMMARY_COLUMNS)), dtype=np.int64)
    st = lib.peakseg_hip_reads_dedup(device, nc, args[1], args[2], args[3], args[4], strand_ptrs, args[5],
                                     BY[by], int(keep), _pointers(ptrs), summary.ctypes.data)
    del alive
    if st != 0:
        raise _status_error("peakseg_hip_reads_dedup", st, lib)
    return out, summary


def compact(reads, strands, keep_count, device=0, lib=None, who="remove_duplicates"):
    """peakseg_hip_reads_compact: the rows with keep_count > 0 of every contig, in order, as
    ([(chromStart, chromEnd, count)], [strand] or None) with count = keep_count, in the kind of
    memory of the reads: room for every row is allocated, as the library asks, and cut to the rows
    written."""
    lib = lib or _native.lib
    args, alive, strand_ptrs = _arguments([tuple(e[:2]) for e in reads], strands, device, who)
    nc = args[0]
    if len(keep_count) != nc:
        raise ValueError("%s: keep_count: one int32 array per contig" % who)
    from .grid import _dense_pointer
    keep_ptrs = []
    for k, v in enumerate(keep_count):
        ptr, n, side, ref = _dense_pointer(k, v, device, who + ": contig %d keep_count")
        if n != args[1][k] or (n and (side == "device") != bool(args[5])):
            raise ValueError("%s: contig %d keep_count does not match its reads (length or memory)"
                             % (who, k))
        alive.append(ref)
        keep_ptrs.append(ptr if n else 0)
    outs, out_ptrs = [], [[], [], [], []]
    for k, entry in enumerate(reads):
        n = int(args[1][k])
        columns = [entry[0], entry[1], keep_count[k]] + ([strands[k]] if strands is not None else [])
        made = []
        for j, v in enumerate(columns):
            new, ptr = _like(v, n)
            made.append(new)
            out_ptrs[j].append(ptr if args[1][k] else 0)
        outs.append(made)
    written = np.zeros(nc, dtype=np.int64)
    st = lib.peakseg_hip_reads_compact(device, nc, args[1], args[2], args[3], strand_ptrs, args[5],
                                       _pointers(keep_ptrs), _pointers(out_ptrs[0]), _pointers(out_ptrs[1]),
                                       _pointers(out_ptrs[2]),
                                       None if strands is None else _pointers(out_ptrs[3]),
                                       written.ctypes.data)
    del alive
    if st != 0:
        raise _status_error("peakseg_hip_reads_compact", st, lib)
    out_reads = [tuple(v[:int(written[k])] for v in made[:3]) for k, made in enumerate(outs)]
    out_strands = None if strands is None else [made[3][:int(written[k])] for k, made in enumerate(outs)]
    return out_reads, out_strands


def remove(reads, strands=None, keep=1, by=None, compact_rows=True, device=0, lib=None,
           who="remove_duplicates"):
    """(the reads per contig as (chromStart, chromEnd, count), the strands per contig or None, the
    summary array) after the marking, compacted or with the rows kept and only count changed"""
    out, summary = mark(reads, strands, keep, by, device, lib, who)
    if not compact_rows:
        return [(e[0], e[1], out[k]) for k, e in enumerate(reads)], strands, summary
    new_reads, new_strands = compact(reads, strands, out, device, lib, who)
    return new_reads, new_strands, summary


def summary_frame(summary):
    import pandas as pd
    return pd.DataFrame({name: summary[:, j].astype(np.int64) for j, name in enumerate(SUMMARY_COLUMNS)})


def deduplicated_for(reads, strands, max_duplicates, extents, device, lib, who):
    """What the *_reads entry points do with max_duplicates=: (the reads to go on with, the
    extents).  None: the reads as they are.  An integer k: at most k units of every key -- by
    five_prime when strands are given, by fragment otherwise -- with the rows kept and the counts
    changed, before any extension.  Default extents stay those of the reads as given."""
    if max_duplicates is None:
        return reads, extents
    from .grid import reads_arguments
    _, alive, ext = reads_arguments(reads, extents, "each", device, who)
    del alive
    new_reads, _, _ = remove(reads, strands, max_duplicates, None, False, device, lib, who)
    return new_reads, ext
