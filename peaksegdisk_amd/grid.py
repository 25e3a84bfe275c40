"""Device-resident (penalty x contig) problem sets: the additive grid entry of the C ABI
(include/peaksegdisk_hip.h, peakseg_hip_problem_set_*).  One problem = one dynamic program
of /root/reference/src/PeakSegFPOPLog.cpp:258-442 for a (contig, penalty) pair."""
import ctypes

import numpy as np

from . import _native


def _dense_pointer(k, v, device, what="from_dense: contig %d", dtype="int32"):
    """(address, length, "host" | "device", the object that keeps the memory alive) of contig k
    of ProblemSet.from_dense (`what`: how the messages name it; from_reads names the array too;
    `dtype`: int32, or int8 for strands); ValueError for what cannot be passed as it is."""
    what = what % k
    if isinstance(v, np.ndarray):
        if v.dtype != np.dtype(dtype):
            raise ValueError("%s has dtype %s, not %s" % (what, v.dtype, dtype))
        if v.ndim != 1 or not v.flags["C_CONTIGUOUS"]:
            raise ValueError("%s is not a contiguous 1-d array" % what)
        return v.ctypes.data, v.shape[0], "host", v
    if type(v).__module__.split(".")[0] == "torch" and hasattr(v, "data_ptr"):
        import torch
        if v.dtype != getattr(torch, dtype):
            raise ValueError("%s has dtype %s, not %s" % (what, v.dtype, dtype))
        if v.dim() != 1 or not v.is_contiguous():
            raise ValueError("%s is not a contiguous 1-d tensor" % what)
        if v.device.type == "cuda":
            index = v.device.index if v.device.index is not None else torch.cuda.current_device()
            if index != device:
                raise ValueError("%s is on cuda:%d, the set on device %d"
                                 % (what, index, device))
            return v.data_ptr(), v.shape[0], "device", v
        if v.device.type != "cpu":
            raise ValueError("%s is on device %s" % (what, v.device))
        return v.data_ptr(), v.shape[0], "host", v
    raise ValueError("%s is a %s, not an %s numpy array or torch tensor"
                     % (what, type(v).__name__, dtype))


ANNOTATIONS = ("noPeaks", "peakStart", "peakEnd", "peaks")  # the codes of label_errors


def annotation_codes(annotation, what="labels"):
    """the annotation column as label_errors passes it on: int32 arrays and tensors as they are, a
    list of the four strings as its codes; ValueError names an unknown string and its index"""
    if isinstance(annotation, np.ndarray) and annotation.dtype.kind in "iu" \
            or hasattr(annotation, "data_ptr"):
        return annotation
    codes = np.empty(len(annotation), dtype=np.int32)
    for i, a in enumerate(annotation):
        if isinstance(a, (int, np.integer)) and not isinstance(a, bool):
            codes[i] = a
        elif a in ANNOTATIONS:
            codes[i] = ANNOTATIONS.index(a)
        else:
            raise ValueError("%s: label %d has annotation %r, not one of %s"
                             % (what, i, a, ", ".join(ANNOTATIONS)))
    return codes


_JOINT_DTYPES = (np.int32,) * 4 + (np.float64, np.int32, np.int32, np.float64, np.int32, np.int64,
                                   np.int32)  # the eleven columns of joint_peaks() and joint_path()


def _joint_groups(group, n_groups, k, m, w_off, e_off, cols):
    """the eleven columns of one joint model -> the list over groups that joint_peaks() returns"""
    import pandas as pd
    result = []
    for g in range(n_groups):
        rows = slice(int(w_off[g]), int(w_off[g + 1]))
        cells = slice(int(e_off[g]), int(e_off[g + 1]))
        entry = {"members": np.flatnonzero(group == g),
                 "joint": pd.DataFrame({name: cols[j][rows] for j, name in enumerate(
                     ("windowStart", "windowEnd", "peakStart", "peakEnd", "objective",
                      "samples_up", "levels"))})}
        for j, name in enumerate(("gain", "up", "sum", "bases")):
            entry[name] = cols[7 + j][cells].reshape(int(k[g]), int(m[g]))
        result.append(entry)
    return result


def read_labels_bed(path):
    """A labels.bed file as the reference's tests write it -- chrom, chromStart, chromEnd,
    annotation, separated by white space -- as (the `labels` entry of one contig for
    ProblemSet.label_errors: (chromStart, chromEnd, annotation codes) int32 arrays, the chrom
    values as a list).  An unknown annotation raises ValueError naming the line."""
    chrom, start, end, codes = [], [], [], []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            fields = line.split()
            if not fields:
                continue
            if len(fields) != 4:
                raise ValueError("%s: line %d does not have four columns" % (path, number))
            if fields[3] not in ANNOTATIONS:
                raise ValueError("%s: line %d: unknown annotation %r (one of %s)"
                                 % (path, number, fields[3], ", ".join(ANNOTATIONS)))
            try:
                start.append(int(fields[1]))
                end.append(int(fields[2]))
            except ValueError:
                raise ValueError("%s: line %d: chromStart and chromEnd must be integers"
                                 % (path, number))
            chrom.append(fields[0])
            codes.append(ANNOTATIONS.index(fields[3]))
    return (np.array(start, dtype=np.int32), np.array(end, dtype=np.int32),
            np.array(codes, dtype=np.int32)), chrom


def _extreme(v, largest):
    """the smallest or largest entry of a read array, wherever it lives"""
    return int((v.max() if largest else v.min()).item())


def reads_arguments(reads, extents, bases_counted, device, who):
    """The read arguments of the C ABI (peakseg_hip_problem_set_create_reads and
    peakseg_hip_reads_pileup_probe) from `reads`: a list, one entry per contig, of
    (chromStart, chromEnd) or (chromStart, chromEnd, count) int32 arrays, validated as from_dense
    validates its contigs.  Returns (the nine ctypes arguments after `device`, the objects
    that keep the memory alive, the extents as a list of (lo, hi))."""
    if len(reads) == 0:
        raise ValueError("%s: no contig" % who)
    if isinstance(bases_counted, str):
        if bases_counted not in ("each", "end"):
            raise ValueError('%s: bases_counted is %r, neither "each" nor "end"' % (who, bases_counted))
        mode = 0 if bases_counted == "each" else 1
    else:
        mode = int(bases_counted)
    if extents is not None and len(extents) != len(reads):
        raise ValueError("%s: extents: one (chromStart, chromEnd) per contig" % who)
    names = ("chromStart", "chromEnd", "count")
    keep, sides, lengths, out_extents = [], [], [], []
    ptrs = ([], [], [])
    for k, entry in enumerate(reads):
        if not isinstance(entry, (tuple, list)) or len(entry) not in (2, 3):
            raise ValueError("%s: contig %d is not (chromStart, chromEnd) or "
                             "(chromStart, chromEnd, count)" % (who, k))
        n = None
        for j in range(3):
            v = entry[j] if j < len(entry) else None
            if v is None:
                if j < 2:
                    raise ValueError("%s: contig %d has no %s" % (who, k, names[j]))
                ptrs[j].append(0)
                continue
            ptr, m, side, ref = _dense_pointer(k, v, device, who + ": contig %d " + names[j])
            if n is not None and m != n:
                raise ValueError("%s: contig %d has %d chromStart and %d %s"
                                 % (who, k, n, m, names[j]))
            n = m
            keep.append(ref)
            sides.append((side, k))
            ptrs[j].append(ptr if m else 0)
        lengths.append(n)
        if extents is None:
            if n == 0:
                raise ValueError("%s: contig %d has no reads: its extent must be given" % (who, k))
            out_extents.append((_extreme(entry[0], False), _extreme(entry[1], True)))
        else:
            out_extents.append((int(extents[k][0]), int(extents[k][1])))
    for side, k in sides:
        if side != sides[0][0]:
            raise ValueError("%s: contig %d is in %s memory but contig 0 is in %s memory; "
                             "one call takes one kind" % (who, k, side, sides[0][0]))
    for lo, hi in out_extents:
        if not (-2 ** 31 <= lo < 2 ** 31 and -2 ** 31 <= hi < 2 ** 31):
            raise ValueError("%s: extents must fit 32-bit integers" % who)
    nc = len(reads)
    args = [nc, (ctypes.c_longlong * nc)(*lengths)]
    args += [(ctypes.c_void_p * nc)(*p) for p in ptrs]
    args += [1 if sides[0][0] == "device" else 0,
             (ctypes.c_int * nc)(*[lo for lo, _ in out_extents]),
             (ctypes.c_int * nc)(*[hi for _, hi in out_extents]), mode]
    return args, keep, out_extents


BASE_FEATURES = ("quartile.0%", "quartile.25%", "quartile.50%", "quartile.75%", "quartile.100%",
                 "mean", "sd", "bases", "data")
FEATURE_PREFIXES = ("", "log+1.", "log.", "log.log.")
FEATURE_NAMES = tuple(prefix + name for prefix in FEATURE_PREFIXES for name in BASE_FEATURES)
MOMENT_WORDS = 6    # bases, runs, S1, Q0, Q1, Q2 of peakseg_hip_problem_set_pack_coverage_stats


def quartile_ranks(bases):
    """(lo, hi, g) of the five type-7 quartiles of a vector of `bases` entries, from integer
    arithmetic: h = (bases - 1) k / 4, lo = floor(h), hi = min(lo + 1, bases - 1), g = h - lo"""
    h4 = [(bases - 1) * k for k in range(5)]
    lo = [h // 4 for h in h4]
    return lo, [min(r + 1, bases - 1) for r in lo], [(h % 4) / 4.0 for h in h4]


def features_from_stats(quartile_lo, quartile_hi, bases, runs, s1, s2):
    """The 36 features (FEATURE_NAMES) of one contig's per-base coverage x from integers, on the
    host: quartile_lo[k], quartile_hi[k]: the order statistics x_(lo), x_(hi) of quartile_ranks(bases);
    bases: len(x); runs: the runs of its run-length encoding; s1 = sum(x); s2 = sum(x ** 2).  The
    quartiles are type 7 (R's default, numpy's "linear"), exact in float64; mean = s1 / bases and
    sd = sqrt((bases s2 - s1^2) / (bases (bases - 1))) are formed from exact quotients of Python
    integers, rounded once (sd is NaN for one base).  Then the nine under log(v + 1), log(v) and
    log(log(v)), as numpy computes them with its warnings silenced: what is undefined is -inf or NaN
    and stays in the vector."""
    import math
    from fractions import Fraction
    bases, runs, s1, s2 = int(bases), int(runs), int(s1), int(s2)
    g = quartile_ranks(bases)[2]
    base = [float(int(a)) + (float(int(b)) - float(int(a))) * gk
            for a, b, gk in zip(quartile_lo, quartile_hi, g)]
    base.append(float(Fraction(s1, bases)))
    base.append(math.sqrt(float(Fraction(bases * s2 - s1 * s1, bases * (bases - 1))))
                if bases > 1 else float("nan"))
    base += [float(bases), float(runs)]
    base = np.array(base, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.concatenate([base, np.log(base + 1.0), np.log(base), np.log(np.log(base))])


class ProblemSet:
    """contigs: list of (count, weight) int32 arrays; problems: list of (contig_index, penalty)."""

    def __init__(self, contigs, problems, device=0, arena_pieces=0, lib=None):
        self._lib = lib or _native.lib
        self._h = ctypes.c_void_p()
        self.dense = False
        self.device = device
        self.contigs = [(np.ascontiguousarray(c, dtype=np.int32),
                         np.ascontiguousarray(w, dtype=np.int32)) for c, w in contigs]
        self.problems = [(int(c), float(p)) for c, p in problems]
        nc = len(self.contigs)
        n_bins = (ctypes.c_int * nc)(*[len(c) for c, _ in self.contigs])
        cptr = (ctypes.c_void_p * nc)(*[c.ctypes.data for c, _ in self.contigs])
        wptr = (ctypes.c_void_p * nc)(*[w.ctypes.data for _, w in self.contigs])
        npb = len(self.problems)
        pc = (ctypes.c_int * npb)(*[c for c, _ in self.problems])
        pp = (ctypes.c_double * npb)(*[p for _, p in self.problems])
        st = self._lib.peakseg_hip_problem_set_create(
            device, nc, n_bins, cptr, wptr, npb, pc, pp, ctypes.c_ulonglong(arena_pieces),
            ctypes.byref(self._h))
        if st != 0:
            raise RuntimeError("peakseg_hip_problem_set_create: status %d: %s" % (
                st, self._lib.peakseg_hip_last_error().decode()))
        self.bins_per_solve = sum(len(self.contigs[c][0]) for c, _ in self.problems)

    @classmethod
    def from_dense(cls, contigs, problems, device=0, arena_pieces=0, lib=None):
        """The set of DENSE coverage: a contig is a 1-d contiguous int32 numpy array or torch
        tensor with one count per base, and the run-length encoding happens on the device
        (peakseg_hip_problem_set_create_dense).  A tensor on cuda:`device` is read in place
        through its data_ptr(), without a copy; numpy arrays and CPU tensors are uploaded by the
        library.  All contigs of one call live on the same side.  The set's contigs are the runs:
        problem p's segment table indexes them, segment_columns() gives base coordinates."""
        self = cls.__new__(cls)
        self._lib = lib or _native.lib
        self._h = ctypes.c_void_p()
        self.dense = True
        self.device = device
        self.problems = [(int(c), float(p)) for c, p in problems]
        if len(contigs) == 0:
            raise ValueError("from_dense: no contig")
        keep, ptrs, sides = [], [], []
        for k, v in enumerate(contigs):
            ptr, n, side, ref = _dense_pointer(k, v, device)
            keep.append(ref)
            ptrs.append(ptr)
            sides.append(side)
            if n == 0:
                ptrs[-1] = 0
        if len(set(sides)) != 1:
            k = next(i for i, sd in enumerate(sides) if sd != sides[0])
            raise ValueError("from_dense: contig %d is in %s memory but contig 0 is in %s memory; "
                             "one call takes one kind" % (k, sides[k], sides[0]))
        self.contig_bases = [int(r.shape[0]) for r in keep]
        nc = len(keep)
        n_bases = (ctypes.c_longlong * nc)(*self.contig_bases)
        cptr = (ctypes.c_void_p * nc)(*ptrs)
        npb = len(self.problems)
        pc = (ctypes.c_int * max(npb, 1))(*[c for c, _ in self.problems])
        pp = (ctypes.c_double * max(npb, 1))(*[p for _, p in self.problems])
        st = self._lib.peakseg_hip_problem_set_create_dense(
            device, nc, n_bases, cptr, 1 if sides[0] == "device" else 0, npb, pc, pp,
            ctypes.c_ulonglong(arena_pieces), ctypes.byref(self._h))
        del keep  # (the library holds no reference to the caller's buffers after the call)
        if st != 0:
            err = RuntimeError("peakseg_hip_problem_set_create_dense: status %d: %s" % (
                st, self._lib.peakseg_hip_last_error().decode()))
            err.status = st
            raise err
        self.contigs = None
        self.bins_per_solve = None
        return self

    @classmethod
    def from_reads(cls, reads, problems, extents=None, bases_counted="each", device=0,
                   arena_pieces=0, lib=None, strands=None, fragment_length=None, max_shift=400,
                   min_shift=0, max_duplicates=None):
        """The set of ALIGNED READS: `reads` is a list, one entry per contig, of
        (chromStart, chromEnd) or (chromStart, chromEnd, count) -- 1-d contiguous int32 numpy
        arrays or torch tensors, one entry per read, in any order.  The coverage is piled up and
        run-length encoded on the device (peakseg_hip_problem_set_create_reads); tensors on
        cuda:`device` are read in place, numpy arrays and CPU tensors are uploaded by the library;
        one call takes one kind of memory.  extents: per contig the (chromStart, chromEnd) whose
        bases are the contig's data, reads clipped to it; None: (min chromStart, max chromEnd) of
        the contig's reads.  bases_counted: "each" base of a read, or only its "end" (last base).
        From here on the set is one of from_dense: contig_bases are the extents' lengths and
        contig_starts their starts, so segment_columns(first_chromStart=pset.contig_starts) gives
        genomic coordinates.
        Single-end reads: strands (one int8 array or tensor per contig, +1 or -1 per read) and
        fragment_length (an integer, one per contig, or "auto": the pooled estimate of the strand
        cross-correlation over the shifts min_shift .. max_shift) extend every read from its 5'
        end to the fragment length on the device first (strand.py); the two go together.  Default
        extents stay those of the reads as given, and the extension is clipped to them.
        max_duplicates: None, or an integer k: duplicates are removed first (dedup.py) -- at most k
        units of every key survive, in input order, by 5' end and strand when strands are given,
        by (chromStart, chromEnd) otherwise -- on the reads as given, before any extension and
        before "auto" estimates the fragment length."""
        from .dedup import deduplicated_for
        from .strand import extended_for
        self = cls.__new__(cls)
        self._lib = lib or _native.lib
        self._h = ctypes.c_void_p()
        self.dense = True
        self.device = device
        self.problems = [(int(c), float(p)) for c, p in problems]
        reads, extents = deduplicated_for(reads, strands, max_duplicates, extents, device, self._lib,
                                          "from_reads")
        reads, extents = extended_for(reads, strands, fragment_length, extents, device, self._lib,
                                      "from_reads", max_shift, min_shift)
        args, keep, ext = reads_arguments(reads, extents, bases_counted, device, "from_reads")
        self.contig_starts = [lo for lo, _ in ext]
        self.contig_bases = [hi - lo for lo, hi in ext]
        npb = len(self.problems)
        pc = (ctypes.c_int * max(npb, 1))(*[c for c, _ in self.problems])
        pp = (ctypes.c_double * max(npb, 1))(*[p for _, p in self.problems])
        st = self._lib.peakseg_hip_problem_set_create_reads(
            device, *args, npb, pc, pp, ctypes.c_ulonglong(arena_pieces), ctypes.byref(self._h))
        del keep  # (the library holds no reference to the caller's buffers after the call)
        if st != 0:
            err = RuntimeError("peakseg_hip_problem_set_create_reads: status %d: %s" % (
                st, self._lib.peakseg_hip_last_error().decode()))
            err.status = st
            raise err
        self.contigs = None
        self.bins_per_solve = None
        return self

    def _fold_layout(self, n_inputs, penalties, folds, who):
        """the attributes of a fold set (before the library is called): folds, penalties, problems"""
        pens = [float(p) for p in penalties]
        if not pens:
            raise ValueError("%s: no penalty" % who)
        self.folds = int(folds)
        self.fold_inputs = n_inputs
        self.fold_penalties = pens
        self.problems = [((i * self.folds + f) * 2, p) for i in range(n_inputs)
                         for f in range(max(self.folds, 0)) for p in pens]
        return (ctypes.c_double * len(pens))(*pens)

    def fold_contig(self, i, f, test=False):
        """the set's contig of input contig i and fold f: the train contig (every unit that is not
        in fold f), or with test the units in fold f"""
        if not (0 <= i < self.fold_inputs and 0 <= f < self.folds):
            raise IndexError("fold_contig: input %d, fold %d" % (i, f))
        return (i * self.folds + f) * 2 + (1 if test else 0)

    def fold_problem(self, i, f, j):
        """the set's problem of input contig i, fold f and penalties[j]: its train contig's model"""
        if not (0 <= i < self.fold_inputs and 0 <= f < self.folds
                and 0 <= j < len(self.fold_penalties)):
            raise IndexError("fold_problem: input %d, fold %d, penalty %d" % (i, f, j))
        return (i * self.folds + f) * len(self.fold_penalties) + j

    @classmethod
    def from_dense_folds(cls, contigs, penalties, folds=4, seed=1, device=0, arena_pieces=0,
                         lib=None):
        """The fold set of DENSE coverage (peakseg_hip_problem_set_create_dense_folds;
        include/peaksegdisk_hip.h has the definition): the unit counts of every base of every input
        contig (given as from_dense takes them) are split at random into `folds` (2, 4 or 8) on the
        device, and the set holds, for input contig i and fold f, the train contig
        fold_contig(i, f) -- every unit that is not in f -- and the test contig
        fold_contig(i, f, test=True), both with the input's bases.  Problem fold_problem(i, f, j)
        is the train contig at penalties[j]; test contigs carry no problem.  From here on the set
        is one of from_dense.  A number of folds that is not 2, 4 or 8 and a base with more than
        peakseg_hip_fold_max_count() (2^20) units raise RuntimeError with .status 23."""
        self = cls.__new__(cls)
        self._lib = lib or _native.lib
        self._h = ctypes.c_void_p()
        self.dense = True
        self.device = device
        if len(contigs) == 0:
            raise ValueError("from_dense_folds: no contig")
        pens = self._fold_layout(len(contigs), penalties, folds, "from_dense_folds")
        keep, ptrs, sides = [], [], []
        for k, v in enumerate(contigs):
            ptr, n, side, ref = _dense_pointer(k, v, device, "from_dense_folds: contig %d")
            keep.append(ref)
            ptrs.append(ptr if n else 0)
            sides.append(side)
        if len(set(sides)) != 1:
            k = next(i for i, sd in enumerate(sides) if sd != sides[0])
            raise ValueError("from_dense_folds: contig %d is in %s memory but contig 0 is in %s "
                             "memory; one call takes one kind" % (k, sides[k], sides[0]))
        nc = len(keep)
        bases = [int(r.shape[0]) for r in keep]
        self.contig_bases = [b for b in bases for _ in range(2 * max(self.folds, 0))]
        st = self._lib.peakseg_hip_problem_set_create_dense_folds(
            device, nc, (ctypes.c_longlong * nc)(*bases), (ctypes.c_void_p * nc)(*ptrs),
            1 if sides[0] == "device" else 0, len(self.fold_penalties), pens,
            ctypes.c_ulonglong(arena_pieces), self.folds, ctypes.c_ulonglong(int(seed) % 2 ** 64),
            ctypes.byref(self._h))
        del keep  # (the library holds no reference to the caller's buffers after the call)
        if st != 0:
            err = RuntimeError("peakseg_hip_problem_set_create_dense_folds: status %d: %s" % (
                st, self._lib.peakseg_hip_last_error().decode()))
            err.status = st
            raise err
        self.contigs = None
        self.bins_per_solve = None
        return self

    @classmethod
    def from_reads_folds(cls, reads, penalties, folds=4, seed=1, extents=None, bases_counted="each",
                         device=0, arena_pieces=0, lib=None):
        """The fold set of ALIGNED READS (peakseg_hip_problem_set_create_reads_folds): every read
        (given as from_reads takes them) goes whole, with its optional count, to one of `folds`
        (2, 4 or 8) folds chosen at random from its place in the caller's arrays; the layout is
        that of from_dense_folds, the contigs those of from_reads: contig_starts and contig_bases
        are the extents', repeated for every fold's train and test contig."""
        self = cls.__new__(cls)
        self._lib = lib or _native.lib
        self._h = ctypes.c_void_p()
        self.dense = True
        self.device = device
        args, keep, ext = reads_arguments(reads, extents, bases_counted, device, "from_reads_folds")
        pens = self._fold_layout(len(reads), penalties, folds, "from_reads_folds")
        repeat = 2 * max(self.folds, 0)
        self.contig_starts = [lo for lo, _ in ext for _ in range(repeat)]
        self.contig_bases = [hi - lo for lo, hi in ext for _ in range(repeat)]
        st = self._lib.peakseg_hip_problem_set_create_reads_folds(
            device, *args, len(self.fold_penalties), pens, ctypes.c_ulonglong(arena_pieces),
            self.folds, ctypes.c_ulonglong(int(seed) % 2 ** 64), ctypes.byref(self._h))
        del keep  # (the library holds no reference to the caller's buffers after the call)
        if st != 0:
            err = RuntimeError("peakseg_hip_problem_set_create_reads_folds: status %d: %s" % (
                st, self._lib.peakseg_hip_last_error().decode()))
            err.status = st
            raise err
        self.contigs = None
        self.bins_per_solve = None
        return self

    def segment_columns(self, first_chromStart=None, torch_device=None):
        """The reference's segments table of every problem of a solved set made by from_dense
        (peakseg_hip_problem_set_pack_segments): chromStart, chromEnd and mean in the
        reference's row order (last segment first); a row's status is its parity (even:
        background, odd: peak).  first_chromStart: the coordinate of each CONTIG's first base
        (default 0).  Without torch_device: a list over problems of (chromStart int32[],
        chromEnd int32[], mean float64[]) numpy arrays.  With torch_device:
        (rows int64 numpy[k + 1] -- problem p's rows are rows[p]:rows[p + 1] --, chromStart,
        chromEnd, mean) where the three are tensors that alias the library's packed buffers:
        nothing is downloaded, and they are valid until the next solve() / close()."""
        k = len(self.problems)
        rows = np.zeros(k, dtype=np.int64)
        first = None
        if first_chromStart is not None:
            first = np.ascontiguousarray(first_chromStart, dtype=np.int32)
            if first.shape != (len(self.contig_bases),):
                raise ValueError("first_chromStart: one value per contig")
        p1, p2, p3 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        total = self._lib.peakseg_hip_problem_set_pack_segments(
            self._h, first.ctypes.data if first is not None else None, rows.ctypes.data,
            ctypes.byref(p1), ctypes.byref(p2), ctypes.byref(p3))
        if total < 0:
            raise RuntimeError("pack_segments: %s" % self._lib.peakseg_hip_last_error().decode())
        total = int(total)
        offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            return (offs, device_array(p1.value or 0, total, np.int32, dev),
                    device_array(p2.value or 0, total, np.int32, dev),
                    device_array(p3.value or 0, total, np.float64, dev))
        start = np.empty(total, dtype=np.int32)
        end = np.empty(total, dtype=np.int32)
        mean = np.empty(total, dtype=np.float64)
        if self._lib.peakseg_hip_problem_set_packed_segments_download(
                self._h, start.ctypes.data, end.ctypes.data, mean.ctypes.data) != 0:
            raise RuntimeError("packed_segments_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        return [(start[offs[p]:offs[p + 1]], end[offs[p]:offs[p + 1]], mean[offs[p]:offs[p + 1]])
                for p in range(k)]

    def segment_stats(self, first_chromStart=None, torch_device=None):
        """What every row of segment_columns() holds, computed on the device from the resident
        runs (peakseg_hip_problem_set_pack_segment_stats), row for row in segment_columns()'
        order: sum (int64, the reads under the segment: the sum of its bases' counts), max (int32,
        its largest count), summitStart and summitEnd (int32, the coordinates of the first run in
        genomic order whose count equals max).  first_chromStart as in segment_columns().
        Without torch_device: a list over problems of (sum, max, summitStart, summitEnd) numpy
        arrays.  With torch_device: (rows int64 numpy[k + 1], sum, max, summitStart, summitEnd)
        where the four are tensors that alias the library's packed buffers: nothing is
        downloaded, and they are valid until the next solve() / close()."""
        k = len(self.problems)
        rows = np.zeros(k, dtype=np.int64)
        first = None
        if first_chromStart is not None:
            first = np.ascontiguousarray(first_chromStart, dtype=np.int32)
            if first.shape != (len(self.contig_bases),):
                raise ValueError("first_chromStart: one value per contig")
        ptr = [ctypes.c_void_p() for _ in range(4)]
        total = self._lib.peakseg_hip_problem_set_pack_segment_stats(
            self._h, first.ctypes.data if first is not None else None, rows.ctypes.data,
            *[ctypes.byref(q) for q in ptr])
        if total < 0:
            raise RuntimeError("pack_segment_stats: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        total = int(total)
        offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        dtypes = (np.int64, np.int32, np.int32, np.int32)
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            return (offs,) + tuple(device_array(q.value or 0, total, dt, dev)
                                   for q, dt in zip(ptr, dtypes))
        cols = [np.empty(total, dtype=dt) for dt in dtypes]
        if self._lib.peakseg_hip_problem_set_packed_segment_stats_download(
                self._h, *[a.ctypes.data for a in cols]) != 0:
            raise RuntimeError("packed_segment_stats_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        return [tuple(a[offs[p]:offs[p + 1]] for a in cols) for p in range(k)]

    def label_errors(self, labels, first_chromStart=None, torch_device=None):
        """The label errors of every problem of a solved set made by from_dense or from_reads,
        counted on the device from the resident tables (peakseg_hip_problem_set_pack_label_errors;
        the definitions are in include/peaksegdisk_hip.h).  labels: a list over CONTIGS of
        (chromStart, chromEnd, annotation) -- the first two 1-d contiguous int32 numpy arrays or
        torch tensors, annotation an int32 array of codes (ANNOTATIONS) or a list of the four
        strings --, an empty entry (or None) for a contig without labels.  Tensors on the set's
        cuda device are read in place; one call takes one kind of memory.  first_chromStart as in
        segment_columns().  Without torch_device: (totals, per_label) -- totals an int32 array
        [n_problems, 5] of errors, fp, fn, possible_fp, possible_fn; per_label a list over problems
        of (count, fp, fn) int32 arrays, one entry per label of the problem's contig in the order
        given.  With torch_device: (rows int64 numpy[k + 1], count, fp, fn, totals) where the four
        are tensors that alias the library's buffers: nothing is downloaded, and they are valid
        until the next solve(), the next label_errors() or close()."""
        k = len(self.problems)
        n_contigs = len(self.contig_bases) if self.dense else len(self.contigs)
        if len(labels) != n_contigs:
            raise ValueError("label_errors: one entry per contig (%d entries, %d contigs)"
                             % (len(labels), n_contigs))
        first = None
        if first_chromStart is not None:
            first = np.ascontiguousarray(first_chromStart, dtype=np.int32)
            if first.shape != (n_contigs,):
                raise ValueError("first_chromStart: one value per contig")
        names = ("chromStart", "chromEnd", "annotation")
        keep, sides, lengths = [], [], []
        ptrs = ([], [], [])
        for c, entry in enumerate(labels):
            if entry is None or len(entry) == 0:
                lengths.append(0)
                for q in ptrs:
                    q.append(0)
                continue
            if len(entry) != 3:
                raise ValueError("label_errors: contig %d is not (chromStart, chromEnd, annotation)"
                                 % c)
            entry = list(entry)
            entry[2] = annotation_codes(entry[2], "label_errors: contig %d" % c)
            n = None
            for j in range(3):
                ptr, m, side, ref = _dense_pointer(c, entry[j], self.device,
                                                   "label_errors: contig %d " + names[j])
                if n is not None and m != n:
                    raise ValueError("label_errors: contig %d has %d chromStart and %d %s"
                                     % (c, n, m, names[j]))
                n = m
                keep.append(ref)
                sides.append((side, c))
                ptrs[j].append(ptr if m else 0)
            lengths.append(n)
        for side, c in sides:
            if side != sides[0][0]:
                raise ValueError("label_errors: contig %d is in %s memory but contig %d is in %s "
                                 "memory; one call takes one kind" % (c, side, sides[0][1], sides[0][0]))
        rows = np.zeros(k, dtype=np.int64)
        out = [ctypes.c_void_p() for _ in range(4)]
        total = self._lib.peakseg_hip_problem_set_pack_label_errors(
            self._h, first.ctypes.data if first is not None else None,
            (ctypes.c_longlong * n_contigs)(*lengths),
            *[(ctypes.c_void_p * n_contigs)(*q) for q in ptrs],
            1 if sides and sides[0][0] == "device" else 0, rows.ctypes.data,
            *[ctypes.byref(q) for q in out])
        del keep  # (the library holds no reference to the caller's buffers after the call)
        if total < 0:
            err = RuntimeError("pack_label_errors: %s" % self._lib.peakseg_hip_last_error().decode())
            err.status = int(-total) if total < -1 else _native.ERROR_DEVICE_SOLVER
            raise err
        total = int(total)
        offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            cols = tuple(device_array(q.value or 0, total, np.int32, dev) for q in out[:3])
            return (offs,) + cols + (device_array(out[3].value or 0, 5 * k, np.int32, dev).view(k, 5),)
        cols = [np.empty(total, dtype=np.int32) for _ in range(3)]
        totals = np.empty((k, 5), dtype=np.int32)
        if self._lib.peakseg_hip_problem_set_packed_label_errors_download(
                self._h, *[a.ctypes.data for a in cols], totals.ctypes.data) != 0:
            raise RuntimeError("packed_label_errors_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        return totals, [tuple(a[offs[p]:offs[p + 1]] for a in cols) for p in range(k)]

    def _first_chromStart(self, first_chromStart):
        if first_chromStart is None:
            return None
        first = np.ascontiguousarray(first_chromStart, dtype=np.int32)
        if first.shape != (self._n_contigs(),):
            raise ValueError("first_chromStart: one value per contig")
        return first

    def _raise_status(self, who, total):
        err = RuntimeError("%s: %s" % (who, self._lib.peakseg_hip_last_error().decode()))
        err.status = int(-total) if total < -1 else _native.ERROR_DEVICE_SOLVER
        raise err

    def region_stats(self, regions, first_chromStart=None, torch_device=None):
        """The coverage of caller-chosen regions of every contig of a set made by from_dense or
        from_reads (solved or not), computed on the device from the resident runs
        (peakseg_hip_problem_set_pack_region_stats; bigWigAverageOverBed's job).  regions: a list
        over CONTIGS of (chromStart, chromEnd) -- 1-d contiguous int32 numpy arrays or torch tensors
        --, an empty entry (or None) for a contig without regions.  Regions come in any order, may
        overlap, and may lie partly or wholly outside their contig; tensors on the set's cuda device
        are read in place; one call takes one kind of memory.  first_chromStart as in
        segment_columns().  Without torch_device: a list over contigs of {"bases": int32[],
        "sum": int64[], "max": int32[]}, one entry per region in the order given: the bases of the
        region inside the contig, the sum of the per-base counts over them, and the largest count
        of a run that meets it.  With torch_device: (rows int64 numpy[n_contigs + 1], bases, sum,
        max) where the three are tensors that alias the library's buffers: nothing is downloaded,
        and they are valid until the next region_stats() or close().  A region with
        chromStart >= chromEnd raises RuntimeError with .status 22, naming the contig and the
        region."""
        n_contigs = self._n_contigs()
        if len(regions) != n_contigs:
            raise ValueError("region_stats: one entry per contig (%d entries, %d contigs)"
                             % (len(regions), n_contigs))
        first = self._first_chromStart(first_chromStart)
        names = ("chromStart", "chromEnd")
        keep, sides, lengths = [], [], []
        ptrs = ([], [])
        for c, entry in enumerate(regions):
            if entry is None or len(entry) == 0:
                lengths.append(0)
                for q in ptrs:
                    q.append(0)
                continue
            if len(entry) != 2:
                raise ValueError("region_stats: contig %d is not (chromStart, chromEnd)" % c)
            n = None
            for j in range(2):
                ptr, m, side, ref = _dense_pointer(c, entry[j], self.device,
                                                   "region_stats: contig %d " + names[j])
                if n is not None and m != n:
                    raise ValueError("region_stats: contig %d has %d chromStart and %d chromEnd"
                                     % (c, n, m))
                n = m
                keep.append(ref)
                sides.append((side, c))
                ptrs[j].append(ptr if m else 0)
            lengths.append(n)
        for side, c in sides:
            if side != sides[0][0]:
                raise ValueError("region_stats: contig %d is in %s memory but contig %d is in %s "
                                 "memory; one call takes one kind" % (c, side, sides[0][1], sides[0][0]))
        out = [ctypes.c_void_p() for _ in range(3)]
        total = self._lib.peakseg_hip_problem_set_pack_region_stats(
            self._h, first.ctypes.data if first is not None else None,
            (ctypes.c_longlong * n_contigs)(*lengths),
            *[(ctypes.c_void_p * n_contigs)(*q) for q in ptrs],
            1 if sides and sides[0][0] == "device" else 0, None, *[ctypes.byref(q) for q in out])
        del keep  # (the library holds no reference to the caller's buffers after the call)
        if total < 0:
            self._raise_status("pack_region_stats", total)
        total = int(total)
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        dtypes = (np.int32, np.int64, np.int32)
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            return (offs,) + tuple(device_array(q.value or 0, total, dt, dev)
                                   for q, dt in zip(out, dtypes))
        cols = [np.empty(total, dtype=dt) for dt in dtypes]
        if self._lib.peakseg_hip_problem_set_packed_region_stats_download(
                self._h, *[a.ctypes.data for a in cols]) != 0:
            raise RuntimeError("packed_region_stats_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        return [{name: a[offs[c]:offs[c + 1]] for name, a in zip(("bases", "sum", "max"), cols)}
                for c in range(n_contigs)]

    def peak_clusters(self, groups, first_chromStart=None, torch_device=None):
        """Which peaks of the set's models are the same peak, and what every model has under each
        of them (peakseg_hip_problem_set_pack_peak_clusters; include/peaksegdisk_hip.h has the
        definitions), on the device from the resident tables of a solved set made by from_dense or
        from_reads.  groups: one integer per PROBLEM, -1 (in no group) or a group 0 .. n_groups - 1;
        n_groups is the largest value + 1.  The members of a group are its problems in increasing
        index; two peaks belong to one cluster when a chain of overlapping peaks joins them.
        first_chromStart as in segment_columns().  Without torch_device: a list over groups of
        {"members": the problems' indices, "clusters": a data frame with the columns clusterStart,
        clusterEnd, peaks, samples in increasing clusterStart, and "peaks", "bases", "sum", "max":
        (clusters, members) arrays -- the member's peaks under the cluster, and the region_stats()
        columns of the cluster as a region of the member's contig}.  With torch_device:
        (clusters int64 numpy[n_groups + 1], entries int64 numpy[n_groups + 1], clusterStart,
        clusterEnd, peaks, samples, m_peaks, m_bases, m_sum, m_max) where the eight are tensors that
        alias the library's buffers (group g's clusters are clusters[g]:clusters[g + 1], its matrix
        entries entries[g]:entries[g + 1], cluster-major); they are valid until the next solve(),
        the next peak_clusters() or close()."""
        group = np.ascontiguousarray(groups, dtype=np.int32) if len(groups) else np.zeros(0, np.int32)
        if group.shape != (len(self.problems),):
            raise ValueError("peak_clusters: one group per problem (%d values, %d problems)"
                             % (group.size, len(self.problems)))
        if not np.array_equal(group, np.asarray(groups)):
            raise ValueError("peak_clusters: groups must be integers")
        n_groups = int(group.max()) + 1 if group.size and group.max() >= 0 else 0
        first = self._first_chromStart(first_chromStart)
        k = np.zeros(max(n_groups, 1), dtype=np.int64)
        m = np.zeros(max(n_groups, 1), dtype=np.int64)
        out = [ctypes.c_void_p() for _ in range(8)]
        total = self._lib.peakseg_hip_problem_set_pack_peak_clusters(
            self._h, first.ctypes.data if first is not None else None, n_groups, group.ctypes.data,
            k.ctypes.data, m.ctypes.data, *[ctypes.byref(q) for q in out])
        if total < 0:
            self._raise_status("pack_peak_clusters", total)
        total = int(total)
        k, m = k[:n_groups], m[:n_groups]
        c_off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
        e_off = np.concatenate([[0], np.cumsum(k * m)]).astype(np.int64)
        entries = int(e_off[-1])
        dtypes = (np.int32,) * 6 + (np.int64, np.int32)
        sizes = (total,) * 4 + (entries,) * 4
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            return (c_off, e_off) + tuple(device_array(q.value or 0, n, dt, dev)
                                          for q, n, dt in zip(out, sizes, dtypes))
        cols = [np.empty(n, dtype=dt) for n, dt in zip(sizes, dtypes)]
        if self._lib.peakseg_hip_problem_set_packed_peak_clusters_download(
                self._h, *[a.ctypes.data for a in cols]) != 0:
            raise RuntimeError("packed_peak_clusters_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        import pandas as pd
        result = []
        for g in range(n_groups):
            rows = slice(int(c_off[g]), int(c_off[g + 1]))
            cells = slice(int(e_off[g]), int(e_off[g + 1]))
            entry = {"members": np.flatnonzero(group == g),
                     "clusters": pd.DataFrame({name: cols[j][rows] for j, name in enumerate(
                         ("clusterStart", "clusterEnd", "peaks", "samples"))})}
            for j, name in enumerate(("peaks", "bases", "sum", "max")):
                entry[name] = cols[4 + j][cells].reshape(int(k[g]), int(m[g]))
            result.append(entry)
        return result

    def joint_peaks(self, groups, penalty=0.0, windows=None, first_chromStart=None,
                    torch_device=None):
        """One common peak per window for all members of a group, and which members carry it
        (peakseg_hip_problem_set_pack_joint_peaks; include/peaksegdisk_hip.h has the definitions:
        PeakSegPipeline's PeakSegJoint step), on the device from the resident runs of a set made by
        from_dense or from_reads.  groups as for peak_clusters().  penalty >= 0: the price of one
        more member with a peak.  windows: None -- the windows are the clusters of peak_clusters()
        (a solved set), each widened by its own width on either side; the call then packs those
        clusters in place of what peak_clusters() packed -- or a list over GROUPS of
        (start, end), 1-d contiguous int32 numpy arrays or torch tensors (an empty entry or None: no
        windows); tensors on the set's cuda device are read in place; one call takes one kind of
        memory; no solve is needed.  Every window is clipped to the extent all members of its group
        share.  first_chromStart as in segment_columns().  Without torch_device: a list over groups
        of {"members": the problems' indices, "joint": a data frame with the columns windowStart,
        windowEnd, peakStart, peakEnd, objective, samples_up, levels (peakStart = peakEnd = -1: no
        joint peak), and "gain" (float64), "up" (int32), "sum" (int64), "bases" (int32): (windows,
        members) arrays}.  With torch_device: (windows int64 numpy[n_groups + 1], entries int64
        numpy[n_groups + 1], windowStart, windowEnd, peakStart, peakEnd, objective, samples_up,
        levels, m_gain, m_up, m_sum, m_bases) where the eleven are tensors that alias the library's
        buffers (group g's windows are windows[g]:windows[g + 1], its matrix entries
        entries[g]:entries[g + 1], window-major); they are valid until the next solve(), the next
        joint_peaks() or close().  A window with start >= end, and a penalty that is negative or
        NaN, raise RuntimeError with .status 22."""
        group, n_groups, first, given, on_device = self._joint_arguments(
            "joint_peaks", groups, windows, first_chromStart)
        room = max(n_groups, 1)
        k = np.zeros(room, dtype=np.int64)
        m = np.zeros(room, dtype=np.int64)
        out = [ctypes.c_void_p() for _ in range(11)]
        total = self._lib.peakseg_hip_problem_set_pack_joint_peaks(
            self._h, first.ctypes.data if first is not None else None, n_groups, group.ctypes.data,
            float(penalty), *([ctypes.addressof(a) for a in given[:3]] if given else [None, None, None]),
            on_device, k.ctypes.data, m.ctypes.data, *[ctypes.byref(q) for q in out])
        del given  # (the library holds no reference to the caller's buffers after the call)
        if total < 0:
            self._raise_status("pack_joint_peaks", total)
        total = int(total)
        k, m = k[:n_groups], m[:n_groups]
        w_off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
        e_off = np.concatenate([[0], np.cumsum(k * m)]).astype(np.int64)
        entries = int(e_off[-1])
        sizes = (total,) * 7 + (entries,) * 4
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            return (w_off, e_off) + tuple(device_array(q.value or 0, n, dt, dev)
                                          for q, n, dt in zip(out, sizes, _JOINT_DTYPES))
        cols = [np.empty(n, dtype=dt) for n, dt in zip(sizes, _JOINT_DTYPES)]
        if self._lib.peakseg_hip_problem_set_packed_joint_peaks_download(
                self._h, *[a.ctypes.data for a in cols]) != 0:
            raise RuntimeError("packed_joint_peaks_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        return _joint_groups(group, n_groups, k, m, w_off, e_off, cols)

    def _joint_arguments(self, who, groups, windows, first_chromStart):
        """the arguments joint_peaks() and joint_path() share -> (group int32[], n_groups,
        first_chromStart or None, the three ctypes tables of given windows followed by what keeps
        their memory alive -- [] for windows=None --, 1 for windows in device memory)"""
        group = np.ascontiguousarray(groups, dtype=np.int32) if len(groups) else np.zeros(0, np.int32)
        if group.shape != (len(self.problems),):
            raise ValueError("%s: one group per problem (%d values, %d problems)"
                             % (who, group.size, len(self.problems)))
        if not np.array_equal(group, np.asarray(groups)):
            raise ValueError("%s: groups must be integers" % who)
        n_groups = int(group.max()) + 1 if group.size and group.max() >= 0 else 0
        first = self._first_chromStart(first_chromStart)
        keep, sides, lengths = [], [], None
        ptrs = ([], [])
        if windows is not None:
            if len(windows) != n_groups:
                raise ValueError("%s: one entry of windows per group (%d entries, %d groups)"
                                 % (who, len(windows), n_groups))
            lengths = []
            for g, entry in enumerate(windows):
                if entry is None or len(entry) == 0:
                    lengths.append(0)
                    for q in ptrs:
                        q.append(0)
                    continue
                if len(entry) != 2:
                    raise ValueError("%s: the windows of group %d are not (start, end)" % (who, g))
                n = None
                for j in range(2):
                    ptr, m, side, ref = _dense_pointer(
                        g, entry[j], self.device, who + ": group %d window " + ("start", "end")[j])
                    if n is not None and m != n:
                        raise ValueError("%s: group %d has %d window starts and %d ends"
                                         % (who, g, n, m))
                    n = m
                    keep.append(ref)
                    sides.append((side, g))
                    ptrs[j].append(ptr if m else 0)
                lengths.append(n)
            for side, g in sides:
                if side != sides[0][0]:
                    raise ValueError("%s: group %d is in %s memory but group %d is in %s "
                                     "memory; one call takes one kind"
                                     % (who, g, side, sides[0][1], sides[0][0]))
        room = max(n_groups, 1)
        given = []
        if lengths is not None:
            given = [(ctypes.c_longlong * room)(*lengths)] + [(ctypes.c_void_p * room)(*q) for q in ptrs]
            given.append(keep)
        return group, n_groups, first, given, 1 if sides and sides[0][0] == "device" else 0

    def joint_path(self, groups, penalties, windows=None, first_chromStart=None, torch_device=None):
        """joint_peaks() at every one of `penalties` in one call
        (peakseg_hip_problem_set_pack_joint_path): what does not depend on the penalty -- the
        level-0 bins, their fold, and the feasibility and the gain of every (candidate, member) --
        is computed once per window, and the number of launches is that of one joint_peaks().
        penalties: 1 to peakseg_hip_joint_path_max_penalties() (16) numbers >= 0 in any order,
        repeats and +inf allowed; the other arguments as joint_peaks().  Without torch_device: a
        list over penalties of exactly what joint_peaks() returns at that penalty, bit for bit.
        With torch_device: (windows int64 numpy[n_groups + 1], entries int64 numpy[n_groups + 1],
        and joint_peaks()'s eleven tensors with a leading penalty dimension: [n_penalties, windows]
        and [n_penalties, entries]), aliases of the library's buffers, valid until the next
        solve(), the next joint_path() or close() -- a joint_peaks() does not touch them, nor the
        other way round.  The penalties' number out of range, and a negative or NaN penalty (named
        by its index), raise RuntimeError with .status 22."""
        group, n_groups, first, given, on_device = self._joint_arguments(
            "joint_path", groups, windows, first_chromStart)
        pens = np.ascontiguousarray(penalties, dtype=np.float64).reshape(-1)
        n_pen = int(pens.size)
        room = max(n_groups, 1)
        k = np.zeros(room, dtype=np.int64)
        m = np.zeros(room, dtype=np.int64)
        out = [ctypes.c_void_p() for _ in range(11)]
        total = self._lib.peakseg_hip_problem_set_pack_joint_path(
            self._h, first.ctypes.data if first is not None else None, n_groups, group.ctypes.data,
            n_pen, pens.ctypes.data,
            *([ctypes.addressof(a) for a in given[:3]] if given else [None, None, None]),
            on_device, k.ctypes.data, m.ctypes.data, *[ctypes.byref(q) for q in out])
        del given  # (the library holds no reference to the caller's buffers after the call)
        if total < 0:
            self._raise_status("pack_joint_path", total)
        total = int(total)
        self._joint_path_penalties = n_pen
        k, m = k[:n_groups], m[:n_groups]
        w_off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
        e_off = np.concatenate([[0], np.cumsum(k * m)]).astype(np.int64)
        entries = int(e_off[-1])
        sizes = (total,) * 7 + (entries,) * 4
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            return (w_off, e_off) + tuple(
                device_array(q.value or 0, n_pen * n, dt, dev).view(n_pen, n)
                for q, n, dt in zip(out, sizes, _JOINT_DTYPES))
        cols = [np.empty(n_pen * n, dtype=dt) for n, dt in zip(sizes, _JOINT_DTYPES)]
        if self._lib.peakseg_hip_problem_set_packed_joint_path_download(
                self._h, *[a.ctypes.data for a in cols]) != 0:
            raise RuntimeError("packed_joint_path_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        return [_joint_groups(group, n_groups, k, m, w_off, e_off,
                              [a[p * n:(p + 1) * n] for a, n in zip(cols, sizes)])
                for p in range(n_pen)]

    def joint_label_errors(self, labels, torch_device=None):
        """The label errors of every model of the last joint_path(), counted on the device
        (peakseg_hip_problem_set_pack_joint_label_errors; include/peaksegdisk_hip.h has the
        definitions).  labels: a list over PROBLEMS of (chromStart, chromEnd, annotation) as
        label_errors() takes them per contig, in the genomic coordinates the joint peaks are in; an
        empty entry (or None) for a problem without labels.  The peaks of a problem in a model are
        the joint peaks of its group's windows at which it is up.  Returns (model_totals int64
        [n_penalties, 5], problem_totals int32 [n_penalties, n_problems, 5], rows): the totals are
        errors, fp, fn, possible_fp, possible_fn, and rows[p][q] is the (count, fp, fn) int32
        arrays of problem q's labels in model p.  With torch_device the totals and the three
        columns ([n_penalties, labels], problem after problem) are tensors that alias the library's
        buffers, as (offsets int64 numpy[n_problems + 1], count, fp, fn, problem_totals,
        model_totals), valid until the next solve(), joint_path(), joint_label_errors() or
        close()."""
        k = len(self.problems)
        if len(labels) != k:
            raise ValueError("joint_label_errors: one entry per problem (%d entries, %d problems)"
                             % (len(labels), k))
        names = ("chromStart", "chromEnd", "annotation")
        keep, sides, lengths = [], [], []
        ptrs = ([], [], [])
        for q, entry in enumerate(labels):
            if entry is None or len(entry) == 0:
                lengths.append(0)
                for col in ptrs:
                    col.append(0)
                continue
            if len(entry) != 3:
                raise ValueError("joint_label_errors: problem %d is not (chromStart, chromEnd, "
                                 "annotation)" % q)
            entry = list(entry)
            entry[2] = annotation_codes(entry[2], "joint_label_errors: problem %d" % q)
            n = None
            for j in range(3):
                ptr, m, side, ref = _dense_pointer(q, entry[j], self.device,
                                                   "joint_label_errors: problem %d " + names[j])
                if n is not None and m != n:
                    raise ValueError("joint_label_errors: problem %d has %d chromStart and %d %s"
                                     % (q, n, m, names[j]))
                n = m
                keep.append(ref)
                sides.append((side, q))
                ptrs[j].append(ptr if m else 0)
            lengths.append(n)
        for side, q in sides:
            if side != sides[0][0]:
                raise ValueError("joint_label_errors: problem %d is in %s memory but problem %d is "
                                 "in %s memory; one call takes one kind"
                                 % (q, side, sides[0][1], sides[0][0]))
        room = max(k, 1)
        out = [ctypes.c_void_p() for _ in range(5)]
        total = self._lib.peakseg_hip_problem_set_pack_joint_label_errors(
            self._h, (ctypes.c_longlong * room)(*lengths),
            *[(ctypes.c_void_p * room)(*col) for col in ptrs],
            1 if sides and sides[0][0] == "device" else 0, *[ctypes.byref(q) for q in out])
        del keep  # (the library holds no reference to the caller's buffers after the call)
        if total < 0:
            self._raise_status("pack_joint_label_errors", total)
        total = int(total)
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        n_pen = self._joint_path_penalties       # (the call succeeded: a path is packed)
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            cols = tuple(device_array(q.value or 0, n_pen * total, np.int32, dev).view(n_pen, total)
                         for q in out[:3])
            return (offs,) + cols + (
                device_array(out[3].value or 0, n_pen * k * 5, np.int32, dev).view(n_pen, k, 5),
                device_array(out[4].value or 0, n_pen * 5, np.int64, dev).view(n_pen, 5))
        cols = [np.empty(n_pen * total, dtype=np.int32) for _ in range(3)]
        totals = np.empty((n_pen, k, 5), dtype=np.int32)
        model = np.empty((n_pen, 5), dtype=np.int64)
        if self._lib.peakseg_hip_problem_set_packed_joint_label_errors_download(
                self._h, *[a.ctypes.data for a in cols], totals.ctypes.data, model.ctypes.data) != 0:
            raise RuntimeError("packed_joint_label_errors_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        rows = [[tuple(a[p * total + offs[q]:p * total + offs[q + 1]] for a in cols)
                 for q in range(k)] for p in range(n_pen)]
        return model, totals, rows

    def _pair_column(self, v, dtype, name):
        """(address, length, "host" | "device", what keeps the memory alive) of a column of
        heldout_loss(): a tensor on the set's cuda device as it is, anything else as a contiguous
        numpy array of `dtype` (integers must be integers)"""
        if type(v).__module__.split(".")[0] == "torch" and hasattr(v, "data_ptr"):
            import torch
            if v.device.type == "cuda":
                want = torch.int32 if dtype == np.int32 else torch.float64
                index = v.device.index if v.device.index is not None else torch.cuda.current_device()
                if v.dtype != want or v.dim() != 1 or not v.is_contiguous():
                    raise ValueError("heldout_loss: %s on the device must be a contiguous 1-d %s "
                                     "tensor" % (name, want))
                if index != self.device:
                    raise ValueError("heldout_loss: %s is on cuda:%d, the set on device %d"
                                     % (name, index, self.device))
                return v.data_ptr(), v.shape[0], "device", v
            v = v.numpy()
        given = np.asarray(v)
        a = np.ascontiguousarray(given, dtype=dtype).reshape(-1)
        if given.ndim > 1 or (dtype == np.int32 and given.size and not np.array_equal(a, given)):
            raise ValueError("heldout_loss: %s must be a 1-d array of %s"
                             % (name, "32-bit integers" if dtype == np.int32 else "numbers"))
        return a.ctypes.data, a.shape[0], "host", a

    def heldout_loss(self, pairs, torch_device=None):
        """The Poisson loss of the set's models on OTHER contigs of the set, on the device from
        the resident tables and runs of a solved set made by from_dense or from_reads
        (peakseg_hip_problem_set_pack_heldout_loss; include/peaksegdisk_hip.h has the definition):
        what scores a model fitted on part of the sampling units by the units that were held out.
        pairs: (problem, contig, scale) -- three 1-d arrays of equal length (integers, integers,
        numbers), or three contiguous tensors on the set's cuda device (int32, int32, float64) that
        are read in place; one call takes one kind of memory.  Pair i scores the model of problem
        problem[i] on contig contig[i], which must have the bases of the problem's own contig, with
        the segment means multiplied by scale[i] > 0.  Pairs may repeat and come in any order.
        Without torch_device: {"loss": float64[], "rows": int32[], "bases": int64[],
        "sum": int64[], "zero_mean_rows": int32[]}, one entry per pair (loss is +inf where a
        segment of mean 0 meets held-out counts; zero_mean_rows counts such segments).  With
        torch_device: the same dict of tensors that alias the library's buffers: nothing is
        downloaded, and they are valid until the next solve(), heldout_loss() or close().  A pair that
        cannot be scored raises RuntimeError with .status 23, naming the pair."""
        if len(pairs) != 3:
            raise ValueError("heldout_loss: pairs is not (problem, contig, scale)")
        cols = [self._pair_column(v, dt, name) for v, dt, name in zip(
            pairs, (np.int32, np.int32, np.float64), ("problem", "contig", "scale"))]
        n = cols[0][1]
        for (_, m, side, _), name in zip(cols, ("problem", "contig", "scale")):
            if m != n:
                raise ValueError("heldout_loss: %d problems and %d entries of %s" % (n, m, name))
            if side != cols[0][2]:
                raise ValueError("heldout_loss: %s is in %s memory but problem is in %s memory; "
                                 "one call takes one kind" % (name, side, cols[0][2]))
        out = [ctypes.c_void_p() for _ in range(5)]
        total = self._lib.peakseg_hip_problem_set_pack_heldout_loss(
            self._h, n, *[q[0] if n else None for q in cols], 1 if cols[0][2] == "device" else 0,
            *[ctypes.byref(q) for q in out])
        del cols  # (the library holds no reference to the caller's buffers after the call)
        if total < 0:
            self._raise_status("pack_heldout_loss", total)
        names = ("loss", "rows", "bases", "sum", "zero_mean_rows")
        dtypes = (np.float64, np.int32, np.int64, np.int64, np.int32)
        if torch_device is not None:
            import torch
            from .parallel import device_array
            dev = torch.device(torch_device)
            return {name: device_array(q.value or 0, n, dt, dev)
                    for name, q, dt in zip(names, out, dtypes)}
        result = [np.empty(n, dtype=dt) for dt in dtypes]
        if self._lib.peakseg_hip_problem_set_packed_heldout_loss_download(
                self._h, *[a.ctypes.data for a in result]) != 0:
            raise RuntimeError("packed_heldout_loss_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        return dict(zip(names, result))

    def _coverage_stats(self, ranks, torch_device=None):
        """one peakseg_hip_problem_set_pack_coverage_stats: ranks int64 [n_contigs, k], k at most
        max_ranks -> (value int32 [n_contigs, k], moments uint64 [n_contigs, 6]); with torch_device
        the value is a tensor that aliases the library's buffer"""
        nc, k = ranks.shape
        value_dev, moments_dev = ctypes.c_void_p(), ctypes.c_void_p()
        total = self._lib.peakseg_hip_problem_set_pack_coverage_stats(
            self._h, k, ranks.ctypes.data if k else None, ctypes.byref(value_dev),
            ctypes.byref(moments_dev))
        if total < 0:
            err = RuntimeError("pack_coverage_stats: %s"
                               % self._lib.peakseg_hip_last_error().decode())
            err.status = int(-total) if total < -1 else _native.ERROR_DEVICE_SOLVER
            raise err
        moments = np.empty((nc, MOMENT_WORDS), dtype=np.uint64)
        value = np.empty((nc, k), dtype=np.int32)
        on_device = torch_device is not None
        if self._lib.peakseg_hip_problem_set_packed_coverage_stats_download(
                self._h, None if on_device or not k else value.ctypes.data,
                moments.ctypes.data) != 0:
            raise RuntimeError("packed_coverage_stats_download: %s"
                               % self._lib.peakseg_hip_last_error().decode())
        if on_device:
            import torch
            from .parallel import device_array
            value = device_array(value_dev.value or 0, nc * k, np.int32,
                                 torch.device(torch_device)).view(nc, k)
        return value, moments

    def _n_contigs(self):
        return len(self.contig_bases) if self.dense else len(self.contigs)

    def coverage_order_statistics(self, ranks, torch_device=None):
        """Order statistics of every contig's per-base coverage x (a set made by from_dense or
        from_reads, solved or not), selected on the device from the resident runs
        (peakseg_hip_problem_set_pack_coverage_stats): for the 0-based rank r, sort(x)[r].  ranks: an
        integer array [n_contigs, k], or one row of k ranks for all contigs; a rank outside
        [0, bases) of its contig raises RuntimeError with .status 20, naming the contig and the rank.
        Returns int32 [n_contigs, k].  More ranks than the library takes in one call
        (peakseg_hip_coverage_stats_max_ranks) make several calls.  With torch_device: a tensor on
        that device -- of a single call it aliases the library's buffer and is valid until the next
        coverage_* call or close(); of several calls it is their copies, joined."""
        nc = self._n_contigs()
        ranks = np.asarray(ranks)
        if ranks.size and not np.issubdtype(ranks.dtype, np.integer):
            raise ValueError("coverage_order_statistics: ranks must be integers")
        if ranks.ndim == 1:
            ranks = np.broadcast_to(ranks, (nc, ranks.shape[0]))
        if ranks.ndim != 2 or ranks.shape[0] != nc:
            raise ValueError("coverage_order_statistics: ranks: [n_contigs, k] or one row for all "
                             "(%d contigs)" % nc)
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        most = int(self._lib.peakseg_hip_coverage_stats_max_ranks())
        k = ranks.shape[1]
        if k <= most:
            return self._coverage_stats(ranks, torch_device)[0]
        parts = []
        for at in range(0, k, most):
            part = self._coverage_stats(np.ascontiguousarray(ranks[:, at:at + most]), torch_device)[0]
            parts.append(part.clone() if torch_device is not None else part)
        if torch_device is not None:
            import torch
            return torch.cat(parts, dim=1)
        return np.concatenate(parts, axis=1)

    @staticmethod
    def _moment_columns(moments):
        s2 = np.empty(len(moments), dtype=object)
        for c, row in enumerate(moments.tolist()):
            s2[c] = row[3] + (row[4] << 17) + (row[5] << 32)
        return {"bases": moments[:, 0].astype(np.int64), "runs": moments[:, 1].astype(np.int64),
                "sum": moments[:, 2].astype(np.int64), "sum_sq": s2}

    def coverage_moments(self):
        """{"bases", "runs", "sum": int64 arrays, "sum_sq": an object array of Python ints}, one
        entry per contig: the number of bases of its per-base coverage x, the runs of its encoding,
        sum(x) and sum(x ** 2) (which may reach 2^84: the device carries it exactly in three 64-bit
        words), summed on the device from the resident runs."""
        return self._moment_columns(
            self._coverage_stats(np.zeros((self._n_contigs(), 0), dtype=np.int64))[1])

    def coverage_quantiles(self, probs=(0, .25, .5, .75, 1)):
        """float64 [n_contigs, len(probs)]: the type-7 quantiles (R's default, numpy's "linear") of
        every contig's per-base coverage x: with h = (len(x) - 1) p, lo = floor(h), g = h - lo,
        x_(lo) + (x_(lo + 1) - x_(lo)) g.  For multiples of 1/4, lo and g come from integer
        arithmetic and the result is np.quantile(x, p) bit for bit.  The order statistics are
        selected on the device (coverage_order_statistics).  NaN or a prob outside [0, 1]: ValueError."""
        probs = [float(p) for p in probs]
        for p in probs:
            if not 0.0 <= p <= 1.0:      # (NaN fails both)
                raise ValueError("coverage_quantiles: prob %r is not in [0, 1]" % p)
        nc = self._n_contigs()
        lo = np.zeros((nc, len(probs)), dtype=np.int64)
        g = np.zeros((nc, len(probs)), dtype=np.float64)
        last = np.zeros((nc, 1), dtype=np.int64)
        if self.dense:
            last[:, 0] = np.asarray(self.contig_bases, dtype=np.int64) - 1
        for j, p in enumerate(probs):
            if (4.0 * p).is_integer():
                h4 = last[:, 0] * int(4.0 * p)
                lo[:, j], g[:, j] = h4 // 4, (h4 % 4) / 4.0
            else:
                h = last[:, 0].astype(np.float64) * p
                lo[:, j] = np.floor(h).astype(np.int64)
                g[:, j] = h - np.floor(h)
        value = self.coverage_order_statistics(
            np.concatenate([lo, np.minimum(lo + 1, last)], axis=1)).astype(np.float64)
        a, b = value[:, :len(probs)], value[:, len(probs):]
        return a + (b - a) * g

    def coverage_features(self):
        """The inputs of a penalty-learning regression: a pandas data frame with one row per contig
        and the 36 columns FEATURE_NAMES -- the quartiles, mean, sd, bases and data (runs) of the
        contig's per-base coverage, and each of them under log(v + 1), log(v) and log(log(v))
        (features_from_stats has the definitions).  One call of the library for the order
        statistics and the moments, from the resident runs; nothing of the coverage is downloaded."""
        import pandas as pd
        nc = self._n_contigs()
        ranks = np.zeros((nc, 10), dtype=np.int64)
        for c in range(nc if self.dense else 0):
            lo, hi, _ = quartile_ranks(int(self.contig_bases[c]))
            ranks[c] = lo + hi
        value, moments = self._coverage_stats(ranks)
        cols = self._moment_columns(moments)
        rows = [features_from_stats(value[c, :5], value[c, 5:], cols["bases"][c], cols["runs"][c],
                                    cols["sum"][c], cols["sum_sq"][c]) for c in range(nc)]
        return pd.DataFrame(np.array(rows, dtype=np.float64).reshape(nc, len(FEATURE_NAMES)),
                            columns=list(FEATURE_NAMES))

    def loss(self, p):
        """The ten fields of the reference's loss.tsv row of problem p (api.col_name_list["loss"]),
        as float64."""
        out = (ctypes.c_double * 10)()
        if self._lib.peakseg_hip_problem_set_loss(self._h, p, out) != 0:
            raise RuntimeError("no loss row for problem %d" % p)
        return np.array(out[:], dtype=np.float64)

    def solve(self):
        """Forward DP + backtrack for every problem; returns (forward_ms, backtrack_ms)."""
        f = ctypes.c_float()
        b = ctypes.c_float()
        st = self._lib.peakseg_hip_problem_set_solve(self._h, ctypes.byref(f), ctypes.byref(b))
        if st != 0:
            err = RuntimeError("peakseg_hip_problem_set_solve: status %d: %s" % (
                st, self._lib.peakseg_hip_last_error().decode()))
            err.status = st
            raise err
        return f.value, b.value

    def result(self, p):
        r = _native.PsdResult()
        if self._lib.peakseg_hip_problem_set_result(self._h, p, ctypes.byref(r)) != 0:
            raise RuntimeError("no result for problem %d" % p)
        return r

    def segments(self, p):
        """(seg_start_index, seg_mean) in the reference's output order (last segment first)."""
        r = self.result(p)
        start = np.empty(max(r.n_segments, 1), dtype=np.int32)
        mean = np.empty(max(r.n_segments, 1), dtype=np.float64)
        n = self._lib.peakseg_hip_problem_set_segments(
            self._h, p, r.n_segments, start.ctypes.data, mean.ctypes.data)
        if n < 0:
            raise RuntimeError("segments(%d): %s" % (p, self._lib.peakseg_hip_last_error().decode()))
        return start[:n], mean[:n]

    def export_db(self, p, chrom_end, path):
        ce = np.ascontiguousarray(chrom_end, dtype=np.int32)
        if self._lib.peakseg_hip_problem_set_export_db(self._h, p, ce.ctypes.data,
                                                       path.encode()) != 0:
            raise RuntimeError("export_db failed")

    @property
    def kernel_build(self):
        """'lat' or 'thr': which build of the forward kernel the last solve() used."""
        return self._lib.peakseg_hip_problem_set_kernel_build(self._h).decode()

    @property
    def hbm_bytes(self):
        return int(self._lib.peakseg_hip_problem_set_bytes(self._h))

    @property
    def checkpoint_interval(self):
        """0: every cost function is kept in HBM; K > 0: checkpointed store (recompute)."""
        return int(self._lib.peakseg_hip_problem_set_checkpoint_interval(self._h))

    @property
    def arena_bytes_used(self):
        """bytes of the arena the last solve() handed out"""
        return int(self._lib.peakseg_hip_problem_set_arena_bytes_used(self._h))

    @property
    def solve_stats(self):
        """(kernel launches, data points worked through) of the last solve(): one launch and the
        sum of the problems' lengths unless a store had to grow."""
        n = ctypes.c_int()
        steps = ctypes.c_ulonglong()
        self._lib.peakseg_hip_problem_set_solve_stats(self._h, ctypes.byref(n), ctypes.byref(steps))
        return n.value, steps.value

    @property
    def arena_stats(self):
        """(pieces per arena block, blocks mapped now, blocks the last solve() mapped while its
        kernels were running)"""
        bp = ctypes.c_ulonglong()
        nb = ctypes.c_int()
        live = ctypes.c_int()
        self._lib.peakseg_hip_problem_set_arena_stats(self._h, ctypes.byref(bp), ctypes.byref(nb),
                                                      ctypes.byref(live))
        return bp.value, nb.value, live.value

    @property
    def park_stats(self):
        """(problems parked by the last solve()'s launches, pieces of the overflow pool those
        parks took)"""
        n = ctypes.c_int()
        pool = ctypes.c_ulonglong()
        self._lib.peakseg_hip_problem_set_park_stats(self._h, ctypes.byref(n), ctypes.byref(pool))
        return n.value, pool.value

    def pack_tables(self):
        """Pack every problem's segment table at its exact size in HBM.  Returns (rows int64[k],
        device address of the packed seg_start int32 array, of the packed seg_mean float64
        array, total rows); the addresses stay valid until the next solve() / close()."""
        rows = np.zeros(len(self.problems), dtype=np.int64)
        ps = ctypes.c_void_p()
        pm = ctypes.c_void_p()
        total = self._lib.peakseg_hip_problem_set_pack_tables(
            self._h, rows.ctypes.data, ctypes.byref(ps), ctypes.byref(pm))
        if total < 0:
            raise RuntimeError("pack_tables: %s" % self._lib.peakseg_hip_last_error().decode())
        return rows, ps.value or 0, pm.value or 0, int(total)

    def packed_download(self, total):
        """the packed tables of pack_tables() as host arrays"""
        start = np.empty(total, dtype=np.int32)
        mean = np.empty(total, dtype=np.float64)
        if self._lib.peakseg_hip_problem_set_packed_download(self._h, start.ctypes.data,
                                                             mean.ctypes.data) != 0:
            raise RuntimeError("packed_download: %s" % self._lib.peakseg_hip_last_error().decode())
        return start, mean

    def cycles_per_step(self, p):
        """shader cycles per data point of problem p in the last solve() (0.0 when unknown,
        e.g. under the SIMT emulator, or when the problem was resumed after a park)"""
        cyc = int(self._lib.peakseg_hip_problem_set_cycles(self._h, p))
        if cyc <= 0 or self.solve_stats[0] != 1:
            return 0.0
        return cyc / float(len(self.contigs[self.problems[p][0]][0]))

    def set_penalty(self, p, penalty):
        """Change one problem's penalty in place; the next solve() reuses contig and arena."""
        if self._lib.peakseg_hip_problem_set_set_penalty(self._h, p, float(penalty)) != 0:
            raise RuntimeError("set_penalty(%d) failed" % p)
        self.problems[p] = (self.problems[p][0], float(penalty))

    def close(self):
        if self._h:
            self._lib.peakseg_hip_problem_set_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
