"""Host-side mirror of the reference's R entry points for the PeakSegFPOP path.

R is not installed in this image, so the layer the reference keeps in R
(/root/reference/R/*.R) is mirrored here in Python with the same names, argument meaning,
file protocol and error messages; the native call goes through the same C ABI the R glue
would use.  Data frames are pandas.DataFrame, R lists are plain classes.

  PeakSegFPOP_file     <- R/PeakSegFPOP_file.R:30-87
  PeakSegFPOP_dir      <- R/PeakSegFPOP_dir.R:47-117   (+ coef / summary, :215-238)
  PeakSegFPOP_df       <- R/PeakSegFPOP_df.R:18-35
  PeakSegFPOP_vec      <- R/PeakSegFPOP_vec.R:9-25
  sequentialSearch_dir <- R/sequentialSearch_dir.R:22-103
  writeBedGraph        <- R/writeBedGraph.R:8-38
  col_name_list        <- R/col.name.list.R:10-18
"""
import math
import os
import shutil
import tempfile
import time

import numpy as np
import pandas as pd

from . import _native

col_name_list = {
    "loss": ["penalty", "segments", "peaks", "bases", "bedGraph.lines", "mean.pen.cost",
             "total.loss", "equality.constraints", "mean.intervals", "max.intervals"],
    "segments": ["chrom", "chromStart", "chromEnd", "status", "mean"],
    "coverage": ["chrom", "chromStart", "chromEnd", "count"],
}


class PeakSegError(RuntimeError):
    """Raised where the reference's glue calls Rf_error (src/interface.cpp:16-55)."""

    def __init__(self, status, message):
        RuntimeError.__init__(self, message)
        self.status = status


def paste(x):
    """R's paste()/as.character() of a scalar: doubles use up to 15 significant digits and
    the narrower of fixed / scientific notation (R formatReal with digits=15)."""
    if isinstance(x, str):
        return x
    if isinstance(x, (bool, np.bool_)):
        return "TRUE" if x else "FALSE"
    if isinstance(x, (int, np.integer)):
        return "%d" % x
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    if x == 0:
        return "0"
    # minimal number of significant digits (<= 15) that reproduces the 15-digit value
    target = float("%.14e" % x)
    nsig = 15
    for d in range(1, 16):
        if float("%.*e" % (d - 1, x)) == target:
            nsig = d
            break
    mant, exp = ("%.*e" % (nsig - 1, x)).split("e")
    kpower = int(exp)
    neg = 1 if x < 0 else 0
    if kpower >= 0:
        left = kpower + 1
        rgt = max(0, nsig - kpower - 1)
    else:
        left = 1
        rgt = nsig - kpower - 1
    w_fixed = neg + left + (rgt + 1 if rgt > 0 else 0)
    w_sci = neg + (nsig + 1 if nsig > 1 else 1) + (5 if abs(kpower) >= 100 else 4)
    if w_fixed <= w_sci:
        return "%.*f" % (rgt, x)
    return "%.*e" % (nsig - 1, x)


# ---- writeBedGraph (R/writeBedGraph.R:8-38) ------------------------------------------------

def writeBedGraph(count_df, coverage_bedGraph):
    if not isinstance(count_df, pd.DataFrame):
        raise ValueError("count.df must be data.frame")
    exp_names = ["chrom", "chromStart", "chromEnd", "count"]
    if list(count_df.columns) != exp_names:
        raise ValueError("count.df must have names " + ", ".join(exp_names))
    if not pd.api.types.is_integer_dtype(count_df["chromStart"]):
        raise ValueError("count.df$chromStart must be integer")
    if not pd.api.types.is_integer_dtype(count_df["chromEnd"]):
        raise ValueError("count.df$chromEnd must be integer")
    if not pd.api.types.is_numeric_dtype(count_df["count"]):
        raise ValueError("count.df$count must be numeric")
    if (count_df["chromStart"] < 0).any():
        raise ValueError("count.df$chromStart must always be non-negative")
    if not (count_df["chromStart"] < count_df["chromEnd"]).all():
        raise ValueError("chromStart must be less than chromEnd for all rows of count.df")
    with open(coverage_bedGraph, "w") as f:
        for chrom, s, e, c in zip(count_df["chrom"], count_df["chromStart"],
                                  count_df["chromEnd"], count_df["count"]):
            f.write("%s\t%d\t%d\t%s\n" % (chrom, s, e, paste(c)))


# ---- PeakSegFPOP_file (R/PeakSegFPOP_file.R:30-87) -----------------------------------------

def _native_interface(bedGraph_file, pen_str, db_file):
    """`.C("PeakSegFPOP_interface", ...)`: run the solver, turn a status into the
    reference's error text (src/interface.cpp:10-56)."""
    status = _native.lib.PeakSegFPOP_disk(
        os.fsencode(bedGraph_file), pen_str.encode(), os.fsencode(db_file))
    if status != 0:
        msg = _native.status_message(status, bedGraph_file, pen_str, db_file)
        detail = _native.last_error()
        if status >= _native.ERROR_NO_HIP_DEVICE and detail:
            msg = "%s (%s)" % (msg, detail)
        raise PeakSegError(status, msg)


def PeakSegFPOP_file(bedGraph_file, pen_str, db_file=None):
    if not (isinstance(bedGraph_file, str) and os.path.exists(bedGraph_file)):
        raise ValueError("bedGraph.file=%s must be the name of a data file to segment"
                         % (bedGraph_file,))
    if not isinstance(pen_str, str):
        raise ValueError("pen.str must be a character string that can be converted to a "
                         "non-negative numeric scalar")
    try:
        penalty = float(pen_str)  # as.numeric(pen.str); "Inf" is fine
    except ValueError:
        penalty = float("nan")
    if not (0 <= penalty <= float("inf")):
        raise ValueError("as.numeric(pen.str)=%s but it must be a non-negative numeric scalar"
                         % paste(penalty))
    norm_file = os.path.realpath(bedGraph_file)
    if db_file is None:
        db_file = "%s_penalty=%s.db" % (norm_file, pen_str)
    if not isinstance(db_file, str):
        raise ValueError("db.file=%s must be a temporary file name where cost function db "
                         "can be written" % (db_file,))
    if os.path.isfile(db_file):
        os.unlink(db_file)
    _native_interface(norm_file, pen_str, db_file)
    result = {"bedGraph.file": norm_file, "penalty": pen_str, "db.file": db_file}
    result["megabytes"] = (os.path.getsize(db_file) / 1024 / 1024
                           if os.path.isfile(db_file) else 0)
    if os.path.isfile(db_file):
        os.unlink(db_file)
    loss_tsv = "%s_penalty=%s_loss.tsv" % (bedGraph_file, pen_str)
    if os.path.getsize(loss_tsv) == 0:
        raise PeakSegError(8, "unable to write to loss output file %s (disk is probably full)"
                           % loss_tsv)
    return result


# ---- PeakSegFPOP_dir (R/PeakSegFPOP_dir.R:47-117) ------------------------------------------

class PeakSegFPOP_dir_result:
    """R list of class c("PeakSegFPOP_dir","list"): $segments, $loss (+ $data, $others)."""

    def __init__(self, segments, loss):
        self.segments = segments
        self.loss = loss
        self.data = None
        self.others = None
        self.classes = ["PeakSegFPOP_dir", "list"]

    def summary(self):  # summary.PeakSegFPOP_dir (R/PeakSegFPOP_dir.R:234-238)
        return self.loss

    def coef(self):  # coef.PeakSegFPOP_dir (R/PeakSegFPOP_dir.R:215-231)
        seg = self.segments
        d = np.diff(seg["mean"].to_numpy())
        changes = pd.DataFrame({
            "type": "segmentation",
            "constraint": np.where(d == 0, "equality", "inequality"),
            "chromEnd": seg["chromEnd"].to_numpy()[1:]})
        peaks = seg[seg["status"] == "peak"].copy()
        peaks.insert(0, "type", "peaks")
        out = PeakSegFPOP_dir_result(seg.assign(type="segmentation")[["type"] + list(seg.columns)],
                                     self.loss)
        out.changes = changes
        out.peaks = peaks
        out.data = self.data
        return out


def _read_table(path, names):
    """fread(file=..., col.names=names) of one of the solver's tab-separated files."""
    if os.path.getsize(path) == 0:
        raise ValueError("empty file %s" % path)
    # (round_trip: the default parser of read_csv is off by an ulp on some 20-digit fields,
    # and a penalty read back from _loss.tsv must print as the string that named the file)
    return pd.read_csv(path, sep="\t", header=None, names=names, na_filter=False,
                       float_precision="round_trip")


def _first_last_line(path, names):
    with open(path, "rb") as f:
        first = f.readline()
        f.seek(0, os.SEEK_END)
        size = f.tell()
        if size == 0 or not first.strip():
            raise ValueError("empty file")
        back = min(size, 4096)
        f.seek(size - back)
        tail = f.read().splitlines()
        last = tail[-1] if tail[-1].strip() else tail[-2]

    def parse(line):
        vals = line.decode().split()
        if len(vals) != len(names):
            raise ValueError("bad column count")
        return dict(zip(names, vals))
    return parse(first), parse(last)


def _already_computed(prob_cov_bedGraph, segments_bed, loss_tsv, timing_tsv):
    """The cache predicate of R/PeakSegFPOP_dir.R:70-93 (any error means recompute)."""
    try:
        timing = _read_table(timing_tsv, ["penalty", "megabytes", "seconds"])
        first_seg, last_seg = _first_last_line(segments_bed, col_name_list["segments"])
        first_cov, last_cov = _first_last_line(prob_cov_bedGraph, col_name_list["coverage"])
        loss = _read_table(loss_tsv, col_name_list["loss"])
        nrow_ok = len(timing) == 1 and len(loss) == 1
        consistent = (int(first_seg["chromEnd"]) - int(last_seg["chromStart"])
                      == int(loss["bases"].iloc[0]))
        start_ok = int(first_cov["chromStart"]) == int(last_seg["chromStart"])
        end_ok = int(last_cov["chromEnd"]) == int(first_seg["chromEnd"])
        if nrow_ok and consistent and start_ok and end_ok:
            return timing, loss
    except Exception:
        pass
    return None


def PeakSegFPOP_dir(problem_dir, penalty_param, db_file=None):
    if not (isinstance(problem_dir, str) and os.path.isdir(problem_dir)):
        raise ValueError("problem.dir=%s must be the name of a directory containing a file "
                         "named coverage.bedGraph" % (problem_dir,))
    ok_type = isinstance(penalty_param, (int, float, str, np.integer, np.floating)) and \
        not isinstance(penalty_param, bool)
    if not ok_type or (isinstance(penalty_param, float) and math.isnan(penalty_param)):
        raise ValueError("penalty.param must be numeric or character, length 1, not missing")
    penalty_str = paste(penalty_param)
    prob_cov_bedGraph = os.path.join(problem_dir, "coverage.bedGraph")
    pre = "%s_penalty=%s" % (prob_cov_bedGraph, penalty_str)
    penalty_segments_bed = pre + "_segments.bed"
    penalty_loss_tsv = pre + "_loss.tsv"
    penalty_timing_tsv = pre + "_timing.tsv"
    cached = _already_computed(prob_cov_bedGraph, penalty_segments_bed, penalty_loss_tsv,
                               penalty_timing_tsv)
    if cached is None:
        t0 = time.time()
        result = PeakSegFPOP_file(prob_cov_bedGraph, penalty_str, db_file)
        seconds = time.time() - t0
        timing = pd.DataFrame({"penalty": [float(penalty_str)],
                               "megabytes": [result["megabytes"]], "seconds": [seconds]})
        with open(penalty_timing_tsv, "w") as f:
            f.write("%s\t%s\t%s\n" % (paste(float(penalty_str)), paste(result["megabytes"]),
                                      paste(seconds)))
        penalty_loss = _read_table(penalty_loss_tsv, col_name_list["loss"])
    else:
        timing, penalty_loss = cached
    penalty_segs = _read_table(penalty_segments_bed, col_name_list["segments"])
    loss = penalty_loss.copy()
    loss["megabytes"] = float(timing["megabytes"].iloc[0])
    loss["seconds"] = float(timing["seconds"].iloc[0])
    return PeakSegFPOP_dir_result(penalty_segs, loss)


# ---- PeakSegFPOP_df / _vec (R/PeakSegFPOP_df.R:18-35, R/PeakSegFPOP_vec.R:9-25) -------------

def _check_pen_num(pen_num):
    if not (isinstance(pen_num, (int, float, np.integer, np.floating))
            and not isinstance(pen_num, bool) and 0 <= pen_num):
        raise ValueError("pen.num must be non-negative numeric scalar")


def PeakSegFPOP_df(count_df, pen_num, base_dir=None):
    _check_pen_num(pen_num)
    if base_dir is None:
        base_dir = tempfile.gettempdir()
    data_dir = os.path.join(base_dir, "%s-%d-%d" % (
        count_df["chrom"].iloc[0], count_df["chromStart"].min(), count_df["chromEnd"].max()))
    shutil.rmtree(data_dir, ignore_errors=True)
    os.makedirs(data_dir, exist_ok=True)
    coverage_bedGraph = os.path.join(data_dir, "coverage.bedGraph")
    writeBedGraph(count_df, coverage_bedGraph)
    L = PeakSegFPOP_dir(data_dir, paste(pen_num))
    L.data = count_df.copy()
    L.classes = ["PeakSegFPOP_df"] + L.classes
    return L


def PeakSegFPOP_vec(count_vec, pen_num):
    _check_pen_num(pen_num)
    count_vec = np.asarray(count_vec)
    if not np.issubdtype(count_vec.dtype, np.integer):
        raise ValueError("count.vec must be integer")
    # rle(count.vec)
    change = np.flatnonzero(np.diff(count_vec) != 0)
    ends = np.concatenate([change + 1, [len(count_vec)]]).astype(np.int64)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    coverage_df = pd.DataFrame({"chrom": "chrUnknown", "chromStart": starts, "chromEnd": ends,
                                "count": count_vec[starts]})
    return PeakSegFPOP_df(coverage_df, pen_num)


# ---- dense coverage in memory (additive: no file anywhere) ----------------------------------

def _read_text_table(text, names):
    """_read_table of what the solver would have written, without the file"""
    import io
    return pd.read_csv(io.StringIO(text), sep="\t", header=None, names=names, na_filter=False,
                       float_precision="round_trip")


def _int32_vector(v, name="count.vec"):
    """an integer vector as the library takes it: int32 arrays and tensors as they are, other
    integer arrays converted when they fit"""
    if hasattr(v, "data_ptr"):
        return v
    v = np.asarray(v)
    if not np.issubdtype(v.dtype, np.integer):
        raise ValueError("%s must be integer" % name)
    if v.dtype != np.int32:
        if v.size and (v.max() > 2 ** 31 - 1 or v.min() < -2 ** 31):
            raise ValueError("%s must fit 32-bit integers" % name)
        v = v.astype(np.int32)
    return np.ascontiguousarray(v)


def _penalty_lists(penalties, n_contigs, noun):
    """one list of penalties for all contigs, or one per contig -> one per contig, checked"""
    pens = list(penalties) if not isinstance(penalties, (int, float, np.integer, np.floating)) \
        else [penalties]
    per_vec = len(pens) > 0 and isinstance(pens[0], (list, tuple, np.ndarray))
    if per_vec:
        if len(pens) != n_contigs:
            raise ValueError("penalties: one list per %s (%d lists, %d %ss)"
                             % (noun, len(pens), n_contigs, noun))
        pens = [list(q) for q in pens]
    else:
        pens = [pens] * n_contigs
    for q in pens:
        for pen_num in q:
            _check_pen_num(pen_num)
    return pens


LABEL_STATUS = ("correct", "false positive", "false negative")


def _label_lists(labels, n_contigs, single, noun):
    """`labels` of PeakSegFPOP_dense / PeakSegFPOP_reads / the target-interval entries -> one
    (chromStart, chromEnd, annotation codes) of host int32 arrays per contig.  A single contig
    takes its entry bare; None or an empty entry is a contig without labels."""
    from .grid import annotation_codes
    if single:
        labels = [labels]
    if len(labels) != n_contigs:
        raise ValueError("labels: one entry per %s (%d entries, %d %ss)"
                         % (noun, len(labels), n_contigs, noun))
    out = []
    for c, entry in enumerate(labels):
        if entry is None or len(entry) == 0:
            out.append(tuple(np.zeros(0, dtype=np.int32) for _ in range(3)))
            continue
        if len(entry) != 3:
            raise ValueError("labels: %s %d is not (chromStart, chromEnd, annotation)" % (noun, c))
        codes = annotation_codes(entry[2], "labels: %s %d" % (noun, c))
        cols = []
        for v in (entry[0], entry[1], codes):
            if hasattr(v, "data_ptr"):
                v = v.cpu().numpy()
            cols.append(_int32_vector(v, "labels"))
        if not (len(cols[0]) == len(cols[1]) == len(cols[2])):
            raise ValueError("labels: %s %d: columns of different lengths" % (noun, c))
        out.append(tuple(cols))
    return out


def _label_frame(chrom, entry, columns):
    """the .label_errors data frame of one model: the contig's labels and what the model does"""
    from .grid import ANNOTATIONS
    count, fp, fn = columns
    status = np.where(fp != 0, LABEL_STATUS[1], np.where(fn != 0, LABEL_STATUS[2], LABEL_STATUS[0]))
    return pd.DataFrame({
        "chrom": chrom, "chromStart": entry[0], "chromEnd": entry[1],
        "annotation": np.array(ANNOTATIONS, dtype=object)[entry[2]] if len(entry[2]) else
        np.zeros(0, dtype=object),
        "count": count, "fp": fp, "fn": fn, "status": status},
        columns=["chrom", "chromStart", "chromEnd", "annotation", "count", "fp", "fn", "status"])


LABEL_TOTALS = ["errors", "fp", "fn", "possible.fp", "possible.fn"]


def _solve_dense_set(make_set, pens, chrom, stats, single, label, labels=None, penalty_model=None,
                     cluster_groups=None, joint_penalty=None, joint_search=None):
    """What PeakSegFPOP_dense and PeakSegFPOP_reads share: the problems of `pens` (one list per
    contig), the set -- make_set(problems) -> (ProblemSet, chromStart of each contig's first
    base) --, its solution, and the reference's data frames, nested as `pens` is.
    penalty_model: `pens` holds one placeholder (Inf) per contig; every problem gets the penalty
    the model predicts from the set's coverage features before the one solve.
    cluster_groups: one group per problem; the solved set's ProblemSet.peak_clusters() is returned
    with the data frames, as (frames, clusters); with joint_penalty its ProblemSet.joint_peaks() on
    the clusters' windows too, as (frames, clusters, joint); with joint_search -- the keyword
    arguments of joint_target.joint_target_interval, `labels` among them -- that search on the
    clusters' windows instead, as (frames, clusters, JointTargetInterval)."""
    if labels is not None:
        labels = _label_lists(labels, len(pens), single, "contig")
    problems, pen_strs = [], []
    for c, q in enumerate(pens):
        for pen_num in q:
            pen_strs.append(paste(pen_num))
            problems.append((c, float(pen_strs[-1])))
    if not problems:
        return [] if single else [[] for _ in pens]
    t0 = time.time()
    try:
        pset, chrom_starts = make_set(problems)
    except RuntimeError as e:
        status = getattr(e, "status", _native.ERROR_DEVICE_SOLVER)
        msg = _native.status_message(status, label, "", "")
        detail = _native.last_error()
        raise PeakSegError(status, "%s (%s)" % (msg, detail) if detail else msg)
    try:
        features = None
        if penalty_model is not None:
            features = pset.coverage_features()
            for p, pen_num in enumerate(predict_penalties(features, penalty_model).tolist()):
                _check_pen_num(pen_num)
                pen_strs[p] = paste(pen_num)
                problems[p] = (problems[p][0], float(pen_strs[p]))
                pset.set_penalty(p, problems[p][1])
        try:
            pset.solve()
        except RuntimeError as e:
            raise PeakSegError(_native.ERROR_DEVICE_SOLVER, str(e))
        columns = pset.segment_columns(first_chromStart=chrom_starts)
        seg_stats = pset.segment_stats(first_chromStart=chrom_starts) if stats else None
        if labels is not None:
            try:
                label_totals, label_cols = pset.label_errors(labels, first_chromStart=chrom_starts)
            except RuntimeError as e:
                raise PeakSegError(getattr(e, "status", _native.ERROR_DEVICE_SOLVER), str(e))
        clusters = None
        if cluster_groups is not None:
            try:
                clusters = pset.peak_clusters(cluster_groups, first_chromStart=chrom_starts)
                if joint_penalty is not None:
                    clusters = (clusters, pset.joint_peaks(cluster_groups, penalty=joint_penalty,
                                                           first_chromStart=chrom_starts))
                elif joint_search is not None:
                    from .joint_target import joint_target_interval
                    clusters = (clusters, joint_target_interval(
                        pset, cluster_groups, first_chromStart=chrom_starts, **joint_search))
            except RuntimeError as e:
                raise PeakSegError(getattr(e, "status", _native.ERROR_DEVICE_SOLVER), str(e))
        rows = [(pset.loss(p), pset.result(p)) for p in range(len(problems))]
    finally:
        pset.close()
    seconds = (time.time() - t0) / len(problems)
    flat = []
    for p, (c, _) in enumerate(problems):
        start, end, mean = columns[p]
        status = np.where(np.arange(len(start)) % 2 == 0, "background", "peak")
        seg_text = "".join("%s\t%d\t%d\t%s\t%g\n" % (chrom, a, b, st, m) for a, b, st, m in zip(
            start.tolist(), end.tolist(), status.tolist(), mean.tolist()))
        f, r = rows[p]
        if f[1] == 1 and f[8] == 0 and f[9] == 0:  # the one-segment model's row (drv:224-243)
            loss_text = "%s\t%d\t%d\t%d\t%d\t%.20g\t%.20g\t%d\t%d\t%d\n" % (
                pen_strs[p], 1, 0, int(f[3]), int(f[4]), f[5], f[6], 0, 0, 0)
            megabytes = 0.0
        else:
            loss_text = "%.20g\t%d\t%d\t%d\t%d\t%.20g\t%.20g\t%d\t%.20g\t%.20g\n" % (
                f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), f[5], f[6], int(f[7]), f[8], f[9])
            n = int(f[4])  # the size of the reference's cost-function database
            megabytes = (32 * n + 12 * (2 * n - 1) + 20 * int(r.total_intervals)) / 1024 / 1024
        loss = _read_text_table(loss_text, col_name_list["loss"])
        loss["megabytes"] = float(megabytes)
        loss["seconds"] = float(seconds)
        flat.append(PeakSegFPOP_dir_result(
            _read_text_table(seg_text, col_name_list["segments"]), loss))
        if stats:
            flat[-1].stats = pd.DataFrame(dict(zip(
                ["reads", "max.count", "summitStart", "summitEnd"], seg_stats[p])))
        if labels is not None:
            flat[-1].label_errors = _label_frame(chrom, labels[c], label_cols[p])
            for name, value in zip(LABEL_TOTALS, label_totals[p].tolist()):
                flat[-1].loss[name] = value
        if features is not None:
            flat[-1].features = features.iloc[c]
    out, o = [], 0
    for q in pens:
        out.append(flat[o:o + len(q)])
        o += len(q)
    out = out[0] if single else out
    if cluster_groups is None:
        return out
    if joint_penalty is not None or joint_search is not None:
        return (out,) + clusters
    return (out, clusters)


def _penalty_source(penalties, penalty_model, n_contigs, noun):
    """the `pens` of _solve_dense_set from exactly one of penalties / penalty_model, checked before
    any device work"""
    if (penalties is None) == (penalty_model is None):
        raise ValueError("exactly one of penalties and penalty_model must be given")
    if penalty_model is None:
        return _penalty_lists(penalties, n_contigs, noun)
    _check_penalty_model(penalty_model)
    return [[float("inf")] for _ in range(n_contigs)]


def PeakSegFPOP_dense(count_vecs, penalties=None, chrom="chrUnknown", chrom_starts=None, device=0,
                      stats=False, labels=None, penalty_model=None):
    """PeakSegFPOP_vec without its files: dense integer coverage (one count per base) is
    run-length encoded and solved on the GPU, and the reference's result comes back as data
    frames.  count_vecs: one vector or a list of them (int32 numpy arrays or torch tensors are
    passed as they are -- a tensor on cuda:`device` is never copied --, other integer arrays
    are converted); penalties: one list for all vectors or one list per vector; chrom_starts:
    the coordinate of each vector's first base (default 0).  Returns, for a single vector, a
    list over its penalties, else a list over vectors of such lists, of PeakSegFPOP_dir_result
    whose $segments and $loss are what PeakSegFPOP_dir reads from the files the file path
    writes for the same runs (means pass through the files' "%g", penalties through paste()).
    stats=True: every result also gets .stats, a data frame with one row per row of .segments and
    the columns reads (the sum of the segment's bases' counts), max.count, summitStart and
    summitEnd (the first run of the segment whose count is max.count), computed on the GPU from
    the resident runs (ProblemSet.segment_stats).
    labels: per vector (bare for a single vector) its labels (chromStart, chromEnd, annotation) --
    annotation a list of noPeaks / peakStart / peakEnd / peaks or their codes 0..3 --, None for a
    vector without labels: every result also gets .label_errors, a data frame chrom, chromStart,
    chromEnd, annotation, count, fp, fn, status (correct / false positive / false negative) with
    one row per label, counted on the GPU (ProblemSet.label_errors), and $loss the columns errors,
    fp, fn, possible.fp and possible.fn.
    penalty_model instead of penalties: {"intercept": float, "weights": {feature name: float}}, a
    fitted log(penalty) = intercept + sum of weight x feature.  The set is made with one problem
    per vector, its coverage features are computed on the GPU (ProblemSet.coverage_features), each
    problem gets its predicted penalty (predict_penalties), and one solve follows: each vector
    yields a list of one result -- what `penalties` [[p]] gives for that penalty -- which also
    carries .features, the vector's row of the feature table.  Exactly one of penalties and
    penalty_model must be given (ValueError)."""
    from .grid import ProblemSet
    single = isinstance(count_vecs, np.ndarray) or hasattr(count_vecs, "data_ptr") or (
        len(count_vecs) > 0 and isinstance(count_vecs[0], (int, np.integer)))
    vecs = [count_vecs] if single else list(count_vecs)
    if len(vecs) == 0:
        raise ValueError("count.vecs must hold at least one vector")
    pens = _penalty_source(penalties, penalty_model, len(vecs), "vector")
    contigs = [_int32_vector(v) for v in vecs]
    if chrom_starts is None:
        chrom_starts = [0] * len(vecs)
    if len(chrom_starts) != len(vecs):
        raise ValueError("chrom.starts: one per vector")
    return _solve_dense_set(
        lambda problems: (ProblemSet.from_dense(contigs, problems, device=device), chrom_starts),
        pens, chrom, stats, single, "<dense counts>", labels, penalty_model)


# ---- aligned reads in memory (additive: the pile-up happens on the GPU) -----------------------

def _read_contigs(reads):
    """(is it a single contig, the list of contigs) of PeakSegFPOP_reads' first argument"""
    if len(reads) == 0:
        raise ValueError("reads must hold at least one contig")
    first = reads[0]
    single = not isinstance(first, (tuple, list)) or (
        len(first) > 0 and isinstance(first[0], (int, np.integer)))
    return single, [reads] if single else list(reads)


def _strand_vector(v):
    """a strand column as the library takes it: int8 arrays and tensors as they are, other integer
    arrays converted (a value that is not +1 or -1 is left for the library to name)"""
    if hasattr(v, "data_ptr"):
        return v
    v = np.asarray(v)
    if not np.issubdtype(v.dtype, np.integer):
        raise ValueError("strand must be integer")
    if v.dtype != np.int8:
        v = np.where((v == 1) | (v == -1), v, 0).astype(np.int8)
    return np.ascontiguousarray(v)


def _stranded_contigs(reads, strands):
    """(single, the contigs, the strands) of the public functions of stranded reads, converted as
    PeakSegFPOP_reads converts its reads"""
    single, contigs = _read_contigs(reads)
    names = ("chromStart", "chromEnd", "count")
    contigs = [tuple(None if v is None else _int32_vector(v, names[j]) for j, v in enumerate(entry))
               if isinstance(entry, (tuple, list)) else entry for entry in contigs]
    if strands is not None:
        strands = [_strand_vector(v) for v in ([strands] if single else list(strands))]
    return single, contigs, strands


def _strand_call(call):
    try:
        return call()
    except RuntimeError as e:
        if not hasattr(e, "status"):
            raise
        msg = _native.status_message(e.status, "<stranded reads>", "", "")
        detail = _native.last_error()
        raise PeakSegError(e.status, "%s (%s)" % (msg, detail) if detail else msg)


def strand_cross_correlation(reads, strands, max_shift=400, extents=None, device=0):
    """The strand cross-correlation of single-end reads, from exact integers computed on the GPU
    (peakseg_hip_reads_strand_xcorr; the definitions are in include/peaksegdisk_hip.h).  reads as
    PeakSegFPOP_reads takes them (one contig or a list of contigs, numpy arrays or cuda tensors);
    strands: per contig an int8 array or tensor with +1 or -1 per read.  A read's tag is its 5'
    base: chromStart of a plus read, chromEnd - 1 of a minus read.  Returns a list over contigs
    of data frames with one row per shift 0 .. max_shift (at most 1023): shift, pairs, sum_plus,
    sq_plus, sum_minus, sq_minus, cross (int64) and correlation = Pearson's r of the plus tags
    against the minus tags `shift` bases downstream, NaN where a variance is not positive."""
    from . import strand
    single, contigs, strands = _stranded_contigs(reads, strands)
    if single and extents is not None:
        extents = [extents]
    tables, _ = _strand_call(lambda: strand.xcorr_tables(contigs, strands, max_shift, extents, device))
    return [strand.curve_frame(t.tolist()) for t in tables]


def estimate_fragment_length(reads, strands, max_shift=400, min_shift=0, extents=None, device=0):
    """The fragment length of single-end reads from the strand cross-correlation pooled over all
    contigs (the column-wise sum of their tables): among the shifts min_shift .. max_shift with a
    finite correlation the one with the largest, the smallest such shift among equals, compared
    exactly in integers; fragment_length = shift + 1.  min_shift is how a caller steps over the
    phantom peak at the read length: reads that map uniquely only at some bases correlate across
    the strands at a shift of about one read length, whatever the fragments are, and a min_shift
    above the read length keeps that peak out of the choice.  Returns a FragmentLength
    (fragment_length, shift, correlation, curve); ValueError when no shift has a finite
    correlation."""
    from . import strand
    single, contigs, strands = _stranded_contigs(reads, strands)
    if single and extents is not None:
        extents = [extents]
    return _strand_call(lambda: strand.estimate(contigs, strands, max_shift, min_shift, extents, device))


def extend_reads(reads, strands, fragment_length, device=0):
    """Single-end reads extended from their 5' ends to fragment_length >= 1 on the GPU
    (peakseg_hip_reads_extend): a plus read becomes [chromStart, chromStart + d), a minus read
    [chromEnd - d, chromEnd), clamped into int32; count passes through.  fragment_length: an
    integer or one per contig.  Returns the list over contigs of (chromStart, chromEnd[, count])
    -- the tuple itself for a single contig -- in the kind of memory it was given (numpy in, numpy
    out; cuda tensors in, cuda tensors out), which every *_reads entry point takes."""
    from . import strand
    single, contigs, strands = _stranded_contigs(reads, strands)
    out = _strand_call(lambda: strand.extend(contigs, strands, fragment_length, device))
    return out[0] if single else out


def remove_duplicates(reads, strands=None, keep=1, by=None, compact=True, device=0):
    """Duplicate removal of aligned reads on the GPU (peakseg_hip_reads_dedup: a stable radix sort of
    the reads' keys; the definitions are in include/peaksegdisk_hip.h): of every key the first `keep`
    units survive, in input order.  reads as extend_reads takes them (one contig or a list, numpy
    arrays or cuda tensors read in place; a row's count is its multiplicity, absent: 1); strands:
    per contig an int8 array or tensor with +1 or -1 per read, or None.  by: "fragment" -- the key
    is (chromStart, chromEnd, strand): paired-end fragments, reads used as they are -- or
    "five_prime" -- (5' base, strand), the rule for single-end reads, which needs strands; None:
    "five_prime" when strands are given, "fragment" otherwise.  Returns a DuplicateRemoval: .reads,
    per contig (chromStart, chromEnd, count) -- the tuple itself for a single contig -- in the kind
    of memory it was given; .strands alike, or None; .summary, a data frame with one row per contig
    and the int64 columns reads, kept, rows_kept, distinct (distinct / reads is the non-redundant
    fraction).  compact=True drops the rows that lose every unit; compact=False keeps every row and
    only changes count, zeros included.  Both forms are what every *_reads entry point,
    strand_cross_correlation and extend_reads take."""
    from . import dedup
    single, contigs, strands = _stranded_contigs(reads, strands)
    new_reads, new_strands, summary = _strand_call(
        lambda: dedup.remove(contigs, strands, keep, by, compact, device))
    return dedup.DuplicateRemoval(new_reads[0] if single else new_reads,
                                  None if new_strands is None else (new_strands[0] if single else new_strands),
                                  dedup.summary_frame(summary))


def PeakSegFPOP_reads(reads, penalties=None, chrom="chrUnknown", extents=None, bases_counted="each",
                      device=0, stats=False, labels=None, penalty_model=None, strands=None,
                      fragment_length=None, max_shift=400, min_shift=0, max_duplicates=None):
    """PeakSegFPOP_dense with the step in front of it: aligned reads are piled up into coverage,
    run-length encoded and solved on the GPU.  reads: one contig -- (chromStart, chromEnd) or
    (chromStart, chromEnd, count), one entry per read, in any order -- or a list of contigs
    (int32 numpy arrays or torch tensors are passed as they are, a tensor on cuda:`device` is
    never copied; other integer arrays are converted); penalties: one list for all contigs or one
    per contig; extents: per contig (a single pair for a single contig) the (chromStart, chromEnd)
    whose bases are the data, default (min chromStart, max chromEnd) of its reads;
    bases_counted: "each" base of a read or only its "end".  Coordinates are genomic: base 0 of a
    contig is its extent's chromStart.  Results, `stats`, `labels` and `penalty_model` as
    PeakSegFPOP_dense.  Single-end reads: strands= and fragment_length= (an integer, one per
    contig, or "auto" with max_shift and min_shift) as ProblemSet.from_reads takes them.
    max_duplicates: None, or the units of every key that remove_duplicates leaves, first of all."""
    from .grid import ProblemSet
    single, contigs, strands = _stranded_contigs(reads, strands)
    if (strands is None) != (fragment_length is None):
        raise ValueError("PeakSegFPOP_reads: strands and fragment_length go together")
    if single and extents is not None:
        extents = [extents]
    pens = _penalty_source(penalties, penalty_model, len(contigs), "contig")

    def make_set(problems):
        pset = ProblemSet.from_reads(contigs, problems, extents=extents,
                                     bases_counted=bases_counted, device=device, strands=strands,
                                     fragment_length=fragment_length, max_shift=max_shift,
                                     min_shift=min_shift, max_duplicates=max_duplicates)
        return pset, pset.contig_starts
    return _solve_dense_set(make_set, pens, chrom, stats, single, "<aligned reads>", labels,
                            penalty_model)


# ---- the penalty without labels: thinning and the held-out loss (additive)

def _select_penalty(make_set, penalties, rule, single, label, refit):
    """What select_penalty_dense and select_penalty_reads share: the fold set of make_set(pens),
    one solve, one heldout_loss over every (sample, fold, penalty), the selections, and with
    refit(penalties, one per sample) -> the fits on all the data."""
    from .heldout import RULES, select_from_set
    if rule not in RULES:
        raise ValueError('rule is %r, neither "min" nor "1se"' % (rule,))
    if penalties is None or len(penalties) == 0:
        raise ValueError("penalties: the penalties to choose among must be given")
    pens = []
    for pen_num in penalties:
        _check_pen_num(pen_num)
        pens.append(float(paste(pen_num)))
    try:
        pset = make_set(pens)
    except RuntimeError as e:
        status = getattr(e, "status", _native.ERROR_DEVICE_SOLVER)
        msg = _native.status_message(status, label, "", "")
        detail = _native.last_error()
        raise PeakSegError(status, "%s (%s)" % (msg, detail) if detail else msg)
    try:
        try:
            pset.solve()
            chosen = select_from_set(pset, rule)
        except RuntimeError as e:
            raise PeakSegError(getattr(e, "status", _native.ERROR_DEVICE_SOLVER), str(e))
    finally:
        pset.close()
    if refit is not None:
        for sel, fits in zip(chosen, refit([[sel.penalty] for sel in chosen])):
            sel.fit = fits[0]
    return chosen[0] if single else chosen


def select_penalty_dense(count_vecs, penalties, folds=4, seed=1, rule="min", refit=False,
                         chrom="chrUnknown", device=0):
    """The penalty of dense coverage without labels, by K-fold thinning (peaksegdisk_amd/heldout.py;
    DESIGN.md section 18): every base's unit counts are split at random into `folds` (2, 4 or 8)
    folds on the GPU, every fold's remaining units are solved at every one of `penalties`, and
    every model is scored by its Poisson loss on the held-out units -- one fold set, one solve, one
    ProblemSet.heldout_loss.  count_vecs as PeakSegFPOP_dense takes them; penalties: the numbers to
    choose among (required: no ladder is invented here), for all vectors; rule: "min" or "1se".
    Returns a HeldoutSelection for a single vector, else a list of them: .table, .summary,
    .train_penalty, and .penalty = train_penalty K / (K - 1) for all the data.  refit=True: .fit is
    PeakSegFPOP_dense's result on the vector at .penalty.  Thinning base by base treats the bases
    as independent, which coverage that shares reads between neighbouring bases is not: with the
    reads at hand select_penalty_reads is the sound form, this one the approximation."""
    from .grid import ProblemSet
    single = isinstance(count_vecs, np.ndarray) or hasattr(count_vecs, "data_ptr") or (
        len(count_vecs) > 0 and isinstance(count_vecs[0], (int, np.integer)))
    vecs = [count_vecs] if single else list(count_vecs)
    if len(vecs) == 0:
        raise ValueError("count.vecs must hold at least one vector")
    contigs = [_int32_vector(v) for v in vecs]

    def fits(per_sample):
        return PeakSegFPOP_dense(contigs, per_sample, chrom=chrom, device=device)
    return _select_penalty(
        lambda pens: ProblemSet.from_dense_folds(contigs, pens, folds=folds, seed=seed, device=device),
        penalties, rule, single, "<dense counts>", fits if refit else None)


def select_penalty_reads(reads, penalties, folds=4, seed=1, rule="min", refit=False,
                         chrom="chrUnknown", extents=None, bases_counted="each", device=0):
    """select_penalty_dense for aligned reads: the units are the reads, each of which goes whole
    (with its optional count) to one fold.  reads, extents and bases_counted as PeakSegFPOP_reads
    takes them.  Thinned Poisson reads are independent Poisson reads, so the held-out loss is an
    honest estimate.  refit=True: .fit is PeakSegFPOP_reads' result at .penalty."""
    from .grid import ProblemSet
    single, contigs = _read_contigs(reads)
    names = ("chromStart", "chromEnd", "count")
    contigs = [tuple(None if v is None else _int32_vector(v, names[j]) for j, v in enumerate(entry))
               if isinstance(entry, (tuple, list)) else entry for entry in contigs]
    if single and extents is not None:
        extents = [extents]

    def fits(per_sample):
        return PeakSegFPOP_reads(contigs, per_sample, chrom=chrom, extents=extents,
                                 bases_counted=bases_counted, device=device)
    return _select_penalty(
        lambda pens: ProblemSet.from_reads_folds(contigs, pens, folds=folds, seed=seed,
                                                 extents=extents, bases_counted=bases_counted,
                                                 device=device),
        penalties, rule, single, "<aligned reads>", fits if refit else None)


# ---- consensus peaks of several samples (additive) ---------------------

class ConsensusPeaks:
    """What consensus_peaks_dense / consensus_peaks_reads return.
    groups: a list over groups of {"samples": the indices of the group's samples, "clusters": a data
    frame chrom, clusterStart, clusterEnd, peaks, samples -- the consensus peaks in increasing
    clusterStart --, "peaks", "bases", "sum", "max": (clusters, samples of the group) arrays};
    fits: a list over samples of PeakSegFPOP_dir_result, each sample's own model.
    clusters, peaks, bases, sum, max: those of the only group (ValueError when there are several)."""

    def __init__(self, groups, fits):
        self.groups = groups
        self.fits = fits

    def _only(self, name):
        if len(self.groups) != 1:
            raise ValueError("%d groups: read .groups[g][%r]" % (len(self.groups), name))
        return self.groups[0][name]

    clusters = property(lambda self: self._only("clusters"))
    peaks = property(lambda self: self._only("peaks"))
    bases = property(lambda self: self._only("bases"))
    sum = property(lambda self: self._only("sum"))
    max = property(lambda self: self._only("max"))


def _consensus_arguments(n_samples, penalties, penalty_model, groups, chrom):
    """(pens of _solve_dense_set, groups int32[n_samples], chrom per group) of the consensus
    entries, checked before any device work in the style of _label_lists"""
    if n_samples == 0:
        raise ValueError("consensus peaks: at least one sample")
    if penalties is not None and not isinstance(penalties, (int, float, np.integer, np.floating)):
        penalties = list(penalties)
        if len(penalties) != n_samples:
            raise ValueError("penalties: one per sample (%d penalties, %d samples)"
                             % (len(penalties), n_samples))
        for q in penalties:
            if isinstance(q, (list, tuple, np.ndarray)):
                raise ValueError("penalties: one number per sample, not a list per sample")
        penalties = [[q] for q in penalties]
    elif penalties is not None:
        penalties = [[penalties]] * n_samples
    pens = _penalty_source(penalties, penalty_model, n_samples, "sample")
    if groups is None:
        groups = np.zeros(n_samples, dtype=np.int32)
    else:
        given = np.asarray(groups)
        if given.shape != (n_samples,):
            raise ValueError("groups: one per sample (%d values, %d samples)" % (given.size, n_samples))
        if not np.issubdtype(given.dtype, np.integer):
            raise ValueError("groups must be integers")
        if given.min() < -1:
            bad = int(np.flatnonzero(given < -1)[0])
            raise ValueError("groups: sample %d is in group %d; -1 is no group" % (bad, given[bad]))
        groups = given.astype(np.int32)
    n_groups = int(groups.max()) + 1
    if isinstance(chrom, str):
        chrom = [chrom] * n_groups
    elif len(chrom) != n_groups:
        raise ValueError("chrom: one name, or one per group (%d names, %d groups)"
                         % (len(chrom), n_groups))
    return pens, groups, list(chrom)


def _consensus_result(solved, groups, chrom):
    fits, clusters = solved
    out = []
    for g, entry in enumerate(clusters):
        frame = entry["clusters"].copy()
        frame.insert(0, "chrom", chrom[g])
        out.append({"samples": entry["members"], "clusters": frame, "peaks": entry["peaks"],
                    "bases": entry["bases"], "sum": entry["sum"], "max": entry["max"]})
    fits = [f[0] for f in fits]
    for fit, g in zip(fits, groups.tolist()):
        if g >= 0:
            fit.segments["chrom"] = chrom[g]
    return ConsensusPeaks(out, fits)


def consensus_peaks_dense(count_vecs, penalties=None, penalty_model=None, groups=None,
                          chrom="chrUnknown", chrom_starts=None, device=0):
    """Samples in, consensus peaks and count matrix out, in one process and without a table leaving
    the device in between: every sample's dense coverage (count_vecs: a list of vectors as
    PeakSegFPOP_dense takes them, one per sample) is encoded and solved as one problem, the peaks of
    the samples of a group are clustered (ProblemSet.peak_clusters: two peaks are one consensus peak
    when a chain of overlapping peaks joins them), and every sample's coverage under every consensus
    peak is summed -- all on the GPU.  penalties: one number for all samples or one per sample;
    penalty_model instead: a fitted model as PeakSegFPOP_dense takes it (exactly one of the two).
    groups: one integer per sample, the genomic region it covers (-1: in none); None: all samples are
    one group.  chrom: one name, or one per group; chrom_starts: the coordinate of each sample's
    first base (default 0): samples of a group may begin and end at different coordinates.
    Returns a ConsensusPeaks."""
    from .grid import ProblemSet
    if isinstance(count_vecs, np.ndarray) and count_vecs.ndim == 1 or hasattr(count_vecs, "data_ptr"):
        raise ValueError("count.vecs: a list of vectors, one per sample")
    vecs = list(count_vecs)
    pens, groups, chrom = _consensus_arguments(len(vecs), penalties, penalty_model, groups, chrom)
    contigs = [_int32_vector(v) for v in vecs]
    if chrom_starts is None:
        chrom_starts = [0] * len(vecs)
    if len(chrom_starts) != len(vecs):
        raise ValueError("chrom.starts: one per sample")
    solved = _solve_dense_set(
        lambda problems: (ProblemSet.from_dense(contigs, problems, device=device), chrom_starts),
        pens, "chrUnknown", False, False, "<dense counts>", None, penalty_model, cluster_groups=groups)
    return _consensus_result(solved, groups, chrom)


def consensus_peaks_reads(reads, penalties=None, penalty_model=None, groups=None, chrom="chrUnknown",
                          extents=None, bases_counted="each", device=0):
    """consensus_peaks_dense with the pile-up in front of it: reads is a list over samples of
    (chromStart, chromEnd) or (chromStart, chromEnd, count) as PeakSegFPOP_reads takes them;
    extents, bases_counted as there.  Coordinates are genomic: a sample's first base is its extent's
    chromStart."""
    from .grid import ProblemSet
    if len(reads) and not isinstance(reads[0], (tuple, list)):
        raise ValueError("reads: a list of samples, each (chromStart, chromEnd[, count])")
    samples = list(reads)
    pens, groups, chrom = _consensus_arguments(len(samples), penalties, penalty_model, groups, chrom)
    names = ("chromStart", "chromEnd", "count")
    contigs = [tuple(None if v is None else _int32_vector(v, names[j]) for j, v in enumerate(entry))
               for entry in samples]

    def make_set(problems):
        pset = ProblemSet.from_reads(contigs, problems, extents=extents,
                                     bases_counted=bases_counted, device=device)
        return pset, pset.contig_starts
    solved = _solve_dense_set(make_set, pens, "chrUnknown", False, False, "<aligned reads>", None,
                              penalty_model, cluster_groups=groups)
    return _consensus_result(solved, groups, chrom)


# ---- joint peaks of several samples (additive) -------------------------

class JointPeaks(ConsensusPeaks):
    """What joint_peaks_dense / joint_peaks_reads return: a ConsensusPeaks whose groups also hold
    "joint": a data frame chrom, windowStart, windowEnd, peakStart, peakEnd, objective, samples_up,
    levels with one row per consensus peak (its window is the cluster widened by its own width on
    either side; peakStart = peakEnd = -1: no joint peak), and "gain", "up", "joint_sum",
    "joint_bases": (clusters, samples of the group) arrays -- each sample's likelihood gain at the
    joint peak, whether it carries it, and its coverage and bases under it.
    joint, gain, up: those of the only group (ValueError when there are several)."""

    joint = property(lambda self: self._only("joint"))
    gain = property(lambda self: self._only("gain"))
    up = property(lambda self: self._only("up"))


def _joint_result(solved, groups, chrom):
    fits, clusters, joint = solved
    out = _consensus_result((fits, clusters), groups, chrom)
    for g, entry in enumerate(joint):
        frame = entry["joint"].copy()
        frame.insert(0, "chrom", chrom[g])
        out.groups[g].update({"joint": frame, "gain": entry["gain"], "up": entry["up"],
                              "joint_sum": entry["sum"], "joint_bases": entry["bases"]})
    return JointPeaks(out.groups, out.fits)


def _joint_penalty(joint_penalty):
    value = float(joint_penalty)
    if not value >= 0.0:
        raise ValueError("joint_penalty %r is negative or not a number" % (joint_penalty,))
    return value


def joint_peaks_dense(count_vecs, penalties=None, penalty_model=None, groups=None, joint_penalty=0.0,
                      chrom="chrUnknown", chrom_starts=None, device=0):
    """consensus_peaks_dense with the next step behind it, still in one process and with nothing
    downloaded in between: for every consensus peak one common peak is fitted at base resolution to
    all samples of its group at once (ProblemSet.joint_peaks; PeakSegPipeline's PeakSegJoint step),
    and every sample is called up or flat there.  joint_penalty >= 0: the price of one more sample
    with a peak.  The other arguments as consensus_peaks_dense.  Returns a JointPeaks."""
    from .grid import ProblemSet
    if isinstance(count_vecs, np.ndarray) and count_vecs.ndim == 1 or hasattr(count_vecs, "data_ptr"):
        raise ValueError("count.vecs: a list of vectors, one per sample")
    vecs = list(count_vecs)
    joint_penalty = _joint_penalty(joint_penalty)
    pens, groups, chrom = _consensus_arguments(len(vecs), penalties, penalty_model, groups, chrom)
    contigs = [_int32_vector(v) for v in vecs]
    if chrom_starts is None:
        chrom_starts = [0] * len(vecs)
    if len(chrom_starts) != len(vecs):
        raise ValueError("chrom.starts: one per sample")
    solved = _solve_dense_set(
        lambda problems: (ProblemSet.from_dense(contigs, problems, device=device), chrom_starts),
        pens, "chrUnknown", False, False, "<dense counts>", None, penalty_model, cluster_groups=groups,
        joint_penalty=joint_penalty)
    return _joint_result(solved, groups, chrom)


def joint_peaks_reads(reads, penalties=None, penalty_model=None, groups=None, joint_penalty=0.0,
                      chrom="chrUnknown", extents=None, bases_counted="each", device=0):
    """joint_peaks_dense with the pile-up in front of it: reads, extents and bases_counted as
    consensus_peaks_reads takes them."""
    from .grid import ProblemSet
    if len(reads) and not isinstance(reads[0], (tuple, list)):
        raise ValueError("reads: a list of samples, each (chromStart, chromEnd[, count])")
    samples = list(reads)
    joint_penalty = _joint_penalty(joint_penalty)
    pens, groups, chrom = _consensus_arguments(len(samples), penalties, penalty_model, groups, chrom)
    names = ("chromStart", "chromEnd", "count")
    contigs = [tuple(None if v is None else _int32_vector(v, names[j]) for j, v in enumerate(entry))
               for entry in samples]

    def make_set(problems):
        pset = ProblemSet.from_reads(contigs, problems, extents=extents,
                                     bases_counted=bases_counted, device=device)
        return pset, pset.contig_starts
    solved = _solve_dense_set(make_set, pens, "chrUnknown", False, False, "<aligned reads>", None,
                              penalty_model, cluster_groups=groups, joint_penalty=joint_penalty)
    return _joint_result(solved, groups, chrom)


# ---- the joint penalty learned from labels (additive) -------------------

def _joint_search(labels, n_samples, width, max_rounds, tol):
    from .joint_target import DEFAULT_TOL, DEFAULT_WIDTH
    tol = DEFAULT_TOL if tol is None else float(tol)
    if not tol > 0:
        raise ValueError("tol %r: a positive number" % (tol,))
    if int(max_rounds) < 2:
        raise ValueError("max_rounds %r: at least 2 (penalty 0, then the ladder)" % (max_rounds,))
    return {"labels": _label_lists(labels, n_samples, False, "sample"),
            "width": DEFAULT_WIDTH if width is None else int(width), "max_rounds": int(max_rounds),
            "tol": tol}


def joint_target_interval_dense(count_vecs, labels, penalties=None, penalty_model=None, groups=None,
                                chrom="chrUnknown", chrom_starts=None, device=0, width=None,
                                max_rounds=20, tol=None):
    """The interval of log(joint penalty) whose joint models have the fewest label errors: the
    single-sample solve and the clusters' windows exactly as joint_peaks_dense has them, then the
    search of joint_target.py on the resident set -- one ProblemSet.joint_path and one
    ProblemSet.joint_label_errors per round, nothing else downloaded.  labels: one entry per SAMPLE,
    (chromStart, chromEnd, annotation) in genomic coordinates, None for a sample without labels;
    annotation as ProblemSet.label_errors takes it.  width: the penalties of a round (default 8, at
    most 16); tol: a flank is closed when its two penalties are within a factor 1 + tol (default
    0.05).  The other arguments as joint_peaks_dense.  Returns (JointTargetInterval,
    ConsensusPeaks): the interval, and the single-sample fits with the clusters searched."""
    from .grid import ProblemSet
    if isinstance(count_vecs, np.ndarray) and count_vecs.ndim == 1 or hasattr(count_vecs, "data_ptr"):
        raise ValueError("count.vecs: a list of vectors, one per sample")
    vecs = list(count_vecs)
    search = _joint_search(labels, len(vecs), width, max_rounds, tol)
    pens, groups, chrom = _consensus_arguments(len(vecs), penalties, penalty_model, groups, chrom)
    contigs = [_int32_vector(v) for v in vecs]
    if chrom_starts is None:
        chrom_starts = [0] * len(vecs)
    if len(chrom_starts) != len(vecs):
        raise ValueError("chrom.starts: one per sample")
    fits, clusters, interval = _solve_dense_set(
        lambda problems: (ProblemSet.from_dense(contigs, problems, device=device), chrom_starts),
        pens, "chrUnknown", False, False, "<dense counts>", None, penalty_model, cluster_groups=groups,
        joint_search=search)
    return interval, _consensus_result((fits, clusters), groups, chrom)


def joint_target_interval_reads(reads, labels, penalties=None, penalty_model=None, groups=None,
                                chrom="chrUnknown", extents=None, bases_counted="each", device=0,
                                width=None, max_rounds=20, tol=None):
    """joint_target_interval_dense with the pile-up in front of it: reads, extents and
    bases_counted as consensus_peaks_reads takes them."""
    from .grid import ProblemSet
    if len(reads) and not isinstance(reads[0], (tuple, list)):
        raise ValueError("reads: a list of samples, each (chromStart, chromEnd[, count])")
    samples = list(reads)
    search = _joint_search(labels, len(samples), width, max_rounds, tol)
    pens, groups, chrom = _consensus_arguments(len(samples), penalties, penalty_model, groups, chrom)
    names = ("chromStart", "chromEnd", "count")
    contigs = [tuple(None if v is None else _int32_vector(v, names[j]) for j, v in enumerate(entry))
               for entry in samples]

    def make_set(problems):
        pset = ProblemSet.from_reads(contigs, problems, extents=extents,
                                     bases_counted=bases_counted, device=device)
        return pset, pset.contig_starts
    fits, clusters, interval = _solve_dense_set(
        make_set, pens, "chrUnknown", False, False, "<aligned reads>", None, penalty_model,
        cluster_groups=groups, joint_search=search)
    return interval, _consensus_result((fits, clusters), groups, chrom)


def learn_joint_penalty_dense(count_vecs, labels, **kwargs):
    """The joint penalty learned from labels: joint_target_interval_dense's JointTargetInterval;
    its .penalty is a float that joint_peaks_dense(joint_penalty=...) takes as it is."""
    return joint_target_interval_dense(count_vecs, labels, **kwargs)[0]


def learn_joint_penalty_reads(reads, labels, **kwargs):
    """learn_joint_penalty_dense from aligned reads (joint_target_interval_reads)."""
    return joint_target_interval_reads(reads, labels, **kwargs)[0]


# ---- coverage features and learned penalties (additive) ----------------

def _check_penalty_model(model):
    """{"intercept": float, "weights": {feature name: float}} or ValueError -> (intercept, weights)"""
    from .grid import FEATURE_NAMES
    if not isinstance(model, dict) or set(model) != {"intercept", "weights"} or \
            not isinstance(model["weights"], dict):
        raise ValueError('penalty_model: {"intercept": float, "weights": {feature name: float}}')
    for name in model["weights"]:
        if name not in FEATURE_NAMES:
            raise ValueError("penalty_model: unknown feature %r" % (name,))
    return float(model["intercept"]), {n: float(w) for n, w in model["weights"].items()}


def predict_penalties(features, model):
    """The penalties a fitted model predicts: features: the data frame of coverage_features /
    problem_features_* (one row per contig); model: {"intercept": float, "weights": {feature name:
    float}}, log(penalty) = intercept + the sum of weight x feature.  Returns a float64 array, one
    penalty per row: exp of the prediction, passed through paste() as every penalty is (15
    significant digits).  ValueError for an unknown feature name, and for a feature with a non-zero
    weight that is not finite for some contig (it names the contig and the feature): a NaN
    never becomes a penalty."""
    intercept, weights = _check_penalty_model(model)
    log_penalty = np.full(len(features), intercept, dtype=np.float64)
    for name, weight in weights.items():
        if weight == 0.0:
            continue
        column = features[name].to_numpy(dtype=np.float64)
        bad = np.flatnonzero(~np.isfinite(column))
        if len(bad):
            raise ValueError("predict_penalties: contig %d: feature %r is %r, and its weight is not zero"
                             % (int(bad[0]), name, float(column[bad[0]])))
        log_penalty += weight * column
    if not np.all(np.isfinite(log_penalty)):
        bad = int(np.flatnonzero(~np.isfinite(log_penalty))[0])
        raise ValueError("predict_penalties: contig %d: the predicted log(penalty) is %r"
                         % (bad, float(log_penalty[bad])))
    with np.errstate(over="ignore"):
        return np.array([float(paste(float(p))) for p in np.exp(log_penalty)], dtype=np.float64)


def _feature_frame(make_set, n_contigs, label):
    """the coverage features of a set made for them alone: a problem per contig at penalty Inf (the
    closed form: never launched)"""
    try:
        pset = make_set([(c, float("inf")) for c in range(n_contigs)])[0]
    except RuntimeError as e:
        status = getattr(e, "status", _native.ERROR_DEVICE_SOLVER)
        msg = _native.status_message(status, label, "", "")
        detail = _native.last_error()
        raise PeakSegError(status, "%s (%s)" % (msg, detail) if detail else msg)
    try:
        return pset.coverage_features()
    finally:
        pset.close()


def problem_features_dense(count_vecs, device=0):
    """The feature table of dense coverage: count_vecs as PeakSegFPOP_dense; a pandas data frame
    with one row per vector and the 36 columns of ProblemSet.coverage_features -- quartiles, mean,
    sd, bases and data (runs), each also under log+1, log and log.log --, computed on the GPU from
    the runs the encoder leaves there."""
    from .grid import ProblemSet
    single = isinstance(count_vecs, np.ndarray) or hasattr(count_vecs, "data_ptr") or (
        len(count_vecs) > 0 and isinstance(count_vecs[0], (int, np.integer)))
    vecs = [count_vecs] if single else list(count_vecs)
    if len(vecs) == 0:
        raise ValueError("count.vecs must hold at least one vector")
    contigs = [_int32_vector(v) for v in vecs]
    return _feature_frame(
        lambda problems: (ProblemSet.from_dense(contigs, problems, device=device), None),
        len(contigs), "<dense counts>")


def problem_features_reads(reads, extents=None, bases_counted="each", device=0):
    """problem_features_dense with the pile-up in front of it: reads, extents and bases_counted as
    PeakSegFPOP_reads."""
    from .grid import ProblemSet
    single, contigs = _read_contigs(reads)
    names = ("chromStart", "chromEnd", "count")
    contigs = [tuple(None if v is None else _int32_vector(v, names[j]) for j, v in enumerate(entry))
               if isinstance(entry, (tuple, list)) else entry for entry in contigs]
    if single and extents is not None:
        extents = [extents]
    return _feature_frame(
        lambda problems: (ProblemSet.from_reads(contigs, problems, extents=extents,
                                                bases_counted=bases_counted, device=device), None),
        len(contigs), "<aligned reads>")


# ---- the target interval of labelled contigs (additive) ---------------

def _target_interval(make_set, n_contigs, labels, width, max_rounds, single, label):
    from . import target
    labels = _label_lists(labels, n_contigs, single, "contig")
    if not (isinstance(max_rounds, (int, np.integer)) and max_rounds >= 1):
        raise ValueError("max_rounds: a positive integer")

    def make(problems):
        try:
            return make_set(problems)
        except RuntimeError as e:
            status = getattr(e, "status", _native.ERROR_DEVICE_SOLVER)
            if status == _native.ERROR_DEVICE_MEMORY:
                raise
            msg = _native.status_message(status, label, "", "")
            detail = _native.last_error()
            raise PeakSegError(status, "%s (%s)" % (msg, detail) if detail else msg)
    out = target.target_interval(make, n_contigs, labels, _check_width(width), int(max_rounds))
    return out[0] if single else out


def targetInterval_dense(count_vecs, labels, width=None, max_rounds=20, chrom_starts=None,
                         device=0):
    """The target interval of labelled coverage: for every vector the interval of log(penalty)
    whose models have the fewest label errors, the target of a penalty-learning regression.
    count_vecs, chrom_starts and device as PeakSegFPOP_dense, labels as its `labels`.  The vectors
    stay resident on the GPU as one problem set with `width` models per vector (None: 8; 1 to
    256), and every round solves what all the searches ask for in one launch and counts the label
    errors of all models on the device.  Returns, for a single vector, a target.TargetInterval,
    else a list of them: min_log_lambda, max_log_lambda (+-inf where the interval has no end),
    lower_exact, upper_exact (the limit is the breakpoint between two neighbouring models, or
    infinite), min_errors, rounds, and models, a data frame penalty, peaks, total.loss, errors,
    fp, fn, round with one row per solved penalty."""
    from .grid import ProblemSet
    single = isinstance(count_vecs, np.ndarray) or hasattr(count_vecs, "data_ptr") or (
        len(count_vecs) > 0 and isinstance(count_vecs[0], (int, np.integer)))
    vecs = [count_vecs] if single else list(count_vecs)
    if len(vecs) == 0:
        raise ValueError("count.vecs must hold at least one vector")
    contigs = [_int32_vector(v) for v in vecs]
    if chrom_starts is None:
        chrom_starts = [0] * len(vecs)
    if len(chrom_starts) != len(vecs):
        raise ValueError("chrom.starts: one per vector")
    return _target_interval(
        lambda problems: (ProblemSet.from_dense(contigs, problems, device=device), chrom_starts),
        len(vecs), labels, width, max_rounds, single, "<dense counts>")


def targetInterval_reads(reads, labels, width=None, max_rounds=20, extents=None,
                         bases_counted="each", device=0):
    """targetInterval_dense with the pile-up in front of it: reads, extents and bases_counted as
    PeakSegFPOP_reads, the rest and the result as targetInterval_dense."""
    from .grid import ProblemSet
    single, contigs = _read_contigs(reads)
    names = ("chromStart", "chromEnd", "count")
    contigs = [tuple(None if v is None else _int32_vector(v, names[j]) for j, v in enumerate(entry))
               if isinstance(entry, (tuple, list)) else entry for entry in contigs]
    if single and extents is not None:
        extents = [extents]

    def make_set(problems):
        pset = ProblemSet.from_reads(contigs, problems, extents=extents,
                                     bases_counted=bases_counted, device=device)
        return pset, pset.contig_starts
    return _target_interval(make_set, len(contigs), labels, width, max_rounds, single,
                            "<aligned reads>")


def coverage_from_reads(chromStart, chromEnd, count=None, chrom="chrUnknown", extent=None,
                        bases_counted="each", device=0, strands=None, fragment_length=None,
                        max_shift=400, min_shift=0, max_duplicates=None):
    """The coverage profile of one contig's aligned reads, piled up and run-length encoded on the
    GPU (peakseg_hip_reads_pileup_probe): the data frame chrom, chromStart, chromEnd, count that
    writeBedGraph and PeakSegFPOP_df take -- integer columns, genomic coordinates, runs of zero
    included, so there are no gaps.  The read arrays as ProblemSet.from_reads takes them;
    extent: the (chromStart, chromEnd) to cover, default (min chromStart, max chromEnd).
    Single-end reads: strands= (one int8 array or tensor) and fragment_length= (an integer, or
    "auto" with max_shift and min_shift) extend the reads first, as ProblemSet.from_reads does.
    max_duplicates: None, or the units of every key that remove_duplicates leaves, first of all."""
    import ctypes
    from .dedup import deduplicated_for
    from .grid import reads_arguments
    from .strand import extended_for
    entry = (chromStart, chromEnd) if count is None else (chromStart, chromEnd, count)
    strand_list = None if strands is None else [strands]
    contigs, extents = _strand_call(lambda: deduplicated_for(
        [entry], strand_list, max_duplicates, None if extent is None else [extent], device, None,
        "coverage_from_reads"))
    contigs, extents = _strand_call(lambda: extended_for(
        contigs, strand_list, fragment_length, extents, device, None, "coverage_from_reads", max_shift,
        min_shift))
    args, keep, ext = reads_arguments(contigs, extents, bases_counted, device, "coverage_from_reads")
    lo, hi = ext[0]
    # a read changes the coverage in at most two places
    capacity = max(1, min(hi - lo, 2 * int(args[1][0]) + 1))
    runs = np.zeros(1, dtype=np.int64)
    cols = [np.empty(capacity, dtype=np.int32) for _ in range(3)]
    st = _native.lib.peakseg_hip_reads_pileup_probe(
        device, *args, None, runs.ctypes.data, *[a.ctypes.data for a in cols])
    del keep
    if st != 0:
        msg = _native.status_message(st, "<aligned reads>", "", "")
        detail = _native.last_error()
        raise PeakSegError(st, "%s (%s)" % (msg, detail) if detail else msg)
    k = int(runs[0])
    value, weight, end = (a[:k] for a in cols)
    return pd.DataFrame({"chrom": chrom, "chromStart": (lo + end - weight).astype(np.int32),
                         "chromEnd": (lo + end).astype(np.int32), "count": value.copy()},
                        columns=col_name_list["coverage"])


# ---- PeakSegFPOP_dir for a batch (additive) --------------------------

class _devices_knob:
    """PEAKSEG_HIP_DEVICES for the duration of one batch call: None leaves the environment as
    it is; "all", a string such as "0,1" or a sequence of device ids sets it, and the previous
    value (or its absence) is restored afterwards."""

    def __init__(self, devices):
        if devices is None or isinstance(devices, str):
            self.value = devices
        else:
            self.value = ",".join("%d" % int(d) for d in devices)

    def __enter__(self):
        self.old = os.environ.get("PEAKSEG_HIP_DEVICES")
        if self.value is not None:
            os.environ["PEAKSEG_HIP_DEVICES"] = self.value

    def __exit__(self, *exc):
        if self.value is None:
            return
        if self.old is None:
            del os.environ["PEAKSEG_HIP_DEVICES"]
        else:
            os.environ["PEAKSEG_HIP_DEVICES"] = self.old


def PeakSegFPOP_dir_batch(problem_dirs, penalty_params, devices=None):
    """PeakSegFPOP_dir for many (problem.dir, penalty) pairs in one call of the native
    PeakSegFPOP_dir_batch: cached results are reused as PeakSegFPOP_dir would
    (R/PeakSegFPOP_dir.R:70-93), every other pair is solved in one device problem set (one
    parse and upload per distinct coverage.bedGraph) and gets its _timing.tsv.  Returns the
    list of PeakSegFPOP_dir results, in order; `.cached` says which were reused.
    devices: "all" or device ids -- one problem set per listed device, solved side by side
    (PEAKSEG_HIP_DEVICES for this call; None: the environment decides)."""
    import ctypes
    if len(problem_dirs) != len(penalty_params):
        raise ValueError("problem_dirs and penalty_params must have the same length")
    n = len(problem_dirs)
    pens = [paste(p) for p in penalty_params]
    dirs = (ctypes.c_char_p * n)(*[os.fsencode(d) for d in problem_dirs])
    pstr = (ctypes.c_char_p * n)(*[p.encode() for p in pens])
    status = (ctypes.c_int * n)()
    cached = (ctypes.c_int * n)()
    with _devices_knob(devices):
        _native.lib.PeakSegFPOP_dir_batch(n, dirs, pstr, status, cached)
    out = []
    for i in range(n):
        bg = os.path.join(problem_dirs[i], "coverage.bedGraph")
        if status[i] != 0:
            msg = _native.status_message(status[i], os.path.realpath(bg), pens[i],
                                         "%s_penalty=%s.db" % (os.path.realpath(bg), pens[i]))
            raise PeakSegError(status[i], msg)
        L = PeakSegFPOP_dir(problem_dirs[i], pens[i])  # reads the files just written (cache hit)
        L.cached = bool(cached[i])
        out.append(L)
    return out


# ---- sequentialSearch_dir (R/sequentialSearch_dir.R:22-103) --------------------------------

def _check_peaks(peaks_int, n_dirs=None):
    """peaks.int of the search wrappers: one non-negative integer (n_dirs None), or one for all
    of n_dirs directories or one per directory -> list"""
    scalar = isinstance(peaks_int, (int, np.integer)) and not isinstance(peaks_int, bool)
    if n_dirs is None:
        if not (scalar and 0 <= peaks_int):
            raise ValueError("is.integer(peaks.int) && length(peaks.int) == 1 && 0 <= peaks.int "
                             "is not TRUE")
        return int(peaks_int)
    peaks = [int(peaks_int)] * n_dirs if scalar else [int(p) for p in peaks_int]
    if len(peaks) != n_dirs or any(p < 0 for p in peaks):
        raise ValueError("peaks.int: one non-negative integer, or one per problem directory")
    return peaks


def _search_result(problem_dir, rows, chosen):
    """sequentialSearch_dir's value from the rows of a native search: the chosen model with
    $others (R/sequentialSearch_dir.R:96-102)."""
    model_list = {}
    for r in rows:
        pen_str = r.penalty_str.decode()
        L = PeakSegFPOP_dir(problem_dir, pen_str)  # the files of this model (cache hit)
        L.loss["iteration"] = r.iteration
        L.loss["under"] = np.nan if r.under_peaks == _native.SEARCH_NA else r.under_peaks
        L.loss["over"] = np.nan if r.over_peaks == _native.SEARCH_NA else r.over_peaks
        model_list[pen_str] = L
    out = model_list[rows[chosen].penalty_str.decode()]
    others = pd.concat([m.loss for m in model_list.values()], ignore_index=True)
    out.others = others.sort_values("iteration", kind="stable").reset_index(drop=True)
    return out


def _search_outcome(status, rows, n_rows, chosen, problem_dir, with_detail):
    """What a native search left for one directory -> its result, or the exception of its failure.
    rows[n_rows] names the model that failed (the table is full: no name)."""
    if status == _native.ERROR_SEARCH_TOO_MANY_PEAKS:
        raise ValueError(_native.last_error())
    if status != 0:
        bg = os.path.realpath(os.path.join(problem_dir, "coverage.bedGraph"))
        pen = rows[n_rows].penalty_str.decode() if n_rows < len(rows) else ""
        msg = _native.status_message(status, bg, pen, "%s_penalty=%s.db" % (bg, pen))
        detail = _native.last_error()
        if with_detail and status >= _native.ERROR_NO_HIP_DEVICE and detail:
            msg = "%s (%s)" % (msg, detail)
        raise PeakSegError(status, msg)
    return _search_result(problem_dir, rows[:n_rows], chosen)


def _search_one(problem_dir, peaks_int, cap, call):
    """A single-directory search: call(dir, peaks, cap, rows, n_rows, chosen) -> status"""
    import ctypes
    peaks_int = _check_peaks(peaks_int)
    if not isinstance(problem_dir, str):
        raise ValueError("is.character(problem.dir) is not TRUE")
    rows = (_native.PsdSearchRow * cap)()
    n_rows = ctypes.c_int(0)
    chosen = ctypes.c_int(-1)
    st = call(os.fsencode(problem_dir), peaks_int, cap, rows, ctypes.byref(n_rows),
              ctypes.byref(chosen))
    return _search_outcome(st, rows, n_rows.value, chosen.value, problem_dir, True)


def _search_many(problem_dirs, peaks_int, cap, devices, call):
    """A lockstep search: call(n, dirs, peaks, cap, rows, n_rows, chosen, status); a failed search
    raises for the first failure"""
    import ctypes
    problem_dirs = list(problem_dirs)
    n = len(problem_dirs)
    peaks_int = _check_peaks(peaks_int, n)
    if not all(isinstance(d, str) for d in problem_dirs):
        raise ValueError("is.character(problem.dir) is not TRUE")
    if n == 0:
        return []
    rows = (_native.PsdSearchRow * (cap * n))()
    dirs = (ctypes.c_char_p * n)(*[os.fsencode(d) for d in problem_dirs])
    peaks = (ctypes.c_int * n)(*peaks_int)
    n_rows = (ctypes.c_int * n)()
    chosen = (ctypes.c_int * n)()
    status = (ctypes.c_int * n)()
    with _devices_knob(devices):
        call(n, dirs, peaks, cap, rows, n_rows, chosen, status)
    return [_search_outcome(status[d], rows[d * cap:(d + 1) * cap], n_rows[d], chosen[d],
                            problem_dirs[d], False) for d in range(n)]


def sequentialSearch_dir(problem_dir, peaks_int, verbose=0):
    """The reference's penalty search for a target number of peaks.  The loop itself runs in
    the native library (PeakSegFPOP_sequential_search: coverage.bedGraph parsed and uploaded
    once, arena reused from one penalty to the next); it visits the reference's penalties and
    leaves the reference's files, from which the result is assembled here."""
    return _search_one(
        problem_dir, peaks_int, 256, lambda d, peaks, cap, *out:
        _native.lib.PeakSegFPOP_sequential_search(d, peaks, int(bool(verbose)), cap, *out))


def sequentialSearch_dir_batch(problem_dirs, peaks_int, verbose=0, devices=None):
    """sequentialSearch_dir over several problem directories at once (additive): each directory
    gets the result sequentialSearch_dir(dir, peaks) gives, but the models the searches ask for
    in the same iteration are computed in one device launch
    (PeakSegFPOP_sequential_search_batch).  peaks_int: one target for all, or one per
    directory.  devices: "all" or device ids -- the directories dealt to one shard per listed
    device (PEAKSEG_HIP_DEVICES for this call; None: the environment decides).  Returns the
    list of results; a failed search raises for the first failure."""
    return _search_many(
        problem_dirs, peaks_int, 256, devices, lambda n, dirs, peaks, cap, *out:
        _native.lib.PeakSegFPOP_sequential_search_batch(n, dirs, peaks, int(bool(verbose)), cap,
                                                        *out))


# ---- the parallel penalty search (additive) ----------------------------

def _check_width(width):
    if width is None:
        return 0
    if not (isinstance(width, (int, np.integer)) and not isinstance(width, bool)
            and 0 <= width <= 256):
        raise ValueError("width: None, or an integer from 0 (the default width) to 256")
    return int(width)


def parallelSearch_dir(problem_dir, peaks_int, width=None, verbose=0, devices=None):
    """The model with peaks_int peaks (or the next simpler one, as sequentialSearch_dir), found
    with `width` models per round instead of one: every round asks for the reference's secant
    penalty and up to width-1 more inside the bracket, all solved in one launch
    (PeakSegFPOP_parallel_search), so the search takes about a third to a half of the dependent
    rounds.  width=None: the library's default; width=1: sequentialSearch_dir's own sequence.
    devices: "all" or device ids -- each round's models dealt over the listed devices
    (PEAKSEG_HIP_DEVICES for this call; None: the environment decides).  Same result shape as
    sequentialSearch_dir: $others has one row per model, `iteration` is the round."""
    def call(d, peaks, cap, *out):
        with _devices_knob(devices):
            return _native.lib.PeakSegFPOP_parallel_search(d, peaks, _check_width(width),
                                                           int(bool(verbose)), cap, *out)
    return _search_one(problem_dir, peaks_int, 1024, call)


def parallelSearch_dir_batch(problem_dirs, peaks_int, width=None, verbose=0, devices=None):
    """parallelSearch_dir over several problem directories in lockstep: each directory gets the
    result parallelSearch_dir(dir, peaks, width) gives, and all the models the searches ask for
    in a round are computed in one launch (PeakSegFPOP_parallel_search_batch).  peaks_int: one
    target for all, or one per directory.  devices: "all" or device ids -- the directories dealt
    to one shard per listed device.  Returns the list of results; a failed search raises for the
    first failure."""
    width = _check_width(width)
    return _search_many(
        problem_dirs, peaks_int, 1024, devices, lambda n, dirs, peaks, cap, *out:
        _native.lib.PeakSegFPOP_parallel_search_batch(n, dirs, peaks, width, int(bool(verbose)),
                                                      cap, *out))
