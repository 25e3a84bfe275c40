"""The set's resident device tables over HISTORIES of service calls.

Every pack_* service of a ProblemSet keeps device tables that grow to what the largest call so far
needed, descriptors made by the first call, and a validity word (peaksegdisk_amd/csrc/peakseg_set.h).
The service's own test module checks single calls on fresh sets; this one checks sequences on one
set: grow, shrink, grow, empty (scenario 1), services taking turns (2), a solve in between (3), a
refusal in between (4) and the byte count over a history with capped twins (5).  The scenario
functions are shared with the emulator rehearsal (tests/test_resident_tables_emu.py).

Expected values never come from the library.  The models are read problem by problem through
ProblemSet.segments() (a plain copy of the solver's output that touches no resident table), and the
step-function contigs' peaks are asserted to be the bumps they were built from.  Every call is then
held against the yardstick of the service's own test module: consensus_ref (regions, clusters),
joint_ref / joint_path_ref, heldout_ref, test_gpu_label_errors.brute_force,
test_gpu_segment_stats.expected_stats, test_gpu_coverage_features.yard_moments and np.sort for the
order statistics.  Integers are compared for equality; the three double columns (the joint objective
and gain, the held-out loss) within the bound their yardsticks derive, and bit for bit between two
calls that were given the same input.  No tolerance is introduced here.

The set: the six step-function contigs of test_gpu_peak_clusters at a tenth of their coordinates
(three samples by two regions, 400 to 2000 bases), alternating(513) of test_gpu_heldout -- 513 rows
at penalty 0, one row served in closed form at +Inf -- and a second contig of 513 bases to score it
on.  Leading dimensions follow 1, 257, 3, 600, 0, 257 where the service takes caller-sized input;
pack_coverage_stats takes at most 16 ranks per contig, and the peaks of peak_clusters are those of
the set's models, so their schedules are the nearest the set offers (see each service).  Groups of
more than 64 members (the joint path's carry) need more problems than this set has and stay with
tests/test_gpu_joint_path.py."""
import ctypes
import os

import numpy as np
import pytest

import test_gpu_coverage_features as t_cov
import test_gpu_heldout as t_held
import test_gpu_joint_peaks as t_joint
import test_gpu_label_errors as t_lab
import test_gpu_peak_clusters as t_clu
import test_gpu_regions as t_reg
import test_gpu_segment_stats as t_seg
from consensus_ref import cluster_ref, region_ref
from heldout_ref import heldout_pair_ref
from joint_path_ref import joint_label_errors_ref
from joint_ref import MarginError, cluster_window, joint_peaks_ref
from test_gpu_dense import as_cuda, as_numpy, rle

GPU = pytest.mark.gpu
INF = float("inf")
SCHEDULE = (1, 257, 3, 600, 0, 257)     # (the last one with another permutation of call 2's input)


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    from peaksegdisk_amd import _native
    assert _native.lib.peakseg_hip_device_count() >= 1, "no HIP device: GPU tests need an MI355X"
    return peaksegdisk_amd


# ---- the set -------------------------------------------------------------------------------------

#            first  length  bumps (start, end, height)
SAMPLES = [(100, 2000, [(200, 250, 50), (300, 360, 60), (500, 540, 50), (800, 950, 70),
                        (1200, 1250, 50), (1500, 1510, 6)]),
           (150, 1500, [(250, 280, 40), (310, 330, 90), (530, 570, 50), (1200, 1250, 30)]),
           (50, 870, [(70, 90, 30), (560, 600, 45), (850, 910, 55)]),
           (0, 600, [(100, 140, 50), (300, 350, 50)]),
           (20, 500, [(130, 180, 50), (400, 410, 80)]),
           (0, 400, [(100, 150, 50)])]
WEAK = (1500, 1510)            # the bump of contig 0 that a penalty of 100 does not pay for
FIRSTS = [s[0] for s in SAMPLES] + [0, 0]
ALTERNATING, SAWTOOTH = 6, 7   # the two contigs of 513 bases
#            contig, penalty
PROBLEMS = [(0, 10.0), (1, 10.0), (2, 10.0), (0, 100.0), (5, 10.0), (3, 10.0), (4, 10.0), (3, INF),
            (ALTERNATING, 0.0), (ALTERNATING, INF), (ALTERNATING, 0.0), (SAWTOOTH, 0.0)]
GROUPS = [0, 0, 0, 0, -1, 1, 1, 1, -1, -1, -1, -1]      # three samples by two regions, as there
GROUPS_B = [0, 0, 1, 1, 3, 2, 2, 3, -1, -1, -1, -1]     # more groups of fewer members
BIG, ONE_ROW = 8, 9            # the problems whose model has 513 rows / one row


def make_vectors():
    vectors = [t_clu.steps(length, first, bumps, ripple=(3,) if c == 0 else ())
               for c, (first, length, bumps) in enumerate(SAMPLES)]
    return vectors + [t_held.alternating(513), ((np.arange(513) % 7) + 1).astype(np.int32)]


def permutation(n, seed):
    return np.random.default_rng(seed).permutation(n) if seed else np.arange(n)


def same(a, b):
    """two lists of arrays (or of bytes) hold the same bytes"""
    if a is None or b is None or len(a) != len(b):
        return False
    return all((x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()) ==
               (y if isinstance(y, bytes) else np.ascontiguousarray(y).tobytes()) for x, y in zip(a, b))


class capped:
    """sets created inside are allowed `room` bytes of device memory"""

    def __init__(self, room):
        self.room = room

    def __enter__(self):
        os.environ["PEAKSEG_HIP_MAX_BYTES"] = str(self.room)

    def __exit__(self, *exc):
        del os.environ["PEAKSEG_HIP_MAX_BYTES"]


class World:
    """the set, its models as the yardsticks need them, and one driver per service.  wraps: the
    inputs of the k-th service call are given as wraps[k % len(wraps)] (numpy arrays, cuda tensors)"""

    def __init__(self, psd, wraps=(as_numpy,), arena_pieces=0, problems=PROBLEMS):
        self.psd = psd
        self.wraps, self.calls, self.side = tuple(wraps), 0, None
        self.vectors, self.firsts = make_vectors(), FIRSTS
        self.pset = psd.ProblemSet.from_dense([as_numpy(v) for v in self.vectors], list(problems),
                                              arena_pieces=arena_pieces)
        self.lib, self.h = self.pset._lib, self.pset._h
        self.svc = {cls.name: cls(self) for cls in SERVICES}
        self.bits = {}          # the double columns by input: the same input, the same bits
        self.solves = 0
        self.solve()

    def __getitem__(self, name):
        return self.svc[name]

    def wrap(self):
        w = self.wraps[self.calls % len(self.wraps)]
        self.calls += 1
        self.side = "host" if w is as_numpy else "device"
        return w

    def solve(self):
        self.pset.solve()
        self.solves += 1
        return self.read_models()

    def read_models(self):
        """the reference's segments table of every problem from ProblemSet.segments(): the rows'
        first run and mean, last segment first, and the run ends of the dense vector"""
        self.raw, self.columns, self.columns0 = [], [], []
        for p, (c, pen) in enumerate(self.pset.problems):
            idx, mean = self.pset.segments(p)
            idx, mean = idx.astype(np.int64), mean.copy()
            ends = rle(self.vectors[c])[2].astype(np.int64)
            start = np.where(idx >= 0, ends[np.maximum(idx, 0)], 0)    # (idx: the run before the row)
            end = np.concatenate([[len(self.vectors[c])], start[:-1]])
            self.raw.append((idx.astype(np.int32), mean))
            self.columns0.append((start.astype(np.int32), end.astype(np.int32), mean))
            self.columns.append(((start + self.firsts[c]).astype(np.int32),
                                 (end + self.firsts[c]).astype(np.int32), mean))
            if c < len(SAMPLES):        # a step function: its peaks are its bumps
                ps, pe = t_clu.member_peaks(self.columns[p])
                want = [(a, b) for a, b, h in SAMPLES[c][2]]
                if pen >= 100.0 and c == 0:
                    want.remove(WEAK)
                if pen == INF:
                    want = []
                assert list(zip(ps.tolist(), pe.tolist())) == want, (p, c, pen)
        rows = [len(col[0]) for col in self.columns]
        for p, (c, pen) in enumerate(self.pset.problems):
            if c == ALTERNATING:
                assert rows[p] == (1 if pen == INF else 513), (p, rows[p])
        return rows

    def peaks(self, p):
        return (len(self.columns[p][0]) - 1) // 2

    def others(self, *names):
        """the downloads of every service but `names`"""
        return {n: s.download() for n, s in self.svc.items() if n not in names}

    def close(self):
        self.pset.close()


def raises(status, needle, call):
    with pytest.raises(RuntimeError) as ei:
        call()
    assert ei.value.status == status and needle in str(ei.value), (status, needle, str(ei.value))


# ---- the services --------------------------------------------------------------------------------

CALLS = [0]       # good service calls made in this process (the children report it)


class Service:
    """call(size, seed) makes one call whose leading dimension is `size` (seed: the permutation the
    input is given in), holds it against the yardstick and returns the columns with the permutation
    undone; download() is the ..._download entry of the C ABI as it is: the columns, or None for -1;
    refuse(size) makes a call of that size with one bad entry and asserts what it reports; dims is
    every dimension of the last good call that sizes a device array."""
    name = None
    sizes = SCHEDULE
    small = 40                 # a good call smaller than most
    device_inputs = True       # the call takes its arrays in device memory too
    second = ()                # a second sequence in which the dimensions move against each other

    def __init__(self, world):
        self.w = world
        self.packed = None     # what sizes the download's arrays
        self.dims = None

    def call(self, size=None, seed=0, wrap=None):
        CALLS[0] += 1
        return self._call(size, seed, wrap)

    def raw_download(self, name, shapes):
        cols = [np.full(n + 1, 0x55, dt) for n, dt in shapes]
        st = getattr(self.w.lib, name)(self.w.h, *[a.ctypes.data for a in cols])
        assert st in (0, -1), (name, st)
        return None if st else [a[:n] for a, (n, _) in zip(cols, shapes)]


class Regions(Service):
    name = "region_stats"

    def inputs(self, n, seed, bad=None):
        w = self.w
        rng = np.random.default_rng(7000 + n)
        c = rng.integers(0, len(w.vectors), n)
        first = np.array(w.firsts)[c]
        length = np.array([len(v) for v in w.vectors])[c]
        s = first - 20 + rng.integers(0, length + 20, n)         # (some hang over an end)
        e = s + rng.integers(1, 300, n)
        if bad is not None:
            e[bad] = s[bad]
        order = permutation(n, seed)
        index = [order[c[order] == k] for k in range(len(w.vectors))]
        regions = [(as_numpy(s[at]), as_numpy(e[at])) if len(at) else None for at in index]
        return c, s, e, index, regions

    def _call(self, n, seed=0, wrap=None):
        w = self.w
        c, s, e, index, regions = self.inputs(n, seed)
        got = w.pset.region_stats(t_reg.wrap_regions(regions, wrap or w.wrap()),
                                  first_chromStart=w.firsts)
        out = [np.zeros(n, dt) for dt in (np.int32, np.int64, np.int32)]
        for k, at in enumerate(index):
            want = region_ref(w.vectors[k], w.firsts[k], s[at], e[at])
            for col, name, x in zip(out, ("bases", "sum", "max"), want):
                assert got[k][name].dtype == col.dtype, (self.name, n, k, name)
                assert np.array_equal(got[k][name], x), (self.name, n, k, name)
                col[at] = got[k][name]
        self.packed, self.dims = n, (n,)
        return out

    def download(self):
        n = self.packed or 0
        return self.raw_download("peakseg_hip_problem_set_packed_region_stats_download",
                                 [(n, np.int32), (n, np.int64), (n, np.int32)])

    def refuse(self, n, wrap=None):
        bad = n // 2
        c, s, e, index, regions = self.inputs(n, 0, bad=bad)
        needle = "contig %d: region %d has" % (c[bad], index[c[bad]].tolist().index(bad))
        raises(22, needle, lambda: self.w.pset.region_stats(
            t_reg.wrap_regions(regions, wrap or self.w.wrap()), first_chromStart=self.w.firsts))


class Labels(Service):
    name = "label_errors"

    def inputs(self, n, seed, bad=None):
        w = self.w
        rng = np.random.default_rng(7100 + n)
        c = rng.integers(0, len(w.vectors), n)
        first = np.array(w.firsts)[c]
        length = np.array([len(v) for v in w.vectors])[c]
        s = first - 10 + rng.integers(0, length, n)
        e = s + rng.integers(1, 200, n)
        code = rng.integers(0, 4, n)
        if bad is not None:
            code[bad] = 7
        order = permutation(n, seed)
        index = [order[c[order] == k] for k in range(len(w.vectors))]
        labels = [tuple(as_numpy(a[at]) for a in (s, e, code)) if len(at) else None for at in index]
        return c, index, labels

    def _call(self, n, seed=0, wrap=None):
        w = self.w
        c, index, labels = self.inputs(n, seed)
        totals, per_label = w.pset.label_errors(t_lab.wrap_labels(labels, wrap or w.wrap()),
                                                first_chromStart=w.firsts)
        assert totals.dtype == np.int32 and totals.shape == (len(w.pset.problems), 5)
        out, rows = [totals], 0
        for p, (k, pen) in enumerate(w.pset.problems):
            entry = t_lab.EMPTY if labels[k] is None else labels[k]
            want = t_lab.brute_force(w.columns[p], entry)
            for name, g, x in zip(("count", "fp", "fn"), per_label[p], want[:3]):
                assert g.dtype == np.int32 and np.array_equal(g, x), (self.name, n, p, name)
                out.append(g[np.argsort(index[k])])
            assert totals[p].tolist() == want[3], (self.name, n, p, totals[p].tolist(), want[3])
            rows += len(index[k])
        self.packed, self.dims = rows, (n, rows)
        return out

    def download(self):
        n = self.packed or 0
        return self.raw_download("peakseg_hip_problem_set_packed_label_errors_download",
                                 [(n, np.int32)] * 3 + [(5 * len(self.w.pset.problems), np.int32)])

    def refuse(self, n, wrap=None):
        from peaksegdisk_amd import _native
        bad = n // 2
        c, index, labels = self.inputs(n, 0, bad=bad)
        needle = "contig %d: label %d has" % (c[bad], index[c[bad]].tolist().index(bad))
        raises(_native.ERROR_LABEL_ARGUMENTS, needle, lambda: self.w.pset.label_errors(
            t_lab.wrap_labels(labels, wrap or self.w.wrap()), first_chromStart=self.w.firsts))


class Coverage(Service):
    """size: ranks per contig (at most 16 in one call); the state of the selection has contigs x
    ranks entries: 8, 72, 24, 128, 0, 72"""
    name = "coverage_order_statistics"
    sizes = (1, 9, 3, 16, 0, 9)
    small = 2
    device_inputs = False

    def ranks(self, k):
        rng = np.random.default_rng(7200 + k)
        return np.stack([rng.integers(0, len(v), k) for v in self.w.vectors]).astype(np.int64)

    def _call(self, k, seed=0, wrap=None):
        w = self.w
        order = permutation(k, seed)
        ranks = np.ascontiguousarray(self.ranks(k)[:, order])
        value, moments = w.pset._coverage_stats(ranks)
        cols = w.pset._moment_columns(moments)
        for c, x in enumerate(w.vectors):
            assert value[c].tolist() == np.sort(x.astype(np.int64))[ranks[c]].tolist(), (self.name, k, c)
            assert (int(cols["bases"][c]), int(cols["runs"][c]), int(cols["sum"][c]),
                    cols["sum_sq"][c]) == t_cov.yard_moments(x), (self.name, k, c)
        self.packed, self.dims = k, (k,)
        return [value[:, np.argsort(order)], moments]

    def download(self):
        nc = len(self.w.vectors)
        return self.raw_download("peakseg_hip_problem_set_packed_coverage_stats_download",
                                 [(nc * (self.packed or 0), np.int32), (nc * 6, np.uint64)])

    def refuse(self, k, wrap=None):
        ranks = self.ranks(k)
        ranks[3, k // 2] = len(self.w.vectors[3])
        raises(20, "contig 3: rank %d" % len(self.w.vectors[3]),
               lambda: self.w.pset.coverage_order_statistics(ranks))


def clusters_expected(w, groups):
    """the eight packed columns of peak_clusters(groups) from the yardsticks, group after group"""
    cols = [[] for _ in range(8)]
    for g in range(max(groups) + 1):
        members = [p for p in range(len(groups)) if groups[p] == g]
        table, m_peaks = cluster_ref([t_clu.member_peaks(w.columns[p]) for p in members])
        for j in range(4):
            cols[j].append(table[:, j])
        matrix = [m_peaks]
        stats = [region_ref(w.vectors[c], w.firsts[c], table[:, 0], table[:, 1])
                 for c in (w.pset.problems[p][0] for p in members)]
        for j in range(3):
            matrix.append(np.stack([s[j] for s in stats], axis=1) if members
                          else np.zeros((len(table), 0), np.int64))
        for j in range(4):
            cols[4 + j].append(matrix[j].reshape(-1))
    dtypes = (np.int32,) * 6 + (np.int64, np.int32)
    return [np.concatenate(c + [np.zeros(0, np.int64)]).astype(dt) for c, dt in zip(cols, dtypes)]


class Clusters(Service):
    """size: the peaks of the members, which are the set's models': 1 (the one-bump contig), 257 (a
    513-row model and that one), 3, 753 (every model in three groups), 0 (nobody in a group)"""
    name = "peak_clusters"
    small = 3
    device_inputs = False
    GROUPINGS = {1: [-1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1, -1],
                 257: [-1, -1, -1, -1, 0, -1, -1, -1, 0, -1, -1, -1],
                 3: [-1, -1, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1],
                 600: [0, 0, 0, 0, -1, 1, 1, 1, 2, -1, 2, 2],
                 0: [-1] * 12,
                 # the second sequence: many groups of one small member; one group of three big
                 # members; a group per problem
                 "many groups": [0, 1, 2, 3, 4, 5, 6, 7, -1, -1, -1, -1],
                 "many peaks": [-1, -1, -1, -1, -1, -1, -1, -1, 0, -1, 0, 0],
                 "all alone": list(range(12))}
    second = ("many groups", "many peaks", "all alone", 3)

    def grouping(self, size, seed=0):
        groups = list(self.GROUPINGS[size])
        if seed:                     # the same groups under other numbers, and an empty group 0
            groups = [g + 1 if g >= 0 else -1 for g in groups]
        peaks = sum(self.w.peaks(p) for p, g in enumerate(groups) if g >= 0)
        if isinstance(size, int) and self.w.solves == 1:      # (the models the sizes were named for)
            assert peaks == size or (size == 600 and peaks >= 600), (size, peaks)
        return groups, peaks

    def _call(self, size, seed=0, wrap=None):
        w = self.w
        groups, peaks = self.grouping(size, seed)
        result = w.pset.peak_clusters(groups, first_chromStart=w.firsts)
        if max(groups) < 0:
            assert result == []
        else:
            t_clu.check_clusters(w.pset, w.vectors, w.firsts, groups, w.columns, result,
                                 "%s %s" % (self.name, size))
        k = sum(len(e["clusters"]) for e in result)
        entries = sum(e["peaks"].size for e in result)
        self.packed = (k, entries)
        self.dims = (sum(g >= 0 for g in groups), max(groups) + 1, peaks, entries)
        out = []
        for e in sorted((e for e in result if len(e["members"])), key=lambda e: e["members"].tolist()):
            out += [e["clusters"].to_numpy()] + [e[n] for n in ("peaks", "bases", "sum", "max")]
        return out

    def download(self):
        k, e = self.packed or (0, 0)
        return self.raw_download("peakseg_hip_problem_set_packed_peak_clusters_download",
                                 [(k, np.int32)] * 4 + [(e, np.int32)] * 2 + [(e, np.int64), (e, np.int32)])

    def refuse(self, size, wrap=None):
        groups, _ = self.grouping(size)
        groups[5] = -3
        raises(22, "problem 5", lambda: self.w.pset.peak_clusters(groups, first_chromStart=self.w.firsts))


_JOINT_REFS = {}    # (members' contigs, window, penalty) -> the yardstick's result, or its MarginError
JOINT_PENALTIES = (5.0, 0.0, 60.0)


def joint_ref(w, contigs, window, penalty):
    key = (tuple(contigs), tuple(window), float(penalty))
    if key not in _JOINT_REFS:
        try:
            _JOINT_REFS[key] = joint_peaks_ref([w.vectors[c] for c in contigs],
                                               [w.firsts[c] for c in contigs], window, penalty)
        except MarginError as e:
            _JOINT_REFS[key] = e
    return _JOINT_REFS[key]


def joint_pool(w, groups):
    """per group the windows a call may draw from: the bumps of its members' contigs, each widened by
    its own width, that the yardstick can decide at every one of JOINT_PENALTIES (it asserts its
    margins before any device result is looked at; joint_ref.py says why)"""
    pool = []
    for g in range(max(groups) + 1):
        contigs = [PROBLEMS[p][0] for p in range(len(groups)) if groups[p] == g]
        usable = []
        for c in sorted(set(contigs)):
            for a, b, h in SAMPLES[c][2]:
                window = cluster_window(a, b)
                if window not in usable and not any(
                        isinstance(joint_ref(w, contigs, window, pen), MarginError)
                        for pen in JOINT_PENALTIES):
                    usable.append(window)
        assert len(usable) >= 3, (g, usable)
        pool.append(usable)
    return pool


def check_joint(w, entry, contigs, windows, penalty, what):
    """one group of joint_peaks() against the yardstick's kept results, as
    test_gpu_joint_peaks.check_group compares them"""
    frame = entry["joint"]
    ints = [n for n in t_joint.FRAME if n != "objective"]
    assert list(frame.columns) == t_joint.FRAME and len(frame) == len(windows), what
    assert all(frame[n].dtype == np.int32 for n in ints) and frame["objective"].dtype == np.float64
    assert entry["gain"].dtype == np.float64 and entry["sum"].dtype == np.int64
    assert entry["up"].dtype == entry["bases"].dtype == np.int32
    assert all(entry[n].shape == (len(windows), len(contigs)) for n in ("gain", "up", "sum", "bases"))
    table, objective = frame[ints].to_numpy(), frame["objective"].to_numpy()
    for k, window in enumerate(windows):
        ref = joint_ref(w, contigs, window, penalty)
        assert table[k].tolist() == [ref[n] for n in ints], (what, k, window, table[k].tolist())
        assert abs(np.longdouble(objective[k]) - ref["objective"]) <= ref["E"], (what, k)
        assert np.all(abs(entry["gain"][k].astype(np.longdouble) - ref["gain"]) <= ref["E"]), (what, k)
        for name in ("up", "sum", "bases"):
            assert np.array_equal(entry[name][k], ref[name]), (what, k, name)
        key = ("joint", tuple(contigs), tuple(window), float(penalty))
        bits = objective[k].tobytes() + entry["gain"][k].tobytes()
        assert w.bits.setdefault(key, bits) == bits, (what, k, "the same window, other bits")


class JointPeaks(Service):
    """size: windows, drawn over the groups; a tuple (grouping, windows) in the second sequence"""
    name = "joint_peaks"
    second = (("B", 9), ("A", 300), ("B", 40))
    n_pen = 0

    def inputs(self, size, seed, bad=None):
        which, n = size if isinstance(size, tuple) else ("A", size)
        groups = GROUPS if which == "A" else GROUPS_B
        pool = joint_pool(self.w, groups)
        rng = np.random.default_rng(7300 + n)
        g = rng.integers(0, len(pool), n)
        j = rng.integers(0, 1 << 20, n)
        order = permutation(n, seed)
        index = [order[g[order] == k] for k in range(len(pool))]
        windows = [[pool[k][j[i] % len(pool[k])] for i in at] for k, at in enumerate(index)]
        if bad is not None:
            k, i = g[bad], index[g[bad]].tolist().index(bad)
            windows[k][i] = (windows[k][i][1], windows[k][i][1])
        return groups, index, windows

    def penalties(self, size):
        return [JOINT_PENALTIES[0]]

    def run(self, groups, windows, pens, wrap):
        return [self.w.pset.joint_peaks(groups, penalty=pens[0], windows=t_joint.wrap_windows(windows, wrap),
                                        first_chromStart=self.w.firsts)]

    def _call(self, size, seed=0, wrap=None):
        w = self.w
        groups, index, windows = self.inputs(size, seed)
        pens = self.penalties(size)
        models = self.run(groups, windows, pens, wrap or w.wrap())
        n = sum(len(at) for at in index)
        rows = [[None] * n for _ in pens]
        entries = members = 0
        for model, pen, out in zip(models, pens, rows):
            assert len(model) == len(windows)
            for g, entry in enumerate(model):
                mine = [p for p in range(len(groups)) if groups[p] == g]
                assert entry["members"].tolist() == mine
                check_joint(w, entry, [PROBLEMS[p][0] for p in mine], windows[g], pen,
                            "%s %s group %d penalty %g" % (self.name, size, g, pen))
                frame = entry["joint"].to_numpy()
                for k, i in enumerate(index[g]):
                    out[i] = frame[k].tobytes() + b"".join(
                        entry[name][k].tobytes() for name in ("gain", "up", "sum", "bases"))
        for g, at in enumerate(index):
            m = sum(x == g for x in groups)
            members += m
            entries += len(at) * m
        self.models, self.groups = models, groups
        self.packed = (len(pens), n, entries)
        self.dims = (len(index), members, n, entries, len(pens))
        return [b"".join(out) for out in rows]

    def download(self):
        reps, k, e = self.packed or (1, 0, 0)
        dtypes = (np.int32,) * 4 + (np.float64, np.int32, np.int32, np.float64, np.int32, np.int64, np.int32)
        return self.raw_download("peakseg_hip_problem_set_packed_%s_download" % self.name,
                                 [((k if j < 7 else e) * reps, dt) for j, dt in enumerate(dtypes)])

    def count(self, size):
        return size[1] if isinstance(size, tuple) else size

    def refuse(self, size, wrap=None):
        bad = self.count(size) // 2
        groups, index, windows = self.inputs(size, 0, bad=bad)
        g = [k for k, at in enumerate(index) if bad in at.tolist()][0]
        needle = "group %d: window %d has start" % (g, index[g].tolist().index(bad))
        raises(22, needle, lambda: self.run(groups, windows, self.penalties(size), wrap or self.w.wrap()))

    def clusters_windows(self, groups, pens):
        """windows=None on a solved set: the clusters of `groups`, each widened by its own width;
        the models against the yardstick on those windows"""
        w = self.w
        if self.n_pen:
            models = w.pset.joint_path(groups, pens, first_chromStart=w.firsts)
        else:
            models = [w.pset.joint_peaks(groups, penalty=pens[0], first_chromStart=w.firsts)]
        n = entries = 0
        for model, pen in zip(models, pens):
            for g, entry in enumerate(model):
                mine = [p for p in range(len(groups)) if groups[p] == g]
                table, _ = cluster_ref([t_clu.member_peaks(w.columns[p]) for p in mine])
                windows = [cluster_window(a, b) for a, b in table[:, :2].tolist()]
                check_joint(w, entry, [PROBLEMS[p][0] for p in mine], windows, pen,
                            "%s clusters as windows, group %d" % (self.name, g))
                if pen == pens[0]:
                    n += len(windows)
                    entries += len(windows) * len(mine)
        self.models, self.groups = models, list(groups)
        self.packed = (len(pens), n, entries)
        return models


class JointPath(JointPeaks):
    """size: (penalties, windows): the rows of the first-level arrays are their product"""
    name = "joint_path"
    sizes = ((1, 1), (1, 257), (3, 1), (3, 200), (1, 0), (1, 257))
    small = (2, 20)
    second = (("B", 3, 9), ("A", 1, 300), ("B", 2, 40))
    n_pen = 1

    def inputs(self, size, seed, bad=None):
        return JointPeaks.inputs(self, size[-1] if len(size) == 2 else (size[0], size[2]), seed, bad)

    def penalties(self, size):
        return list(JOINT_PENALTIES[:size[-2]])

    def run(self, groups, windows, pens, wrap):
        return self.w.pset.joint_path(groups, pens, windows=t_joint.wrap_windows(windows, wrap),
                                      first_chromStart=self.w.firsts)

    def count(self, size):
        return size[-1]


class JointLabels(Service):
    """size: labels, over the problems; the rows are labels x the penalties of the packed path"""
    name = "joint_label_errors"

    def inputs(self, n, seed, bad=None):
        w = self.w
        rng = np.random.default_rng(7500 + n)
        q = rng.integers(0, len(PROBLEMS), n)
        s = rng.integers(0, 2000, n)
        e = s + rng.integers(1, 300, n)
        code = rng.integers(0, 4, n)
        if bad is not None:
            code[bad] = -1
        order = permutation(n, seed)
        index = [order[q[order] == k] for k in range(len(PROBLEMS))]
        labels = [tuple(as_numpy(a[at]) for a in (s, e, code)) if len(at) else None for at in index]
        return q, index, labels

    def _call(self, n, seed=0, wrap=None):
        w = self.w
        path = w["joint_path"]
        q, index, labels = self.inputs(n, seed)
        model, totals, rows = w.pset.joint_label_errors(t_lab.wrap_labels(labels, wrap or w.wrap()))
        want = joint_label_errors_ref(path.models, labels)
        assert model.dtype == np.int64 and np.array_equal(model, want[0]), (self.name, n)
        assert totals.dtype == np.int32 and np.array_equal(totals, want[1]), (self.name, n)
        out = [model, totals]
        for p in range(len(path.models)):
            for k in range(len(PROBLEMS)):
                for g, x in zip(rows[p][k], want[2][p][k]):
                    assert g.dtype == np.int32 and np.array_equal(g, x), (self.name, n, p, k)
                    out.append(g[np.argsort(index[k])])
        self.packed, self.dims = (len(path.models), n), (n, len(path.models))
        return out

    def download(self):
        reps, n = self.packed or (1, 0)
        k = len(PROBLEMS)
        return self.raw_download("peakseg_hip_problem_set_packed_joint_label_errors_download",
                                 [(reps * n, np.int32)] * 3 + [(reps * k * 5, np.int32), (reps * 5, np.int64)])

    def refuse(self, n, wrap=None):
        from peaksegdisk_amd import _native
        bad = n // 2
        q, index, labels = self.inputs(n, 0, bad=bad)
        needle = "problem %d: label %d has" % (q[bad], index[q[bad]].tolist().index(bad))
        raises(_native.ERROR_LABEL_ARGUMENTS, needle, lambda: self.w.pset.joint_label_errors(
            t_lab.wrap_labels(labels, wrap or self.w.wrap())))


class Heldout(Service):
    """size: pairs; in the second sequence many pairs on the one-row model (few rows), then fewer
    pairs on the 513-row models (many rows), then both"""
    name = "heldout_loss"
    #       problem, contig: every model on its own contig, those of 513 bases on both of them
    POOL = [(0, 0), (1, 1), (2, 2), (3, 0), (4, 5), (5, 3), (6, 4), (7, 3), (8, 6), (8, 7), (9, 6),
            (9, 7), (10, 7), (11, 6), (11, 7)]
    SCALES = (1.0, 0.5, 1.0 / 3.0)
    second = (("one row", 300), ("513 rows", 40), ("all", 5))
    POOLS = {"all": POOL, "one row": [(7, 3), (9, 6), (9, 7)], "513 rows": [(8, 6), (8, 7), (10, 7)]}

    def inputs(self, size, seed, bad=None):
        which, n = size if isinstance(size, tuple) else ("all", size)
        pool = self.POOLS[which]
        rng = np.random.default_rng(7600 + n)
        j = rng.integers(0, len(pool), n)
        problem = np.array([pool[i][0] for i in j], np.int32)
        contig = np.array([pool[i][1] for i in j], np.int32)
        scale = np.array([self.SCALES[i] for i in rng.integers(0, 3, n)], np.float64)
        if bad is not None:
            contig[bad] = len(self.w.vectors)
        order = permutation(n, seed)
        return problem[order], contig[order], scale[order], order

    def _call(self, size, seed=0, wrap=None):
        w = self.w
        problem, contig, scale, order = self.inputs(size, seed)
        n = len(order)
        out = w.pset.heldout_loss(t_held.wrap_pairs(wrap or w.wrap(), problem, contig, scale))
        names = ("loss", "rows", "bases", "sum", "zero_mean_rows")
        assert [out[k].dtype for k in names] == [np.float64, np.int32, np.int64, np.int64, np.int32]
        rows = 0
        for i, key in enumerate(zip(problem.tolist(), contig.tolist(), scale.tolist())):
            ref = w.bits.get(("heldout ref",) + key)
            if ref is None:
                ref = w.bits[("heldout ref",) + key] = heldout_pair_ref(
                    w.columns0[key[0]], w.vectors[key[1]], key[2])
            for name in names[1:]:
                assert int(out[name][i]) == ref[name], (self.name, size, i, name)
            if ref["zero_mean_rows"]:
                assert out["loss"][i] == INF
            else:
                assert abs(float(out["loss"][i]) - ref["loss"]) <= ref["tol"], (self.name, size, i)
            bits = out["loss"][i].tobytes()
            assert w.bits.setdefault(("heldout",) + key, bits) == bits, (self.name, size, i)
            rows += ref["rows"]
        self.packed, self.dims = n, (n, rows)
        inverse = np.argsort(order)
        return [out[name][inverse] for name in names]

    def download(self):
        n = self.packed or 0
        return self.raw_download("peakseg_hip_problem_set_packed_heldout_loss_download",
                                 [(n, dt) for dt in (np.float64, np.int32, np.int64, np.int64, np.int32)])

    def refuse(self, size, wrap=None):
        n = size[1] if isinstance(size, tuple) else size
        problem, contig, scale, _ = self.inputs(size, 0, bad=n // 2)
        raises(23, "pair %d:" % (n // 2), lambda: self.w.pset.heldout_loss(
            t_held.wrap_pairs(wrap or self.w.wrap(), problem, contig, scale)))

    def forget(self):
        """(a solve changes the models: what was scored before is no yardstick any more)"""
        for key in [k for k in self.w.bits if k[0] in ("heldout", "heldout ref")]:
            del self.w.bits[key]


class Fixed(Service):
    """the three services whose sizes are the models': the rows change through a solve only"""
    sizes = ()
    device_inputs = False

    def refuse(self, size, wrap=None):
        """a first_chromStart that takes a contig past 2^31 - 1: -1 and its text"""
        firsts = list(self.w.firsts)
        firsts[2] = 2 ** 31 - 100
        with pytest.raises(RuntimeError, match="contig 2: .* is no 32-bit coordinate"):
            getattr(self.w.pset, self.name)(first_chromStart=firsts)


class SegmentColumns(Fixed):
    name = "segment_columns"

    def _call(self, size=None, seed=0, wrap=None):
        w = self.w
        got = w.pset.segment_columns(first_chromStart=w.firsts)
        assert len(got) == len(w.columns)
        for p, (g, x) in enumerate(zip(got, w.columns)):
            assert [a.dtype for a in g] == [np.int32, np.int32, np.float64]
            assert same(list(g), list(x)), (self.name, p)
        self.packed = sum(len(x[0]) for x in w.columns)
        self.dims = (self.packed,)
        return [np.concatenate([g[j] for g in got]) for j in range(3)]

    def download(self):
        n = self.packed or 0
        return self.raw_download("peakseg_hip_problem_set_packed_segments_download",
                                 [(n, np.int32), (n, np.int32), (n, np.float64)])


class SegmentStats(Fixed):
    name = "segment_stats"

    def _call(self, size=None, seed=0, wrap=None):
        w = self.w
        got = w.pset.segment_stats(first_chromStart=w.firsts)
        assert len(got) == len(w.columns)
        for p, (c, pen) in enumerate(w.pset.problems):
            want = t_seg.expected_stats(w.vectors[c], w.columns[p][0], w.columns[p][1], w.firsts[c])
            assert [a.dtype for a in got[p]] == [np.int64, np.int32, np.int32, np.int32]
            for name, g, x in zip(("sum", "max", "summitStart", "summitEnd"), got[p], want):
                assert np.array_equal(g, x), (self.name, p, name)
        self.packed = sum(len(x[0]) for x in w.columns)
        self.dims = (self.packed,)
        return [np.concatenate([g[j] for g in got]) for j in range(4)]

    def download(self):
        n = self.packed or 0
        return self.raw_download("peakseg_hip_problem_set_packed_segment_stats_download",
                                 [(n, np.int64), (n, np.int32), (n, np.int32), (n, np.int32)])


class PackTables(Fixed):
    name = "pack_tables"

    def _call(self, size=None, seed=0, wrap=None):
        w = self.w
        rows, _, _, total = w.pset.pack_tables()
        assert rows.tolist() == [len(x[0]) for x in w.raw] and total == int(rows.sum())
        start, mean = w.pset.packed_download(total)
        assert start.tobytes() == np.concatenate([x[0] for x in w.raw]).tobytes(), self.name
        assert mean.tobytes() == np.concatenate([x[1] for x in w.raw]).tobytes(), self.name
        self.packed, self.dims = total, (total,)
        return [start, mean]

    def download(self):
        n = self.packed or 0
        return self.raw_download("peakseg_hip_problem_set_packed_download",
                                 [(n, np.int32), (n, np.float64)])


SERVICES = [Regions, Labels, Coverage, Clusters, JointPeaks, JointPath, JointLabels, Heldout,
            SegmentStats, SegmentColumns, PackTables]
HISTORY_SERVICES = [cls.name for cls in SERVICES if cls.sizes]
CAPPED_SERVICES = ["peak_clusters", "joint_peaks", "joint_path", "heldout_loss"]
MODEL_SERVICES = ["peak_clusters", "joint_peaks", "joint_path", "joint_label_errors", "heldout_loss",
                  "segment_stats", "label_errors", "segment_columns", "pack_tables"]


def history_of(cls):
    sizes = list(cls.sizes)
    return [(size, 11 if k == len(sizes) - 1 else 0) for k, size in enumerate(sizes)] + \
        [(size, 0) for size in cls.second]


def prepare(w, name):
    """what a service needs packed before its first call"""
    if name == "joint_label_errors":
        w["joint_path"].call((3, 12))


# ---- scenario 1 and the first half of 5: grow, shrink, grow, empty; the byte count ----------------

def run_history(w, name, history, refused_at=None):
    """the calls of `history` = [(size, seed)] on w's service `name`, each against its yardstick and
    downloaded; hbm_bytes never decreases, and does not change across a call that is no larger in
    any dimension than an earlier one that was given the same kind of memory.  -> (the columns of
    every call, hbm_bytes after every call)"""
    svc = w[name]
    outs, seen, trace = [], [], [w.pset.hbm_bytes]
    for k, (size, seed) in enumerate(history):
        if k == refused_at:
            break
        if name == "joint_label_errors" and size == "another path":
            w["joint_path"].call((1, 30))
            assert svc.download() is None                 # the header: until the next pack_joint_path
            outs.append(None)
            trace.append(w.pset.hbm_bytes)
            continue
        out = svc.call(size, seed)
        down = svc.download()
        assert down is not None, (name, size)
        now = w.pset.hbm_bytes
        assert now >= trace[-1], (name, size, now, trace[-1])
        if any(side == w.side and all(a <= b for a, b in zip(svc.dims, dims)) for dims, side in seen):
            assert now == trace[-1], (name, size, svc.dims, now, trace[-1])
        seen.append((svc.dims, w.side))
        outs.append(out)
        trace.append(now)
    return outs, trace


def scenario_history(psd, name, wraps=(as_numpy,)):
    """scenario 1 for one service: 1, 257, 3, 600, 0, 257 permuted -- the last equals the second
    once the permutation is undone -- and the service's second sequence"""
    cls = {c.name: c for c in SERVICES}[name]
    history = history_of(cls)
    if name == "joint_label_errors":       # the penalties of the path move against the labels
        history = history + [("another path", 0), (500, 0), (2, 0)]
    w = World(psd, wraps)
    try:
        prepare(w, name)
        outs, trace = run_history(w, name, history)
        assert same(outs[1], outs[len(cls.sizes) - 1]), (name, "call 2 and call 6 differ")
        assert trace[-1] > trace[0]
    finally:
        w.close()


# ---- the second half of scenario 5: twins under a cap ---------------------------------------------

ARENA_PIECES = 1 << 20      # the same arena in the set and its twins, whatever they are allowed


def scenario_capped_twins(psd, name):
    """the history of scenario 1 again on a twin allowed exactly what the first set held at its
    end: every call succeeds with the same columns; on a twin allowed 8 bytes less the call at which
    the first set reached that size is refused with ERROR_DEVICE_MEMORY, nothing is packed, and the
    set answers a smaller call.  For the services that ask whether a call fits before they allocate
    (the others have no such question to answer)."""
    from peaksegdisk_amd import _native
    cls = {c.name: c for c in SERVICES}[name]
    history = history_of(cls)
    if name == "peak_clusters":     # (its second sequence ends on growth that is not asked about:
        history = history[:len(cls.sizes)]                    # the groups' arrays, not the matrix)
    w = World(psd, arena_pieces=ARENA_PIECES)
    try:
        start = w.pset.hbm_bytes
        w["region_stats"].call(30)            # (another service's table, to look at after the refusal)
        outs, trace = run_history(w, name, history)
    finally:
        w.close()
    final = trace[-1]
    with capped(final):
        twin = World(psd, arena_pieces=ARENA_PIECES)
    try:
        assert twin.pset.hbm_bytes == start
        twin["region_stats"].call(30)
        again, trace2 = run_history(twin, name, history)
        assert trace2 == trace
        assert all(same(a, b) for a, b in zip(outs, again))
    finally:
        twin.close()
    at = trace.index(final) - 1                       # the call that reached the maximum
    assert all(b <= final - 8 for b in trace[:at + 1]), trace
    with capped(final - 8):
        twin = World(psd, arena_pieces=ARENA_PIECES)
    try:
        svc = twin[name]
        twin["region_stats"].call(30)
        earlier, trace3 = run_history(twin, name, history, refused_at=at)
        assert trace3 == trace[:at + 1] and all(same(a, b) for a, b in zip(outs, earlier))
        kept = twin.others(name)
        before = twin.pset.hbm_bytes
        with pytest.raises(RuntimeError, match="do not fit") as ei:
            svc.call(*history[at])
        assert ei.value.status == _native.ERROR_DEVICE_MEMORY == 14
        assert svc.download() is None
        if name == "peak_clusters":      # (the members and peaks of the call are there by then: the
            assert before <= twin.pset.hbm_bytes <= final          # header speaks of the matrix)
        else:
            assert twin.pset.hbm_bytes == before
        now = twin.others(name)
        assert all(same(kept[n], now[n]) or (kept[n] is None and now[n] is None) for n in kept)
        # ... also once a service that is not asked about has taken the set past what it is allowed:
        # a call that needs no more memory than its tables have fits
        twin["region_stats"].call(2000 + (final - twin.pset.hbm_bytes) // 40)
        assert twin.pset.hbm_bytes > final - 8
        smaller = svc.call(cls.small)
        assert svc.download() is not None and len(smaller)
    finally:
        twin.close()


# ---- scenario 2: services taking turns -----------------------------------------------------------

def pack_everything(w):
    """every service packed once at a middling size -> its columns; joint peaks and the path on given
    windows, so that the clusters stay those of peak_clusters()"""
    outs = {}
    for name, size in (("segment_columns", None), ("segment_stats", None), ("pack_tables", None),
                       ("label_errors", 70), ("region_stats", 90), ("coverage_order_statistics", 5),
                       ("peak_clusters", 600), ("joint_peaks", 25), ("joint_path", (2, 15)),
                       ("joint_label_errors", 80), ("heldout_loss", 60)):
        outs[name] = w[name].call(size)
    return outs


def unchanged(w, kept, but=()):
    now = w.others(*but)
    for name, cols in now.items():
        assert cols is not None and same(cols, kept[name]), (name, "changed by a call of", but)


def scenario_turns(psd, wraps=(as_numpy,)):
    """pack A, download it, call B, download A again through the C ABI: the same bytes.  B is each
    of pack_region_stats, pack_coverage_stats and pack_heldout_loss against every other service, at
    a size that makes B's tables grow; then pack_joint_peaks and pack_joint_path against each
    other."""
    w = World(psd, wraps)
    try:
        pack_everything(w)
        kept = w.others()
        assert all(cols is not None for cols in kept.values())
        for name, size in (("region_stats", 700), ("coverage_order_statistics", 16),
                           ("heldout_loss", 400), ("region_stats", 2), ("heldout_loss", 3),
                           ("coverage_order_statistics", 0)):
            w[name].call(size, seed=3)
            unchanged(w, kept, but=(name,))
            kept[name] = w[name].download()
        w["joint_peaks"].call(310, seed=5)
        unchanged(w, kept, but=("joint_peaks",))
        kept["joint_peaks"] = w["joint_peaks"].download()
        w["joint_path"].call((3, 120), seed=5)
        # (the label errors of a path go with it: the header ends them at the next pack_joint_path)
        unchanged(w, kept, but=("joint_path", "joint_label_errors"))
        assert w["joint_label_errors"].download() is None
    finally:
        w.close()


def scenario_clusters_as_windows(psd, wraps=(as_numpy,)):
    """pack_peak_clusters(G1), then pack_joint_peaks / pack_joint_path (G2, no windows): the windows
    are the clusters of G2, and the call packs them exactly as pack_peak_clusters(G2) would -- the
    download gives G2's whole table, columns and matrix, never a mixture"""
    w = World(psd, wraps)
    try:
        for name, pens in (("joint_peaks", [5.0]), ("joint_path", [5.0, 60.0])):
            w["peak_clusters"].call(600)
            first = w["peak_clusters"].download()
            w[name].clusters_windows(GROUPS_B, pens)
            want = clusters_expected(w, GROUPS_B)
            w["peak_clusters"].packed = (len(want[0]), len(want[4]))
            got = w["peak_clusters"].download()
            assert got is not None and not same(got, first)
            assert [a.dtype for a in got] == [a.dtype for a in want]
            assert same(got, want), name
            assert w[name].download() is not None
    finally:
        w.close()


# ---- scenario 3: a solve in between --------------------------------------------------------------

ROUNDS = [{BIG: INF, ONE_ROW: 0.0, 0: 100.0, 3: 10.0},     # 513 rows -> 1, 1 -> 513, 6 peaks <-> 5
          {BIG: 0.0, ONE_ROW: INF, 0: 10.0, 3: 100.0}]     # ... and back


def pack_model_services(w):
    w["peak_clusters"].call(600)
    w["joint_peaks"].clusters_windows(GROUPS, [5.0])
    w["joint_path"].clusters_windows(GROUPS, [5.0, 60.0])
    for name, size in (("joint_label_errors", 80), ("heldout_loss", 120), ("segment_stats", None),
                       ("label_errors", 70), ("segment_columns", None), ("pack_tables", None)):
        w[name].call(size)


def scenario_resolve(psd, wraps=(as_numpy,)):
    """every model-dependent service packed; set_penalty on four problems so that row counts change
    in both directions; solve().  Before any re-pack every model-dependent download says "nothing
    packed", and region and coverage stats download what they did.  Then every service again, against
    the yardsticks of the NEW models; and the same once more with the penalties put back."""
    w = World(psd, wraps)
    try:
        w["region_stats"].call(90)
        w["coverage_order_statistics"].call(5)
        free = ("region_stats", "coverage_order_statistics")
        for penalties in ROUNDS:
            pack_model_services(w)
            kept = w.others()
            assert all(cols is not None for cols in kept.values())
            rows_before = [len(x[0]) for x in w.columns]
            for p, pen in penalties.items():
                w.pset.set_penalty(p, pen)
            w["heldout_loss"].forget()
            rows_after = w.solve()
            assert rows_after[BIG] != rows_before[BIG] and rows_after[ONE_ROW] != rows_before[ONE_ROW]
            assert abs(rows_after[0] - rows_before[0]) == 2 == abs(rows_after[3] - rows_before[3])
            now = w.others()
            for name in MODEL_SERVICES:
                assert now[name] is None, (name, "serves the models of the solve before")
            for name in free:
                assert same(now[name], kept[name]), name
        pack_model_services(w)
        unchanged(w, {n: kept[n] for n in free}, but=MODEL_SERVICES)
    finally:
        w.close()


# ---- scenario 4: a refusal in between ------------------------------------------------------------

REFUSALS = {"region_stats": (50, 300, 20), "label_errors": (50, 300, 20),
            "coverage_order_statistics": (4, 12, 2), "peak_clusters": (3, 600, 1),
            "joint_peaks": (30, 200, 10), "joint_path": ((2, 20), (3, 100), (1, 10)),
            "joint_label_errors": (50, 300, 20), "heldout_loss": (50, 300, 20),
            "segment_columns": (None, None, None), "segment_stats": (None, None, None)}


def scenario_refusal(psd, name, refusing_wrap=None, wraps=(as_numpy,)):
    """a good call, a LARGER call that is refused for one bad entry, a smaller good call.  The
    refusal reports what the service's own tests say; its download then says "nothing packed";
    every other service downloads what it did; a refusal decided on the host leaves hbm_bytes as it
    was; the next call meets its yardstick.  refusing_wrap=as_cuda: the refused call has its arrays
    in device memory and is refused by its first launch (check words), and the call after it has
    host arrays on the same contigs."""
    w = World(psd, wraps)
    try:
        pack_everything(w)
        good, refused, after = REFUSALS[name]
        svc = w[name]
        svc.call(good)
        kept = w.others(name)
        before = w.pset.hbm_bytes
        svc.refuse(refused, refusing_wrap)
        assert svc.download() is None, (name, "serves a table after a refusal")
        if refusing_wrap is None:
            assert w.pset.hbm_bytes == before, (name, "a refusal on the host allocated")
        gone = ("joint_label_errors",) if name == "joint_path" else ()
        unchanged(w, kept, but=(name,) + gone)
        svc.call(after, wrap=as_numpy if refusing_wrap is not None else None)
        assert svc.download() is not None
        unchanged(w, kept, but=(name,) + gone)
    finally:
        w.close()


REFUSING = sorted(REFUSALS)
CHECK_WORDS = ["region_stats", "label_errors", "joint_label_errors", "heldout_loss", "joint_peaks",
               "joint_path"]


# ---- MI355X ----------------------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("name", HISTORY_SERVICES)
def test_gpu_history(psd, name):
    scenario_history(psd, name)


@GPU
@pytest.mark.parametrize("name", CAPPED_SERVICES)
def test_gpu_capped_twins(psd, name):
    scenario_capped_twins(psd, name)


@GPU
def test_gpu_services_taking_turns(psd):
    scenario_turns(psd)


@GPU
def test_gpu_clusters_as_windows(psd):
    scenario_clusters_as_windows(psd)


@GPU
def test_gpu_solve_in_between(psd):
    scenario_resolve(psd)


@GPU
@pytest.mark.parametrize("name", REFUSING)
def test_gpu_refusal_in_between(psd, name):
    scenario_refusal(psd, name)


_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_resident_tables as rt
rt.child_main(sys.argv[1])
print("tables-child ok: %%d calls" %% rt.CALLS[0])
"""


def run_child(which, timeout, calls):
    import re
    import subprocess
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code, which], capture_output=True, text=True,
                       timeout=timeout)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "tables-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
    assert int(re.search(r"tables-child ok: (\d+) calls", p.stdout).group(1)) >= calls


def child_main(which):
    """host and device inputs in one history: the inputs alternate between numpy arrays and cuda
    tensors from call to call on the same set (the host copies have capacities of their own that a
    device call does not grow)"""
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    both = (as_numpy, as_cuda)
    if which == "histories":
        for name in HISTORY_SERVICES:
            if {c.name: c for c in SERVICES}[name].device_inputs:
                scenario_history(psd, name, both)
                scenario_history(psd, name, both[::-1])
    elif which == "turns":
        scenario_turns(psd, both)
        scenario_turns(psd, both[::-1])
        scenario_clusters_as_windows(psd, both)
        scenario_resolve(psd, both)
    elif which == "refusals":
        for name in CHECK_WORDS:
            scenario_refusal(psd, name, refusing_wrap=as_cuda, wraps=both)
    else:
        raise ValueError(which)


@GPU
@pytest.mark.parametrize("which, calls", [("histories", 90), ("turns", 55), ("refusals", 70)])
def test_gpu_alternating_host_and_device_inputs(psd, which, calls):
    run_child(which, 240, calls)
