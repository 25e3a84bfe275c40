"""The yardstick of ProblemSet.joint_peaks: the definitions of include/peaksegdisk_hip.h restated in
plain numpy from per-base vectors -- np.cumsum in int64 for the sums, Python integers for the
feasibility products, np.longdouble for t, gain and G.

joint_peaks_ref() returns the choice of EVERY level of the search, with the runner-up's G and the
error bound  E = sum_i 2^-50 (T_i + |t1| + |t2| + |t3| + |t4|)  at the best candidate.  Why that
bound: the device's log is within 1 ulp and its division within 1 unit (peakseg_detmath.h), there
are two conversions, one product and three additions, so a term is off by at most
2^-51 S + 2^-51 |t| plus 3 * 2^-53 sum |t| for the additions, which the bound covers.

A scenario is usable only if, at every level, best - runner-up > 4 E: then no rounding of the
device can change a choice, and peaks, up, sums, bases and levels are compared for equality, gain
and objective within E.  The yardstick asserts the margin itself (MarginError), before any device
result is looked at; a scenario that fails is redesigned (sharper steps), not loosened.  Two more
margins of the same kind, for the same reason:
  - a window WITHOUT a joint peak has best = runner-up = 0 at level 0, so there the condition is
    that every candidate's G is 0 whatever the rounding: every member is infeasible at it (an exact
    integer test) or has gain - penalty < -4 E;
  - `up` is compared for equality, so every member feasible at the final peak has
    |gain - penalty| > 4 E."""
import collections
import hashlib

import numpy as np

BINS = 64


class MarginError(AssertionError):
    pass


def _term(S, L, real):
    """t(S, L) = S log(S / L), 0 where S = 0; S, L int64 arrays"""
    s = S.astype(real)
    q = np.where(S > 0, s, real(1)) / np.where(S > 0, L.astype(real), real(1))
    return np.where(S > 0, s * np.log(q), real(0))


def _above(a, la, b, lb):
    """a * la > b * lb, exactly"""
    if float(max(a.max(), b.max(), 1)) * float(max(la.max(), lb.max(), 1)) < 2.0 ** 62:
        return a * la > b * lb
    return np.array([int(x) * int(l) > int(y) * int(k) for x, l, y, k in zip(a, la, b, lb)], bool)


# What does not depend on the penalty -- per member its gain, feasibility, S2 and share of E at a
# set of candidates -- is kept for the last few (members' counts in the window, candidates): the
# tests of the joint path ask for the same window at up to 16 penalties in a row.  The key is the
# content, so a hit returns what the computation would.
_KEPT = collections.OrderedDict()
_KEEP = 8


class _Window:
    def __init__(self, vectors, firsts, ws, we, penalty, real):
        self.ws, self.we, self.penalty, self.real = ws, we, penalty, real
        self.cums = []
        for v, first in zip(vectors, firsts):
            part = np.asarray(v[ws - first:we - first], dtype=np.int64)
            self.cums.append(np.concatenate([[0], np.cumsum(part, dtype=np.int64)]))
        digest = hashlib.sha256(b"".join(c.tobytes() for c in self.cums)).digest()
        self.key = (digest, len(self.cums), ws, we, np.dtype(real).str)

    def members_at(self, s, e):
        """candidates s[], e[] (int64) -> per member (gain[], feasible[], S2[], its share of E[])"""
        key = self.key + (s.tobytes(), e.tobytes())
        if key in _KEPT:
            _KEPT.move_to_end(key)
            return _KEPT[key]
        real, ws, we = self.real, self.ws, self.we
        l1, l2, l3 = s - ws, e - s, we - e
        members = []
        for cum in self.cums:
            T = cum[-1]
            s1 = cum[s - ws]
            s2 = cum[e - ws] - s1
            s3 = T - cum[e - ws]
            ok = _above(s2, l1, s1, l2) & _above(s2, l3, s3, l2)
            t1, t2, t3 = _term(s1, l1, real), _term(s2, l2, real), _term(s3, l3, real)
            t4 = _term(np.array([T]), np.array([we - ws]), real)[0]
            gain = ((t1 + t2) + t3) - t4
            share = real(2.0 ** -50) * (real(T) + abs(t1) + abs(t2) + abs(t3) + abs(t4))
            members.append((gain, ok, s2, share))
        _KEPT[key] = members
        while len(_KEPT) > _KEEP:
            _KEPT.popitem(last=False)
        return members

    def evaluate(self, s, e):
        """candidates s[], e[] (int64) -> G[], E[], worst slack of a feasible member[], and per
        member (gain[], feasible[], S2[])"""
        real = self.real
        G = np.zeros(len(s), real)
        E = np.zeros(len(s), real)
        slack = np.full(len(s), -np.inf, real)
        members = []
        for gain, ok, s2, share in self.members_at(s, e):
            more = gain - real(self.penalty)
            G = G + np.where(ok & (more > 0), more, real(0))
            E = E + share
            slack = np.where(ok, np.maximum(slack, more), slack)
            members.append((gain, ok, s2))
        return G, E, slack, members


def clip_window(firsts, lengths, window):
    """the window clipped to the intersection of the members' extents -> (ws, we), we >= ws"""
    if len(firsts) == 0:
        return 0, 0
    lo = max(int(f) for f in firsts)
    hi = min(int(f) + int(n) for f, n in zip(firsts, lengths))
    ws, we = max(int(window[0]), lo), min(int(window[1]), hi)
    return ws, max(ws, we)


def cluster_window(cluster_start, cluster_end):
    """the window of a cluster: widened by its own width on either side"""
    w = int(cluster_end) - int(cluster_start)
    return int(cluster_start) - w, int(cluster_end) + w


def joint_peaks_ref(per_base_vectors, firsts, window, penalty, real=np.longdouble, check_margin=True):
    """The joint peak of the members (per-base int vectors with the coordinate of their first base)
    on `window` = (start, end) as given, at `penalty`.  -> a dict: windowStart, windowEnd, peakStart,
    peakEnd (-1: none), objective, samples_up, levels, E (the bound at the final peak), gain[], up[],
    sum[], bases[] per member, and trace: per level {b, s, e, G, runner_up, E}.  real=np.float64,
    check_margin=False: the host path that tools/joint_timing.py times."""
    m = len(per_base_vectors)
    ws, we = clip_window(firsts, [len(v) for v in per_base_vectors], window)
    W = we - ws
    none = {"windowStart": ws, "windowEnd": we, "peakStart": -1, "peakEnd": -1, "objective": real(0),
            "samples_up": 0, "levels": 0, "E": real(0), "gain": np.zeros(m, real),
            "up": np.zeros(m, np.int32), "sum": np.zeros(m, np.int64), "bases": np.zeros(m, np.int32),
            "trace": []}
    if W < 3 or m == 0:
        return none
    win = _Window(per_base_vectors, firsts, ws, we, penalty, real)
    b = 1
    while -(-W // b) > BINS:
        b *= 2
    n = -(-W // b)
    i, j = np.triu_indices(n - 1, 1)                    # 0 <= i < j <= n - 2
    s, e = ws + (i + 1).astype(np.int64) * b, ws + (j + 1).astype(np.int64) * b
    trace = []
    while True:
        G, E, slack, members = win.evaluate(s, e)
        order = np.lexsort((e, s, -G))                  # largest G, then smallest s, then smallest e
        best = int(order[0])
        runner = np.partition(G, -2)[-2] if len(G) > 1 else real(-np.inf)
        level = {"b": b, "s": int(s[best]), "e": int(e[best]), "G": G[best], "runner_up": runner,
                 "E": E[best]}
        if not trace and not G[best] > 0:
            if check_margin and not np.all(slack < -4 * E):
                c = int(np.argmax(slack + 4 * E))
                raise MarginError("no joint peak, but candidate (%d, %d) has a feasible member with "
                                  "gain - penalty = %g against E = %g" % (s[c], e[c], slack[c], E[c]))
            none["trace"] = [level]
            return none
        if check_margin and not G[best] - runner > 4 * E[best]:
            raise MarginError("level %d (b = %d): best G %.17g at (%d, %d), runner-up %.17g, E %g"
                              % (len(trace), b, G[best], s[best], e[best], runner, E[best]))
        trace.append(level)
        if b == 1:
            break
        b //= 2
        p, q = np.meshgrid(np.arange(-4, 5, dtype=np.int64), np.arange(-4, 5, dtype=np.int64),
                           indexing="ij")
        s, e = (level["s"] + p * b).ravel(), (level["e"] + q * b).ravel()
        keep = (ws < s) & (s < e) & (e < we)
        s, e = s[keep], e[keep]
    gain = np.array([g[best] if ok[best] else real(0) for g, ok, _ in members], real)
    feas = np.array([bool(ok[best]) for _, ok, _ in members])
    if check_margin:
        for k in np.flatnonzero(feas):
            if not abs(gain[k] - real(penalty)) > 4 * E[best]:
                raise MarginError("member %d: gain %.17g is within 4 E = %g of the penalty %g"
                                  % (k, gain[k], 4 * E[best], penalty))
    up = (feas & (gain > real(penalty))).astype(np.int32)
    return {"windowStart": ws, "windowEnd": we, "peakStart": level["s"], "peakEnd": level["e"],
            "objective": G[best], "samples_up": int(up.sum()), "levels": len(trace), "E": E[best],
            "gain": gain, "up": up, "sum": np.array([int(s2[best]) for _, _, s2 in members], np.int64),
            "bases": np.full(m, level["e"] - level["s"], np.int32), "trace": trace}
