"""The target interval of the joint penalty: the interval of log(joint penalty) whose joint models
have the fewest label errors, the counterpart of target.py for the
multi-sample chain.  Host logic over ProblemSet.joint_path / joint_label_errors -- one of each per
round --: it has no device code of its own.

The level-by-level search has no exact breakpoints in the penalty, so the search brackets: it
evaluates penalties and narrows the two flanks of the best run until each lies within a factor
1 + tol.  One fact is used (DESIGN.md section 17 has the one-line proof): at level 0 every
candidate's G is non-increasing in the penalty, so a model without any joint peak -- the empty
model -- is the model of every larger penalty, and its errors are the labels' possible_fn.

JointSearch is a pure function of the rows it has been given: it can be replayed without a
device."""
import math

import numpy as np
import pandas as pd

DEFAULT_WIDTH = 8
DEFAULT_TOL = 0.05    # a choice, not a measurement: an end known to 5 % moves the midpoint of an
                      # interval in log(penalty) by at most 0.025, far inside the fit's margin 1
FLOOR = 1.0 / 1024    # penalty 0's stand-in, as a fraction of the smallest gain: the search for a
                      # lower end goes no further down
MODEL_COLUMNS = ["penalty", "peaks", "samples_up", "errors", "fp", "fn", "round"]


class JointTargetInterval:
    """What a search found: min_log_lambda, max_log_lambda (float, +-inf allowed: every penalty
    evaluated between their exps has min_errors errors), lower_closed, upper_closed (the end is
    within a factor 1 + tol of a penalty with more errors, or infinite), min_errors, rounds,
    models (a data frame with one row per evaluated penalty), and penalty: a joint penalty inside
    the interval -- exp of the midpoint of two finite ends, exp(max - 1) or exp(min + 1) for one
    infinite end (the margin 1 of the fit's hinge), 0.0 for two."""

    def __init__(self, lower, upper, lower_closed, upper_closed, min_errors, rounds, models):
        self.min_log_lambda, self.max_log_lambda = lower, upper
        self.lower_closed, self.upper_closed = lower_closed, upper_closed
        self.min_errors, self.rounds, self.models = min_errors, rounds, models
        if math.isinf(lower) and math.isinf(upper):
            self.penalty = 0.0
        elif math.isinf(lower):
            self.penalty = math.exp(upper - 1.0)
        elif math.isinf(upper):
            self.penalty = math.exp(lower + 1.0)
        else:
            self.penalty = math.exp(0.5 * (lower + upper))

    def __repr__(self):
        return "JointTargetInterval(%r, %r, closed=(%r, %r), min_errors=%d, rounds=%d, %d models)" % (
            self.min_log_lambda, self.max_log_lambda, self.lower_closed, self.upper_closed,
            self.min_errors, self.rounds, len(self.models))


def _log(x):
    return math.log(x) if x > 0 else -math.inf


class JointSearch:
    """next_penalties(width) -> the penalties of the next round ([]: finished); add(penalty, peaks,
    samples_up, errors, fp, fn) for each of them; after round 1, scale(smallest, largest): the
    smallest and largest positive gain of the model at penalty 0 (None, None: it has none);
    result().

    Round 1 asks for penalty 0 alone.  Round 2: `width` penalties log-spaced from the smallest to
    the largest gain.  While no empty model has been met: the largest penalty so far doubled, again
    and again.  Then, among the evaluated penalties, the run of fewest errors that is widest in
    log(penalty) -- among equal widths the run of the larger penalties --, extended to -inf where it
    holds penalty 0 and to +inf where it holds an empty model.  Each finite flank is the gap
    between the run's outermost penalty and its neighbour with more errors; it is closed when the
    two are within a factor 1 + tol.  Open gaps share the round's slots evenly, placed log-evenly
    inside.  Below, penalty 0 is stood in for by FLOOR times the smallest gain, which is evaluated
    itself: the gap between the two counts as closed."""

    def __init__(self, tol=DEFAULT_TOL):
        if not tol > 0:
            raise ValueError("tol %r: a positive number" % (tol,))
        self.tol = float(tol)
        self.rows = {}            # penalty -> row
        self.asked = set()
        self.round = 0
        self.gains = None         # (smallest, largest) positive gain at penalty 0, or (None, None)
        self.finished = False

    def scale(self, smallest, largest):
        if smallest is None or largest is None:
            self.gains = (None, None)
            return
        smallest, largest = float(smallest), float(largest)
        if not 0 < smallest <= largest < math.inf:
            raise ValueError("scale: 0 < smallest <= largest, not %r and %r" % (smallest, largest))
        self.gains = (smallest, largest)

    def add(self, penalty, peaks, samples_up, errors, fp, fn):
        penalty = float(penalty)
        if penalty not in self.asked:
            raise ValueError("add: penalty %r was not asked for" % penalty)
        self.rows[penalty] = {"penalty": penalty, "peaks": int(peaks), "samples_up": int(samples_up),
                              "errors": int(errors), "fp": int(fp), "fn": int(fn),
                              "round": self.round}

    # ---- the runs known so far --------------------------------------------------------------
    def _floor(self):
        return self.gains[0] * FLOOR

    def _closed(self, a, b):
        """the gap between the evaluated penalties a < b needs no more work"""
        if a == 0:
            return b <= self._floor() * (1.0 + self.tol)
        return b <= a * (1.0 + self.tol)

    def chosen(self):
        """(min errors, first index, last index, lower, upper, lower gap or None, upper gap or None)
        of the chosen run over the evaluated penalties in increasing order; a gap is (a, b, closed)"""
        rows = [self.rows[p] for p in sorted(self.rows)]
        best = min(r["errors"] for r in rows)
        out, k = None, 0
        while k < len(rows):
            if rows[k]["errors"] != best:
                k += 1
                continue
            j = k
            while j + 1 < len(rows) and rows[j + 1]["errors"] == best:
                j += 1
            first, last = rows[k]["penalty"], rows[j]["penalty"]
            empty = any(r["peaks"] == 0 for r in rows[k:j + 1])
            lower = -math.inf if first == 0 else math.log(first)
            upper = math.inf if empty else _log(last)
            lower_gap = upper_gap = None
            if first > 0:          # (penalty 0 is always evaluated: there is a neighbour below)
                a = rows[k - 1]["penalty"]
                lower_gap = (a, first, self._closed(a, first))
            if not empty and j + 1 < len(rows):
                b = rows[j + 1]["penalty"]
                upper_gap = (last, b, self._closed(last, b))
            size = upper - lower if upper > lower else 0.0
            # (>=: among equal widths the run of the larger penalties, as target.py)
            if out is None or size >= out[0]:
                out = (size, k, j, lower, upper, lower_gap, upper_gap)
            k = j + 1
        return (best,) + out[1:]

    # ---- a round ------------------------------------------------------------------------------
    def _take(self, out, value, width):
        value = float(value)
        if len(out) < width and value not in self.asked and math.isfinite(value) and value >= 0:
            self.asked.add(value)
            out.append(value)

    def _inside(self, out, a, b, slots, width):
        """up to `slots` penalties log-evenly inside the gap a < b"""
        if a == 0:
            floor = self._floor()
            if floor >= b:
                return
            self._take(out, floor, width)
            a, slots = floor, slots - 1
        for k in range(1, slots + 1):
            value = math.exp(math.log(a) + (math.log(b) - math.log(a)) * k / (slots + 1.0))
            if a < value < b:
                self._take(out, value, width)

    def next_penalties(self, width=DEFAULT_WIDTH):
        width = max(1, int(width))
        if self.finished:
            return []
        missing = self.asked - set(self.rows)
        if missing:
            raise ValueError("next_penalties: %d penalties asked for were not added" % len(missing))
        self.round += 1
        out = []
        if self.round == 1:
            self._take(out, 0.0, width)
            return out
        if self.gains is None:
            raise ValueError("next_penalties: scale() was not called after round 1")
        if self.gains[0] is None:                    # no gain at penalty 0: the empty model everywhere
            pass
        elif self.round == 2:
            lo, hi = math.log(self.gains[0]), math.log(self.gains[1])
            for k in range(width):
                self._take(out, math.exp(0.5 * (lo + hi) if width == 1 else lo + (hi - lo) * k / (width - 1.0)),
                           width)
        elif not any(r["peaks"] == 0 for r in self.rows.values()):
            top = max(max(self.rows), self.gains[1])
            for k in range(1, width + 1):
                self._take(out, top * 2.0 ** k, width)
        else:
            gaps = [g for g in self.chosen()[-2:] if g is not None and not g[2]]
            for k, (a, b, _) in enumerate(gaps):
                self._inside(out, a, b, (width - len(out)) // (len(gaps) - k), width)
        if not out:                                  # both flanks closed or infinite
            self.finished = True
            self.round -= 1
        return out

    def result(self):
        best, _, _, lower, upper, lower_gap, upper_gap = self.chosen()
        rows = sorted(self.rows.values(), key=lambda r: (r["round"], r["penalty"]))
        return JointTargetInterval(lower, upper, lower_gap is None or lower_gap[2],
                                   upper_gap is None or upper_gap[2], best, self.round,
                                   pd.DataFrame(rows, columns=MODEL_COLUMNS))


def joint_target_interval(pset, groups, labels, windows=None, first_chromStart=None,
                          width=DEFAULT_WIDTH, max_rounds=20, tol=DEFAULT_TOL):
    """The search on a ProblemSet made by from_dense or from_reads: one joint_path() and one
    joint_label_errors() per round.  groups, windows, first_chromStart as joint_path() takes them
    (windows=None: a solved set's clusters); labels as joint_label_errors() takes them, one entry
    per problem.  Returns a JointTargetInterval."""
    from . import _native
    width = min(max(1, int(width) if width else DEFAULT_WIDTH),
                int(_native.lib.peakseg_hip_joint_path_max_penalties()))
    search = JointSearch(tol)
    for _ in range(int(max_rounds)):
        penalties = search.next_penalties(width)
        if not penalties:
            break
        models = pset.joint_path(groups, penalties, windows=windows, first_chromStart=first_chromStart)
        totals, _, _ = pset.joint_label_errors(labels)
        for p, penalty in enumerate(penalties):
            peaks = sum(int((entry["joint"]["peakStart"] >= 0).sum()) for entry in models[p])
            up = sum(int(entry["joint"]["samples_up"].sum()) for entry in models[p])
            search.add(penalty, peaks, up, totals[p][0], totals[p][1], totals[p][2])
        if search.round == 1:
            gains = np.concatenate([entry["gain"].ravel() for entry in models[0]] + [np.zeros(0)])
            gains = gains[gains > 0]
            search.scale(*((float(gains.min()), float(gains.max())) if gains.size else (None, None)))
    return search.result()
