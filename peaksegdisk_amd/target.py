"""The target interval of a labelled contig: the interval of log(penalty) whose models have the
fewest label errors, found with several models per round on a resident problem set (DESIGN.md
section 12).  Host logic over ProblemSet.set_penalty / solve / loss / label_errors: it has no
device code of its own.

Every contig of a call owns `width` problem slots of one set; a round sets the penalties the
contigs ask for (slots nobody needs hold Inf, which is served in closed form), solves the set once
and counts the label errors of all its models once.  A contig's search is the class Search below,
a pure function of the rows it has been given, so it can be replayed without a device."""
import ctypes
import math

import pandas as pd

from . import _native

DEFAULT_WIDTH = 8   # the parallel search's default
MODEL_COLUMNS = ["penalty", "peaks", "total.loss", "errors", "fp", "fn", "round"]


def paste_penalty(lib, x):
    """a penalty as it travels: the 15-digit string of the searches, and the double it names"""
    buf = ctypes.create_string_buffer(64)
    lib.peakseg_hip_paste_double(float(x), buf, len(buf))
    text = buf.value.decode()
    return text, float(text)


def place_penalties(lib, under, over, secant, extras):
    """the parallel search's ladder between the penalties `over` < `under`
    (peakseg_hip_search_place_penalties)"""
    if extras <= 0:
        return []
    out = (ctypes.c_double * extras)()
    n = lib.peakseg_hip_search_place_penalties(float(under), float(over), float(secant), extras, out)
    return list(out[:n])


class Model:
    """rows of equal peaks: one model, from its smallest to its largest solved penalty.  Its loss
    and its errors are those of the first of its rows to be solved: total.loss is computed from
    the penalised cost and differs in its last digits from one penalty to the next, and a secant
    penalty that moved with it would never be the one already solved."""

    def __init__(self, row, first):
        self.peaks, self.errors, self.loss = row["peaks"], first["errors"], first["total.loss"]
        self.lo = self.hi = row["penalty"]


class TargetInterval:
    """What a search found: min_log_lambda, max_log_lambda (float, +-inf allowed), lower_exact,
    upper_exact (the limit is a breakpoint between two models proved neighbours, or infinite),
    min_errors, rounds, and models: a data frame with one row per solved penalty."""

    def __init__(self, lower, upper, lower_exact, upper_exact, min_errors, rounds, models):
        self.min_log_lambda, self.max_log_lambda = lower, upper
        self.lower_exact, self.upper_exact = lower_exact, upper_exact
        self.min_errors, self.rounds, self.models = min_errors, rounds, models

    def __repr__(self):
        return "TargetInterval(%r, %r, exact=(%r, %r), min_errors=%d, rounds=%d, %d models)" % (
            self.min_log_lambda, self.max_log_lambda, self.lower_exact, self.upper_exact,
            self.min_errors, self.rounds, len(self.models))


class Search:
    """One contig's search.  next_penalties(width) -> the penalty strings of the next round ([]:
    finished); add(penalty string, peaks, total loss, errors, fp, fn) for each of them; result()."""

    def __init__(self, lib):
        self.lib = lib
        self.rows = []
        self.asked = {}       # penalty string -> its double
        self.solved = {}      # penalty string -> the peaks of its model
        self.first = {}       # peaks -> the first row solved with that many
        self.round = 0
        self.finished = False

    # ---- the path known so far ------------------------------------------------------------
    def path(self):
        """the models by increasing penalty.  Rows that break the monotone decrease of peaks with
        the penalty (the cost near penalty 0 is unstable) are no bracket
        ends: walking down from the largest penalty, a row with fewer peaks than the row kept
        before it is passed over."""
        models = []
        for row in sorted(self.rows, key=lambda r: -r["penalty"]):
            if models and row["peaks"] < models[-1].peaks:
                continue
            if models and row["peaks"] == models[-1].peaks:
                models[-1].lo = row["penalty"]   # (walking down: the model's smallest so far)
            else:
                models.append(Model(row, self.first[row["peaks"]]))
        return models[::-1]

    def gap(self, a, b):
        """(secant penalty as it travels or None, closed?) of the neighbours a (more peaks), b"""
        secant = (b.loss - a.loss) / float(a.peaks - b.peaks)
        if not (math.isfinite(secant) and secant >= 0):
            return None, False
        text, value = paste_penalty(self.lib, secant)
        # closed: the model solved at the secant penalty has the peaks of a or of b.  (Asked by
        # its string, not by comparing penalties: within rounding of the breakpoint the two
        # models cost the same and the solver may return either on either side.)
        solved = self.solved.get(text)
        return value, solved is not None and solved in (a.peaks, b.peaks)

    def chosen(self, models):
        """(first, last) model of the run of fewest errors that is widest in log(penalty), its
        limits and whether they are exact"""
        best = min(m.errors for m in models)
        runs, k = [], 0
        while k < len(models):
            if models[k].errors != best:
                k += 1
                continue
            j = k
            while j + 1 < len(models) and models[j + 1].errors == best:
                j += 1
            runs.append((k, j))
            k = j + 1
        out = None
        for first, last in runs:
            lower, lower_exact, lower_open = self.limit(models, first, -1)
            upper, upper_exact, upper_open = self.limit(models, last, +1)
            size = upper - lower if upper > lower else 0.0
            # (>=: among equal widths the run of the larger penalties, the simpler model)
            if out is None or size >= out[0]:
                out = (size, first, last, lower, upper, lower_exact, upper_exact, lower_open,
                       upper_open)
        return (best,) + out[1:]

    def limit(self, models, k, side):
        """the limit of a run on the side of model k: (log penalty, exact?, the open gap (a, b) that
        a round has to work on, or None)"""
        m = models[k]
        if side < 0 and k == 0:
            return (-math.inf, True, None) if m.lo == 0 else (math.log(m.lo), False, None)
        if side > 0 and k == len(models) - 1:
            return (math.inf, True, None) if m.hi == math.inf else (math.log(m.hi), False, None)
        a, b = (models[k - 1], m) if side < 0 else (m, models[k + 1])
        secant, closed = self.gap(a, b)
        if closed:
            return (math.log(secant) if secant > 0 else -math.inf), True, None
        inside = m.lo if side < 0 else m.hi   # the nearest solved penalty of the run
        return (math.log(inside) if inside > 0 else -math.inf), False, (a, b, secant)

    # ---- a round ----------------------------------------------------------------------------
    def reserve(self, out, value, a, b):
        text, value = paste_penalty(self.lib, value)
        if text in self.asked or not (a.hi < value < b.lo):
            return False
        self.asked[text] = value
        out.append(text)
        return True

    def next_penalties(self, width):
        if self.finished:
            return []
        self.round += 1
        if self.round == 1:
            self.asked = {"0": 0.0, "Inf": math.inf}
            return ["0", "Inf"]
        chosen = self.chosen(self.path())
        gaps = [g for g in chosen[-2:] if g is not None]
        out = []
        for a, b, secant in gaps:           # first the secant penalties
            if len(out) < width and secant is not None:
                self.reserve(out, secant, a, b)
        for k, (a, b, secant) in enumerate(gaps):   # then the ladders, the slots split evenly
            room = (width - len(out)) // (len(gaps) - k)
            if room <= 0 or secant is None:
                continue
            for value in place_penalties(self.lib, b.lo, a.hi, secant, room):
                if room > 0 and self.reserve(out, value, a, b):
                    room -= 1
        if not out:   # both flanks closed or infinite -- or nothing left to ask between them
            self.finished = True
            self.round -= 1
        return out

    def add(self, text, peaks, total_loss, errors, fp, fn):
        self.solved[text] = int(peaks)
        self.rows.append({"penalty": self.asked[text], "peaks": int(peaks),
                          "total.loss": float(total_loss), "errors": int(errors), "fp": int(fp),
                          "fn": int(fn), "round": self.round})
        self.first.setdefault(int(peaks), self.rows[-1])

    def result(self):
        best, first, last, lower, upper, lower_exact, upper_exact, _, _ = self.chosen(self.path())
        return TargetInterval(lower, upper, lower_exact, upper_exact, best, self.round,
                              pd.DataFrame(self.rows, columns=MODEL_COLUMNS))


def target_interval(make_set, n_contigs, labels, width=DEFAULT_WIDTH, max_rounds=20):
    """The searches of n_contigs contigs in lockstep.  make_set(problems) -> (ProblemSet made by
    from_dense or from_reads, first_chromStart per contig); labels as ProblemSet.label_errors
    takes them.  Returns one TargetInterval per contig.  A round that meets ERROR_DEVICE_MEMORY
    halves the width for the rest of the call."""
    width = int(width) if width else DEFAULT_WIDTH
    slots = max(width, 2)      # round 1 asks for two models, one of them in closed form
    while True:
        try:
            pset, firsts = make_set([(c, math.inf) for c in range(n_contigs) for _ in range(slots)])
            break
        except RuntimeError as e:
            if getattr(e, "status", 0) != _native.ERROR_DEVICE_MEMORY or slots <= 2:
                raise
            width = max(1, width // 2)
            slots = max(width, 2)
    try:
        searches = [Search(pset._lib) for _ in range(n_contigs)]
        for _ in range(max_rounds):
            asked = [s.next_penalties(width) for s in searches]
            if not any(asked):
                break
            while True:
                for c, texts in enumerate(asked):
                    for k in range(slots):
                        pen = searches[c].asked[texts[k]] if k < len(texts) else math.inf
                        if pset.problems[c * slots + k][1] != pen:
                            pset.set_penalty(c * slots + k, pen)
                try:
                    pset.solve()
                    break
                except RuntimeError as e:
                    if getattr(e, "status", 0) != _native.ERROR_DEVICE_MEMORY or width <= 1:
                        raise
                    width = max(1, width // 2)
                    for s, texts in zip(searches, asked):   # what does not fit may be asked again
                        if s.round > 1:                     # (round 1's Inf model costs nothing)
                            for text in texts[width:]:
                                del s.asked[text]
                            del texts[width:]
            totals, _ = pset.label_errors(labels, first_chromStart=firsts)
            for c, texts in enumerate(asked):
                for k, text in enumerate(texts):
                    p = c * slots + k
                    loss = pset.loss(p)
                    searches[c].add(text, loss[2], loss[6], totals[p][0], totals[p][1], totals[p][2])
        return [s.result() for s in searches]
    finally:
        pset.close()
