"""A state-machine model of one lane of the flat tracer's loop (tracer.hip trace_impl: the retire at
the loop top, the deferred camera ray, the fetch, the camera phase's shading, the main scan's
shading or pending hit), driven exhaustively, to decide whether a finished quantum's retire may
wait one iteration (the deferred retire, not built).

The model follows the kernel's order inside a wave-iteration:
  top     retire (by the rule under test); a deferred camera ray is set up (newray -> fresh);
          a lane that needs an item takes the next one (q changes: a fetched item or a stolen
          range alike) or, with none left, is done, which ends the model's loop;
  camera  a lane with a pending result, or a fresh camera ray and a list to trace it from, is
          shaded: the sample goes on with a bounce, or ends (acc += contribution; at a quantum's
          end fin; at the item's end fin and need, and the lane sits the main scan out; else the
          next sample's camera ray starts at once, fresh);
  main    the ray is traced; a hit, or any result of a lane with fin set, waits as pending for
          the next camera phase; a sky ray of a lane without fin ends the sample here (acc +=,
          fin / need as above, the next camera ray deferred: newray).
Every segment's outcome (sky, a bounce, the depth limit), whether a fresh ray has a list, and
whether the fetch is put off an iteration are free choices; items hold 1 to 3 quanta of G = 1, 2
or 4 samples, the last quantum whole or one short.

Three rules:
  immediate  the kernel's: a lane with fin retires at the next loop top;
  issue      the proposed deferral: the wave retires only when some fin lane has waited once, or
             is also need or done, or the loop exits (other lanes may force a retire at any top:
             a free choice here); "waited once => retire now";
  safe       the proposal plus what the hazard needs: a fin lane that can end a sample in this
             iteration's camera phase (pending, or a camera ray about to be traced) retires now.
Checked for each: every quantum retired exactly once and before q changes, no retire waits more
than one iteration, and acc never takes the next quantum's sample before the retire. The kernel's
rule holds all four. The proposal breaks the last one: a quantum that ends in iteration i leaves
its lane either with a result pending (the end came in the camera phase; the main scan's result
of a fin lane always waits) or with a camera ray deferred to the top of i + 1, and either can end
the next sample in the camera phase of i + 1, ahead of a retire at the top of i + 2. The safe rule
holds all four, and never defers: every fin lane is such a lane, so there is nothing to gain.
"""
import itertools

import pytest

SKY, BOUNCE, LIMIT = "sky", "bounce", "limit"
MAX_SEGMENTS = 3  # segments per sample the search follows (a sample of 1 to 3 iterations)


class Violation(Exception):
    pass


class Lane:
    def __init__(self, items, g, rule, choices):
        self.items, self.g, self.rule = list(items), g, rule
        self.choices = choices  # iterator of free choices, exhausted => StopIteration
        self.need, self.done, self.fin, self.waited = True, False, False, False
        self.pending, self.fresh, self.newray, self.tracing = None, False, False, False
        self.q, self.sample, self.end, self.nseg = None, 0, 0, 0
        self.acc = []          # (q, quantum) of every sample summed in acc since it was zeroed
        self.fin_q = None      # the pixel the finished quantum belongs to
        self.retired, self.max_wait, self.deferred = [], 0, 0
        self.next_item, self.put_off = 0, False

    def pick(self, options):
        return options[next(self.choices) % len(options)]

    # ---- the pieces of an iteration --------------------------------------------------------
    def retire(self):
        quanta = set(self.acc)
        if len(quanta) != 1:
            raise Violation(f"acc holds samples of {sorted(quanta)} at the retire")
        (qq, quantum), = quanta
        if qq != self.q or qq != self.fin_q:
            raise Violation(f"retire of pixel {qq} after q changed to {self.q}")
        self.retired.append((qq, quantum))
        self.max_wait = max(self.max_wait, 1 if self.waited else 0)
        self.acc, self.fin, self.waited = [], False, False

    def end_sample(self, defer_ray):
        if self.fin:
            raise Violation("acc += while a finished quantum waits in acc")
        self.acc.append((self.q, self.sample // self.g))
        self.sample += 1
        self.nseg, self.tracing = 0, False
        if self.sample == self.end:
            self.fin, self.need, self.fin_q = True, True, self.q
        else:
            if self.sample % self.g == 0:
                self.fin, self.fin_q = True, self.q
            if defer_ray:
                self.newray = True
            else:
                self.fresh = self.tracing = True

    def shade(self, outcome, defer_ray):
        self.nseg += 1
        if outcome == SKY or outcome == LIMIT:
            self.end_sample(defer_ray)
        # a bounce: the lane's ray goes on

    def outcome(self):
        return self.pick([SKY, LIMIT] if self.nseg + 1 >= MAX_SEGMENTS else [SKY, BOUNCE, LIMIT])

    def must_retire(self, forced):
        if not self.fin:
            return False
        if self.rule == "immediate":
            return True
        must = forced or self.waited or self.need or self.done
        if self.rule == "safe":
            must = must or self.pending is not None or self.fresh or self.newray
        return must

    def iteration(self):
        """One wave-iteration; False when the loop exits."""
        # -- top: the retire
        forced = self.pick([False, True]) if self.fin and self.rule != "immediate" else False
        if self.must_retire(forced):
            self.retire()
        elif self.fin:
            self.waited = True
            self.deferred += 1
        if self.newray:
            self.newray, self.fresh, self.tracing = False, True, True
        # -- top: the fetch (it may be put off once), the exit, a stolen range for a done lane
        if self.need and not self.done:
            if self.next_item < len(self.items) and not self.put_off and self.pick([False, True]):
                self.put_off = True  # the fetch deferred: the lane idles through this iteration
            elif self.next_item < len(self.items):
                self.take(self.items[self.next_item], self.next_item)
                self.next_item += 1
            else:
                self.done = True
        if self.done:
            if self.fin:
                raise Violation("the loop exits with a quantum not retired")
            return False
        # -- the camera phase
        if self.pending is not None:
            out, self.pending = self.pending, None
            self.fresh = False
            self.shade(out, False)
        elif self.fresh and self.tracing and self.pick([True, False]):  # its quarter has a list
            self.fresh = False
            self.shade(self.outcome(), False)
        if self.need:
            return True
        # -- the main scan and its shading
        if not self.tracing:
            return True
        out = self.outcome()
        self.fresh = False
        if out != SKY or self.fin:
            self.pending = out
        else:
            self.shade(out, True)
        return True

    def take(self, item, index):
        if self.fin:
            raise Violation("q changes with a quantum not retired")
        self.q, self.sample, self.end = index, 0, item
        self.need, self.fresh, self.tracing, self.nseg, self.put_off = False, True, True, 0, False


def run(items, g, rule, script):
    """One run under the script of free choices (padded with zeros); the lane at the loop's exit."""
    lane = Lane(items, g, rule, itertools.chain(script, itertools.repeat(0)))
    for _ in range(200):
        if not lane.iteration():
            break
    else:
        raise AssertionError("the model did not finish")
    want = [(i, k) for i, n in enumerate(items) for k in range(-(-n // g))]
    if lane.retired != want:
        raise Violation(f"retired {lane.retired}, want {want}")
    return lane


def explore(items, g, rule, depth):
    """Every script of `depth` free choices in 0..2 (a choice among fewer options wraps): the
    violations found and the lanes that finished."""
    bad, lanes = [], []
    for script in itertools.product(range(3), repeat=depth):
        try:
            lanes.append(run(items, g, rule, script))
        except Violation as v:
            bad.append((script, str(v)))
    return bad, lanes


CASES = [(items, g) for g in (1, 2, 4)
         for items in ([g], [2 * g], [3 * g], [g, g], [2 * g - (g > 1), g], [g, 3 * g - (g > 1)])]


@pytest.mark.parametrize("items,g", CASES)
def test_the_kernels_rule_holds(items, g):
    bad, lanes = explore(items, g, "immediate", 8)
    assert not bad, bad[:3]
    assert lanes and all(lane.max_wait == 0 for lane in lanes)


def test_the_proposed_deferral_adds_to_acc_before_the_retire():
    found = set()
    for items, g in CASES:
        bad, _ = explore(items, g, "issue", 8)
        found |= {what for _, what in bad}
    assert "acc += while a finished quantum waits in acc" in found
    # the only way it fails: nothing is lost, retired late across q, or left at the exit
    assert found == {"acc += while a finished quantum waits in acc"}, found
    # the shortest counterexample: one item of two quanta of one sample; sample 0 leaves through
    # the sky in the main scan of iteration 0 (fin, the camera ray deferred), nothing forces the
    # retire at the top of iteration 1, whose camera phase traces that ray into the sky
    with pytest.raises(Violation, match="acc \\+= while"):
        # choices: fetch not put off; no list for the first ray; sky in the main scan; the retire
        # not forced; a list for the second ray; sky
        run([2], 1, "issue", [0, 1, 0, 0, 0, 0])


@pytest.mark.parametrize("items,g", CASES)
def test_the_safe_rule_never_defers(items, g):
    bad, lanes = explore(items, g, "safe", 8)
    assert not bad, bad[:3]
    assert lanes and all(lane.deferred == 0 and lane.max_wait == 0 for lane in lanes)
