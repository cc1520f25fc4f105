"""The twin harness of tests/test_graph_staleness_gpu.py: two contexts built by the same function, `plain` with RTOC_OPT_GRAPH off
and `graph` with it on, driven through the same calls and held to each other bit for bit.

A captured hipGraph freezes whatever the launchers read from the context at capture time (pointers, strides, counts, the kernels
chosen, scalars).  run_graphed (robotoc_amd/csrc/rt_context.hpp) trusts the graph while the context's epoch is the one it was
captured at, so a setter that changes such a value and forgets the epoch makes the next replay solve the previous problem without
any sign.  The protocol of `Twin.case` turns that into a failed assertion: three runs (warm-up, capture, replay), the mutation on
both contexts, three more runs, every run compared with np.array_equal on everything the sequence can write.  It fails by name:

  StaleReplay    an output of the graph context differs from the plain one's;
  NeverReplays   the replay counter did not advance where it must (a repair that merely stops graphing), or advanced where it
                 must not (a path that is not graphed);
  NoRecapture    a mutation that must start a new epoch did not: the three runs after it moved the replay counter by 3 (the graph
                 captured before it was replayed at once) where warm-up, capture + replay, replay move it by exactly 2 -- or the
                 other way round for a call that must leave the graph standing;
  MissingEffect  the mutation did not change the plain context's outputs, so equality afterwards proves nothing -- unless the
                 case names other evidence (`Effect`): a numerically neutral mutation (a stream, a bind to a copy, the same grid
                 again, a clone) shows what it did some other way.

The harness knows nothing of the library: contexts are whatever `restore`, `outputs` and `replays` understand, which is how
tests/test_graph_mutators.py runs it on plain Python fakes without a GPU."""
import numpy as np


class TwinFailure(AssertionError):
    pass


class StaleReplay(TwinFailure):
    """the graph context's outputs differ from the plain context's"""


class NeverReplays(TwinFailure):
    """the replay counter did not move as the case requires"""


class NoRecapture(TwinFailure):
    """the replay counter shows that the sequence was not captured anew after the mutation (or was, where it must not be)"""


class MissingEffect(TwinFailure):
    """the mutation left the plain context's outputs as they were and the case names no other evidence"""


class Effect:
    """Named evidence that replaces the default effect guard: check(twin, before, after) raises or returns False when the mutation
    cannot be shown to have acted.  before / after: the plain context's outputs of the last run before and the first run after."""

    def __init__(self, name, check):
        if not name or not callable(check):
            raise TypeError("an Effect is a name and a callable")
        self.name, self.check = name, check


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def differing(a, b):
    """names of the outputs that differ between two output dictionaries (NaN equals NaN: poison that nobody overwrote)"""
    if set(a) != set(b):
        return sorted(set(a) ^ set(b))
    return [k for k in a if not _same(a[k], b[k])]


class Twin:
    """plain, graph: the two contexts.  restore(ctx): the same inputs again (and the poison).  outputs(ctx) -> {name: array | None}:
    everything the launch sequence can write.  replays(ctx) -> int: the replay counter."""

    def __init__(self, plain, graph, restore, outputs, replays):
        self.plain, self.graph = plain, graph
        self._restore, self._outputs, self._replays = restore, outputs, replays
        self.last = None   # the plain context's outputs of the last run

    def both(self, fn):
        """apply a call to both contexts, the plain one first; returns both results"""
        return fn(self.plain), fn(self.graph)

    def replay_count(self):
        return self._replays(self.graph)

    def run(self, launch, what=""):
        """restore the same inputs on both, launch on both, hold every output of the graph context to the plain one's"""
        self.both(self._restore)
        self.both(launch)
        want, got = self._outputs(self.plain), self._outputs(self.graph)
        bad = differing(want, got)
        if bad:
            raise StaleReplay("%s: the graph context differs from the plain one in %s" % (what or "run", ", ".join(bad)))
        if self._replays(self.plain) != 0:
            raise NeverReplays("%s: the plain context replayed a graph" % (what or "run"))
        self.last = want
        return want

    def _three(self, launch, what, replay):
        n0 = self.replay_count()
        first = None
        for k in range(3):
            out = self.run(launch, "%s, run %d" % (what, k))
            first = out if first is None else first
        moved = self.replay_count() - n0
        if replay and moved <= 0:
            raise NeverReplays("%s: three runs and the replay counter stayed at %d" % (what, n0))
        if not replay and moved != 0:
            raise NeverReplays("%s: the replay counter moved by %d on a path that is not graphed" % (what, moved))
        return first, moved

    def case(self, mutate, launch, effect=None, name="case", replay_before=True, replay_after=True, recapture=None, guard=None):
        """warm-up, capture, replay; the mutation on both; three more runs, each bit-equal, and graphing must have resumed within
        them; the effect guard.  replay_before / replay_after = False: the replay counter must NOT move there (the line search).
        recapture = True: the mutation starts a new epoch, so the three runs after it are a plain one, the capture with its first
        launch and one replay -- the counter moves by exactly 2; False: the graph stands and is replayed three times; None: either.
        guard: the outputs the default effect guard looks at -- what the launch WRITES, where the mutation itself rewrites a buffer
        that is also an output (an upload, new event times) and the comparison of everything would hold trivially."""
        if effect is not None and not isinstance(effect, Effect):
            raise TypeError("effect: None (the plain outputs must change) or an Effect that names the replacement evidence")
        self._three(launch, name + " before the mutation", replay_before)
        before = self.last
        self.both(mutate)
        after, moved = self._three(launch, name + " after the mutation", replay_after)
        if recapture is not None and replay_after and moved != (2 if recapture else 3):
            raise NoRecapture("%s: the replay counter moved by %d in the three runs after the mutation, not by %d (%s)"
                              % (name, moved, 2 if recapture else 3, "a new epoch: plain run, capture + replay, replay" if recapture
                                 else "the graph stands: three replays"))
        if effect is None:
            changed = differing(before, after)
            if guard is not None:
                missing = [k for k in guard if k not in before or k not in after]
                if missing:
                    raise TypeError("%s: the guard names outputs that do not exist: %s" % (name, missing))
                changed = [k for k in guard if not _same(before[k], after[k])]
            if not changed:
                raise MissingEffect("%s: the mutation changed no output of the plain context" % name)
        elif effect.check(self, before, after) is False:
            raise MissingEffect("%s: no evidence of '%s'" % (name, effect.name))
        return before, after

    def inert(self, launch, name="path"):
        """a path that is not graphed: one plain-vs-graph run, results equal and the replay counter does not move"""
        n0 = self.replay_count()
        out = self.run(launch, name)
        if self.replay_count() != n0:
            raise NeverReplays("%s: the replay counter moved on a path that is not graphed" % name)
        return out
