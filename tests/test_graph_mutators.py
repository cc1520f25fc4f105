"""CPU side of the RTOC_OPT_GRAPH staleness tests.

Completeness: every function declared in include/rtoc.h and include/rtoc_robot.h is classified exactly once in
tests/graph_mutators.py, every RTOC_OPT_* enumerator has an option case, and every case the table names exists in
tests/test_graph_staleness_gpu.py -- a new setter or option fails here until it is classified and given a case.

The harness (tests/graph_twin.py) on fake contexts, plain Python objects whose "graph" keeps the arguments of its capture: the
protocol reports a stale replay, a missing effect, a context that never replays again and a mutation that did not start a new
epoch, each by name."""
import os
import re

import numpy as np
import pytest

import graph_mutators as gm
from graph_twin import Effect, MissingEffect, NeverReplays, NoRecapture, StaleReplay, Twin, differing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", h) for h in ("rtoc.h", "rtoc_robot.h")]


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def declared_functions(paths=HEADERS):
    """names of the functions the headers declare: `type rtoc_name(` at the start of a declaration, outside comments"""
    names = []
    for p in paths:
        names += re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(rtoc_\w+)\s*\(", _code(p), flags=re.M)
    return names


def declared_options(paths=HEADERS):
    out = []
    for p in paths:
        out += re.findall(r"\b(RTOC_OPT_\w+)\s*=\s*\d+", _code(p))
    return out


def unclassified(functions):
    known = gm.classes()
    return sorted(set(functions) - set(known)), sorted(set(known) - set(functions))


# ---- completeness -----------------------------------------------------------------------------------------------------------------
def test_the_parser_finds_the_abi():
    fns, opts = declared_functions(), declared_options()
    assert len(fns) == len(set(fns)) and len(fns) > 100
    for n in ("rtoc_create", "rtoc_error_string", "rtoc_device_ptr", "rtoc_set_grid", "rtoc_parnmpc_update_solution", "rtoc_foot_step_refs",
              "rtoc_solve_loop", "rtoc_wrench_cone_matrix"):   # int, const char*, void*, and the multi-line declarations
        assert n in fns, n
    assert len(opts) == len(set(opts)) > 0 and "RTOC_OPT_GRAPH" in opts and "RTOC_OPT_SWITCHING_TRANSPORT" in opts


def test_every_function_is_classified_exactly_once():
    missing, stale = unclassified(declared_functions())
    assert not missing, "declared in the headers and not classified in tests/graph_mutators.py: %s" % missing
    assert not stale, "classified and not declared any more: %s" % stale
    for n, cases in list(gm.MUTATORS.items()) + list(gm.UNDECLARED_MUTATORS.items()):
        assert cases, "the mutator %s names no case" % n
    assert not set(gm.UNDECLARED_MUTATORS) & set(declared_functions())


def test_a_new_declaration_fails_the_completeness_check(tmp_path):
    """a dummy setter and a dummy option added to a scratch copy of the header are reported"""
    scratch = tmp_path / "rtoc.h"
    text = open(HEADERS[0]).read()
    text = text.replace("int rtoc_sync(rtoc_ctx* ctx);", "int rtoc_sync(rtoc_ctx* ctx);\nint rtoc_set_dummy_knob(rtoc_ctx* ctx,\n    double value);")
    text = text.replace("RTOC_OPT_GRAPH = 9,", "RTOC_OPT_GRAPH = 9, RTOC_OPT_DUMMY = 18,")
    scratch.write_text(text)
    paths = [str(scratch), HEADERS[1]]
    missing, stale = unclassified(declared_functions(paths))
    assert missing == ["rtoc_set_dummy_knob"] and not stale
    assert sorted(set(declared_options(paths)) - set(gm.OPTION_CASES)) == ["RTOC_OPT_DUMMY"]


def test_every_option_has_an_option_case():
    opts = declared_options()
    assert sorted(opts) == sorted(gm.OPTION_CASES), sorted(set(opts) ^ set(gm.OPTION_CASES))
    # and the numbers the tests use are the header's
    from robotoc_amd import types
    for name, value in re.findall(r"\b(RTOC_OPT_\w+)\s*=\s*(\d+)", _code(HEADERS[0])):
        assert getattr(types, name[len("RTOC_"):]) == int(value), name


def test_every_named_case_exists():
    import test_graph_staleness_gpu as gpu
    for case in gm.named_cases():
        m = re.fullmatch(r"(test_\w+)(?:\[(.+)\])?", case)
        assert m, case
        fn, param = m.groups()
        assert callable(getattr(gpu, fn, None)), "tests/test_graph_staleness_gpu.py has no %s" % fn
        if param is not None:
            assert param in gpu.CASE_IDS.get(fn, ()), "%s has no case %s" % (fn, param)
    # no case of the module may skip or expect a failure
    src = open(gpu.__file__).read()
    assert not re.search(r"pytest\.skip|mark\.skip|xfail|importorskip", src)
    marks = gpu.pytestmark if isinstance(gpu.pytestmark, list) else [gpu.pytestmark]
    assert [m.name for m in marks] == ["gpu"]


# ---- the harness on fakes -----------------------------------------------------------------------------------------------------------
class FakeContext:
    """Computes out = gain * x + bias from its state at the time of the launch (label is state no launch reads).  With use_graph a
    launch follows run_graphed: a plain run at a new epoch, then a capture that KEEPS THE ARGUMENTS it saw, then replays of those
    arguments while the epoch stands.  forgets: the setters that do not bump the epoch (the bug the twin cases look for);
    stops_graphing: a `repair` that never replays again after any setter."""

    def __init__(self, use_graph, forgets=(), stops_graphing=False):
        self.use_graph, self.forgets, self.stops_graphing = use_graph, set(forgets), stops_graphing
        self.gain, self.bias, self.label = 2.0, 1.0, 0
        self.epoch, self.replays, self.x, self.out = 0, 0, None, None
        self.captured, self.warm_epoch, self.broken = None, None, False

    def set(self, name, value):
        setattr(self, name, value)
        if name not in self.forgets:
            self.epoch += 1
        if self.stops_graphing:
            self.broken = True

    def upload(self, x):
        self.x = np.array(x, dtype=float)

    def launch(self):
        args = (self.gain, self.bias)
        if self.use_graph and not self.broken:
            if self.captured is not None and self.captured[0] == self.epoch:
                args = self.captured[1]
                self.replays += 1
            elif self.warm_epoch != self.epoch:
                self.warm_epoch = self.epoch
            else:
                self.captured = (self.epoch, args)
                self.replays += 1
        self.out = args[0] * self.x + args[1]


def _fake_twin(**kw):
    x = np.arange(4.0)
    return Twin(FakeContext(False), FakeContext(True, **kw), lambda c: c.upload(x), lambda c: dict(out=c.out, label=np.array(c.label)),
                lambda c: c.replays)


def _launch(c):
    c.launch()


def test_fake_sound_setter_passes_and_replays():
    tw = _fake_twin()
    before, after = tw.case(lambda c: c.set("gain", 3.0), _launch, name="gain")
    assert differing(before, after) == ["out"] and tw.replay_count() == 4   # capture + replay, twice
    assert tw.plain.replays == 0


def test_fake_stale_replay_is_reported_by_name():
    tw = _fake_twin(forgets=["gain"])
    with pytest.raises(StaleReplay, match=r"gain after the mutation, run 0.*differs.*out"):
        tw.case(lambda c: c.set("gain", 3.0), _launch, name="gain")


def test_fake_missing_effect_is_reported_by_name():
    tw = _fake_twin()
    with pytest.raises(MissingEffect, match="changed no output"):
        tw.case(lambda c: c.set("gain", 2.0), _launch, name="the same gain")
    # a forgotten bump behind a mutation without effect is exactly what the guard is for: equality alone would have passed
    tw = _fake_twin(forgets=["gain"])
    with pytest.raises(MissingEffect):
        tw.case(lambda c: c.set("gain", 2.0), _launch, name="the same gain, bump forgotten")


def test_fake_named_effect_replaces_the_guard():
    tw = _fake_twin()
    neutral = Effect("the label reads back", lambda t, before, after: t.graph.label == 7 and not differing(before, after))
    with pytest.raises(MissingEffect, match="the label reads back"):
        tw.case(lambda c: None, _launch, effect=neutral, name="nothing set")
    tw = _fake_twin()
    seen = Effect("the label reads back", lambda t, before, after: t.graph.label == 7 and after["label"] == 7)
    tw.case(lambda c: c.set("label", 7), _launch, effect=seen, name="label")
    with pytest.raises(TypeError):
        tw.case(lambda c: None, _launch, effect=lambda *a: True)   # evidence without a name is an error of the harness
    with pytest.raises(TypeError):
        Effect("", lambda *a: True)


def test_fake_never_replays_again_is_reported_by_name():
    tw = _fake_twin(stops_graphing=True)
    with pytest.raises(NeverReplays, match="after the mutation.*stayed at 2"):
        tw.case(lambda c: c.set("gain", 3.0), _launch, name="gain")
    # and a path that must not replay but does
    tw = _fake_twin()
    with pytest.raises(NeverReplays, match="not graphed"):
        tw.inert(_launch) and tw.inert(_launch)
    tw = _fake_twin()
    with pytest.raises(NeverReplays, match="moved by"):
        tw.case(lambda c: c.set("gain", 3.0), _launch, name="gain", replay_after=False)


def test_fake_inert_path_and_equal_nan():
    tw = Twin(FakeContext(False), FakeContext(False), lambda c: c.upload([np.nan, 1.0]), lambda c: dict(out=c.out, none=None), lambda c: c.replays)
    out = tw.inert(_launch, "no graph at all")
    assert np.isnan(out["out"][0]) and out["none"] is None      # poison that nobody overwrote compares equal, like a buffer that is absent
    assert differing(dict(a=np.zeros(2)), dict(a=np.zeros(3))) == ["a"] and differing(dict(a=None), dict(a=np.zeros(1))) == ["a"]
    assert differing(dict(a=np.zeros(2)), dict(b=np.zeros(2))) == ["a", "b"]


def test_fake_missing_recapture_is_reported_by_name():
    """a neutral mutation whose bump is forgotten: every output equal, the old graph replayed three times instead of a new capture"""
    neutral = Effect("the label reads back", lambda t, before, after: t.graph.label == 7)
    tw = _fake_twin(forgets=["label"])
    with pytest.raises(NoRecapture, match="moved by 3 .* not by 2"):
        tw.case(lambda c: c.set("label", 7), _launch, effect=neutral, name="label", recapture=True)
    tw = _fake_twin()
    tw.case(lambda c: c.set("label", 7), _launch, effect=neutral, name="label", recapture=True)
    # and a call that must leave the graph standing
    tw = _fake_twin()
    with pytest.raises(NoRecapture, match="moved by 2 .* not by 3"):
        tw.case(lambda c: c.set("label", 7), _launch, effect=neutral, name="label", recapture=False)
    tw = _fake_twin()
    tw.case(lambda c: None, _launch, effect=Effect("nothing to see", lambda t, b, a: not differing(b, a)), name="nothing", recapture=False)


def test_fake_guard_looks_only_at_what_the_launch_writes():
    """`label` is an output the mutation itself rewrites: with the guard on `out` a mutation no launch reads is a missing effect"""
    tw = _fake_twin()
    tw.case(lambda c: c.set("label", 7), _launch, name="label, every output")   # holds trivially
    tw = _fake_twin()
    with pytest.raises(MissingEffect):
        tw.case(lambda c: c.set("label", 7), _launch, name="label, guarded", guard=("out",))
    tw = _fake_twin()
    tw.case(lambda c: c.set("gain", 3.0), _launch, name="gain, guarded", guard=("out",))
    with pytest.raises(TypeError):
        tw.case(lambda c: c.set("gain", 4.0), _launch, name="gain", guard=("nothing",))
