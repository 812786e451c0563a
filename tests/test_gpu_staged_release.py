"""What the four kinds of staged input (traces, operations, steps, calls) share and no other module checks (csrc/zkm_internal.h
zkm_copy_fence; the Python handles' one base class).

Freed while in flight: a handle staged from page-locked memory is freed at once, without ready(), and its source overwritten with junk.
free() waits for the queued work before the block goes back to the allocator, so the live bytes are what they were, and the unstaged call
of the same segment -- which takes its blocks from the same allocator -- gives the words it gave before.  It runs a second time beside
a block of the released size, taken in front of it and filled with a pattern, which keeps the pattern: no late copy lands in it.

ready() and the lifetime on every kind: ready() answers True or False right after the stage, True once waited for; a second free() does
nothing; a dropped handle, the end of a `with` block and Context.close() each give the live bytes back (test_gpu_staged_ordering.py has
the last three for StagedTrace: here the other four classes)."""
import gc

import numpy as np
import pytest

from . import segment_ops_fixtures as SF
from .test_gpu_calls_entry import assert_expansions_equal
from .test_gpu_calls_stage import pinned_copy, wanted
from .test_gpu_cpu_steps import two  # noqa: F401  (a module-scoped fixture)
from .test_gpu_segment_ops import assert_tables_equal, tables_of
from .test_segments_batch import _segment

pytestmark = pytest.mark.gpu

PATTERN = np.uint64(0x0123456789ABCDEF)
KINDS = ["segment", "trace", "ops", "steps", "calls"]


def pinned_steps(zkm, ctx, st, pins):
    """The step list with its records and rows in page-locked memory."""
    return zkm.CpuSteps(pinned_copy(ctx, st.steps, pins), pinned_copy(ctx, st.raw_rows, pins))


def downloaded(ctx, built):
    """[(the twelve tables, log_ns)] of a segments_tables* call, the handles freed."""
    out = []
    for st, lg in built:
        out.append((tables_of(st, lg, ctx), lg))
        st.free()
    return out


@pytest.fixture(scope="module")
def host(ctx, zkm, oracle, two):  # noqa: F811
    """The small segments of the other modules, in pageable host memory: the sample program's operations; the two step lists of 2^8 and
    2^9 rows with the operations beside them; the calls of the segment with a call of every kind, and their expansion."""
    kw, expansion = wanted(ctx, zkm, "all")
    return {"raw": SF.build_segment_ops(oracle)[0], "steps": [s for s, _, _ in two["own"]], "beside": [o for _, o, _ in two["own"]], "kw": kw,
            "expansion": expansion}


@pytest.fixture(scope="module")
def cases(ctx, zkm, host):
    """Per kind: stage(pins) -> a handle staged from page-locked copies (appended to pins) of the kind's small segment, unstaged() -> the
    words of the unstaged call on the same segment, and `want`: those words, computed once here and left unchanged."""
    from zkm_amd import tables as T
    out = {}
    # traces: the committed twelve-table segment; one table of it alone (the widest) for stage_trace
    tr, lg = _segment(0)
    wide = max(range(12), key=lambda i: tr[i].size)
    prove = lambda: ctx.prove_segment(tr, lg, public_values=[5, 3])
    out["segment"] = (lambda pins: ctx.stage_segment([pinned_copy(ctx, t, pins) for t in tr], lg), prove)
    out["trace"] = (lambda pins: ctx.stage_trace(pinned_copy(ctx, tr[wide], pins), T.WIDTH[T.TABLE_ENUM_ORDER[wide]], lg[wide]), prove)
    raw, steps, beside, kw = host["raw"], host["steps"], host["beside"], host["kw"]

    def stage_ops(pins):
        pinned = SF.segment_ops(zkm, raw).to_pinned(ctx)
        pins += [v for k, v in pinned.lists.items() if not k.endswith("_off")]
        return ctx.stage_segment_ops(pinned)
    out["ops"] = (stage_ops, lambda: downloaded(ctx, ctx.segments_tables([SF.segment_ops(zkm, raw)])))
    out["steps"] = (lambda pins: ctx.cpu_steps_stage([pinned_steps(zkm, ctx, s, pins) for s in steps]),
                    lambda: downloaded(ctx, ctx.segments_tables_steps(steps, beside)))

    def stage_calls(pins):
        p = dict(kw, steps=pinned_steps(zkm, ctx, kw["steps"], pins))
        for name in ("extend", "compress", "keccak", "io", "insns"):
            if kw[name] is not None:
                p[name] = tuple(pinned_copy(ctx, a, pins) for a in kw[name])
        return ctx.segments_calls_stage([zkm.SegmentCalls(**p)])

    def expand():
        with ctx.segments_calls_expand([zkm.SegmentCalls(**kw)]) as x:
            return x.download(0)
    out["calls"] = (stage_calls, expand)
    # (the unstaged calls once: they may grow the download area, and what they give is the yardstick)
    want = {kind: host["expansion"] if kind == "calls" else unstaged() for kind, (_, unstaged) in out.items() if kind != "trace"}
    want["trace"] = want["segment"]
    return {kind: (stage, unstaged, want[kind]) for kind, (stage, unstaged) in out.items()}


def assert_same_words(kind, got, want):
    if kind == "calls":
        assert_expansions_equal(got, want, kind)
    elif kind in ("segment", "trace"):
        assert list(got[2]) == list(want[2]) and (got[1] == want[1]).all() and (got[0] == want[0]).all(), kind
    else:
        for (g, glg), (w, wlg) in zip(got, want):
            assert glg == wlg
            assert_tables_equal(g, w)


@pytest.mark.parametrize("kind", KINDS)
def test_freed_while_in_flight(ctx, cases, kind):
    stage, unstaged, want = cases[kind]
    pins, probe, h = [], None, None
    try:
        live = ctx.memory()[0]
        h = stage(pins)
        held = ctx.memory()[0] - live
        assert held > 0 and pins
        h.free()                             # at once: no ready() in between
        for a in pins:
            a.reshape(-1).view(np.uint8)[:] = 0xDB
        assert ctx.memory()[0] == live, "free() kept %d live bytes" % (ctx.memory()[0] - live)
        # the unstaged call with the released blocks in the allocator's lists, for it to take ...
        assert_same_words(kind, unstaged(), want)
        assert ctx.memory()[0] == live
        # ... and once more beside a probe of the released size.  A handle of ONE block: the allocator's exact-size list hands that very
        # block out again (the calls' handle has several: the probe is then a block that is as good)
        probe = ctx.alloc(held // 8).upload(np.full(held // 8, PATTERN, dtype=np.uint64))
        assert_same_words(kind, unstaged(), want)
        left = probe.download()
        assert (left == PATTERN).all(), "a copy landed in the released block after free(): word %d" % int(np.nonzero(left != PATTERN)[0][0])
    finally:
        if h is not None:
            h.free()                         # (a failure in front of the free above: the sources outlive the uploads)
        if probe is not None:
            probe.free()
        for a in pins:
            ctx.free_pinned(a)
    assert ctx.memory()[0] == live


@pytest.mark.parametrize("kind", KINDS)
def test_ready_answers_on_every_kind_and_a_second_free_does_nothing(ctx, cases, kind):
    stage = cases[kind][0]
    pins, h = [], None
    try:
        live = ctx.memory()[0]
        h = stage(pins)
        assert h.ready() in (True, False)    # (in flight or landed: never an error)
        assert h.ready(wait=True) is True and h.ready() is True
        h.free()
        assert h.h is None and ctx.memory()[0] == live
        h.free()
        assert ctx.memory()[0] == live
    finally:
        if h is not None:
            h.free()
        for a in pins:
            ctx.free_pinned(a)


def stagers(zkm, c, host):
    """The four classes beside StagedTrace, each staged on context c from pageable host memory."""
    calls = lambda: [zkm.SegmentCalls(**host["kw"])]
    return {"StagedOps": lambda: c.stage_segment_ops(SF.segment_ops(zkm, host["raw"])), "StagedSteps": lambda: c.cpu_steps_stage(host["steps"]),
            "ExpandedCalls": lambda: c.segments_calls_expand(calls()), "StagedCalls": lambda: c.segments_calls_stage(calls())}


class LookBeforeDestroy:
    """The library as a Context sees it, with the allocator's live bytes noted when the context is destroyed."""

    def __init__(self, lib, ctx, seen):
        self._lib, self._ctx, self._seen = lib, ctx, seen

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def zkm_ctx_destroy(self, h):
        self._seen.append(self._ctx.memory()[0])
        return self._lib.zkm_ctx_destroy(h)


@pytest.mark.parametrize("cls", ["StagedOps", "StagedSteps", "ExpandedCalls", "StagedCalls"])
def test_dropped_scoped_or_outliving_its_context_a_handle_returns_its_blocks(zkm, host, cls):
    c = zkm.Context(0)
    try:
        stage = stagers(zkm, c, host)[cls]
        stage().free()                       # (the first call may create what the context keeps: streams, the download area)
        live = c.memory()[0]
        h = stage()
        assert type(h).__name__ == cls and isinstance(h, zkm._StagedHandle) and c.memory()[0] > live
        del h
        gc.collect()
        assert c.memory()[0] == live, "a dropped %s kept its blocks" % cls
        with stage() as h:
            assert c.memory()[0] > live
        assert h.h is None and c.memory()[0] == live
        h.free()                             # (a second free is a no-op)
        h, seen = stage(), []
        assert c.memory()[0] > live
        c.L = LookBeforeDestroy(c.L, c, seen)
        c.close()
        assert seen == [live], "close() destroyed the context with a %s outstanding" % cls
        assert h.h is None
        h.free()                             # a no-op: the context that owned it is gone
    finally:
        c.close()
