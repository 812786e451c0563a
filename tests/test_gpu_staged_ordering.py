"""Staged traces consumed while their upload is still in flight (include/zkm_hip.h "staged traces").  A driver stages the next segment
from page-locked memory and hands it to the next prove call at once; every stream of that call -- the context's compute stream, the
commit lanes' compute and copy streams, the context's copy stream -- must come after the upload and after the canonicalising pass of a
copy the caller did not vouch for.  Each case first queues a large pinned decoy on the consuming context's two copy streams, so the
inputs under test land tens of milliseconds after the prove call has started (the test asserts that they have not landed yet), and then
compares every word with the proofs of the same segments from plain host arrays.  Also here: a StagedTrace that is dropped, used as a
context manager or outlives its Context neither leaks nor dangles."""
import contextlib
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_segments_batch import _segment

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001
DECOY_COLS, DECOY_LOG_N = 32, 24          # 4 GiB: four 1 GiB pieces, two ahead of the inputs on each copy stream

# commit_lanes x aux_pipeline: both lane paths (all auxiliary commitments on lanes, or built behind the table proofs) at 2, 4, 8 lanes
LANES = [(2, 0), (2, 1), (4, 0), (4, 1), (8, 0), (8, 1)]
LANE_IDS = ["lanes%d-aux%d" % la for la in LANES]
CASES = "abcde"


def _variants(case, lanes, aux, k):
    """k segment variants no other case of this file uses: an unordered read must never find a block that held the same data."""
    slot = CASES.index(case) * len(LANES) + LANES.index((lanes, aux))
    return [1 + 4 * slot + i for i in range(k)]


def _expected(ctx, v):
    """(traces, log_n, public values, proof) of variant v, the proof made on the session context from plain host arrays."""
    tr, lg = _segment(v)
    pub = [v, 3]
    return tr, lg, pub, ctx.prove_segment(tr, lg, public_values=pub)


def _check(got, want, what):
    proofs, chal, offs = got
    wproofs, wchal, woffs = want
    assert list(offs) == list(woffs), "%s: proof layout differs" % what
    bad = np.nonzero(proofs != wproofs)[0]
    assert bad.size == 0, "%s: %d words differ, the first is word %d (table %d)" % (
        what, bad.size, bad[0], int(np.searchsorted(woffs, bad[0], side="right")) - 1)
    assert (chal == wchal).all(), "%s: CTL challenges differ" % what


@pytest.fixture(scope="module")
def decoy(ctx):
    """A page-locked host matrix (zkm_host_alloc memory is pinned for the whole process, whichever context allocated it)."""
    a = ctx.pinned_array(DECOY_COLS << DECOY_LOG_N)
    yield a
    ctx.free_pinned(a)


@contextlib.contextmanager
def _fresh(zkm, lanes, aux):
    """A fresh context with the case's lane settings: its blocks never held another case's data.  Whatever it staged is freed (the
    uploads waited for) before its pinned inputs go, also when a comparison failed."""
    c = zkm.Context(0)
    c.case, c.handles = (lanes, aux), []
    try:
        c.set_tuning("commit_lanes", lanes)
        c.set_tuning("aux_pipeline", aux)
        yield c
    finally:
        for st in c.handles:
            st.free()
        c.close()


@pytest.fixture
def consumer(zkm, request):
    with _fresh(zkm, *request.param) as c:
        yield c


def _pinned(c, a):
    p = c.pinned_array(a.size)
    p[:] = a
    return p


def _columns(m, table):
    from zkm_amd import tables as T
    w = T.WIDTH[T.TABLE_ENUM_ORDER[table]]
    return [m.reshape(w, -1)[k] for k in range(w)]


def _stage(c, method, *args, **kw):
    st = getattr(c, method)(*args, **kw)
    c.handles.append(st)
    return st


def _consume(c, staged, control, prove):
    """Either (control) wait for every input upload, or assert that none has landed yet; then prove at once."""
    for st in staged:
        if control:
            assert st.ready(wait=True) is True
        else:
            assert st.ready() is False, "the input upload finished before the prove call: enlarge the decoy"
    return prove()


def _segments_case(c, ctx, decoy, variants, forms, control):
    """Segments staged with stage_segment in the given forms ("block", "columns", "loose") behind the decoy, one lock-step call."""
    want = [_expected(ctx, v) for v in variants]
    host = []
    for (tr, lg, pub, _), form in zip(want, forms):
        pin = [_pinned(c, t) for t in tr]
        if form == "loose":                  # every small word + p in a third of the tables: canonicalised when first consumed
            for t in pin[::3]:
                small = t < (1 << 32) - 1
                t[small] += np.uint64(P)
        host.append((pin, lg, form))
    _stage(c, "stage_trace", decoy, DECOY_COLS, DECOY_LOG_N)
    staged = []
    for pin, lg, form in host:
        if form == "columns":
            staged.append(_stage(c, "stage_segment", [_columns(t, i) for i, t in enumerate(pin)], lg))
        else:
            staged.append(_stage(c, "stage_segment", pin, lg, canonical=form != "loose"))
    got = _consume(c, staged, control,
                   lambda: c.prove_segments([(st.tables(), w[1], w[2]) for st, w in zip(staged, want)]))
    for v, g, w, form in zip(variants, got, want, forms):
        _check(g, w[3], "lanes %d aux %d, segment %d (%s)" % (c.case + (v, form)))
    return got


@pytest.mark.parametrize("consumer", LANES, ids=LANE_IDS, indirect=True)
def test_a_staged_segments_proven_at_once(consumer, ctx, decoy, oracle):
    """Three segments staged in block form from pinned memory, consumed by one prove_segments call while still in flight."""
    variants = _variants("a", *consumer.case, 3)
    got = _segments_case(consumer, ctx, decoy, variants, ["block"] * 3, control=False)
    if consumer.case == (4, 1):              # (the defaults) every segment against the CPU oracle's prove_with_traces as well
        from zkm_amd import tables as T
        ctl_tables, ctls = T.all_cross_table_lookups()
        for v, (proofs, chal, _) in zip(variants, got):
            (tr, lg), pub = _segment(v), [v, 3]
            tables = [(T.TABLE_ENUM_ORDER[i], tr[i], T.WIDTH[T.TABLE_ENUM_ORDER[i]], lg[i], ctl_tables[i]) for i in range(12)]
            ref, rchal, _ = oracle.prove_with_traces(tables, ctls, public_values=pub)
            bad = np.nonzero(proofs != ref)[0]
            assert bad.size == 0, "segment %d: first word differing from the oracle's is %d" % (v, bad[0])
            assert (chal == rchal).all()


@pytest.mark.parametrize("consumer", LANES, ids=LANE_IDS, indirect=True)
def test_b_staged_columns_and_loose_words_proven_at_once(consumer, ctx, decoy):
    """One segment staged per column, one not vouched canonical: the lanes also come after the canonicalising pass."""
    _segments_case(consumer, ctx, decoy, _variants("b", *consumer.case, 3), ["block", "columns", "loose"], control=False)


def _tables_case(c, ctx, decoy, v, control):
    """One segment as twelve separate stage_trace matrices, traces[t] of prove_segment."""
    from zkm_amd import tables as T
    tr, lg, pub, want = _expected(ctx, v)
    pin = [_pinned(c, t) for t in tr]
    _stage(c, "stage_trace", decoy, DECOY_COLS, DECOY_LOG_N)
    staged = [_stage(c, "stage_trace", pin[i], T.WIDTH[T.TABLE_ENUM_ORDER[i]], lg[i]) for i in range(12)]
    got = _consume(c, staged, control, lambda: c.prove_segment(staged, lg, public_values=pub))
    _check(got, want, "lanes %d aux %d, segment %d" % (c.case + (v,)))


@pytest.mark.parametrize("consumer", LANES, ids=LANE_IDS, indirect=True)
def test_c_staged_tables_of_one_segment_proven_at_once(consumer, ctx, decoy):
    _tables_case(consumer, ctx, decoy, _variants("c", *consumer.case, 1)[0], control=False)


def _lockstep_columns_case(c, ctx, decoy, variants, control):
    """Segments of equal heights in column-pointer form (one lock-step group per table, gathered on the copy streams): the first, the
    last and the densest column of every table a StagedTrace of its own (many boundary columns are nearly all zero, which stale memory
    may match), the others pinned host columns."""
    want = [_expected(ctx, v) for v in variants]
    pins = [[_columns(_pinned(c, t), i) for i, t in enumerate(w[0])] for w in want]
    _stage(c, "stage_trace", decoy, DECOY_COLS, DECOY_LOG_N)
    staged, segs = [], []
    for cols, w in zip(pins, want):
        tabs = []
        for i, tc in enumerate(cols):
            tc = list(tc)
            for k in sorted({0, len(tc) - 1, int(np.argmax([np.count_nonzero(x) for x in tc]))}):
                tc[k] = _stage(c, "stage_trace", tc[k], 1, w[1][i])
                staged.append(tc[k])
            tabs.append(tc)
        segs.append((tabs, w[1], w[2]))
    got = _consume(c, staged, control, lambda: c.prove_segments(segs))
    for v, g, w in zip(variants, got, want):
        _check(g, w[3], "lanes %d aux %d, segment %d" % (c.case + (v,)))


@pytest.mark.parametrize("consumer", LANES, ids=LANE_IDS, indirect=True)
def test_d_lockstep_column_pointers_with_staged_columns_proven_at_once(consumer, ctx, decoy):
    _lockstep_columns_case(consumer, ctx, decoy, _variants("d", *consumer.case, 2), control=False)


@pytest.mark.parametrize("consumer", LANES, ids=LANE_IDS, indirect=True)
def test_e_control_the_same_calls_after_the_uploads_have_landed(consumer, ctx, decoy, zkm):
    """(a) -- (d) with ready(wait=True) before each prove call: a failure above is one of ordering, not of staging.  Every part has a
    fresh context of its own (and variants of its own) like the cases it controls."""
    lanes, aux = consumer.case
    a, b, cc, d = [_variants("e", lanes, aux, 4)[0] + 100 * k for k in range(4)]   # (clear of every other case's variants)
    _segments_case(consumer, ctx, decoy, [a, a + 1, a + 2], ["block"] * 3, control=True)
    for part in range(3):
        with _fresh(zkm, lanes, aux) as c:
            if part == 0:
                _segments_case(c, ctx, decoy, [b, b + 1, b + 2], ["block", "columns", "loose"], control=True)
            elif part == 1:
                _tables_case(c, ctx, decoy, cc, control=True)
            else:
                _lockstep_columns_case(c, ctx, decoy, [d, d + 1], control=True)


# ------------------------------------------------------------------ staged handles neither leak nor dangle
def _transient(c):
    return c.memory()[0] - c.resident_bytes()


def test_dropped_or_scoped_staged_trace_returns_its_block(zkm):
    """A StagedTrace dropped without free() gives its block (and its events) back when it is collected; `with` frees it on exit."""
    c = zkm.Context(0)
    try:
        m = np.arange(8 << 12, dtype=np.uint64)
        st = c.stage_trace(m, 8, 12)
        assert _transient(c) > 0
        del st
        gc.collect()
        c.synchronize()
        assert _transient(c) == 0, "a dropped StagedTrace kept its block"
        with c.stage_trace(m, 8, 12) as st:
            assert st.ready(wait=True) is True
        assert st.h is None
        st.free()                            # (a second free is a no-op)
        c.synchronize()
        assert _transient(c) == 0
    finally:
        c.close()


CHILD = r"""
import gc, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import zkm_amd
c = zkm_amd.Context(0)
m = c.pinned_array(8 << 12)
m[:] = np.arange(m.size, dtype=np.uint64)
st = c.stage_trace(m, 8, 12, canonical=False)
seg = c.stage_trace([m[:1 << 12]], 1, 12)
c.close()                                    # frees both handles first (the upload from m has landed before m goes)
assert st.h is None and seg.h is None, "close() left a staged handle outstanding"
st.free()                                    # no-ops: the context that owned them is gone
seg.free()
del st, seg
gc.collect()
c2 = zkm_amd.Context(0)
with c2.stage_trace(np.arange(8 << 12, dtype=np.uint64), 8, 12) as st:
    pass
c2.close()
print("CHILD OK")
"""


def test_staged_trace_freed_after_its_context_closed():
    """close() with staged handles outstanding frees them; free() afterwards is a no-op, not a use-after-free (in a child process: a
    regression is a failed exit status, not a crashed test run)."""
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, "child exited %d\n%s" % (r.returncode, r.stderr[-2000:])
