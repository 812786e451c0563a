"""GPU suite: the bootstrap kernel built on the device from a segment's image (zkm_boot_witness and the zkm_*_boot calls) against the
model in Python integers (tests/boot_model.py), word for word: the kernels alone on images A, B and C; whole segments (the boot's rows in
front of the sample program's) at the heights of into_tables on the joined lists; K segments in one call with three host waits; the
proofs; every refusal.  Images (boot_model.image_a / _b / _c): A one data page, a ragged last row, the root page; B three words and no
page; C six pages (more than four chains: a second wave of the chain kernel), one of them sparse."""

import numpy as np
import pytest

from zkm_amd import tables as T

from . import boot_fixtures as BF
from . import boot_model as BM
from . import segment_ops_fixtures as SF
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

ORDER = ["b", "a", "c"]
PUBS = [[1, 2, 3], [7, 1], [9]]


@pytest.fixture(scope="module")
def segs(oracle):
    return {k: BF.segment(oracle, k) for k in ORDER}


def device_tables(staged, log_ns, ctx):
    """The twelve matrices of a built segment as DeviceBuffers (not owned)."""
    from zkm_amd import DeviceBuffer
    out = []
    for ptr, t, lg in zip(staged.tables(), SF.ORDER, log_ns):
        buf = DeviceBuffer.__new__(DeviceBuffer)
        buf.ctx, buf.words, buf.ptr = ctx, T.WIDTH[t] << lg, ptr
        out.append(buf)
    return out


def image_and_ops(zkm, seg, **kw):
    return BF.boot_image(zkm, seg["image"], **kw), SF.segment_ops(zkm, seg["exec"])


@pytest.mark.parametrize("name", ORDER)
@pytest.mark.parametrize("quad", [0, 1])
def test_boot_witness_equals_the_model(ctx, zkm, segs, name, quad):
    seg, m = segs[name], segs[name]["model"]
    im = BF.boot_image(zkm, seg["image"])
    assert im.counts() == m.counts()
    ctx.set_tuning("boot_chain_quad", quad)
    try:
        rows, mem, po, ts, dig = ctx.boot_witness(im)
    finally:
        ctx.set_tuning("boot_chain_quad", 0)
    for got, want, what in ((dig, m.digests, "digests"), (po, m.poseidon_inputs, "poseidon inputs"), (ts, m.poseidon_ts, "timestamps"),
                            (mem, m.memory_ops, "memory ops"), (rows, m.cpu_rows, "cpu rows")):
        assert got.shape == want.shape, what
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: first differing word at %s" % (what, bad[0])


def test_boot_witness_takes_a_device_image(ctx, zkm, segs):
    seg = segs["a"]
    addrs, values = BM.arrays(seg["image"][0])
    da, dv = ctx.alloc((addrs.size + 1) // 2).upload(np.resize(addrs, (addrs.size + 1) // 2 * 2).view(np.uint64)), \
        ctx.alloc((values.size + 1) // 2).upload(np.resize(values, (values.size + 1) // 2 * 2).view(np.uint64))
    im = zkm.BootImage(da, dv, *seg["image"][1:], npages=2, nwords=addrs.size)
    rows = ctx.boot_witness(im)[0]
    assert (rows == seg["model"].cpu_rows).all()
    da.free()
    dv.free()


@pytest.mark.parametrize("name", ORDER)
def test_segment_tables_boot_word_for_word(ctx, zkm, segs, name):
    seg = segs[name]
    im, ops = image_and_ops(zkm, seg)
    assert ctx.segment_tables_boot(im, ops, sizing=True) == seg["log_ns"]
    live = ctx.memory()[0]
    staged, lg = ctx.segment_tables_boot(im, ops)
    with staged:
        assert lg == seg["log_ns"]
        assert_tables_equal(tables_of(staged, lg, ctx), [t[1] for t in seg["tables"]])
        assert ctx.segment_check_ctls(staged, lg).kind == 0
    assert ctx.memory()[0] == live
    # the same from device-resident lists: the joined lists are assembled on the device
    dev = ops.to_device(ctx)
    staged, lg = ctx.segment_tables_boot(im, dev)
    with staged:
        assert_tables_equal(tables_of(staged, lg, ctx), [t[1] for t in seg["tables"]])
    dev.free()


def test_three_segments_in_one_call_with_three_host_waits(ctx, zkm, segs):
    pairs = [image_and_ops(zkm, segs[k]) for k in ORDER]
    images, ops = [p[0] for p in pairs], [p[1].to_device(ctx) for p in pairs]
    for st, _ in ctx.segments_tables_boot(images, ops):      # (the first call grows the pinned download area: a wait of its own)
        st.free()
    before = ctx.host_waits()
    built = ctx.segments_tables_boot(images, ops)
    assert ctx.host_waits() - before == 3
    for (st, lg), k in zip(built, ORDER):
        assert lg == segs[k]["log_ns"]
        assert_tables_equal(tables_of(st, lg, ctx), [t[1] for t in segs[k]["tables"]])
        st.free()
    for o in ops:
        o.free()


def test_proofs(ctx, zkm, oracle, segs):
    pairs = [image_and_ops(zkm, segs[k]) for k in ORDER]
    ctx.set_tuning("verify", 1)
    try:
        alone = [ctx.prove_segment_ops_boot(im, ops, public_values=pub) for (im, ops), pub in zip(pairs, PUBS)]
    finally:
        ctx.set_tuning("verify", 0)
    # the blobs are those of zkm_prove_segment on the built block
    im, ops = pairs[1]
    staged, lg = ctx.segment_tables_boot(im, ops)
    with staged:
        p, c, o = ctx.prove_segment(device_tables(staged, lg, ctx), lg, public_values=PUBS[1])
    assert o == alone[1][2] and (c == alone[1][1]).all() and (p == alone[1][0]).all()
    seg = segs["a"]
    assert oracle.verify_all(seg["tables"], seg["ctls"], p, c, public_values=PUBS[1]) == 0
    got = ctx.prove_segments_ops_boot([p[0] for p in pairs], [p[1] for p in pairs], public_values=PUBS)
    for s, ((p, c, o), (pa, ca, oa)) in enumerate(zip(got, alone)):
        assert o == oa and (c == ca).all(), s
        bad = np.nonzero(p != pa)[0]
        assert bad.size == 0, "segment %d: first differing proof word %d" % (s, bad[0])


def test_refusals_name_the_address_and_leave_the_context_usable(ctx, zkm, segs):
    seg = segs["a"]
    d, root, image_id, entry = seg["image"]
    ops = SF.segment_ops(zkm, seg["exec"])
    good = BF.boot_image(zkm, seg["image"])
    live = ctx.memory()[0]

    def refused(im, *words, o=ops):
        with pytest.raises(zkm.ZkmError) as e:
            ctx.segment_tables_boot(im, o)
        msg = str(e.value)
        assert "zkm_segment_tables_boot" in msg and "Cpu" in msg, msg
        for w in words:
            assert w in msg, msg
        assert ctx.memory()[0] == live

    addrs, values = BM.arrays(d)
    swapped = addrs.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    refused(zkm.BootImage(swapped, values, root, image_id, entry), "0x%08x" % swapped[11], "multiple of 4")
    odd = addrs.copy()
    odd[20] += 2
    refused(zkm.BootImage(odd, values, root, image_id, entry), "0x%08x" % odd[20], "multiple of 4")
    short = SF.segment_ops(zkm, dict(seg["exec"], cpu_rows=seg["exec"]["cpu_rows"][:-1]))
    refused(zkm.BootImage(addrs, values, root, image_id, entry, npages=3), "npages = 3", "holds 2 page-aligned", o=short)   # (one boot row more)
    missing = {a: v for a, v in d.items() if a != 0x80FFFFE8}
    refused(zkm.BootImage.from_dict(missing, root, image_id, entry), "0x80ffffe8", "missing")
    flipped = dict(d)
    flipped[0x7FFFF010] ^= 1
    refused(zkm.BootImage.from_dict(flipped, root, image_id, entry), "page hash mismatch", "0x7ffff000")
    refused(zkm.BootImage(addrs, values, bytes(32), image_id, entry), "root hash mismatch", "0x81020000")
    refused(zkm.BootImage(addrs, values, root, bytes(32), entry), "image id mismatch", "0x81021000")
    refused(good, "rows", "not a power of two", o=short)
    # without `check` the mismatches pass (the rows carry the digests as they are); a missing hash word is still refused
    st, _ = ctx.segment_tables_boot(zkm.BootImage(addrs, values, root, bytes(32), entry, check=False), ops)
    st.free()
    refused(zkm.BootImage.from_dict(missing, root, image_id, entry, check=False), "0x80ffffe8")
    # the context still builds image A
    staged, lg = ctx.segment_tables_boot(good, ops)
    with staged:
        assert_tables_equal(tables_of(staged, lg, ctx), [t[1] for t in seg["tables"]])
    assert ctx.memory()[0] == live
