"""GPU suite: zkm_image_hash / zkm_images_hash against the model of the emulator's split-time hashing (tests/image_model.py), word for
word and under every value of "image_hash_form" (0 by chain count, 1 the 16-lane row form, 2 the quad form).  Cases (image_model.CASE_*):
A one dirty page, every ancestor fresh, the last slot of every level; B six pages over four L1 and three L2 pages, one page all ones and
one all zero; C a second split on B's hash pages, from host memory and from device memory; D no dirty page; E seventeen pages under one L1
page (a ragged last wave in both forms) and three images in one call; F the bootstrap's checker accepts the assembled image; G refusals."""
import ctypes as C

import numpy as np
import pytest

from . import image_model as IM

pytestmark = pytest.mark.gpu

FORMS = [0, 1, 2]


def arrays(case):
    """(indices, n x 1024 words) of a case's dirty pages."""
    idx = sorted(case["dirty"])
    return np.array(idx, dtype=np.uint32), np.array([case["dirty"][p] for p in idx], dtype=np.uint32).reshape(-1, 1024)


def under_form(ctx, form, fn):
    ctx.set_tuning("image_hash_form", form)
    try:
        return fn()
    finally:
        ctx.set_tuning("image_hash_form", 0)


def assert_equals_model(got, want, what=""):
    plan, pages, root, image_id = got
    w_plan, w_pages, w_root, w_id = want
    assert plan.tolist() == w_plan, what
    w_pages = np.array(w_pages, dtype=np.uint32)
    assert pages.shape == w_pages.shape, what
    bad = np.argwhere(pages != w_pages)
    assert bad.size == 0, "%s: first differing word: page 0x%x word %d" % (what, w_plan[bad[0][0]], bad[0][1])
    assert root == w_root, what + ": root"
    assert image_id == w_id, what + ": image id"


def known_of(prev_plan, prev_pages, new_dirty):
    """The pages of a previous result that are in the plan of new_dirty: (indices, words, their positions in the previous plan)."""
    new_plan = set(IM.plan(new_dirty))
    pos = [i for i, q in enumerate(prev_plan) if q in new_plan]
    return np.array([prev_plan[i] for i in pos], dtype=np.uint32), np.ascontiguousarray(np.asarray(prev_pages)[pos]), pos


@pytest.mark.parametrize("form", FORMS)
def test_a_one_page_with_fresh_ancestors(ctx, form):
    case = IM.CASE_A
    before = ctx.host_waits()
    got = under_form(ctx, form, lambda: ctx.image_hash(arrays(case), None, case["pc"], case["registers"]))
    assert ctx.host_waits() - before == 1
    assert_equals_model(got, IM.solved("a"), "A")


@pytest.mark.parametrize("form", FORMS)
def test_b_six_pages_over_every_level(ctx, oracle, form):
    case = IM.CASE_B
    got = under_form(ctx, form, lambda: ctx.image_hash(arrays(case), None, case["pc"], case["registers"]))
    assert len(got[0]) == 8
    assert_equals_model(got, IM.solved("b", oracle), "B")


def runtime(zkm):
    """The HIP runtime the library itself is bound to, for a device-to-device gather the C ABI has no call for: a symbol looked up
    through the library's own handle is found in the runtime it was linked against, whichever other copy (a Python package may bring
    its own) the process has loaded beside it."""
    return zkm.load()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("form", FORMS)
def test_c_a_second_split_on_the_first_ones_pages(ctx, zkm, oracle, form, where):
    first, second = IM.solved("c", oracle)
    b, c2 = IM.CASE_B, IM.CASE_C2

    def run():
        if where == "host":
            plan1, pages1, _, _ = ctx.image_hash(arrays(b), None, b["pc"], b["registers"])
            k_idx, k_words, _ = known_of(plan1.tolist(), pages1, c2["dirty"])
            return ctx.image_hash(arrays(c2), (k_idx, k_words), c2["pc"], c2["registers"])
        out1, gathered = ctx.alloc(8 * 512), ctx.alloc(4 * 512)
        try:
            plan1, dev1, _, _ = ctx.image_hash(arrays(b), None, b["pc"], b["registers"], out=out1)
            assert dev1 is out1
            assert (out1.download().view(np.uint32).reshape(8, 1024) == np.array(first[1], dtype=np.uint32)).all()
            k_idx, _, pos = known_of(plan1.tolist(), np.zeros((8, 1024), np.uint32), c2["dirty"])
            assert pos == [0, 1, 4, 7]
            hip = runtime(zkm)
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            for k, p in enumerate(pos):           # the known pages, contiguous, straight from the first call's device output
                assert hip.hipMemcpy(gathered.ptr + 4096 * k, out1.ptr + 4096 * p, 4096, 3) == 0
            assert hip.hipDeviceSynchronize() == 0
            return ctx.image_hash(arrays(c2), (k_idx, gathered), c2["pc"], c2["registers"])
        finally:
            out1.free()
            gathered.free()
    assert_equals_model(under_form(ctx, form, run), second, "C (%s)" % where)


@pytest.mark.parametrize("form", FORMS)
def test_d_no_dirty_page_changes_only_the_root_and_the_id(ctx, oracle, form):
    first, second = IM.solved("d", oracle)
    case = IM.CASE_D2
    known = (np.array([IM.ROOT_INDEX], dtype=np.uint32), np.array(first[1][-1], dtype=np.uint32))
    got = under_form(ctx, form, lambda: ctx.image_hash(None, known, case["pc"], case["registers"]))
    assert_equals_model(got, second, "D")
    root_before = np.array(first[1][-1], dtype=np.uint32)
    changed = np.nonzero(got[1][0] != root_before)[0]
    assert changed.size and changed.min() >= 256 and changed.max() < 256 + 39
    assert got[2] != first[2] and got[3] != first[3]


@pytest.mark.parametrize("form", FORMS)
def test_e_a_ragged_last_wave_and_three_images_in_one_call(ctx, oracle, form):
    cases = IM.CASE_E
    want = [IM.solved("e%d" % i, oracle) for i in range(3)]
    assert [len(c["dirty"]) for c in cases] == [1, 17, 6] and len(want[1][0]) == 3

    def run():
        alone = [ctx.image_hash(arrays(c), None, c["pc"], c["registers"]) for c in cases]
        return alone, ctx.images_hash([(arrays(c), None, c["pc"], c["registers"]) for c in cases])
    alone, together = under_form(ctx, form, run)
    for i in range(3):
        assert_equals_model(alone[i], want[i], "E alone %d" % i)
        assert_equals_model(together[i], want[i], "E together %d" % i)
        assert (alone[i][1] == together[i][1]).all() and alone[i][2:] == together[i][2:]


@pytest.mark.parametrize("form", FORMS)
def test_f_the_bootstrap_accepts_the_assembled_image(ctx, zkm, oracle, form):
    case = IM.CASE_B
    dirty = arrays(case)
    plan, pages, root, image_id = under_form(ctx, form, lambda: ctx.image_hash(dirty, None, case["pc"], case["registers"]))
    im = zkm.boot_image_from_pages(dirty, plan, pages, root, image_id, case["pc"], check=True)
    assert im.npages == 14 and im.nwords == 14 * 1024
    digests = ctx.boot_witness(im)[4]
    assert digests.shape == (15, 4) and digests[13].tobytes() == root and digests[14].tobytes() == image_id
    bad = pages.copy()
    bad[0, 8] ^= 1                               # a hash word of dirty page 1, changed on the host
    live = ctx.memory()[0]
    with pytest.raises(zkm.ZkmError, match="page hash mismatch"):
        ctx.boot_witness(zkm.boot_image_from_pages(dirty, plan, bad, root, image_id, case["pc"], check=True))
    assert ctx.memory()[0] == live
    assert (ctx.boot_witness(im)[4] == digests).all()


def test_g_refusals_name_the_index_and_leave_the_context_usable(ctx, zkm, oracle):
    case = IM.CASE_B
    idx, words = arrays(case)
    live = ctx.memory()[0]
    L = zkm.load()

    def refused(dirty, known, *parts, images=None):
        with pytest.raises(zkm.ZkmError) as e:
            if images is None:
                ctx.image_hash(dirty, known, case["pc"], case["registers"])
            else:
                ctx.images_hash(images)
        for p in parts:
            assert p in str(e.value), str(e.value)
        assert ctx.memory()[0] == live

    swapped = idx.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    refused((swapped, words), None, "zkm_image_hash", "dirty index 3 = 0x7f", "not above")
    twice = idx.copy()
    twice[1] = twice[0]
    refused((twice, words), None, "dirty index 1 = 0x0", "not above")
    high = idx.copy()
    high[5] = 0x80000
    refused((high, words), None, "dirty index 5 = 0x80000", "not below 0x80000")
    page = np.zeros((1, 1024), dtype=np.uint32)
    refused((idx, words), (np.array([0x80002], dtype=np.uint32), page), "known index 0 = 0x80002", "not a hash page of the plan")
    two = np.zeros((2, 1024), dtype=np.uint32)
    refused((idx, words), (np.array([0x81000, 0x80000], dtype=np.uint32), two), "known index 1 = 0x80000", "not above")
    refused(None, None, "compute image ID fail", "0x81020")
    # a null pointer with a nonzero count, straight through the C ABI
    st = zkm.ImagePagesStruct()
    st.dirty_index, st.ndirty, st.dirty_words = idx.ctypes.data, idx.size, None
    out, root, image_id, err = np.zeros((8, 1024), np.uint32), (C.c_uint8 * 32)(), (C.c_uint8 * 32)(), C.c_char_p()
    assert L.zkm_image_hash(ctx.h, C.byref(st), out.ctypes.data, root, image_id, C.byref(err)) != 0 and b"null pointer with a nonzero count" in err.value
    st.dirty_words = words.ctypes.data
    assert L.zkm_image_hash(ctx.h, C.byref(st), None, root, image_id, C.byref(err)) != 0 and b"null argument" in err.value
    assert ctx.memory()[0] == live
    # of several images, the refusal names the image's position
    good = ((idx, words), None, case["pc"], case["registers"])
    refused(None, None, "zkm_images_hash", "image 1", "dirty index 5 = 0x80000", images=[good, ((high, words), None, 0, bytes(156))])
    # the context still hashes case B
    got = ctx.image_hash((idx, words), None, case["pc"], case["registers"])
    assert got[2] == IM.solved("b", oracle)[2] and ctx.memory()[0] == live
