"""CPU suite: the model of the emulator's split-time hashing (tests/image_model.py) and zkm_image_hash_plan.  The oracle's batched C
permutation gives what Python integers give on case A; the plan through ctypes is the model's; the model's whole image -- dirty, L1, L2
and root pages with the root and the id -- is accepted by boot_model.Boot(check=True), an independent restatement of the prover's
bootstrap_kernel.rs, and refused after one flipped word in an L2 page; a dirty all-zero page's L1 slot is a fresh L1 page's fill."""
import numpy as np
import pytest

from . import boot_model as BM
from . import image_model as IM


def test_the_oracle_path_equals_python_integers_on_case_a(oracle):
    a, a_c = IM.solved("a"), IM.solved("a_c", oracle)
    assert a == a_c
    assert IM.const_digests() == IM._CACHE["consts"]
    pl, pages, root, image_id = a
    assert pl == [0x80FFF, 0x8101F, 0x81020] and len(root) == 32 and len(image_id) == 32
    # all three ancestors are fresh, and the last slot at every level is used
    c = IM._CACHE["consts"]
    assert pages[0][:1016] == c[0] * 127 and pages[0][1016:] != c[0]
    assert pages[1][:1016] == c[1] * 127 and pages[1][1016:] != c[1]
    regs = IM.CASE_A["registers"]
    want_root = c[2] * 128
    want_root[256:256 + 39] = [int.from_bytes(regs[4 * i:4 * i + 4], "little") for i in range(39)]
    assert pages[2][:248] == want_root[:248] and pages[2][256:] == want_root[256:] and pages[2][248:256] != c[2]


def test_plan_through_ctypes_equals_the_model(zkm):
    for dirty in ([], [0], [0x7FFFF], sorted(IM.CASE_B["dirty"]), sorted(IM.CASE_C2["dirty"]), sorted(IM.CASE_E[1]["dirty"]), list(range(0, 0x80000, 4097))):
        assert zkm.image_hash_plan(dirty).tolist() == IM.plan(dirty), dirty
    assert zkm.image_hash_plan([]).tolist() == [0x81020]
    b = sorted(IM.CASE_B["dirty"])
    assert len(IM.plan(b)) == 8 and [q >> 12 for q in IM.plan(b)] == [0x80] * 4 + [0x81] * 4
    # a capacity shorter than the count: the count comes back, only `capacity` entries are written
    L = zkm.load()
    idx = np.array(b, dtype=np.uint32)
    out = np.full(8, 0xDEADBEEF, dtype=np.uint32)
    assert L.zkm_image_hash_plan(idx.ctypes.data, idx.size, out.ctypes.data, 3) == 8
    assert out.tolist() == IM.plan(b)[:3] + [0xDEADBEEF] * 5
    assert L.zkm_image_hash_plan(idx.ctypes.data, idx.size, None, 0) == 8
    assert L.zkm_image_hash_plan(None, 0, out.ctypes.data, 8) == 1 and out[0] == 0x81020


def test_the_bootstrap_checker_accepts_the_model_image_and_refuses_a_flipped_l2_word():
    pl, pages, root, image_id = IM.solved("a")
    image = IM.boot_image(IM.CASE_A["dirty"], pl, pages)
    assert len(image) == 4 * 1024
    boot = BM.Boot(image, root, image_id, IM.CASE_A["pc"], check=True)
    assert len(boot.digests) == 5 and BM.digest_bytes(boot.digests[3]) == root and BM.digest_bytes(boot.digests[4]) == image_id
    flipped = dict(image)
    flipped[(0x8101F << 12) + 4 * 5] ^= 1 << 9             # a word of the L2 page that is no slot of a dirty page's ancestor
    with pytest.raises(BM.BootError, match="page hash mismatch at 0x8101f000"):
        BM.Boot(flipped, root, image_id, IM.CASE_A["pc"], check=True)


def test_a_zero_page_hashes_to_the_fill_of_a_fresh_l1_page(oracle):
    pl, pages, _, _ = IM.solved("b", oracle)
    c = IM._CACHE["consts"]
    l1 = pages[pl.index(0x80001)]                      # page 0x80 is all zero: slot 0 of L1 page 0x80001
    assert IM.CASE_B["dirty"][0x80] == [0] * 1024 and l1[:8] == c[0] and l1 == c[0] * 128
    assert pages[pl.index(0x80000)][8:16] != c[0]      # page 1 is all ones


def test_two_splits_keep_the_pages_of_the_first(oracle):
    first, second = IM.solved("c", oracle)
    assert first == IM.solved("b", oracle)
    pl1, pages1 = first[0], first[1]
    pl2, pages2 = second[0], second[1]
    assert pl2 == [0x80000, 0x80001, 0x80246, 0x81000, 0x81004, 0x81020]
    # slot 0 of L1 page 0x80000 (page 0, not dirty in the second split) is the first split's
    assert pages2[0][:8] == pages1[0][:8] and pages2[0][8:16] != pages1[0][8:16]
    # no dirty page: only the root page's registers, the root and the id change
    _, (pl3, pages3, root3, id3) = IM.solved("d", oracle)
    assert pl3 == [0x81020] and pages3[0][:256] == pages1[-1][:256] and pages3[0][256 + 39:] == pages1[-1][256 + 39:]
    assert root3 != first[2] and id3 != first[3]
