"""CPU suite: tests/boot_model.py -- the bootstrap kernel in Python integers that the device code is compared with -- pinned to the
constraint system, independently of the device: a segment that opens with the model's rows (boot_fixtures.build_boot_segment) satisfies
every CPU and PoseidonSponge constraint and all fifteen cross-table lookups (CPU <-> Memory, CPU <-> PoseidonSponge,
PoseidonSponge <-> Memory, PoseidonSponge <-> Poseidon among them); the bootstrap address checks of channels 3..7, dead in
test_cpu_table.py (its fixture boots through channels 0..2), are live here; and zkm_boot_counts agrees with the model."""
import numpy as np
import pytest

from zkm_amd import tables as T

from . import boot_fixtures as BF
from . import boot_model as BM
from . import cpu_fixtures as CF

P = CF.P
CPU, PS, ME = 1, 3, 11          # Table::all() positions


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_constraints_and_lookups_hold_on_the_models_segment(oracle, name):
    seg = BF.segment(oracle, name)
    m = seg["model"]
    image = seg["image"][0]
    pages = sum(1 for a in image if a & 0xFFF == 0)
    assert m.counts() == (-(-len(image) // 8) + pages + 3, len(image) + 4096 * pages + 45, 129 * pages + 2, pages + 1, 129 * pages + 2)
    for pos, count in ((CPU, 741), (PS, None)):
        tid, trace, w, lg, _ = seg["tables"][pos]
        n, bad = oracle.debug_constraints(tid, trace, w, lg)
        assert bad is None and (count is None or n == count), (pos, bad)
    assert oracle.check_ctls(seg["tables"], seg["ctls"]) == 0


def test_shapes_of_the_three_images(oracle):
    a, b, c = (BF.segment(oracle, k) for k in "abc")
    assert len(a["image"][0]) == 1037 and a["nboot"] == 135 and len(a["model"].digests) == 3
    assert 0x80FFF000 not in a["image"][0] and all(0x80FFFFE0 + 4 * i in a["image"][0] for i in range(8))
    assert int(a["model"].cpu_rows[129, CF.ch(4, 0)]) == 1 and int(a["model"].cpu_rows[129, CF.ch(5, 0)]) == 0      # the ragged last row
    assert len(b["image"][0]) == 3 and len(b["model"].digests) == 1 and b["nboot"] == 4
    assert len(c["model"].digests) == 7 and sum(1 for x in c["image"][0] if 0x7FFFD000 <= x < 0x7FFFE000) == 2       # the sparse page
    # the stride of the sponge's addresses: what zkm_segment_ops' contiguous form cannot say
    assert [int(v) for v in a["model"].sponge_rows[0, 3:11]] == [0x7FFFF000 + 4 * i for i in range(8)]


def test_bootstrap_address_checks_of_channels_3_to_7_are_live(oracle):
    """Single-cell corruptions (+1 and +2^32) of the channel cells 3..8 of a boot row that uses all eight channels: constraints 9..18
    (context and segment of channels 3..7) become nonzero.  Constraints 19 and 20 belong to the ninth channel, which the bootstrap never
    uses (it writes eight words a row): `is_bootstrap * used * address` needs two changed cells there, which the last lines show."""
    seg = BF.segment(oracle, "a")
    _, trace, _, lg, _ = seg["tables"][CPU]
    n = 1 << lg
    rows = trace.reshape(259, n).T.copy()
    assert all(rows[0, CF.ch(k, 0)] == 1 for k in range(8)) and rows[0, CF.ch(8, 0)] == 0
    live = np.zeros(741, dtype=bool)
    for c in range(CF.ch(3, 0), CF.ch(8, 5) + 1):
        old = rows[0, c]
        for delta in (1, 1 << 32):
            rows[0, c] = (int(old) + delta) % P
            live |= oracle.row_constraints(T.TABLE_CPU, rows[0], rows[1], True, False) != 0
        rows[0, c] = old
    assert set(range(9, 19)) <= set(np.nonzero(live)[0].tolist()) and not live[19] and not live[20]
    rows[0, CF.ch(8, 0)] = 1
    for f, k in ((2, 19), (3, 20)):
        rows[0, CF.ch(8, f)] = 1
        assert oracle.row_constraints(T.TABLE_CPU, rows[0], rows[1], True, False)[k] != 0
        rows[0, CF.ch(8, f)] = 0


def test_a_flipped_hash_word_is_caught(oracle):
    d, root, image_id, entry = BM.image_a()
    d = dict(d)
    d[0x80FFFFE4] ^= 0x100
    with pytest.raises(BM.BootError, match="page hash mismatch at 0x7ffff000"):
        BM.Boot(d, root, image_id, entry)
    # unchecked, the rows go through as they are -- and the lookups still hold: the hash is checked by the bootstrap, not by a table
    seg = BF.build_boot_segment(oracle, (d, root, image_id, entry), check=False)
    assert oracle.check_ctls(seg["tables"], seg["ctls"]) == 0
    # a changed digest in the sponge's CPU row, on the other hand, breaks CPU <-> PoseidonSponge
    tid, trace, w, lg, c = seg["tables"][CPU]
    bad = trace.copy()
    bad[CF.GEN * (1 << lg) + 130] ^= 1
    assert oracle.check_ctls(seg["tables"][:CPU] + [(tid, bad, w, lg, c)] + seg["tables"][CPU + 1:], seg["ctls"]) != 0
    with pytest.raises(BM.BootError, match="missing hash word"):
        BM.Boot({a: v for a, v in d.items() if a != 0x80FFFFE8}, root, image_id, entry)


def test_boot_counts_against_the_model(zkm, oracle):
    for name in "abc":
        seg = BF.segment(oracle, name)
        assert BF.boot_image(zkm, seg["image"]).counts() == seg["model"].counts()
    L = zkm.load()
    L.zkm_boot_counts(None, None, None, None, None, None)      # pure: null pointers are passed over
