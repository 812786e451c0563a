"""CPU suite: the premise of the verifier's constraint kernel (stark.hip k_verify_line).  The device evaluates every table's constraints
over the base field only; the verifier needs them at openings v = v0 + v1 X in F[X] / (X^2 - 7).  It evaluates them on the base-field
rows v0 + t v1 for t = 0..4 and interpolates, which is exact as long as every constraint is a polynomial of degree <= 3 in the row
values (constraint_degree 3, quotient_degree_factor 2).  Checked here with the oracle's base-field row evaluator on random rows, the
first / last row flags on and off: the fourth finite difference over t = 0..4 of every constraint of every table is zero.  This is
what breaks first if a table ever gains a constraint of higher degree (the library then answers FAILED "constraint degree above 3")."""
import numpy as np

P = 0xFFFFFFFF00000001
NAMES = ["Poseidon", "Logic", "KeccakSponge", "Keccak", "Memory", "PoseidonSponge", "ShaExtend", "ShaExtendSponge", "ShaCompress",
         "ShaCompressSponge", "Arithmetic", "Cpu"]           # ZKM_TABLE_* order


def differences(values):
    """k-th forward differences at 0, k = 0..4, of five vectors of field elements (lists of Python ints)."""
    d = [list(v) for v in values]
    for k in range(1, 5):
        for i in range(4, k - 1, -1):
            d[i] = [(a - b) % P for a, b in zip(d[i], d[i - 1])]
    return d


def test_every_constraint_has_degree_at_most_three_on_a_line(zkm, oracle):
    lib = zkm.load()
    rng = np.random.default_rng(2024)
    reach3 = []
    for tid, name in enumerate(NAMES):
        w = int(lib.zkm_table_width(tid))
        assert w
        third = False
        for first, last in ((False, False), (True, False), (False, True)):
            v0, v1, n0, n1 = ([int(x) % P for x in rng.integers(0, 1 << 63, w, dtype=np.uint64) * 2 + rng.integers(0, 2, w, dtype=np.uint64)]
                              for _ in range(4))
            vals = []
            for t in range(5):
                lv = np.array([(a + t * b) % P for a, b in zip(v0, v1)], dtype=np.uint64)
                nv = np.array([(a + t * b) % P for a, b in zip(n0, n1)], dtype=np.uint64)
                vals.append([int(x) for x in oracle.row_constraints(tid, lv, nv, first, last)])
            assert len(vals[0]) > 0 and len({len(v) for v in vals}) == 1, name
            d = differences(vals)
            assert not any(d[4]), (name, first, last, [i for i, x in enumerate(d[4]) if x][:5])
            third = third or any(d[3])
        if third:
            reach3.append(name)
    print("tables whose constraints reach degree 3:", reach3)
    assert len(reach3) == 10         # (fixed seed) the bound is tight: degree 3 is reached, so the fifth point is a real check
