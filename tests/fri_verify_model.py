"""plonky2's verify_fri_proof (fri/verifier.rs) for an arbitrary FriInstanceInfo, in Python integers, from the published algorithm: the
independent judge of zkm_fri_verify (tests/test_gpu_fri_verify.py) and, through it, of zkm_fri_prove's general path.

Written out here, sharing nothing with the library: the duplex challenger (iop/challenger.rs), fri_verify_proof_of_work,
fri_combine_initial with ReducingFactor's reduce / shift, compute_evaluation by plain Lagrange interpolation over the coset (no
barycentric weights, not the kernel's one-pass formula), Merkle verification with hash_or_noop / two_to_one (hash/merkle_proofs.rs
verify_merkle_proof_to_cap) and the final polynomial.  The permutation is tests/poseidon_model.py's; the field's two generators are the
public constants of plonky2's GoldilocksField.  The only thing read of the library's is the layout of the blob (include/zkm_hip.h "FRI
proof blob"), restated in parse().  tests/test_fri_verify_model.py pins this model to the CPU oracle where the oracle reaches.

verify() returns (code, query, tree, layer) with the codes of ZKM_VERIFY_* and the finding plonky2 meets first: the proof of work; then
the lowest query, inside it the oracles' Merkle proofs in ascending order, per layer the evaluation check before the Merkle proof, then
the final polynomial."""
import functools

from . import poseidon_model as pm

P = pm.P
OK, POW, INITIAL_MERKLE, FRI_EVAL, FRI_MERKLE, FINAL_POLY = 0, 5, 6, 7, 8, 9      # ZKM_VERIFY_* (include/zkm_hip.h)
MULTIPLICATIVE_GROUP_GENERATOR = 14293326489335486720      # GoldilocksField: the coset shift
POWER_OF_TWO_GENERATOR = 7277203076849721926               # of order 2^32
assert pow(POWER_OF_TWO_GENERATOR, 1 << 32, P) == 1 and pow(POWER_OF_TWO_GENERATOR, 1 << 31, P) == P - 1
W = 7                                                       # the quadratic extension is F[X] / (X^2 - 7)
MAGIC = int.from_bytes(b"ZKMFRIPF", "little")


# ---------------------------------------------------------------- field
def root_of_unity(bits):
    return pow(POWER_OF_TWO_GENERATOR, 1 << (32 - bits), P)


def reverse_bits(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def add2(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub2(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def mul2(a, b):
    return ((a[0] * b[0] + W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def inv2(a):
    norm = (a[0] * a[0] - W * a[1] * a[1]) % P
    assert norm, "division by zero"
    k = pow(norm, P - 2, P)
    return (a[0] * k % P, -a[1] * k % P)


def pow2(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = mul2(r, a)
        a = mul2(a, a)
        e >>= 1
    return r


# ---------------------------------------------------------------- hashing
@functools.lru_cache(maxsize=1 << 16)
def _permute(state):
    return tuple(pm.permute(list(state)))


def hash_or_noop(words):
    """PoseidonHash::hash_or_noop: a leaf of at most four words is its own digest (zero-padded), else hash_no_pad: the overwrite-mode
    sponge of rate 8."""
    words = [int(w) for w in words]
    if len(words) <= 4:
        return tuple(words + [0] * (4 - len(words)))
    state = (0,) * 12
    for c in range(0, len(words), 8):
        chunk = words[c:c + 8]
        state = _permute(tuple(chunk) + state[len(chunk):])
    return state[:4]


def two_to_one(left, right):
    return _permute(tuple(left) + tuple(right) + (0, 0, 0, 0))[:4]


def merkle_ok(leaf, index, cap, siblings):
    """verify_merkle_proof_to_cap: cap = list of digests, siblings = list of digests from the leaf up."""
    cur = hash_or_noop(leaf)
    for s in siblings:
        cur = two_to_one(s, cur) if index & 1 else two_to_one(cur, s)
        index >>= 1
    return cur == tuple(cap[index])


# ---------------------------------------------------------------- challenger
class Challenger:
    """plonky2 Challenger<F, PoseidonHash>: sponge state, input buffer, output buffer (popped from the end)."""

    def __init__(self, state=None, inputs=(), outputs=()):
        self.state, self.inputs, self.outputs = [int(x) for x in (state if state is not None else [0] * 12)], [int(x) for x in inputs], \
            [int(x) for x in outputs]

    def copy(self):
        return Challenger(self.state, self.inputs, self.outputs)

    def key(self):
        return (tuple(self.state), tuple(self.inputs), tuple(self.outputs))

    def _duplex(self):
        self.state[:len(self.inputs)] = self.inputs
        self.inputs = []
        self.state = list(_permute(tuple(self.state)))
        self.outputs = self.state[:8]

    def observe(self, words):
        for w in words:
            self.outputs = []
            self.inputs.append(int(w))
            if len(self.inputs) == 8:
                self._duplex()

    def get(self):
        if self.inputs or not self.outputs:
            self._duplex()
        return self.outputs.pop()

    def get_ext(self):
        a = self.get()
        return (a, self.get())


# ---------------------------------------------------------------- the blob
def num_layers(params, log_n):
    """FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits).reduction_arity_bits"""
    layers, d = 0, log_n
    while d > params["final_poly_bits"] and d + params["rate_bits"] - params["arity_bits"] >= params["cap_height"] and d >= params["arity_bits"]:
        d -= params["arity_bits"]
        layers += 1
    return layers


def digests(words):
    words = [int(w) for w in words]
    assert len(words) % 4 == 0
    return [tuple(words[i:i + 4]) for i in range(0, len(words), 4)]


def ext_values(words):
    words = [int(w) for w in words]
    return [(words[i], words[i + 1]) for i in range(0, len(words), 2)]


def offsets(params, log_n, oracle_cols):
    """Word offsets of the blob's fields (include/zkm_hip.h "FRI proof blob"): a dict with caps[l], final, pow, queries, round (words of
    one query round) and, inside a round, oracle[k] = (evals, siblings), layer[l] = (evals, siblings, sibling count)."""
    L, lde_bits, cap, ab = num_layers(params, log_n), log_n + params["rate_bits"], params["cap_height"], params["arity_bits"]
    o = {"L": L, "F": 1 << (log_n - L * ab), "lde_bits": lde_bits, "caps": [24 + l * (4 << cap) for l in range(L)]}
    o["final"] = 24 + L * (4 << cap)
    o["pow"] = o["final"] + 2 * o["F"]
    o["queries"] = o["pow"] + 1
    at, o["oracle"], o["layer"] = 0, [], []
    for cols in oracle_cols:
        o["oracle"].append((at, at + cols))
        at += cols + 4 * (lde_bits - cap)
    for l in range(L):
        count = lde_bits - ab * (l + 1) - cap
        o["layer"].append((at, at + (2 << ab), count))
        at += (2 << ab) + 4 * count
    o["round"] = at
    o["total"] = o["queries"] + params["num_queries"] * at
    return o


def parse(params, log_n, oracle_cols, blob):
    """The FRI proof blob -> FriProof as plain lists."""
    o = offsets(params, log_n, oracle_cols)
    blob = [int(w) for w in blob[:o["total"]]]
    assert blob[0] == MAGIC and len(blob) == o["total"]
    proof = {"caps": [digests(blob[c:c + (4 << params["cap_height"])]) for c in o["caps"]],
             "final": ext_values(blob[o["final"]:o["pow"]]), "pow": blob[o["pow"]], "rounds": []}
    nsib = o["lde_bits"] - params["cap_height"]
    for q in range(params["num_queries"]):
        r = blob[o["queries"] + q * o["round"]:o["queries"] + (q + 1) * o["round"]]
        initial = [(r[e:s], digests(r[s:s + 4 * nsib])) for e, s in o["oracle"]]
        steps = [(ext_values(r[e:s]), digests(r[s:s + 4 * count])) for e, s, count in o["layer"]]
        proof["rounds"].append((initial, steps))
    return proof


# ---------------------------------------------------------------- verify_fri_proof
def reduce_ext(alpha, values):
    """ReducingFactor::reduce: sum_j alpha^j v_j"""
    acc = (0, 0)
    for v in reversed(values):
        acc = add2(mul2(acc, alpha), v)
    return acc


def compute_evaluation(x, within, arity_bits, evals, beta):
    """The polynomial through the coset's 2^arity_bits values, at beta: plain Lagrange interpolation."""
    arity = 1 << arity_bits
    g = root_of_unity(arity_bits)
    evals = [evals[reverse_bits(i, arity_bits)] for i in range(arity)]          # reverse_index_bits
    start = x * pow(g, arity - reverse_bits(within, arity_bits), P) % P
    points = [start * pow(g, i, P) % P for i in range(arity)]
    total = (0, 0)
    for i in range(arity):
        num, den = (1, 0), 1
        for j in range(arity):
            if j != i:
                num = mul2(num, sub2(beta, (points[j], 0)))
                den = den * (points[i] - points[j]) % P
        total = add2(total, mul2(mul2(num, evals[i]), (pow(den, P - 2, P), 0)))
    return total


def fri_challenges(params, log_n, proof, challenger):
    """fri/challenges.rs fri_challenges on a parsed proof: (alpha, betas, the proof-of-work response, the query indices)"""
    alpha = challenger.get_ext()
    betas = []
    for cap in proof["caps"]:
        challenger.observe([w for d in cap for w in d])
        betas.append(challenger.get_ext())
    challenger.observe([w for v in proof["final"] for w in v])
    challenger.observe([proof["pow"]])
    response = challenger.get()
    indices = [challenger.get() % (1 << (log_n + params["rate_bits"])) for _ in range(params["num_queries"])]
    return alpha, betas, response, indices


def verify(params, log_n, oracle_cols, caps, batches, opened, blob, challenger):
    """verify_fri_proof.  caps[k]: oracle k's cap words; batches: [((c0, c1), [(oracle, poly), ..])]; opened[b]: 2 * npolys words;
    challenger: the state zkm_fri_prove was entered with (advanced in place: compare it only when the proof is accepted).
    Returns (code, query, tree, layer)."""
    proof = parse(params, log_n, oracle_cols, blob)
    ab, lde_bits = params["arity_bits"], log_n + params["rate_bits"]
    caps = [digests(c) for c in caps]
    alpha, betas, response, indices = fri_challenges(params, log_n, proof, challenger)
    # fri_verify_proof_of_work: leading zeros of the response
    if response >> (64 - params["pow_bits"]):
        return (POW, 0, 0, 0)
    # PrecomputedReducedOpenings
    reduced_openings = [reduce_ext(alpha, ext_values(o)) for o in opened]
    for q, (x_index, (initial, steps)) in enumerate(zip(indices, proof["rounds"])):
        # fri_verify_initial_proof
        for k, (row, path) in enumerate(initial):
            if not merkle_ok(row, x_index, caps[k], path):
                return (INITIAL_MERKLE, q, k, 0)
        x = MULTIPLICATIVE_GROUP_GENERATOR * pow(root_of_unity(lde_bits), reverse_bits(x_index, lde_bits), P) % P
        # fri_combine_initial
        total = (0, 0)
        for (point, polys), reduced in zip(batches, reduced_openings):
            evals = [(initial[o][0][p], 0) for o, p in polys]
            numerator = sub2(reduce_ext(alpha, evals), reduced)
            denominator = sub2((x, 0), (int(point[0]), int(point[1])))
            total = add2(mul2(total, pow2(alpha, len(polys))), mul2(numerator, inv2(denominator)))     # alpha.shift(sum), then +=
        old_eval = total
        for l, (evals, path) in enumerate(steps):
            within, coset = x_index & ((1 << ab) - 1), x_index >> ab
            if evals[within] != old_eval:
                return (FRI_EVAL, q, 0, l)
            old_eval = compute_evaluation(x, within, ab, evals, betas[l])
            if not merkle_ok([w for v in evals for w in v], coset, proof["caps"][l], path):
                return (FRI_MERKLE, q, 0, l)
            x = pow(x, 1 << ab, P)
            x_index = coset
        if reduce_ext((x, 0), proof["final"]) != old_eval:      # final_poly.eval(subgroup_x)
            return (FINAL_POLY, q, 0, 0)
    return (OK, 0, 0, 0)
