"""integration/rust/verify_hip.rs: the reference items it relies on -- verify_proof's argument list (verifier.rs:27-31), the fields of
AllProof, GrandProductChallengeSet, GrandProductChallenge and AllStark it reads, NUM_TABLES, and the two call sites it replaces
(fixed_recursive_verifier.rs) -- exist in the reference as the file uses them, and every library item it names is declared in
zkm_hip_sys.rs with the header's argument names and pointer shapes.  The facts are stored in tests/golden/reference_verify_api.json
(names, visibilities and argument lists only), so the suite needs no reference tree; with ZKM_REFERENCE_ROOT naming a checkout the
checks read that tree instead, and `python tests/test_rust_verify_names.py <reference checkout>` rewrites the JSON file from it."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, item_visibility, strip_comments, struct_fields  # noqa: E402

FILE = os.path.join(ROOT, "integration", "rust", "verify_hip.rs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_verify_api.json")
SRC = {"verifier": "prover/src/verifier.rs", "proof": "prover/src/proof.rs", "ctl": "prover/src/cross_table_lookup.rs",
       "all_stark": "prover/src/all_stark.rs", "recursion": "prover/src/fixed_recursive_verifier.rs", "config": "prover/src/config.rs"}


def params_of(sig):
    """[[name, type]] of a parameter list; commas inside <...> belong to the type."""
    parts, depth, cur = [], 0, ""
    for ch in sig:
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    parts.append(cur)
    return [[n.strip(), re.sub(r"\s+", " ", t.strip())] for n, t in (x.split(":", 1) for x in parts if x.strip())]


def reference_facts(root):
    src = {k: strip_comments(open(os.path.join(root, p)).read()) for k, p in SRC.items()}
    fields = lambda s, n: {f: [vis, re.sub(r"\s+", " ", ty)] for f, (vis, ty) in (struct_fields(s, n) or {}).items()}
    sig = re.search(r"pub fn verify_proof<[^(]*\(([^)]*)\)\s*->\s*Result<\(\)>", src["verifier"], flags=re.S).group(1)
    return {
        "files": SRC,
        "verify_proof_params": params_of(sig),
        "fields": {"AllProof": fields(src["proof"], "AllProof"), "GrandProductChallengeSet": fields(src["ctl"], "GrandProductChallengeSet"),
                   "GrandProductChallenge": fields(src["ctl"], "GrandProductChallenge"),
                   "AllStark": {k: v for k, v in fields(src["all_stark"], "AllStark").items() if k == "cross_table_lookups"},
                   "StarkConfig": fields(src["config"], "StarkConfig")},
        "visibility": {"AllProof": item_visibility(src["proof"], "AllProof"), "AllStark": item_visibility(src["all_stark"], "AllStark"),
                       "NUM_TABLES": item_visibility(src["all_stark"], "NUM_TABLES"), "StarkConfig": item_visibility(src["config"], "StarkConfig"),
                       "verify_proof": item_visibility(src["verifier"], "verify_proof")},
        "recursion_calls_verify_proof": len(re.findall(r"verify_proof\(all_stark, all_proof\.clone\(\), config\)\.unwrap\(\)", src["recursion"])),
    }


def facts():
    root = os.environ.get("ZKM_REFERENCE_ROOT")
    return reference_facts(root) if root else json.load(open(FIXTURE))["facts"]


def source():
    return strip_comments(open(FILE).read())


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_verify_proof_hip_takes_the_references_argument_list():
    f = facts()
    assert f["verify_proof_params"] == [["all_stark", "&AllStark<F, D>"], ["all_proof", "AllProof<F, C, D>"], ["config", "&StarkConfig"]]
    assert f["recursion_calls_verify_proof"] == 2 and f["visibility"]["verify_proof"] == "pub"
    sig = re.search(r"pub fn verify_proof_hip<F, C, const D: usize>\(([^)]*)\)\s*->\s*Result<\(\)>", source()).group(1)
    assert params_of(sig) == [["ctx", "*mut zkm_ctx"]] + f["verify_proof_params"]


def test_every_field_read_exists_in_the_reference():
    f = facts()
    src = source()
    reads = {"AllProof": set(re.findall(r"\ball_proof\.([a-z_]+)\b(?!\()", src)), "AllStark": set(re.findall(r"\ball_stark\.([a-z_]+)\b(?!\()", src))}
    assert reads["AllProof"] == {"stark_proofs", "ctl_challenges", "public_values"} == set(f["fields"]["AllProof"])
    assert reads["AllStark"] == {"cross_table_lookups"} == set(f["fields"]["AllStark"])
    # ctl_challenges is pub(crate): the file lives in the zkm-prover crate, as its header says
    assert f["fields"]["AllProof"]["ctl_challenges"] == ["pub(crate)", "GrandProductChallengeSet<F>"] and "prover/src/verify_hip.rs" in open(FILE).read()
    assert re.search(r"ctl_challenges\.challenges\.iter\(\)", src) and "challenges" in f["fields"]["GrandProductChallengeSet"]
    assert set(re.findall(r"\bc\.([a-z_]+)\.to_canonical_u64", src)) == {"beta", "gamma"} <= set(f["fields"]["GrandProductChallenge"])
    assert "num_challenges" in f["fields"]["StarkConfig"] and re.search(r"config\.num_challenges", src)
    for n in ("AllProof", "AllStark", "StarkConfig"):
        assert f["visibility"][n] == "pub", n
    assert f["visibility"]["NUM_TABLES"] in ("pub", "pub(crate)")


def test_crate_imports_resolve():
    imports = crate_imports(source())
    assert sorted(imports) == [(("all_stark",), "AllStark"), (("all_stark",), "NUM_TABLES"), (("config",), "StarkConfig"), (("proof",), "AllProof"),
                               (("proof_blob",), "stark_proof_to_blob"), (("prove_hip",), "public_values_words"), (("prove_hip",), "zkm_config")]
    assert re.search(r"pub fn stark_proof_to_blob<F, C, const D: usize>\(p: &StarkProofWithMetadata<F, C, D>, config: &StarkConfig\) -> Vec<u64>",
                     read("integration", "rust", "proof_blob.rs"))
    assert re.search(r"pub fn public_values_words\(pv: &PublicValues\) -> Vec<u64>", read("integration", "rust", "prove_hip.rs"))
    assert re.search(r"pub fn zkm_config\(c: &StarkConfig\) -> zkm_stark_config", read("integration", "rust", "prove_hip.rs"))


def test_the_file_names_only_declared_library_items():
    sys_rs = strip_comments(read("integration", "rust", "zkm_hip_sys.rs"))
    consts = set(re.findall(r"pub const (ZKM_\w+):", sys_rs))
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+)\b", source())) - {"zkm_config"}
    assert "zkm_verify_segments" in used and "zkm_verify_report" in used
    assert set(re.findall(r"\b(ZKM_[A-Z_]+)\b", source())) <= consts
    rep = re.search(r"pub struct ZkmVerifyReport \{(.*?)\n\}", sys_rs, flags=re.S).group(1)
    for x in re.findall(r"\breport\.([a-z_]+)\b", source()):
        assert re.search(r"pub %s:" % x, rep), x


if __name__ == "__main__":
    root = sys.argv[1]
    json.dump({"about": "facts about the reference's verify_proof, AllProof and the challenge structs used by tests/test_rust_verify_names.py; "
                        "regenerate with `python tests/test_rust_verify_names.py <reference checkout>`",
               "facts": reference_facts(root)}, open(FIXTURE, "w"), indent=1, sort_keys=True)
    print("wrote", FIXTURE)
