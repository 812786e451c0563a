"""The reference items integration/rust/memory_hip.rs uses (crate::witness::memory: MemoryOp, MemoryAddress, MemoryOpKind) exist in
the reference with the visibility, fields and variants the file relies on -- the checks tests/test_rust_names.py makes for the other
crate files, for this module.  The facts about the reference are stored in tests/golden/reference_memory_api.json, so the suite
needs no reference tree; with ZKM_REFERENCE_ROOT naming a checkout of the reference the checks read that tree instead, and
`python tests/test_rust_memory_names.py <reference checkout>` rewrites the JSON file from it."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, enum_variants, item_visibility, strip_comments, struct_fields  # noqa: E402

FILE = os.path.join(ROOT, "integration", "rust", "memory_hip.rs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_memory_api.json")
MODULE = "prover/src/witness/memory.rs"


def reference_facts(root):
    """What the checks need to know about prover/src/witness/memory.rs of a reference checkout."""
    mem = strip_comments(open(os.path.join(root, MODULE)).read())
    parent = strip_comments(open(os.path.join(root, "prover", "src", "witness", "mod.rs")).read())
    lib = strip_comments(open(os.path.join(root, "prover", "src", "lib.rs")).read())

    def fields(name):
        f = struct_fields(mem, name)
        heads = {u: re.match(r"&?\s*([A-Za-z][A-Za-z0-9_]*)", ty) for u, (_, ty) in f.items()}
        return {u: [vis, heads[u].group(1) if heads[u] else None] for u, (vis, _) in f.items()}
    return {
        "module": MODULE,
        "module_visibility": {"witness": item_visibility(lib, "witness"), "witness::memory": item_visibility(parent, "memory")},
        "visibility": {n: item_visibility(mem, n) for n in ("MemoryOp", "MemoryOpKind", "MemoryAddress")},
        "fields": {n: fields(n) for n in ("MemoryOp", "MemoryAddress")},
        "variants": {"MemoryOpKind": sorted(enum_variants(mem, "MemoryOpKind"))},
    }


def facts():
    root = os.environ.get("ZKM_REFERENCE_ROOT")
    return reference_facts(root) if root else json.load(open(FIXTURE))["facts"]


def source():
    return strip_comments(open(FILE).read())


def test_crate_imports_resolve_in_the_reference():
    f = facts()
    imports = crate_imports(source())
    assert imports, "memory_hip.rs imports nothing from the crate: the parser found nothing to check"
    for path, item in imports:
        assert path == ("witness", "memory"), "crate::%s is not covered by tests/golden/reference_memory_api.json" % "::".join(path)
        assert f["visibility"].get(item) in ("pub", "pub(crate)"), "crate::witness::memory::%s is not visible to the crate" % item
    # a module of the same crate reaches a pub(crate) module
    assert all(v in ("pub", "pub(crate)") for v in f["module_visibility"].values()), f["module_visibility"]


def test_field_accesses_and_variants_exist():
    f = facts()
    src = source()
    op, addr = f["fields"]["MemoryOp"], f["fields"]["MemoryAddress"]
    assert op["address"][1] == "MemoryAddress" and op["kind"][1] == "MemoryOpKind" and op["value"][1] == "u32"
    used_op = set(re.findall(r"\bop\.([a-z_][a-z0-9_]*)", src))
    used_addr = set(re.findall(r"\bop\.address\.([a-z_][a-z0-9_]*)", src))
    assert used_op == {"filter", "address", "timestamp", "kind", "value"} and used_addr == {"context", "segment", "virt"}
    assert used_op <= set(op) and used_addr <= set(addr)
    # the file reads those fields from outside their module: each must be visible to the crate
    for fields, used in ((op, used_op), (addr, used_addr)):
        for u in used:
            assert fields[u][0] in ("pub", "pub(crate)"), u
    variants = set(re.findall(r"\bMemoryOpKind::([A-Z][A-Za-z0-9_]*)", src))
    assert variants and variants <= set(f["variants"]["MemoryOpKind"])


if __name__ == "__main__":
    ref = sys.argv[1]
    with open(FIXTURE, "w") as fh:
        json.dump({"about": "facts about the reference's prover/src/witness/memory.rs used by tests/test_rust_memory_names.py; "
                            "regenerate with `python tests/test_rust_memory_names.py <reference checkout>`",
                   "facts": reference_facts(ref)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("facts ->", FIXTURE)
