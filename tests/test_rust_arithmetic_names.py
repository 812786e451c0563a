"""The reference items integration/rust/arithmetic_hip.rs uses (crate::arithmetic: Operation, BinaryOperator, the fields of
Operation::BinaryOperation, BinaryOperator::row_filter) exist in the reference with the visibility, variants and fields the file
relies on -- the checks tests/test_rust_memory_names.py makes for memory_hip.rs, for this module.  The facts about the reference are
stored in tests/golden/reference_arithmetic_api.json, so the suite needs no reference tree; with ZKM_REFERENCE_ROOT naming a
checkout of the reference the checks read that tree instead, and `python tests/test_rust_arithmetic_names.py <reference checkout>`
rewrites the JSON file from it."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, enum_variants, item_visibility, strip_comments  # noqa: E402

FILE = os.path.join(ROOT, "integration", "rust", "arithmetic_hip.rs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_arithmetic_api.json")
MODULE = "prover/src/arithmetic/mod.rs"


def variant_fields(src, enum, variant):
    """{field: type head} of a struct-like enum variant."""
    body = re.search(r"\benum\s+%s\b[^{]*\{(.*?)\n\}" % re.escape(enum), src, flags=re.S).group(1)
    m = re.search(r"\b%s\s*\{([^}]*)\}" % re.escape(variant), body)
    return {f: re.match(r"([A-Za-z][A-Za-z0-9_]*)", ty.strip()).group(1)
            for f, ty in re.findall(r"([a-z_][a-z0-9_]*)\s*:\s*([^,]+)", m.group(1))} if m else None


def reference_facts(root):
    """What the checks need to know about prover/src/arithmetic/mod.rs of a reference checkout."""
    mod = strip_comments(open(os.path.join(root, MODULE)).read())
    lib = strip_comments(open(os.path.join(root, "prover", "src", "lib.rs")).read())
    ret = re.search(r"\bfn\s+row_filter\s*\(&self\)\s*->\s*([A-Za-z0-9_]+)", mod)
    return {
        "module": MODULE,
        "module_visibility": {"arithmetic": item_visibility(lib, "arithmetic")},
        "visibility": {n: item_visibility(mod, n) for n in ("Operation", "BinaryOperator", "row_filter")},
        "variants": {"Operation": sorted(enum_variants(mod, "Operation")), "BinaryOperator": sorted(enum_variants(mod, "BinaryOperator"))},
        "variant_fields": {"Operation::BinaryOperation": variant_fields(mod, "Operation", "BinaryOperation")},
        "row_filter_returns": ret.group(1) if ret else None,
    }


def facts():
    root = os.environ.get("ZKM_REFERENCE_ROOT")
    return reference_facts(root) if root else json.load(open(FIXTURE))["facts"]


def source():
    return strip_comments(open(FILE).read())


def test_crate_imports_resolve_in_the_reference():
    f = facts()
    imports = crate_imports(source())
    assert imports, "arithmetic_hip.rs imports nothing from the crate: the parser found nothing to check"
    for path, item in imports:
        assert path == ("arithmetic",), "crate::%s is not covered by tests/golden/reference_arithmetic_api.json" % "::".join(path)
        assert f["visibility"].get(item) in ("pub", "pub(crate)"), "crate::arithmetic::%s is not visible to the crate" % item
    assert all(v in ("pub", "pub(crate)") for v in f["module_visibility"].values()), f["module_visibility"]


def test_variant_fields_and_row_filter_exist():
    """The one variant is matched exhaustively (Operation has no other), its fields exist with the types the packing needs, and
    row_filter is callable from the crate and returns the usize the file casts."""
    f = facts()
    src = source()
    assert f["variants"]["Operation"] == ["BinaryOperation"]
    fields = f["variant_fields"]["Operation::BinaryOperation"]
    assert fields["operator"] == "BinaryOperator" and fields["input0"] == fields["input1"] == "u32"
    m = re.search(r"Operation::BinaryOperation\s*\{([^}]*)\}", src)
    used = [u.strip() for u in m.group(1).split(",") if u.strip() and u.strip() != ".."]
    assert used == ["operator", "input0", "input1"] and set(used) <= set(fields)
    assert set(re.findall(r"\boperator\.([a-z_][a-z0-9_]*)\(", src)) == {"row_filter"}
    assert f["visibility"]["row_filter"] in ("pub", "pub(crate)") and f["row_filter_returns"] == "usize"
    assert len(f["variants"]["BinaryOperator"]) == 26


if __name__ == "__main__":
    ref = sys.argv[1]
    with open(FIXTURE, "w") as fh:
        json.dump({"about": "facts about the reference's prover/src/arithmetic/mod.rs used by tests/test_rust_arithmetic_names.py; "
                            "regenerate with `python tests/test_rust_arithmetic_names.py <reference checkout>`",
                   "facts": reference_facts(ref)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("facts ->", FIXTURE)
