"""integration/rust/check_ctls_hip.rs: the reference items it relies on -- check_ctls' argument list (cross_table_lookup.rs:1496-1499),
the fields of Column, Filter, TableWithColumns and CrossTableLookup it reads (private to `cross_table_lookup`: the file is a child of
that module), Table and Table::all -- exist in the reference as the file uses them, and every library item it names is declared in
zkm_hip_sys.rs with the header's argument names and pointer shapes.  The facts are stored in
tests/golden/reference_check_ctls_api.json, so the suite needs no reference tree; with ZKM_REFERENCE_ROOT naming a checkout the checks
read that tree instead, and `python tests/test_rust_check_ctls_names.py <reference checkout>` rewrites the JSON file from it."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, item_visibility, strip_comments, struct_fields  # noqa: E402

FILE = os.path.join(ROOT, "integration", "rust", "check_ctls_hip.rs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_check_ctls_api.json")
SRC = {"ctl": "prover/src/cross_table_lookup.rs", "all_stark": "prover/src/all_stark.rs", "prover": "prover/src/prover.rs"}
STRUCTS = ["Column", "Filter", "TableWithColumns", "CrossTableLookup"]
NEW = ["zkm_check_ctls", "zkm_segment_check_ctls"]


def reference_facts(root):
    src = {k: strip_comments(open(os.path.join(root, p)).read()) for k, p in SRC.items()}
    fields = lambda s, n: {f: [vis, re.sub(r"\s+", " ", ty)] for f, (vis, ty) in (struct_fields(s, n) or {}).items()}
    sig = re.search(r"fn check_ctls<F: Field>\(([^)]*)\)", src["ctl"]).group(1)
    return {
        "files": SRC,
        "fields": {n: fields(src["ctl"], n) for n in STRUCTS},
        "visibility": {n: item_visibility(src["ctl"], n) for n in STRUCTS} | {"Table": item_visibility(src["all_stark"], "Table"),
                                                                              "all_stark_module_has_all": bool(re.search(r"fn all\(\) -> \[Self; NUM_TABLES\]", src["all_stark"]))},
        "check_ctls_params": [[n, re.sub(r"\s+", " ", t)] for n, t in re.findall(r"(\w+)\s*:\s*([^,]+?)\s*(?:,|$)", sig.strip())],
        "prover_calls_check_ctls": bool(re.search(r"check_ctls\(&trace_poly_values, &all_stark\.cross_table_lookups\)", src["prover"])),
        "testutils_is_a_child_module": bool(re.search(r"pub\(crate\) mod testutils \{\s*use super::\*;", src["ctl"])),
    }


def facts():
    root = os.environ.get("ZKM_REFERENCE_ROOT")
    return reference_facts(root) if root else json.load(open(FIXTURE))["facts"]


def source():
    return strip_comments(open(FILE).read())


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_check_ctls_hip_takes_the_references_argument_list():
    f = facts()
    assert f["check_ctls_params"] == [["trace_poly_values", "&[Vec<PolynomialValues<F>>]"], ["cross_table_lookups", "&[CrossTableLookup<F>]"]]
    assert f["prover_calls_check_ctls"]
    sig = re.search(r"pub fn check_ctls_hip<F: PrimeField64>\(([^)]*)\)", source()).group(1)
    params = [[n, re.sub(r"\s+", " ", t)] for n, t in re.findall(r"(\w+)\s*:\s*([^,]+?)\s*(?:,|$)", sig.strip())]
    assert params == [["ctx", "*mut zkm_ctx"]] + f["check_ctls_params"]
    assert "panic!(" in source()


def test_every_field_read_exists_in_the_reference():
    """A child module of cross_table_lookup may read its parent's private fields (the reference's own testutils does: use super::*)."""
    f = facts()
    src = source()
    assert f["testutils_is_a_child_module"]
    sup = re.search(r"use super::\{([^}]*)\};", src).group(1)
    assert sorted(x.strip() for x in sup.split(",")) == sorted(STRUCTS)
    for n in STRUCTS:
        assert f["visibility"][n] in ("pub", "pub(crate)"), n
    # bindings of the file -> the struct they are
    reads = {"Column": re.findall(r"\bc\.([a-z_]+)\b(?!\()", src), "TableWithColumns": re.findall(r"\bt\.([a-z_]+)\b(?!\()", src) + ["table"],
             "CrossTableLookup": re.findall(r"\bctl\.([a-z_]+)\b(?!\()", src)}
    reads["TableWithColumns"] = [x for x in reads["TableWithColumns"] if x not in ("len", "iter")]
    for n, names in reads.items():
        assert names, n
        for x in names:
            assert x in f["fields"][n], (n, x)
    assert set(reads["Column"]) == {"linear_combination", "next_row_linear_combination", "constant"} == set(f["fields"]["Column"])
    assert {"columns", "filter", "table"} == set(f["fields"]["TableWithColumns"])
    assert set(reads["CrossTableLookup"]) == {"looking_tables", "looked_table"} == set(f["fields"]["CrossTableLookup"])
    pat = re.search(r"Some\(Filter \{ ([a-z_, ]+) \}\)", src).group(1)
    assert {x.strip() for x in pat.split(",")} == {"products", "constants"} == set(f["fields"]["Filter"])
    assert f["fields"]["Column"]["linear_combination"][1].startswith("Vec<(usize, F)>")
    assert f["fields"]["Filter"]["products"][1].startswith("Vec<(Column<F>, Column<F>)>")
    assert f["fields"]["TableWithColumns"]["filter"][1].startswith("Option<Filter<F>>")


def test_crate_imports_resolve():
    f = facts()
    imports = crate_imports(source())
    assert sorted(imports) == [(("all_stark",), "Table"), (("prove_hip",), "zkm_table_id")]
    assert f["visibility"]["Table"] == "pub" and f["visibility"]["all_stark_module_has_all"]
    assert re.search(r"pub fn zkm_table_id\(t: Table\) -> i32", read("integration", "rust", "prove_hip.rs"))


def test_the_file_names_only_declared_library_items():
    sys_rs = strip_comments(read("integration", "rust", "zkm_hip_sys.rs"))
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+)\b", source())) - {"zkm_table_id"}
    assert set(NEW) <= used
    # the report's fields the file reads exist in the mirror
    rep = re.search(r"pub struct ZkmCtlReport \{(.*?)\n\}", sys_rs, flags=re.S).group(1)
    for x in re.findall(r"\breport\.([a-z_]+)\b", source()):
        assert re.search(r"pub %s:" % x, rep), x


if __name__ == "__main__":
    root = sys.argv[1]
    json.dump({"about": "facts about the reference's cross_table_lookup structs and check_ctls used by tests/test_rust_check_ctls_names.py; "
                        "regenerate with `python tests/test_rust_check_ctls_names.py <reference checkout>`",
               "facts": reference_facts(root)}, open(FIXTURE, "w"), indent=1, sort_keys=True)
    print("wrote", FIXTURE)
