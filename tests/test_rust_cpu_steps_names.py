"""The reference items integration/rust/cpu_steps_hip.rs uses -- the variants of witness::operation::Operation it maps to step kinds, the
operators, branch and move conditions it matches on, the fields of RegistersState it reads, the module paths it imports them by, the
five assignments of simulate_cpu's padding row and the register decode hands BGEZ -- exist in the reference as the file relies on them.
The facts are stored in tests/golden/reference_cpu_steps_api.json, so the suite needs no reference tree; with ZKM_REFERENCE_ROOT naming
a checkout the checks read that tree instead, and `python tests/test_rust_cpu_steps_names.py <reference checkout>` rewrites the JSON file
from it."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, enum_variants, item_visibility, strip_comments, struct_fields  # noqa: E402

FILE = os.path.join(ROOT, "integration", "rust", "cpu_steps_hip.rs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_cpu_steps_api.json")
SRC = {"operation": "prover/src/witness/operation.rs", "state": "prover/src/witness/state.rs", "witness_mod": "prover/src/witness/mod.rs",
       "transition": "prover/src/witness/transition.rs", "arithmetic": "prover/src/arithmetic/mod.rs", "columns": "prover/src/cpu/columns/mod.rs",
       "cpu_mod": "prover/src/cpu/mod.rs", "generation": "prover/src/generation/mod.rs", "lib": "prover/src/lib.rs"}


def reference_facts(root):
    src = {k: strip_comments(open(os.path.join(root, p)).read()) for k, p in SRC.items()}
    body = re.search(r"\benum\s+Operation\b[^{]*\{(.*?)\n\}", src["operation"], flags=re.S).group(1)
    pad = re.search(r"let mut row = CpuColumnsView::<F>::default\(\);(.*?)loop \{", src["generation"], flags=re.S).group(1)
    return {
        "files": SRC,
        "operation_variants": {m.group(1): len([a for a in (m.group(2) or "").split(",") if a.strip()])
                               for m in re.finditer(r"^\s*([A-Z][A-Za-z0-9]*)(?:\(([^)]*)\))?,", body, flags=re.M)},
        "binary_operators": sorted(enum_variants(src["arithmetic"], "BinaryOperator")),
        "branch_conds": sorted(enum_variants(src["operation"], "BranchCond")),
        "mov_conds": sorted(enum_variants(src["operation"], "MovCond")),
        "registers_fields": {f: [vis, ty] for f, (vis, ty) in struct_fields(src["state"], "RegistersState").items()},
        "visibility": {"Operation": item_visibility(src["operation"], "Operation"), "BranchCond": item_visibility(src["operation"], "BranchCond"),
                       "MovCond": item_visibility(src["operation"], "MovCond"), "BinaryOperator": item_visibility(src["arithmetic"], "BinaryOperator"),
                       "RegistersState": item_visibility(src["state"], "RegistersState"), "CpuColumnsView": item_visibility(src["columns"], "CpuColumnsView"),
                       "operation_module": item_visibility(src["witness_mod"], "operation"), "state_module": item_visibility(src["witness_mod"], "state"),
                       "columns_module": item_visibility(src["cpu_mod"], "columns"), "witness_module": item_visibility(src["lib"], "witness"),
                       "arithmetic_module": item_visibility(src["lib"], "arithmetic")},
        "cpu_columns_view_is_repr_c": bool(re.search(r"#\[repr\(C\)\]\s*(?:#\[[^\]]*\]\s*)*pub struct CpuColumnsView", src["columns"])),
        "pad_row_assignments": re.findall(r"row\.([a-z_]+)\s*=", pad),
        "bgez_second_source": re.search(r"Operation::Branch\(BranchCond::GE, rs, (\w+), offset\)", src["transition"]).group(1),
        "signext_widths": sorted(set(re.findall(r"Operation::Signext\(rd, rt, (\d+)\)", src["transition"]))),
        "count_clo_flag": re.search(r"Operation::Count\((\w+), rs, rd\)\),?\s*//\s*CLO", open(os.path.join(root, SRC["transition"])).read()).group(1),
    }


def facts():
    root = os.environ.get("ZKM_REFERENCE_ROOT")
    return reference_facts(root) if root else json.load(open(FIXTURE))["facts"]


def source():
    return strip_comments(open(FILE).read())


def test_imports_resolve_and_are_visible():
    f = facts()
    imports = set(crate_imports(source()))
    assert {(("witness", "operation"), "Operation"), (("witness", "operation"), "BranchCond"), (("witness", "operation"), "MovCond"),
            (("witness", "state"), "RegistersState"), (("cpu", "columns"), "CpuColumnsView"), (("arithmetic",), "BinaryOperator")} <= imports
    assert all(v in ("pub", "pub(crate)") for v in f["visibility"].values()), f["visibility"]
    assert f["cpu_columns_view_is_repr_c"]


def test_every_operation_variant_matched_exists_with_its_arity():
    f = facts()
    src = source()
    used = {}
    for m in re.finditer(r"Operation::([A-Z][A-Za-z]*)(?:\(([^)]*)\))?", src):
        used.setdefault(m.group(1), set()).add(m.group(2))
    assert len(used) >= 20
    for name, shapes in used.items():
        assert name in f["operation_variants"], name
        for shape in shapes:
            if shape is None:
                assert f["operation_variants"][name] == 0, name
            elif ".." not in shape:
                assert len(shape.split(",")) == f["operation_variants"][name], (name, shape)
            else:
                assert len([a for a in shape.split(",") if a.strip() != ".."]) <= f["operation_variants"][name], (name, shape)
    # the operations without a kind are the ones the file's head names: they go RAW
    assert set(f["operation_variants"]) - set(used) == {"KeccakGeneral", "Pc", "GetContext", "SetContext"}
    ops = set(re.findall(r"\b([A-Z]{2,6})\b(?=[ |,)])", re.search(r"pub fn step_kind.*?\n}\n", src, flags=re.S).group(0))) - {"EQ", "NE"}
    assert ops and ops <= set(f["binary_operators"]), ops - set(f["binary_operators"])
    assert {"GE", "LT", "LE", "GT"} <= set(f["branch_conds"]) and set(f["mov_conds"]) == {"EQ", "NE"}
    assert f["signext_widths"] == ["16", "8"] and f["count_clo_flag"] == "true"


def test_registers_fields_and_the_padding_row():
    f = facts()
    used = set(re.findall(r"\bregisters\.([a-z_]+)\b", source()))
    assert used == {"program_counter", "next_pc", "is_kernel", "context"}
    want = {"program_counter": "usize", "next_pc": "usize", "is_kernel": "bool", "context": "usize"}
    assert {k: f["registers_fields"][k] for k in used} == {k: ["pub", t] for k, t in want.items()}
    # the five assignments the PAD kind restates (csrc/cpu_steps.hip; tests/test_gpu_cpu_steps.py holds the kernel to them), and what BGEZ reads
    assert f["pad_row_assignments"] == ["clock", "context", "program_counter", "next_program_counter", "is_exit_kernel"]
    assert f["bgez_second_source"] == "0u8"


def test_the_wrappers_name_only_declared_library_items():
    sys_rs = strip_comments(open(os.path.join(ROOT, "integration", "rust", "zkm_hip_sys.rs")).read())
    consts = set(re.findall(r"pub const (ZKM_\w+)", sys_rs))
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+)\b", source()))
    assert {"zkm_prove_segments_ops_steps", "zkm_segments_tables_steps", "zkm_cpu_steps_counts", "zkm_cpu_step", "zkm_cpu_steps"} <= used
    used_consts = set(re.findall(r"\b(ZKM_[A-Z0-9_]+)\b", source()))
    assert used_consts <= consts, used_consts - consts
    header = open(os.path.join(ROOT, "include", "zkm_hip.h")).read()
    for name, value in re.findall(r"pub const (ZKM_(?:STEP|SYSCALL)_\w+): u32 = (\d+);", sys_rs):
        assert re.search(r"#define %s %su?\n" % (name, value), header), name
    assert len(re.findall(r"#define ZKM_(?:STEP|SYSCALL)_\w+ ", header)) == len(re.findall(r"pub const ZKM_(?:STEP|SYSCALL)_\w+:", sys_rs))
    assert "pub(crate) fn size_then_prove(" in open(os.path.join(ROOT, "integration", "rust", "segment_hip.rs")).read()
    assert re.search(r"pub fn check\(rc: c_int, err: \*mut c_char\)", sys_rs)


if __name__ == "__main__":
    ref = sys.argv[1]
    with open(FIXTURE, "w") as fh:
        json.dump({"about": "facts about the reference's Operation, RegistersState and padding row used by tests/test_rust_cpu_steps_names.py; "
                            "regenerate with `python tests/test_rust_cpu_steps_names.py <reference checkout>`",
                   "facts": reference_facts(ref)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("facts ->", FIXTURE)
