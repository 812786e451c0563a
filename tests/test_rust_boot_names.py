"""The reference items integration/rust/boot_hip.rs uses -- the fields of Program (cpu/kernel/elf.rs) it reads, the module path it imports
them by, the emulator's cycle budget and address constants that csrc/bootstrap.hip restates -- exist in the reference as the files rely on
them; and the bootstrap is the first thing generate_traces does while the exit kernel has no caller.  The facts are stored in
tests/golden/reference_boot_api.json, so the suite needs no reference tree; with ZKM_REFERENCE_ROOT naming a checkout the checks read that
tree instead, and `python tests/test_rust_boot_names.py <reference checkout>` rewrites the JSON file from it."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, item_visibility, strip_comments, struct_fields  # noqa: E402

FILE = os.path.join(ROOT, "integration", "rust", "boot_hip.rs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_boot_api.json")
SRC = {"elf": "prover/src/cpu/kernel/elf.rs", "kernel_mod": "prover/src/cpu/kernel/mod.rs", "cpu_mod": "prover/src/cpu/mod.rs",
       "generation": "prover/src/generation/mod.rs", "state": "emulator/src/state.rs", "memory": "emulator/src/memory.rs",
       "page": "emulator/src/page.rs", "bootstrap": "prover/src/cpu/bootstrap_kernel.rs"}


def reference_facts(root):
    raw = {k: open(os.path.join(root, p)).read() for k, p in SRC.items()}
    src = {k: strip_comments(v) for k, v in raw.items()}
    const = lambda s, n: re.sub(r"\s+", " ", re.search(r"pub const %s: \w+ = ([^;]+);" % n, s).group(1))
    return {
        "files": SRC,
        "program_fields": {f: [vis, re.sub(r"\s+", " ", ty)] for f, (vis, ty) in struct_fields(src["elf"], "Program").items()},
        "visibility": {"Program": item_visibility(src["elf"], "Program"), "elf_module": item_visibility(src["kernel_mod"], "elf"),
                       "kernel_module": item_visibility(src["cpu_mod"], "kernel")},
        "constants": {n: const(src[k], n) for k, n in (("state", "PAGE_LOAD_CYCLES"), ("state", "PAGE_HASH_CYCLES"), ("state", "IMAGE_ID_CYCLES"),
                                                         ("memory", "HASH_ADDRESS_BASE"), ("memory", "HASH_ADDRESS_END"),
                                                         ("memory", "ROOT_HASH_ADDRESS_BASE"), ("memory", "END_PC_ADDRESS"),
                                                         ("page", "PAGE_ADDR_SIZE"))},
        "bootstrap_calls_in_generation": len(re.findall(r"^\s*generate_bootstrap_kernel::<", src["generation"], flags=re.M)),
        "exit_kernel_calls_in_generation": len(re.findall(r"^\s*generate_exit_kernel::<", src["generation"], flags=re.M)),
        "exit_kernel_commented_out": bool(re.search(r"^\s*//\s*generate_exit_kernel::<", raw["generation"], flags=re.M)),
        "bootstrap_chunks_of_8": bool(re.search(r"program\.image\.iter\(\)\.chunks\(8\)", src["bootstrap"])),
    }


def facts():
    root = os.environ.get("ZKM_REFERENCE_ROOT")
    return reference_facts(root) if root else json.load(open(FIXTURE))["facts"]


def source():
    return strip_comments(open(FILE).read())


def test_program_fields_and_the_import_path_exist():
    f = facts()
    imports = crate_imports(source())
    assert (("cpu", "kernel", "elf"), "Program") in imports
    assert f["visibility"] == {"Program": "pub", "elf_module": "pub(crate)", "kernel_module": "pub"}
    used = set(re.findall(r"\bprogram\.([a-z_]+)\b", source()))
    assert used == {"image", "entry", "pre_hash_root", "pre_image_id"}
    want = {"image": "BTreeMap<u32, u32>", "entry": "u32", "pre_hash_root": "[u8; 32]", "pre_image_id": "[u8; 32]"}
    assert {k: f["program_fields"][k] for k in used} == {k: ["pub", t] for k, t in want.items()}


def test_the_constants_the_device_code_restates():
    c = facts()["constants"]
    assert c == {"PAGE_LOAD_CYCLES": "128", "PAGE_HASH_CYCLES": "1", "IMAGE_ID_CYCLES": "3", "HASH_ADDRESS_BASE": "0x80000000",
                 "HASH_ADDRESS_END": "0x81020000", "ROOT_HASH_ADDRESS_BASE": "0x81021000", "END_PC_ADDRESS": "ROOT_HASH_ADDRESS_BASE + 4 * 8",
                 "PAGE_ADDR_SIZE": "12"}
    dev = open(os.path.join(ROOT, "zkm_amd", "csrc", "bootstrap.hip")).read()
    assert "HASH_BASE = 0x80000000u, ROOT_PAGE = 0x81020000u, ID_BASE = 0x81021000u" in dev and "PAGE_BLOCKS = 129" in dev
    from tests import boot_model as BM
    assert (BM.HASH_BASE, BM.ROOT_PAGE, BM.ID_BASE) == (0x80000000, 0x81020000, 0x81021000)


def test_bootstrap_opens_every_segment_and_the_exit_kernel_has_no_caller():
    f = facts()
    assert f["bootstrap_calls_in_generation"] >= 1 and f["bootstrap_chunks_of_8"]
    assert f["exit_kernel_calls_in_generation"] == 0 and f["exit_kernel_commented_out"]


def test_the_wrappers_name_only_declared_library_items():
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+)\b", source()))
    assert {"zkm_prove_segments_ops_boot", "zkm_boot_image"} <= used
    assert re.search(r"pub fn boot_image_from_segment\(program: &Program\) -> BootImageHost", source())
    assert "pub(crate) fn size_then_prove(" in open(os.path.join(ROOT, "integration", "rust", "segment_hip.rs")).read()


if __name__ == "__main__":
    ref = sys.argv[1]
    with open(FIXTURE, "w") as fh:
        json.dump({"about": "facts about the reference's Program, bootstrap kernel and emulator constants used by tests/test_rust_boot_names.py; "
                            "regenerate with `python tests/test_rust_boot_names.py <reference checkout>`",
                   "facts": reference_facts(ref)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("facts ->", FIXTURE)
