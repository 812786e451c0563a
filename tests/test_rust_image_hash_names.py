"""The reference items integration/rust/image_hash_hip.rs uses -- Memory's page maps, CachedPage and its data, the functions split_segment
calls between two segments, the emulator's address constants that csrc/image_hash.hip restates -- exist in the reference as the file
relies on them.  The facts (names, visibilities, field types and constants only) are stored in tests/golden/reference_image_hash_api.json,
so the suite needs no reference tree; with ZKM_REFERENCE_ROOT naming a checkout the checks read that tree instead, and
`python tests/test_rust_image_hash_names.py <reference checkout>` rewrites the JSON file from it."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, functions, item_visibility, strip_comments, struct_fields  # noqa: E402

FILE = os.path.join(ROOT, "integration", "rust", "image_hash_hip.rs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_image_hash_api.json")
SRC = {"memory": "emulator/src/memory.rs", "page": "emulator/src/page.rs", "state": "emulator/src/state.rs", "lib": "emulator/src/lib.rs"}
MEMORY_FNS = ["poseidon", "hash_page", "alloc_hash_page", "set_hash_range", "update_page_hash", "compute_image_id"]


def reference_facts(root):
    src = {k: strip_comments(open(os.path.join(root, p)).read()) for k, p in SRC.items()}
    const = lambda s, n: re.sub(r"\s+", " ", re.search(r"pub(?:\(crate\))? const %s: \w+ = ([^;]+);" % n, s).group(1))
    fields = lambda s, n: {f: [vis, re.sub(r"\s+", " ", ty)] for f, (vis, ty) in struct_fields(s, n).items()}
    split = next(body for sig, body in functions(src["state"]) if re.search(r"\bfn\s+split_segment\b", sig))
    update = next(body for sig, body in functions(src["memory"]) if re.search(r"\bfn\s+update_page_hash\b", sig))
    # (the signature holds a `;` -- an array type -- which functions() takes for a declaration: cut by hand, up to the next item)
    image_id = re.search(r"\bfn\s+compute_image_id\b(.*?)\n    (?:pub )?fn ", src["memory"], flags=re.S).group(1)
    return {
        "files": SRC,
        "memory_fields": {k: v for k, v in fields(src["memory"], "Memory").items() if k in ("pages", "wtrace")},
        "cached_page_fields": fields(src["page"], "CachedPage"),
        "visibility": dict({"page_module": item_visibility(src["lib"], "page"), "memory_module": item_visibility(src["lib"], "memory"),
                            "CachedPage": item_visibility(src["page"], "CachedPage"), "get_registers_bytes": item_visibility(src["state"], "get_registers_bytes"),
                            "split_segment": item_visibility(src["state"], "split_segment")},
                           **{n: item_visibility(src["memory"], n) for n in MEMORY_FNS}),
        "cached_page_new": bool(re.search(r"pub fn new\(\) -> Self", src["page"])),
        "constants": {n: const(src[k], n) for k, n in (("memory", "HASH_ADDRESS_BASE"), ("memory", "HASH_ADDRESS_END"),
                                                         ("memory", "ROOT_HASH_ADDRESS_BASE"), ("memory", "REGISTERS_OFFSET"),
                                                         ("memory", "SPONGE_RATE"), ("memory", "POSEIDON_RATE_BYTES"), ("page", "PAGE_ADDR_SIZE"),
                                                         ("page", "PAGE_SIZE"), ("page", "MAX_MEMORY"))},
        "root_page_index": re.search(r"let root_page = (0x[0-9a-fA-F]+)u32", image_id).group(1),
        "registers_bytes": re.search(r"registers: &\[u8; ([0-9 *]+)\]", src["memory"]).group(1),
        "hash_levels": len(re.findall(r"self\.wtrace\[\d\]\.clear\(\)", update)),
        "split_hashes_before_image_id": 0 <= split.find("update_page_hash()") < split.find("compute_image_id("),
    }


def facts():
    root = os.environ.get("ZKM_REFERENCE_ROOT")
    return reference_facts(root) if root else json.load(open(FIXTURE))["facts"]


def source():
    return strip_comments(open(FILE).read())


def test_the_page_maps_and_the_page_type_exist():
    f = facts()
    page_map = "BTreeMap<u32, Rc<RefCell<CachedPage>>>"
    assert f["memory_fields"] == {"pages": ["private", page_map], "wtrace": ["private", "[%s; 3]" % page_map]}
    assert f["cached_page_fields"]["data"] == ["pub", "[u8; PAGE_SIZE]"] and f["cached_page_new"]
    assert f["visibility"]["page_module"] == "pub" and f["visibility"]["CachedPage"] == "pub"
    imports = crate_imports(source())
    assert (("page",), "CachedPage") in imports and (("page",), "PAGE_SIZE") in imports
    assert source().count("&" + page_map) == 2 and "&mut " + page_map in source()
    assert set(re.findall(r"\bpage\.borrow(?:_mut)?\(\)\.([a-z_]+)\b", source())) == {"data"}


def test_the_functions_the_call_replaces():
    f = facts()
    v = f["visibility"]
    assert v["update_page_hash"] == "pub" and v["compute_image_id"] == "pub" and v["get_registers_bytes"] == "pub" and v["split_segment"] == "pub"
    assert all(v[n] is not None for n in ("poseidon", "hash_page", "alloc_hash_page", "set_hash_range"))
    assert f["hash_levels"] == 3 and f["split_hashes_before_image_id"]
    assert f["registers_bytes"] == "39 * 4" and "registers: &[u8; 39 * 4]" in source()


def test_the_constants_the_device_code_restates():
    f = facts()
    assert f["constants"] == {"HASH_ADDRESS_BASE": "0x80000000", "HASH_ADDRESS_END": "0x81020000", "ROOT_HASH_ADDRESS_BASE": "0x81021000",
                              "REGISTERS_OFFSET": "0x400", "SPONGE_RATE": "8", "POSEIDON_RATE_BYTES": "SPONGE_RATE * 4", "PAGE_ADDR_SIZE": "12",
                              "PAGE_SIZE": "1 << PAGE_ADDR_SIZE", "MAX_MEMORY": "0x80000000"}
    assert f["root_page_index"] == "0x81020"
    dev = open(os.path.join(ROOT, "zkm_amd", "csrc", "image_hash.hip")).read()
    assert "MAIN_PAGES = 0x80000u, L1_BASE = 0x80000u, L2_BASE = 0x81000u, ROOT_INDEX = 0x81020u" in dev
    assert "PAGE_WORDS = 1024, PAGE_BLOCKS = 129, REG_WORD = 0x400 / 4, REG_WORDS = 39" in dev
    # 0x80000000 + (q << 5) as page and slot: the L1, L2 and root bases follow from MAX_MEMORY, PAGE_ADDR_SIZE and the 32-byte digest
    hash_page_of = lambda q: (0x80000000 + (q << 5)) >> 12
    assert (hash_page_of(0), hash_page_of(0x7FFFF), hash_page_of(0x80000), hash_page_of(0x80FFF), hash_page_of(0x81000), hash_page_of(0x8101F)) == \
        (0x80000, 0x80FFF, 0x81000, 0x8101F, 0x81020, 0x81020)
    from tests import image_model as IM
    assert (IM.L1_BASE, IM.L2_BASE, IM.ROOT_INDEX, IM.MAIN_PAGES, IM.REGISTERS_OFFSET) == (0x80000, 0x81000, 0x81020, 0x80000, 0x400)
    assert "pub const ROOT_PAGE_INDEX: u32 = 0x81020;" in source()


def test_the_wrapper_names_only_declared_library_items():
    sys_rs = strip_comments(open(os.path.join(ROOT, "integration", "rust", "zkm_hip_sys.rs")).read())
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+)\b", source()))
    assert {"zkm_image_hash", "zkm_image_hash_plan", "zkm_image_pages", "zkm_ctx"} <= used
    assert "pub fn check(rc: c_int, err: *mut c_char)" in sys_rs and "check(rc, err)?" in source()
    assert re.search(r"pub fn split_hashes_hip\(", source()) and re.search(r"pub struct SplitHashes", source())
    # every field of the mirror is set where the wrapper builds it
    fields = re.search(r"pub struct ZkmImagePages\s*\{(.*?)\}", sys_rs, flags=re.S).group(1)
    names = re.findall(r"pub ([a-z_]+):", fields)
    built = re.search(r"zkm_image_pages\s*\{(.*?)\};", source(), flags=re.S).group(1)
    assert sorted(re.findall(r"\b([a-z_]+)(?=:|,|\s*$)", re.sub(r":[^,]*", ":", built))) == sorted(names), built


if __name__ == "__main__":
    ref = sys.argv[1]
    with open(FIXTURE, "w") as fh:
        json.dump({"about": "facts about the reference emulator's Memory, CachedPage, split-time hashing functions and address constants used by "
                            "tests/test_rust_image_hash_names.py; regenerate with `python tests/test_rust_image_hash_names.py <reference checkout>`",
                   "facts": reference_facts(ref)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("facts ->", FIXTURE)
