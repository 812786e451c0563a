"""The items integration/rust/calls_hip.rs relies on exist as it uses them: the four recorders' logs with the fields and methods it reads,
the two helpers of segment_hip.rs, every field of the header's struct zkm_segment_calls in its initialiser, and the library items it
names in the extern block.  The four recorders point a caller with several kinds at it.  With ZKM_REFERENCE_ROOT naming a checkout of the
reference, the hook points its head comment names (GenerationState, Traces::clock) are looked up there; without one that test is
skipped."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, fn_arity, item_visibility, strip_comments, struct_fields  # noqa: E402

RUST = os.path.join(ROOT, "integration", "rust")
RECORDERS = ("sha_calls_hip.rs", "keccak_calls_hip.rs", "io_calls_hip.rs", "insn_rows_hip.rs")


def read(name):
    return open(os.path.join(RUST, name)).read()


def source():
    return strip_comments(read("calls_hip.rs"))


def test_every_crate_import_is_a_visible_item_of_a_sibling_file():
    imports = crate_imports(source())
    assert {item for _, item in imports} == {"StepLog", "InsnRowLog", "IoCallLog", "KeccakCallLog", "ShaCallLog", "size_then_prove", "SegmentProofs"}
    for path, item in imports:
        assert len(path) == 1, path
        assert item_visibility(strip_comments(read(path[0] + ".rs")), item) in ("pub", "pub(crate)"), (path, item)


def test_the_logs_have_the_fields_and_methods_read():
    src = source()
    logs = {"sha": ("sha_calls_hip.rs", "ShaCallLog"), "keccak": ("keccak_calls_hip.rs", "KeccakCallLog"), "io": ("io_calls_hip.rs", "IoCallLog"),
            "insns": ("insn_rows_hip.rs", "InsnRowLog"), "steps": ("cpu_steps_hip.rs", "StepLog")}
    seen = 0
    for var, (file, name) in logs.items():
        text = strip_comments(read(file))
        fields = struct_fields(text, name)
        body = text[text.index("impl %s" % name):]
        for member, call in re.findall(r"(?<![.\w])%s\.([a-z_0-9]+)(\()?" % var, src):
            if call:
                assert fn_arity(body, member) == 0, (name, member)
            else:
                assert fields[member][0] == "pub", (name, member)
            seen += 1
    assert seen >= 20
    assert fn_arity(strip_comments(read("segment_hip.rs")), "size_then_prove") == 4


def test_the_initialiser_names_every_field_of_the_headers_struct():
    import zkm_amd
    literal = re.search(r"let raw = ZkmSegmentCalls \{(.*?)\};", source(), flags=re.S).group(1)
    named = re.findall(r"(?:^|,)\s*([a-z_0-9]+)(?=\s*[:,]|\s*$)", literal)
    assert named == zkm_amd.abi.tagged()["zkm_segment_calls"]
    mirror = struct_fields(strip_comments(read("zkm_hip_sys.rs")), "ZkmSegmentCalls")
    assert list(mirror) == named and all(v[0] == "pub" for v in mirror.values())
    counts = re.search(r"pub struct CallsCounts \{(.*?)\}", source(), flags=re.S).group(1)
    assert tuple(re.findall(r"pub ([a-z_]+): usize", counts)) == zkm_amd.CALLS_COUNTS


def test_it_names_the_new_entry_points_and_the_recorders_point_at_it():
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+)\b", source()))
    assert {"zkm_segment_calls_steps", "zkm_segments_calls_expand", "zkm_expanded_calls_get", "zkm_expanded_calls_free", "zkm_segments_tables_calls",
            "zkm_prove_segments_ops_calls"} <= used
    assert "pub fn prove_segments_ops_calls_raw(" in source() and "pub fn prove_segments_ops_steps_raw(" in read("cpu_steps_hip.rs")
    for file in RECORDERS:
        head = read(file).split("\nuse ")[0]
        assert "calls_hip.rs" in head and "zkm_prove_segments_ops_calls" in head and "Context.calls_expand" not in head, file


@pytest.mark.skipif(not os.environ.get("ZKM_REFERENCE_ROOT"), reason="needs a checkout of the reference (ZKM_REFERENCE_ROOT)")
def test_the_hook_points_of_the_head_comment_exist_in_the_reference():
    root = os.environ["ZKM_REFERENCE_ROOT"]
    state = strip_comments(open(os.path.join(root, "prover/src/generation/state.rs")).read())
    traces = strip_comments(open(os.path.join(root, "prover/src/witness/traces.rs")).read())
    assert item_visibility(state, "GenerationState") in ("pub", "pub(crate)")
    assert "traces" in struct_fields(state, "GenerationState")
    assert re.search(r"pub fn clock\(&self\)", traces)
    head = read("calls_hip.rs").split("\nuse ")[0]
    assert "GenerationState" in head and "Traces" in head
