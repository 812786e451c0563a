#!/usr/bin/env python3
"""tools/fri_single_path_compare.py -- the single FRI calls before and after they became the stacked bodies at one member.
Takes the result files of tools/fri_stack_time.py runs in the order they were made -- parent, new, parent, new (ZKM_HIP_LIB pointing at a
build of the parent commit, then at this tree's), once per height (LOG_N) -- and compares the "single" arms: eight fri_prove calls (at
6 and at 28 queries) and eight from_values / from_coeffs constructors.  The tolerance is the session's own noise floor, the difference
between the two parent medians of an arm; an arm holds when neither new median exceeds the larger parent median plus that difference.
Usage: fri_single_path_compare.py OUT.json P1.json N1.json P2.json N2.json [P1 N1 P2 N2 of the next height ...]"""
import json
import sys


def single_arms(r):
    arms = {"fri_prove_x8, %d queries" % p["num_queries"]: p["fri_prove_x8"] for p in r["prove"]}
    arms.update({"%s single_x8" % what: c["single_x8"] for what, c in r["commit"].items()})
    return arms


def main():
    out_path, paths = sys.argv[1], sys.argv[2:]
    assert paths and len(paths) % 4 == 0, __doc__
    out = {"about": "tools/fri_single_path_compare.py: the single arms of tools/fri_stack_time.py on a build of the parent commit (P) and on this "
                    "tree's (N), runs interleaved P N P N on one card; bound = larger parent median + |difference of the parent medians|",
           "heights": [], "all_hold": True}
    for i in range(0, len(paths), 4):
        runs = [json.load(open(p)) for p in paths[i:i + 4]]
        assert len({r["log_n"] for r in runs}) == 1, "four runs of one height"
        arms = [single_arms(r) for r in runs]
        cmp = {}
        for name in arms[0]:
            p1, n1, p2, n2 = (a[name]["ms"]["median_ms"] for a in arms)
            noise = abs(p1 - p2)
            bound = max(p1, p2) + noise
            cmp[name] = {"parent_medians_ms": [p1, p2], "new_medians_ms": [n1, n2], "noise_floor_ms": round(noise, 3), "bound_ms": round(bound, 3),
                         "host_waits": {"parent": arms[0][name]["host_waits"], "new": arms[1][name]["host_waits"]},
                         "launch_scopes": {"parent": arms[0][name]["launch_scopes"], "new": arms[1][name]["launch_scopes"]},
                         "holds": bool(max(n1, n2) <= bound)}
            out["all_hold"] = out["all_hold"] and cmp[name]["holds"]
        out["heights"].append({"log_n": runs[0]["log_n"], "reps": runs[0]["reps"], "comparison": cmp,
                               "runs": dict(zip(("parent_1", "new_1", "parent_2", "new_2"), runs))})
    text = json.dumps(out, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(json.dumps({"all_hold": out["all_hold"], "heights": [{"log_n": h["log_n"], "comparison": h["comparison"]} for h in out["heights"]]}, indent=1))


if __name__ == "__main__":
    main()
