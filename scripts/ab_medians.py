#!/usr/bin/env python3
"""Table of medians of an alternating parent / branch run of the operation benchmarks (developer tool).

    python scripts/ab_medians.py DIR --condense ab_bench.jsonl     the four runs of every script, one line per row
                                     [--scripts add,extract,dense]  (of these scripts only)
    python scripts/ab_medians.py ab_bench.jsonl                    the table

DIR holds bench_<script>_<parent1|branch1|parent2|branch2>.jsonl, the JSON lines of scripts/bench_<script>.py run from two
checkouts in that order.  Counts and check fields of a row must be equal in its four runs; a condensed line keeps the row's
keys, the parent's ms and ms_all and the branch's ms; the rows of a baseline (torch, another operation) are other code
and are left out.  The table has, for every row, the four medians, the bound -- what the parent disagrees with itself by:
the larger of the gap between its two medians and the largest max - min of ms_all in one of its runs -- and BEYOND where
a median of the branch exceeds the parent's larger one by more than the bound."""
import json
import os
import sys

SCRIPTS = ("select", "reduce", "emult", "extract", "add", "dense")
RUNS = ("parent1", "branch1", "parent2", "branch2")
KEYS = ("workload", "op", "form", "impl", "mode", "nrhs")
SAME = ("tuples_in", "tuples_out", "same_tuples", "same_bits", "nnz_P", "nnz_PtAP", "rows_light", "rows_mid", "rows_heavy", "tuples", "rows")
OURS = ("spsamd_", "emult_path", "extract")


def condense(d, scripts=SCRIPTS):
    for s in scripts:
        runs = []
        for tag in RUNS:
            rows = [json.loads(ln) for ln in open(os.path.join(d, "bench_%s_%s.jsonl" % (s, tag)))]
            runs.append({tuple((q, r[q]) for q in KEYS if q in r): r for r in rows})
        assert all(list(x) == list(runs[0]) for x in runs), s
        for k in runs[0]:
            four = [x[k] for x in runs]
            r = four[0]
            ours = str(r["impl"]).startswith(OURS) if "impl" in r else not str(r["mode"]).startswith("torch")
            if r.get("ms") is None or not ours:
                continue
            for q in SAME:
                assert all(x.get(q) == four[0].get(q) for x in four), (s, k, q)
            yield {"script": s, **dict(k), **{tag: {"ms": x["ms"], "ms_all": x.get("ms_all", [])} if tag[0] == "p" else x["ms"]
                                            for tag, x in zip(RUNS, four)}}


def main():
    src = sys.argv[1]
    scripts = sys.argv[sys.argv.index("--scripts") + 1].split(",") if "--scripts" in sys.argv else SCRIPTS
    rows = list(condense(src, scripts)) if os.path.isdir(src) else [json.loads(ln) for ln in open(src)]
    if "--condense" in sys.argv:
        with open(sys.argv[sys.argv.index("--condense") + 1], "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
        return
    print("| script | row | parent 1 | parent 2 | branch 1 | branch 2 | bound | max(branch) − max(parent) | |")
    print("|---|---|---|---|---|---|---|---|---|")
    bad = []
    for r in rows:
        name = " ".join(str(r[q]) for q in KEYS if q in r)
        mp, mb = (r["parent1"]["ms"], r["parent2"]["ms"]), (r["branch1"], r["branch2"])
        spread = max((max(x) - min(x) for x in (r["parent1"]["ms_all"], r["parent2"]["ms_all"]) if x), default=0.0)
        bound = max(abs(mp[0] - mp[1]), spread)
        beyond = max(mb) > max(mp) + bound
        if beyond:
            bad.append("%s: %s" % (r["script"], name))
        print("| %s | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %+.3f | %s |" % (
            r["script"], name, *mp, *mb, bound, max(mb) - max(mp), "BEYOND" if beyond else ""))
    print("\nbeyond the bound:", ", ".join(bad) or "none")


if __name__ == "__main__":
    main()
