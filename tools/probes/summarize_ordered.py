"""Summary of tools/probes/pmc_ordered.sh output: the ordered gridder's mean
duration under the kernel trace, every SQ counter as its mean per dispatch,
and the issue model of tools/probes/summarize_seq.py (same measured costs per
wave64 instruction class) -- what the kernel's own instruction stream costs to
issue against how long it ran.

    python tools/probes/summarize_ordered.py OUTDIR \
        [--out profiles/ordered/pmc.json]

The SQ classes count a packed v_pk_fma_f32 as one f32 instruction like a plain
v_fma_f32; the packed share of the f32 class comes from the mirror loop's ISA
listing (--frac-f32-packed): per mirror pair 1 packed phase FMA, 4 packed
multiplies, 8 packed FMAs and 8 packed adds beside the 5 plain f32 ops of
revolutions() -- 21 of 26.
"""
import argparse
import glob
import json
import os
from collections import defaultdict

from summarize_seq import CLOCK_HZ, COST, N_SIMD, rows, to_csv

TAG = "kernel_gridder_ordered_mi355x"


def short(name):
    if TAG not in name:
        return None
    s = name.split(TAG + "<", 1)[1].split(">", 1)[0].strip()
    return "gridder_ordered_" + {"32": "s32", "64": "s64"}.get(s, "generic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--out")
    ap.add_argument("--frac-f32-packed", type=float, default=21 / 26)
    ap.add_argument("--frac-int32-quarter", type=float, default=0.0,
                    help="the loop's int32 ops are xor / compare / select")
    args = ap.parse_args()
    dur = defaultdict(list)
    for db in glob.glob(os.path.join(args.dir, "ktrace", "**", "*.db"),
                        recursive=True):
        for r in rows(to_csv(db, "kernel")):
            k = short(r["Kernel_Name"])
            if k:
                dur[k].append(int(r["End_Timestamp"]) -
                              int(r["Start_Timestamp"]))
    per = defaultdict(lambda: defaultdict(float))
    for db in sorted(glob.glob(os.path.join(args.dir, "p*", "**", "*.db"),
                               recursive=True)):
        for r in rows(to_csv(db, "counter")):
            k = short(r["Kernel_Name"])
            if k:
                per[(k, db, r["Dispatch_Id"])][r["Counter_Name"]] += \
                    float(r["Counter_Value"])
    cnt = defaultdict(lambda: defaultdict(list))
    for (k, _, _), cs in per.items():
        for c, v in cs.items():
            cnt[k][c].append(v)
    out = {}
    for k in sorted(set(dur) | set(cnt)):
        c = {n: sum(v) / len(v) for n, v in cnt[k].items()}
        d = dur.get(k, [])
        e = {"launches": len(d),
             "mean_ms": round(sum(d) / len(d) / 1e6, 4) if d else None,
             "counters": {n: round(v) for n, v in sorted(c.items())}}
        if "SQ_INSTS_VALU" in c and d:
            cvt = c.get("SQ_INSTS_VALU_CVT", 0)
            i32 = c.get("SQ_INSTS_VALU_INT32", 0)
            i64 = c.get("SQ_INSTS_VALU_INT64", 0)
            f32 = sum(c.get(n, 0) for n in ("SQ_INSTS_VALU_FMA_F32",
                                            "SQ_INSTS_VALU_ADD_F32",
                                            "SQ_INSTS_VALU_MUL_F32"))
            trans = c.get("SQ_INSTS_VALU_TRANS_F32", 0)
            other = c["SQ_INSTS_VALU"] - cvt - i32 - i64 - f32 - trans
            q, pk = args.frac_int32_quarter, args.frac_f32_packed
            part = {
                "cvt": cvt * COST["cvt"],
                "int32": i32 * (q * COST["int32_quarter"] +
                                (1 - q) * COST["int32_plain"]),
                "int64": i64 * COST["int64"],
                "f32_packed": f32 * pk * COST["fma_f32_pk"],
                "f32_plain": f32 * (1 - pk) * COST["f32_plain"],
                "trans_f32": trans * COST["trans"],
                "other": max(other, 0) * COST["other"]}
            cyc = sum(part.values())
            t_issue = cyc / N_SIMD / CLOCK_HZ
            e["valu_mix"] = {"cvt": cvt, "int32": i32, "int64": i64,
                             "f32": f32, "trans_f32": trans, "other": other,
                             "total": c["SQ_INSTS_VALU"]}
            e["issue_model"] = {
                "t_issue_ms": round(t_issue * 1e3, 4),
                "frac": round(t_issue / (e["mean_ms"] / 1e3), 4),
                "share_of_issue": {n: round(v / cyc, 4)
                                   for n, v in part.items()},
                "costs": COST, "frac_int32_quarter": q,
                "frac_f32_packed": round(pk, 4)}
        out[k] = e
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
