#!/usr/bin/env python
"""Build profiles/rNN_pmc_traffic.json from two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE) of bench.py.

usage: make_traffic_json.py <fetch counter_collection.csv> <write counter_collection.csv> <frames_per_step> [commit] > profiles/r06_pmc_traffic.json
Bytes per launch = FETCH_SIZE*f + WRITE_SIZE (KB -> bytes); f = 2 for kernels whose reads are 16 B/lane streams (gfx950's
FETCH_SIZE counts 64 B per 128-B request, MI355X_MICROARCH.md §HBM), 1 otherwise (uncalibrated).  Launches of one bench
"kernel" (prof name) are summed: k_level(fused) = all k_level<R,mode> launches of a step, etc.

Kernels are matched by BASE NAME (the function's name without namespace, template arguments and parameters), never by template
text: a new template parameter must not drop a kernel out of its group or out of the wide-load list (k_triy_chns's reads were
reported at half their size that way, twice).  A dispatch of one of this library's kernels (acfhip::) that matches no group is an
error: the file is still printed, the names go to stderr and the exit status is 1.
"""
import collections
import csv
import json
import re
import sys

# base-name prefixes whose reads are 16-byte-per-lane streams (k_cascade_tile3 / tileD, k_smooth_grad / _grad_tri, ...)
WIDE = ("k_cascade_tile", "k_cascade_tail3", "k_grad_mag_vec", "k_tri_x5v", "k_chns", "k_resample_half", "k_resample_strip", "k_smooth_vec",
        "k_smooth_grad", "k_tail_scan")
# ... and k_triy_chns<MAXO, UT, ..> where UT (M, O and U or the checkpoints' M tile in blocks: 16-byte loads per lane) is set
WIDE_IF_ARG = {"k_triy_chns": (1, "true")}
# (base-name prefix, group), first match wins
GROUP = [("k_cascade_tile", "k_cascade_tile"), ("k_cascade_tail", "k_cascade_tail3"), ("k_tail_scan", "k_tail_scan"), ("k_level", "k_level(fused)"),
         ("k_triy_chns", "k_triy_chns"), ("k_sort_map", "k_sort_map"), ("k_nms", "k_nms"), ("k_export", "k_export"),
         ("k_chns", "k_chns"), ("k_smooth_vec", "k_smooth_vec"), ("k_smooth_grad_tri", "k_smooth_grad_tri"), ("k_smooth_grad", "k_smooth_grad"), ("k_smooth_tri1", "k_smooth_tri1(image)"), ("k_grad_mag", "k_grad_mag"), ("k_tri_x", "k_tri_x"),
         ("k_tri_y", "k_tri_y"), ("k_resample", "k_resample(image)")]


def split_name(kn):
    """(is this library's, base name, template arguments) of a demangled kernel name"""
    s = re.sub(r"^\s*void\s+", "", kn.strip())
    s = re.sub(r"\s*\[clone[^\]]*\]|\.kd$", "", s)
    m = re.match(r"((?:[A-Za-z_]\w*::)*)([A-Za-z_]\w*)\s*(?:<(.*?)>)?\s*(?:\(|$)", s)
    if not m:
        return False, s, []
    args = [a.strip() for a in m.group(3).split(",")] if m.group(3) else []
    return "acfhip::" in m.group(1) or m.group(2).startswith("k_"), m.group(2), args


def is_wide(base, args):
    if base.startswith(WIDE):
        return True
    if base in WIDE_IF_ARG:
        i, v = WIDE_IF_ARG[base]
        return len(args) > i and args[i] == v
    return False


def group_of(base):
    for pat, g in GROUP:
        if base.startswith(pat):
            return g
    return None


def per_dispatch(path, counter):
    d = collections.defaultdict(float)
    name = {}
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] == counter:
            d[r["Dispatch_Id"]] += float(r["Counter_Value"])
            name[r["Dispatch_Id"]] = r["Kernel_Name"]
    return d, name


def main():
    fetch, fn = per_dispatch(sys.argv[1], "FETCH_SIZE")
    write, wn = per_dispatch(sys.argv[2], "WRITE_SIZE")
    frames = int(sys.argv[3])
    commit = sys.argv[4] if len(sys.argv) > 4 else None
    unmatched = collections.Counter()
    foreign = collections.Counter()

    def agg(vals, names, scale_wide):
        tot = collections.defaultdict(float)
        cnt = collections.Counter()
        for k, v in vals.items():
            ours, base, args = split_name(names[k])
            g = group_of(base) if ours else None
            if g is None:
                (unmatched if ours else foreign)[base] += 1
                continue
            f = 2.0 if (scale_wide and is_wide(base, args)) else 1.0
            tot[g] += v * f * 1024.0
            cnt[g] += 1
        return tot, cnt
    ft, fc = agg(fetch, fn, True)
    wt, wc = agg(write, wn, False)
    # number of bench steps seen = launches of the tile kernel
    steps = max(fc.get("k_cascade_tile", 1), 1)
    out = {"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (two counters-only passes of bench.py with one context, no tracing: profiles/triy_replay.md), MI355X",
           "note": __doc__.split("\n\n")[1].strip().replace("\n", " "),
           "frames_per_step": frames,
           "kernels": {g: int((ft.get(g, 0) + wt.get(g, 0)) / steps) for g in sorted(set(ft) | set(wt))}}
    if commit:
        out["commit"] = commit
    out["MB_per_frame"] = {g: round(v / frames / 1e6, 2) for g, v in out["kernels"].items()}
    out["fetch_MB_per_frame"] = {g: round(v / steps / frames / 1e6, 2) for g, v in sorted(ft.items())}  # (after the wide-load correction)
    out["write_MB_per_frame"] = {g: round(v / steps / frames / 1e6, 2) for g, v in sorted(wt.items())}
    out["total_MB_per_frame"] = round(sum(out["MB_per_frame"].values()), 1)
    if foreign:
        out["not_counted"] = {"what": "dispatches of kernels that are not this library's (the framework's copies and fills)", "dispatches": dict(sorted(foreign.items()))}
    print(json.dumps(out, indent=1))
    if unmatched:
        sys.stderr.write("make_traffic_json: kernels of this library in no group (add them to GROUP): %s\n" % dict(sorted(unmatched.items())))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
