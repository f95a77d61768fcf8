"""L2 (TCC) hit and miss request counts of the solver kernels from a rocprofv3
--pmc TCC_HIT_sum TCC_MISS_sum CSV, summed per kernel class and averaged over
its dispatches.

Usage: python tools/l2_from_pmc.py COUNTER_CSV [OUT_JSON]
"""
import csv
import json
import re
import sys
from collections import defaultdict

SOLVER = ("k_setup", "k_dir", "k_col", "k_ls", "k_bb", "k_persist")


def main():
    tot = defaultdict(lambda: defaultdict(float))
    disp = defaultdict(set)
    for r in csv.DictReader(open(sys.argv[1])):
        key = next((k for k in SOLVER if re.search(r"bsgp\w*::" + k + r"<", r["Kernel_Name"])), None)
        if key is None:
            continue
        tot[key][r["Counter_Name"]] += float(r["Counter_Value"])
        disp[key].add(r.get("Dispatch_Id") or r.get("Correlation_Id"))
    out = {}
    for k, c in tot.items():
        n = max(1, len(disp[k]))
        hit, miss = c.get("TCC_HIT_sum", 0.0) / n, c.get("TCC_MISS_sum", 0.0) / n
        out[k] = {"tcc_hit_per_launch": hit, "tcc_miss_per_launch": miss,
                  "hit_rate": hit / (hit + miss) if hit + miss else None, "launches": n}
    if len(sys.argv) > 2:
        json.dump(out, open(sys.argv[2], "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
