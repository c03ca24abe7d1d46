"""Mean per dispatch of every counter of one kernel in the csv tree of a `rocprofv3 --pmc ... --output-format csv -d DIR` pass.
usage: pmc_kernel_mean.py DIR [kernel name substring = k_tower1wa]"""
import collections
import csv
import glob
import sys

kernel = sys.argv[2] if len(sys.argv) > 2 else "k_tower1wa"
tot, disp = collections.defaultdict(float), collections.defaultdict(set)
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if kernel in r["Kernel_Name"]:
            tot[r["Counter_Name"]] += float(r["Counter_Value"])
            disp[r["Counter_Name"]].add(r["Dispatch_Id"])
for k in sorted(tot):
    print("%s: %d dispatches, mean per dispatch %.1f" % (k, len(disp[k]), tot[k] / max(len(disp[k]), 1)))
