"""Per-kernel figures of the delivery launches and the receive check from
rocprofv3's csv files (profiles/deliver_time_counters.txt is
this script's output).  The passes, each a run of its own of
tools/prof/deliver_time.py with one window (--rounds 1), the counters never
beside tracing, for S in mtu, zipf and DIR the directory given here:

  rocprofv3 --kernel-trace --stats -d DIR/trace_S -o trace --output-format csv -- \\
      python3 tools/prof/deliver_time.py --shape S --rounds 1
  rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY \\
      -d DIR/pmc1_S -o pmc --output-format csv -- python3 tools/prof/deliver_time.py --shape S --rounds 1
  rocprofv3 --pmc FETCH_SIZE -d DIR/pmc2_S -o pmc --output-format csv -- \\
      python3 tools/prof/deliver_time.py --shape S --rounds 1

  python3 tools/prof/deliver_counters.py DIR > profiles/deliver_time_counters.txt

A line per kernel and pass: the trace pass's kernel_stats row (calls, total,
average, min, max in ns), and per counter the number of launches with the
median, least and greatest value over them (the warm-up launches included;
the records kernel runs in both the records and the grouped call).  The
counters are what rocprofv3 reports, summed over the device; FETCH_SIZE is in
its own unit and is only compared between kernels of the same pass.  Not part
of the product."""
import collections
import csv
import glob
import os
import re
import sys

KEEP = re.compile(r"deliver_\w+?_kernel|rx_verify_kernel")


def main():
    root = sys.argv[1]
    for d in sorted(glob.glob(os.path.join(root, "*"))):
        if not os.path.isdir(d):
            continue
        tag = os.path.basename(d)
        for f in sorted(glob.glob(os.path.join(d, "**", "*.csv"), recursive=True)):
            with open(f, newline="") as fh:
                rows = list(csv.DictReader(fh))
            if not rows:
                continue
            if "kernel_stats" in os.path.basename(f):
                for r in rows:
                    m = KEEP.search(r.get("Name", ""))
                    if m:
                        print(tag, "stats", m.group(0), {k: v for k, v in r.items() if k != "Name"})
            elif "counter_collection" in os.path.basename(f):
                acc = collections.defaultdict(list)
                for r in rows:
                    m = KEEP.search(r.get("Kernel_Name", ""))
                    if m:
                        acc[m.group(0), r["Counter_Name"]].append(float(r["Counter_Value"]))
                for (k, c), v in sorted(acc.items()):
                    v.sort()
                    print(tag, "pmc", k, c, "n", len(v), "median", v[len(v) // 2], "min", v[0], "max", v[-1])


if __name__ == "__main__":
    main()
