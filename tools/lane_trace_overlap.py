"""Developer tool: reads the kernel trace of a `rocprofv3 --kernel-trace --output-format csv` run and says, for the last
launches of the four-slot search kernel, how launch i+1's begin lies against launch i's end: a positive gap is idle time
between two launches, a negative one is overlap.
    python tools/lane_trace_overlap.py DIR [last N launches] [skip M at the end]"""
import csv
import glob
import os
import sys

out_dir = sys.argv[1]
last = int(sys.argv[2]) if len(sys.argv) > 2 else 100
rows = []
for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(path)):
        if "tls_slim_kernel" in r.get("Kernel_Name", ""):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
rows.sort()
skip = int(sys.argv[3]) if len(sys.argv) > 3 else 0   # launches at the end of the trace to leave out
rows = rows[len(rows) - skip - last:len(rows) - skip]
if len(rows) < 2:
    sys.exit("no launches of tls_slim_kernel in %s" % out_dir)
gaps = sorted(rows[i + 1][0] - rows[i][1] for i in range(len(rows) - 1))
dur = sorted(e - s for s, e in rows)
span = rows[-1][1] - rows[0][0]
print("%d launches: duration median %.2f us (min %.2f, max %.2f); begin(i+1) - end(i): median %.2f us, min %.2f, max %.2f; "
      "%d of %d begin before the previous one ends; span per launch %.2f us"
      % (len(rows), dur[len(dur) // 2] / 1e3, dur[0] / 1e3, dur[-1] / 1e3, gaps[len(gaps) // 2] / 1e3, gaps[0] / 1e3,
         gaps[-1] / 1e3, sum(1 for g in gaps if g < 0), len(gaps), span / 1e3 / len(rows)))
