"""k_dct_sym / k_cg_step dispatches of a rocprofv3 --kernel-trace directory by kernel, grid (workgroups) and workgroup size:
count, median, mean and total.  `python profiles/tools/trace_dct.py DIR`"""
import sys, glob, csv, statistics as st, collections
d = sys.argv[1]
g = collections.defaultdict(list); tot = 0.0
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        tot += dur
        n = r["Kernel_Name"]
        if "k_dct_sym" in n or "k_cg_step" in n:
            n = n.split("(")[0].replace("void ", "")
            key = (n, tuple(int(r["Grid_Size_" + a]) // max(int(r["Workgroup_Size_" + a]), 1) for a in "XYZ"), int(r["Workgroup_Size_X"]))
            g[key].append(dur)
print(d, "all kernels %.1f ms" % (tot / 1e3))
for k, v in sorted(g.items()):
    print("  %-28s grid %-12s wg %4d  n %6d  median %6.2f us  mean %6.2f us  total %8.2f ms" % (k[0], k[1], k[2], len(v), st.median(v), st.mean(v), sum(v) / 1e3))
