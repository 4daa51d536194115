"""Per-kernel summary of a rocprofv3 --kernel-trace results DB (rocpd sqlite): calls, median, min, mean and max in
microseconds (the averages hide single slow calls).  Optional further arguments: substrings, only kernels whose name
holds one of them are listed."""
import sqlite3, statistics, sys
db = sqlite3.connect(sys.argv[1])
cur = db.cursor()
only = sys.argv[2:]
tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
kd = [t for t in tabs if 'kernel_dispatch' in t][0]
ks = [t for t in tabs if 'kernel_symbol' in t][0]
q = f"select s.kernel_name, (d.end-d.start)/1000.0 from {kd} d join {ks} s on d.kernel_id=s.id"
per = {}
for name, us in cur.execute(q):
    per.setdefault(name, []).append(us)
for name, v in sorted(per.items(), key=lambda kv: -statistics.mean(kv[1])):
    short = name.replace("_ZN4rrtx12_GLOBAL__N_1", "").replace("rrtx::(anonymous namespace)::", "").replace("void ", "", 1)
    if only and not any(o in short for o in only):
        continue
    print(f"{short[:60]:60s} calls {len(v):4d}  median {statistics.median(v):8.2f}  min {min(v):8.2f}  "
          f"mean {statistics.mean(v):8.2f}  max {max(v):8.2f}")
