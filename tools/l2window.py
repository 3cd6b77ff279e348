"""level-2 window of the last frames of a rocprofv3 --kernel-trace database: python l2window.py x.db out.txt"""
import sqlite3, sys
c = sqlite3.connect(sys.argv[1])
cols = [r[1] for r in c.execute("pragma table_info(kernels)").fetchall()]
out = open(sys.argv[2], "w")
print("columns", cols, file=out)
qcol = "queue" if "queue" in cols else ("queue_id" if "queue_id" in cols else "stream")
rows = c.execute(f"select name, stream, {qcol}, start, end from kernels order by start").fetchall()
scans = [r[3] for r in rows if "job_scan" in r[0]]
for fi in (-2, -1):
    t0 = scans[fi]
    t1 = scans[fi + 1] if fi != -1 else 1e30
    fr = [r for r in rows if t0 <= r[3] < t1]
    print(f"=== frame {fi}: {(max(r[4] for r in fr) - t0) / 1e6:.2f} ms, {len(fr)} kernels", file=out)
    short = lambda n: n.split("(")[0].replace("rhccq::", "").replace("void ", "")[:40]
    # level-2 window: behind the last level-1 assignment (mbk_assign_grid of the big problems ends level 1; take t > 100 ms of a 4K frame, else everything)
    lim = 100e6 if (max(r[4] for r in fr) - t0) > 120e6 else 0
    by = {}
    for n, s, q, a, b in fr:
        if a - t0 < lim: continue
        by.setdefault((s, q), []).append((short(n), (a - t0) / 1e3, (b - a) / 1e3))
    for key, ev in sorted(by.items(), key=lambda kv: str(kv[0])):
        print(f"  stream {key[0]} queue {key[1]}: {len(ev)} kernels, {ev[0][1] / 1e3:.2f}..{(ev[-1][1] + ev[-1][2]) / 1e3:.2f} ms", file=out)
        names = {}
        for n, a, d in ev: names.setdefault(n, []).append((a, d))
        for n, l in sorted(names.items(), key=lambda kv: kv[1][0][0]):
            per = (l[-1][0] - l[0][0]) / (len(l) - 1) if len(l) > 1 else 0.0
            print(f"      {n:40s} x{len(l):5d} first {l[0][0] / 1e3:8.3f} ms last {l[-1][0] / 1e3:8.3f} ms  mean {sum(d for _, d in l) / len(l):8.2f} us  max {max(d for _, d in l):8.2f}  period {per:7.2f} us", file=out)
    if fi == -1:
        print("--- every kernel of the window, last frame: t_ms dur_us stream queue name", file=out)
        for n, s, q, a, b in fr:
            if a - t0 >= lim: print(f"{(a - t0) / 1e6:9.4f} {(b - a) / 1e3:8.2f} {s} {q} {short(n)}", file=out)
out.close()
print(open(sys.argv[2]).read()[:6000])
