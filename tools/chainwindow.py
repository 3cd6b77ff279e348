"""diagnostic: who runs beside the frame's chain launch.  Per frame of a rocprofv3 --kernel-trace database of tools/nativeframe.py: the chain launch (stream, hardware queue,
start, end), per stream and queue the first / last kernel, the step kernels and the assignment, and behind 60 ms the kernels that end a class's level 1 (cluster_sums, remap)
and start level 2 / level 3 (mt_uniforms, eps_components):  python tools/chainwindow.py x.db"""
import sqlite3, sys
c = sqlite3.connect(sys.argv[1])
cols = [r[1] for r in c.execute("pragma table_info(kernels)").fetchall()]
qcol = "queue" if "queue" in cols else ("queue_id" if "queue_id" in cols else "stream")
rows = c.execute(f"select name, stream, {qcol}, start, end from kernels order by start").fetchall()
scans = [r[3] for r in rows if "job_scan" in r[0]]
short = lambda n: n.split("(")[0].replace("rhccq::", "").replace("void ", "")[:36]
for fi in range(len(scans)):
    t0 = scans[fi]; t1 = scans[fi + 1] if fi + 1 < len(scans) else 1e30
    fr = [r for r in rows if t0 <= r[3] < t1]
    end = max(r[4] for r in fr)
    print(f"=== frame {fi}: {(end - t0) / 1e6:.2f} ms, {len(fr)} kernels")
    for n, s, q, a, b in fr:
        if "mbk_init3" in n and (b - a) > 20e6:
            print(f"  chain launch: stream {s} queue {q}: {(a - t0) / 1e6:.3f} .. {(b - t0) / 1e6:.3f} ms = {(b - a) / 1e6:.3f} ms")
    by = {}
    for n, s, q, a, b in fr: by.setdefault((s, q), []).append((short(n), (a - t0) / 1e6, (b - t0) / 1e6))
    for key, ev in sorted(by.items(), key=lambda kv: kv[1][0][1]):
        st = [e for e in ev if e[0].startswith(("mbk_update", "mbk_pipe", "mbk_batch_estep", "mbk_fold", "mbk_fix", "mbk_draw0"))]
        asg = [e for e in ev if e[0].startswith("mbk_assign")]
        line = f"  stream {key[0]} queue {key[1]}: {len(ev)} kernels {ev[0][1]:.3f}..{ev[-1][2]:.3f} ms"
        if st: line += f"; steps {st[0][1]:.3f}..{st[-1][2]:.3f} ({len(st)})"
        if asg: line += f"; assign {asg[0][1]:.3f}..{asg[-1][2]:.3f}"
        print(line)
    # kernels between 60 and 125 ms that are not steps: who runs when (merge / first positions / level-2 set-up)
    for n, s, q, a, b in fr:
        sn = short(n)
        if 60e6 < a - t0 and sn.startswith(("job_index_entries", "mbk_order", "mt_uniforms", "cluster_sums", "remap", "eps_")):
            print(f"    {(a - t0) / 1e6:9.3f} ms {(b - a) / 1e3:8.1f} us stream {s} queue {q} {sn}")
