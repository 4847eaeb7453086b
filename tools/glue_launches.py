"""Compute-queue launches of the training step that do no work on the model, from a rocprofv3 kernel trace (rocpd sqlite) of
bench.py: ATen element-wise / reduce / fill kernels, runtime copies and fills (`__amd_rocclr_*`), and the GEMM instantiations with
a k-strided B operand (`gemm_bf16_kernel<., true, ...>`).  Steps are delimited by the gradient-norm kernel, as in
stream_analysis.py; the compute queue is the one with the most kernel time.   Usage: glue_launches.py <db> [nsteps]"""
import re
import sqlite3
import sys

db = sys.argv[1]
nsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 12
c = sqlite3.connect(db)
cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
qcol = next((k for k in ("queue_id", "stream_id", "queue", "stream") if k in cols), None)
if qcol is None:
    sys.exit("no queue / stream column in this trace")
rows = c.execute(f"select start, end, name, {qcol} from kernels order by start").fetchall()
marks = [r for r in rows if "sumsq_kernel" in r[2]]
nsteps = min(nsteps, len(marks) - 1)
t0, t1 = marks[-nsteps - 1][1], marks[-1][1]
sel = [r for r in rows if r[0] >= t0 and r[1] <= t1]
busy = {}
for s, e, n, q in sel:
    busy[q] = busy.get(q, 0) + e - s
main = max(busy, key=busy.get)
KSTRIDED = re.compile(r"gemm_bf16_kernel<\w+, ?true")


def kind(name):
    if "__amd_rocclr" in name:
        return "runtime"
    if "at::" in name or "at_cuda_detail" in name or "rocprim" in name:
        return "aten"
    if KSTRIDED.search(name):
        return "gemm-kstrided-B"
    return None


print(f"{db}: {nsteps} steps, wall {(t1 - t0) / nsteps / 1e6:.3f} ms per step; queues by kernel time per step:")
for q in sorted(busy, key=lambda q: -busy[q]):
    ks = [r for r in sel if r[3] == q]
    glue = [r for r in ks if kind(r[2]) in ("runtime", "aten")]
    print(f"  {qcol} {q}: {len(ks) / nsteps:7.1f} launches, {busy[q] / nsteps / 1e6:7.3f} ms; glue (ATen + runtime) "
          f"{len(glue) / nsteps:6.1f} launches, {sum(e - s for s, e, _, _ in glue) / nsteps / 1e6:6.3f} ms{'   <- compute queue' if q == main else ''}")
# the vocabulary projection's data gradient: the first GEMM on the compute queue behind the loss gradient (ctc_grad_kernel)
mainq = [r for r in sel if r[3] == main]
vg = {}
for i, (s, e, n, _) in enumerate(mainq):
    if "ctc_grad_kernel" in n:
        nxt = next((r for r in mainq[i + 1:i + 12] if "gemm" in r[2]), None)
        if nxt is not None:
            vg.setdefault(nxt[2], []).append(nxt[1] - nxt[0])
for n, d in vg.items():
    print(f"vocabulary data gradient: {len(d)} launches, avg {sum(d) / len(d) / 1e3:.2f} us, min {min(d) / 1e3:.2f}, max {max(d) / 1e3:.2f}  {n[:110]}")
for q in sorted(busy, key=lambda q: -busy[q]):
    groups = {}
    for s, e, n, qq in sel:
        k = kind(n)
        if qq != q or k is None:
            continue
        g = groups.setdefault((k, n), [0, 0, 0])
        g[0] += 1
        g[1] += e - s
        g[2] = max(g[2], e - s)
    if not groups:
        continue
    print(f"\n{qcol} {q}{' (compute queue)' if q == main else ''}: launches/step  us/step  avg_us  max_us  kind  kernel")
    for (k, n), (cnt, tot, mx) in sorted(groups.items(), key=lambda kv: (kv[0][0], -kv[1][1])):
        print(f"  {cnt / nsteps:6.2f} {tot / nsteps / 1e3:8.2f} {tot / cnt / 1e3:7.2f} {mx / 1e3:7.2f}  {k:15s} {n[:150]}")
    for k in ("aten", "runtime", "gemm-kstrided-B"):
        sub = [v for (kk, _), v in groups.items() if kk == k]
        if sub:
            print(f"  total {k}: {sum(v[0] for v in sub) / nsteps:.1f} launches, {sum(v[1] for v in sub) / nsteps / 1e3:.1f} us per step")
