"""Leg overlap of the last hsrans_encode_host_pipelined call in a rocprofv3 --kernel-trace --memory-copy-trace --output-format csv run
(profiles/r09_host_encode_overlap.txt): each leg's busy time and how much of it overlaps the others.
Run: python tools/trace_overlap.py <trace dir> <slices of the call>.  Upload = the host-to-device copies, download = the runtime's copy kernels (__amd_rocclr_copyBuffer: device to
page-locked host), encode = the library's kernels."""
import csv
import glob
import sys

d, n_slices = sys.argv[1], int(sys.argv[2])
kt = [r for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True) for r in csv.DictReader(open(f))]
ct = [r for f in glob.glob(f"{d}/**/*memory_copy_trace.csv", recursive=True) for r in csv.DictReader(open(f))]
iv = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
up = sorted(iv(r) for r in ct if "HOST_TO_DEVICE" in r["Direction"])[-n_slices:]
t0 = up[0][0]
down = sorted(iv(r) for r in kt if "copyBuffer" in r["Kernel_Name"] and iv(r)[0] >= t0) + sorted(iv(r) for r in ct if "DEVICE_TO_HOST" in r["Direction"] and iv(r)[0] >= t0)
enc = sorted(iv(r) for r in kt if "hsrans" in r["Kernel_Name"] and iv(r)[0] >= t0)
t1 = max(e for _, e in up + down + enc)


def union(v):
    tot, cur = 0, None
    for s, e in sorted(v):
        if cur is None or s > cur[1]:
            tot += cur[1] - cur[0] if cur else 0
            cur = [s, e]
        else:
            cur[1] = max(cur[1], e)
    return tot + (cur[1] - cur[0] if cur else 0)


ms = lambda ns: f"{ns / 1e6:.2f} ms"
legs = {"upload (H2D copies)": up, "encode (library kernels)": enc, "download (copy kernels, D2H)": down}
print(f"last pipelined call, {n_slices} slices: {ms(t1 - t0)} from its first upload's start to its last operation's end")
for k, v in legs.items():
    print(f"  {k:30s} {len(v):4d} ops, busy {ms(union(v))}")
names = list(legs)
for i in range(3):
    for j in range(i + 1, 3):
        a, b = legs[names[i]], legs[names[j]]
        print(f"  overlap of {names[i]} and {names[j]}: {ms(union(a) + union(b) - union(a + b))}")
print(f"  sum of the three legs' busy times {ms(sum(union(v) for v in legs.values()))} against {ms(t1 - t0)} wall")
