"""Condenses a rocprofv3 kernel trace of bench.py (rocprofv3 --kernel-trace --output-format csv -d DIR -- python3
bench.py --steps 20 --warmup 5): per-launch averages of the tracking kernels, a window of four launches from the middle
of the open-loop leg, the correlator's cycle, and how far the next batch's table kernels run ahead of the end of the
running correlator.   usage: python tools/trk_overlap.py DIR TAG"""
import csv
import glob
import re
import statistics as st
import sys

d, tag = sys.argv[1], sys.argv[2]
found = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))
if not found:
    sys.exit(f"no *kernel_trace.csv under {d}")
f = found[0]


def short(n):
    m = re.search(r'(\w+_kernel)', n)
    return m.group(1) if m else n[:30]


rows = list(csv.DictReader(open(f)))
ks = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name']), r.get('Queue_Id', '?')) for r in rows)
by = {}
for k in ks:
    by.setdefault(k[2], []).append((k[1] - k[0]) / 1e3)
print(f"== {tag}: per-launch averages (us), n")
for n in sorted(by):
    if n.startswith('trk_'):
        print(f"{n:28s} {st.mean(by[n]):9.2f} {len(by[n]):6d}")
corr = [k for k in ks if k[2].startswith('trk_corr_ps')]
# steady state: the middle of the open-loop leg (launches with ~ the median duration, 32 per step)
mid = len(corr) // 2
win = corr[mid:mid + 4]
t0 = win[0][0]
print(f"== {tag}: window")
for k in ks:
    if k[0] >= t0 - 600e3 and k[0] <= win[-1][1] and k[2].startswith('trk_'):
        print(f"{(k[0]-t0)/1e3:9.1f} -> {(k[1]-t0)/1e3:9.1f} us ({(k[1]-k[0])/1e3:6.1f})  q{k[3]} {k[2]}")
# cycle and overlap over launches mid-200 .. mid+200
lo, hi = max(1, mid - 200), min(len(corr) - 1, mid + 200)
cyc = [(corr[i + 1][0] - corr[i][0]) / 1e3 for i in range(lo, hi)]
gap = [(corr[i + 1][0] - corr[i][1]) / 1e3 for i in range(lo, hi)]
print(f"== {tag}: corr start->start median {st.median(cyc):.1f} us, corr end -> next corr start median {st.median(gap):.1f} us")
exp = [k for k in ks if k[2].startswith('trk_expand')]
edg = [k for k in ks if k[2].startswith('trk_edges')]
pln = [k for k in ks if k[2].startswith('trk_plan4')]
# for each correlator in the range: the first expand that starts after this correlator started (the next batch's)
lead, elead = [], []
for i in range(lo, hi):
    c = corr[i]
    nx = [e for e in exp if e[0] > c[0] and e[0] < corr[i + 1][0]]
    if nx:
        lead.append((c[1] - nx[0][0]) / 1e3)
    ne = [e for e in edg if e[0] > c[0] and e[0] < corr[i + 1][0]]
    if ne:
        elead.append((c[1] - ne[0][1]) / 1e3)
if lead:
    print(f"== {tag}: next batch's trk_expand starts before this trk_corr_ps ends by median {st.median(lead):.1f} us "
          f"(min {min(lead):.1f}, max {max(lead):.1f}; negative = after), n {len(lead)}")
if elead:
    print(f"== {tag}: next batch's trk_edges ends before this trk_corr_ps ends by median {st.median(elead):.1f} us")
pc = [(pln[i + 1][0] - pln[i][1]) / 1e3 for i in range(len(pln) // 2 - 200, len(pln) // 2 + 200) if 0 <= i < len(pln) - 1]
if pc:
    print(f"== {tag}: trk_plan4 end -> next start median {st.median(pc):.1f} us")
