"""Reads a `rocprofv3 --kernel-trace` csv of a run of tools/heightfield_probe.py beside the plan that run wrote: the timed batches are the LAST dispatches of each
batch size's part of the trace (the two parts are split at the longest pause, where the second engine is created), in the plan's order; every batch must hold the
kernel its variant names.  Prints, per batch size and variant, the median over the seven batches of the batch's median kernel duration, and the lowest and highest batch.

    python tools/heightfield_trace.py heightfield_probe.json <dir>/*_kernel_trace.csv"""
import csv, json, sys
import numpy as np

plan = [p for p in json.load(open(sys.argv[1]))["plan"] if p["phase"] == "timed"]
rows = []
with open(sys.argv[2]) as fh:
    for r in csv.DictReader(fh):
        name = r["Kernel_Name"]
        if "walk_step_ground_kernel" in name or "walk_step_heightfield_kernel" in name:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "heightfield" in name))
rows.sort()
starts = np.array([r[0] for r in rows])
cut = int(np.argmax(np.diff(starts))) + 1
sizes = sorted({p["n"] for p in plan})
assert len(sizes) == 2
for n, part in zip(sizes, (rows[:cut], rows[cut:])):
    batches = [p for p in plan if p["n"] == n]
    tail = part[-sum(p["launches"] for p in batches):]
    at, out = 0, {}
    for p in batches:
        seg = tail[at:at + p["launches"]]; at += p["launches"]
        assert {s[2] for s in seg} == {p["variant"] != "ground step"}, p
        out.setdefault(p["variant"], []).append(float(np.median([s[1] - s[0] for s in seg])) / 1000.0)
    for v, med in out.items():
        print(f"n {n:6d}  {v:36s} kernel duration {np.median(med):6.2f} us (batches {min(med):6.2f} .. {max(med):6.2f})")
