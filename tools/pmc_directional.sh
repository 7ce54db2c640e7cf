#!/bin/bash
# Run ON THE GPU BOX: what bounds the directional-light pass?  SQ issue / wait counters and the texture path's busy counters of
# directional_lights_kernel beside sphere_lights_kernel over the same two fields (tools/directional_time.py --launches), each group in a
# pass of its own, counters with the kernel trace only.  tools/pmc_directional.sh [output directory]  ->  <output directory>/summary.txt
# (default: build/pmc_directional, which git ignores)
set -u
cd "$(cd "$(dirname "$0")/.." && pwd)"
export TMPDIR=/tmp
OUT=${1:-build/pmc_directional}
rm -rf "$OUT"; mkdir -p "$OUT"
CMD="python tools/directional_time.py --launches 3"
i=0
while read -r pass; do
  [ -z "$pass" ] && continue
  i=$((i + 1))
  timeout -k 10 170 rocprofv3 --kernel-trace --output-format csv --pmc $pass -d "$OUT/p$i" -o pmc -- $CMD > "$OUT/p$i.out" 2> "$OUT/p$i.log"
  rc=$?
  if [ $rc -ne 0 ]; then echo "pass $i ($pass) ended with status $rc: stopping" >> "$OUT/errors.txt"; break; fi
done <<'PASSES'
GRBM_GUI_ACTIVE SQ_WAVES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VMEM SQ_INSTS_SALU
SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INST_LEVEL_VMEM SQ_INSTS_SMEM
TA_TA_BUSY_sum TA_BUSY_avr TD_TD_BUSY_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCC_HIT_sum TCC_MISS_sum
PASSES
python - "$OUT" <<'PY' > "$OUT/summary.txt"
import csv, glob, sys, collections
acc = collections.defaultdict(lambda: collections.defaultdict(list))
dur = collections.defaultdict(list)
def key(r):
    # the two frames launch different grids: told apart by the grid size
    return "%s  grid %s" % (r["Kernel_Name"], r.get("Grid_Size", r.get("Grid_Size_X", "?")))
for f in glob.glob(sys.argv[1] + "/p*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "sphere_lights_kernel" not in r["Kernel_Name"] and "directional_lights_kernel" not in r["Kernel_Name"]: continue
        acc[key(r)][r["Counter_Name"]].append(float(r["Counter_Value"]))
for f in glob.glob(sys.argv[1] + "/p1/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if key(r) in acc: dur[key(r)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for k, cs in sorted(acc.items()):
    print(k)
    if dur[k]: print("   launches %d  avg %.1f us (under the first counter pass)" % (len(dur[k]), sum(dur[k]) / len(dur[k])))
    for n, v in sorted(cs.items()):
        print("   %-40s %16.1f  (n=%d)" % (n, sum(v) / len(v), len(v)))
PY
cat "$OUT/errors.txt" 2>/dev/null
cat "$OUT/summary.txt"
