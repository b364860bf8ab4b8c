# the headline line of bench.py with the three placements of its resident arrays, interleaved in ONE call
# (--full: each line also carries the live memory floor of its run); the lines go to $OUT [$TMPDIR/placement_ab]
set -e
O=${OUT:-${TMPDIR:-/tmp}/placement_ab}
mkdir -p $O
for i in 1 2 3; do
  for pl in torch plain tuned; do
    python bench.py --full --no-cpu-baseline --no-secondary --steps 100 --placement $pl "$@" 2>$O/err_${pl}_$i.log | tail -1 > $O/${pl}_$i.json
  done
done
python - "$O" <<'PY'
import json, os, sys
o = sys.argv[1]
for pl in ("torch","plain","tuned"):
    r=[json.load(open(os.path.join(o, "%s_%d.json"%(pl,i)))) for i in (1,2,3)]
    print("%-6s"%pl," ".join("%.4f (min %.4f, frac %.3f)"%(d["ms_per_step"],d["roofline"]["kernel_ms_min"],d["roofline"]["frac"]) for d in r), " floors", " ".join("%.3f"%d["roofline"]["mixed_read_write_floor"]["ms"] for d in r))
print(json.load(open(os.path.join(o, "tuned_1.json")))["config"]["placement"])
PY
