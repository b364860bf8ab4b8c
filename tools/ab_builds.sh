# A/B of two builds of the library on the headline (C3, placed arrays): interleaved pairs in ONE call (same box), one process
# per run.  usage: tools/ab_builds.sh <other libpfmscan.so | other checkout> [out dir]; WIDTHS="12 18" PAIRS=3 STEPS=200 RUN_SECONDS=170
# A library is loaded by THIS tree's bindings (PFMSCAN_LIB), which needs the same PFMSCAN_ABI_VERSION; across an ABI change give the
# other build's CHECKOUT (built: its own rnascan_amd/libpfmscan.so and tools/hbm_mixed): its bench.py then runs from there.
# Every run has its own time limit and keeps its stderr; the first run that fails ends the script (nothing more is started
# on a card that has just faulted).  The table's last line per width holds what a claim needs: both medians of
# roofline.kernel_ms and the other build's own spread.
set -euo pipefail
OTHER=$(readlink -f "$1")
O=${2:-build/ab_builds}
mkdir -p $O
for w in ${WIDTHS:-12 18}; do
 for i in $(seq 1 ${PAIRS:-3}); do
  if [ -d "$OTHER" ]; then
   (cd "$OTHER" && timeout -k 10 ${RUN_SECONDS:-170} python bench.py --gpus 1 --steps ${STEPS:-200} --warmup 3 --width $w) 2>$O/other_w${w}_$i.err | tail -1 > $O/other_w${w}_$i.json
  else
   PFMSCAN_LIB=$OTHER timeout -k 10 ${RUN_SECONDS:-170} python bench.py --gpus 1 --steps ${STEPS:-200} --warmup 3 --width $w 2>$O/other_w${w}_$i.err | tail -1 > $O/other_w${w}_$i.json
  fi
  timeout -k 10 ${RUN_SECONDS:-170} python bench.py --gpus 1 --steps ${STEPS:-200} --warmup 3 --width $w 2>$O/this_w${w}_$i.err | tail -1 > $O/this_w${w}_$i.json
 done
done
O=$O python - <<'PY' | tee $O/ab_other_vs_this.txt
import json, os, statistics as st
O = os.environ["O"]
n = int(os.environ.get("PAIRS", "3"))
for w in [int(x) for x in os.environ.get("WIDTHS", "12 18").split()]:
    ms = {k: [json.load(open("%s/%s_w%d_%d.json" % (O, k, w, i)))["roofline"]["kernel_ms"] for i in range(1, n + 1)] for k in ("other", "this")}
    for i in range(n):
        print("w=%2d pair %d  other %.4f  this %.4f" % (w, i + 1, ms["other"][i], ms["this"][i]))
    a, b = st.median(ms["other"]), st.median(ms["this"])
    print("w=%2d median other %.4f  this %.4f  gain %.4f ms (%.2f %%)  other's spread (max - min) %.4f" %
          (w, a, b, a - b, 100 * (a - b) / a, max(ms["other"]) - min(ms["other"])))
PY
