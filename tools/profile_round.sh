#!/bin/bash
# The round's committed profile set (run on the GPU box): usage: tools/profile_round.sh <tag> <commit> <out dir>
#   <out dir>/<tag>_b_serial_stats.csv / _c_2streams_stats.csv : rocprofv3 --kernel-trace --stats of one / two micro-batches
#                                                                 of two videos (25 / 50 UNet forwards at batch 2)
#   <out dir>/<tag>_a_pmc.txt + <tag>_pmc_traffic.json          : the three --pmc passes folded per kernel
#   <out dir>/<tag>_clock_in_kernel.json                         : shader clock held inside the K loops (experiments build stamps)
#   <out dir>/<tag>_bench.json                                   : the --full bench line (per_template FLOPs)
#   <out dir>/<tag>_per_template.txt                             : fraction of peak per kernel template
set -eu
TAG=${1:?usage: profile_round.sh <tag> <commit> <out dir>}; COMMIT=${2:?usage: profile_round.sh <tag> <commit> <out dir>}
R=${GRAFT_REPO_ROOT:?GRAFT_REPO_ROOT is unset: run this on the GPU box (gpurun exports it)}
OUT=${3:?usage: profile_round.sh <tag> <commit> <out dir> (relative to the repository root)}
mkdir -p "$R/$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/${TAG}_ps" -- python3 "$R/bench.py" --concurrent 1 --steps 2 --warmup 0 --no-cpu-baseline --no-roofline --no-decode --no-batch1-leg > "$R/$OUT/${TAG}_b_serial.json" 2> "$R/$OUT/${TAG}_b_serial.err"
cp "$(find "$R/$OUT/${TAG}_ps" -name "*kernel_stats.csv" | head -1)" "$R/$OUT/${TAG}_b_serial_stats.csv"
rm -rf "$R/$OUT/${TAG}_ps"
echo serial done
rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/${TAG}_p2" -- python3 "$R/bench.py" --steps 4 --warmup 0 --no-cpu-baseline --no-roofline --no-decode --no-batch1-leg > "$R/$OUT/${TAG}_c_2streams.json" 2> "$R/$OUT/${TAG}_c_2streams.err"
cp "$(find "$R/$OUT/${TAG}_p2" -name "*kernel_stats.csv" | head -1)" "$R/$OUT/${TAG}_c_2streams_stats.csv"
rm -rf "$R/$OUT/${TAG}_p2"
echo two-streams done
cd "$R"
bash tools/pmc_forward.sh "$OUT/${TAG}_pmc"
python3 tools/pmc_forward_summary.py "$OUT/${TAG}_pmc" "$OUT/${TAG}_pmc_traffic.json" "$COMMIT" > "$OUT/${TAG}_a_pmc.txt"
rm -rf "$OUT/${TAG}_pmc/fetch" "$OUT/${TAG}_pmc/write" "$OUT/${TAG}_pmc/mfma"
echo pmc done
python3 tools/clock_in_kernel.py "$OUT/${TAG}_clock_in_kernel.json" "$COMMIT" > "$OUT/${TAG}_clock_in_kernel.txt" 2>&1
echo clock done
python3 bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"
python3 tools/per_template_summary.py "$OUT/${TAG}_b_serial_stats.csv" "$OUT/${TAG}_bench.json" 25 > "$OUT/${TAG}_per_template.txt"
cat "$OUT/${TAG}_per_template.txt"
