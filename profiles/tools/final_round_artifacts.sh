#!/bin/bash
# Round artifacts: the full bench command (JSON line with the roofline / half-split / CPU-baseline legs), its rocprofv3
# kernel-trace summary, the reduced-precision mode lines, the N = 2 self-launch rehearsal on one device.  Everything lands
# under $OUT (default bench_outputs/ in the repository root) and is copied into profiles/ by hand.
cd "$(dirname "$0")/../.." && export TMPDIR=/tmp
OUT=${OUT:-bench_outputs}
mkdir -p "$OUT"
python3 bench.py --full > "$OUT/r03_bench_line.json" 2> "$OUT/r03_bench.err"
tail -c 600 "$OUT/r03_bench_line.json"; echo
rm -rf "$OUT/prof_bench"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_bench" -- python3 bench.py --full --no-cpu-baseline > "$OUT/r03_bench_profiled_line.json" 2>/dev/null
cp "$OUT"/prof_bench/*/*kernel_stats.csv "$OUT/r03_bench_ffhq_gblur_heun30_b8_kernel_stats.csv"
python3 bench.py --full --no-cpu-baseline --unet-dtype fp16x3 > "$OUT/r03_bench_line_fp16x3_mode.json" 2>/dev/null
python3 bench.py --full --no-cpu-baseline --unet-dtype fp16 > "$OUT/r03_bench_line_fp16_mode.json" 2>/dev/null
python3 bench.py --full --no-cpu-baseline --unet-dtype bf16 > "$OUT/r03_bench_line_bf16_mode.json" 2>/dev/null
python3 bench.py --full --no-cpu-baseline --unet-dtype bf16x3 > "$OUT/r03_bench_line_bf16x3_mode.json" 2>/dev/null
FH_BENCH_ONE_DEVICE=1 python3 bench.py --full --gpus 2 --batch 4 --no-cpu-baseline > "$OUT/r03_bench_line_gpus2_rehearsal.json" 2>/dev/null
head -c 300 "$OUT/r03_bench_line_bf16_mode.json"; echo; head -c 300 "$OUT/r03_bench_line_gpus2_rehearsal.json"; echo
head -12 "$OUT/r03_bench_ffhq_gblur_heun30_b8_kernel_stats.csv" | cut -c1-160
