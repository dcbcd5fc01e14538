# kernel trace of the whole k = 63 bench command (count + counter_to_asm + assemble_w), one step, under $OUT/prof_asm63
: "${OUT:?set OUT to the directory the results go to}"
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(cd "$R" && mkdir -p "$OUT" && cd "$OUT" && pwd) || exit 1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_asm63 -- python3 $R/bench.py --full --k 63 --steps 1 --warmup 0 --no-cpu-baseline > $O/prof_asm63.log 2>&1
