# Round 4's profile material in one call on the GPU box (OUT = the results directory, relative to the repository root):
#   OUT=<dir> bash tools/r04.sh ; then here:  python tools/make_profiles.py r04 ; python tools/sq_summary.py r04pmc r04 ; cp the force-dist lines
: "${OUT:?set OUT to the directory the results go to}"
cd "$(dirname "$0")/.."
bash tools/refresh_profiles.sh r04 > $OUT/r04_refresh.log 2>&1 || { tail -5 $OUT/r04_refresh.log; exit 1; }
mkdir -p $OUT/prof_r04
python bench.py --full --force-dist --gbp 6.25 --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_r04/fd31.json 2> $OUT/prof_r04/fd31.err &&
python bench.py --full --force-dist --gbp 6.25 --k 63 --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_r04/fd63.json 2> $OUT/prof_r04/fd63.err &&
bash tools/pmc_leaf.sh r04pmc > $OUT/r04_pmc.log 2>&1
tail -2 $OUT/prof_r04/bench.json | cut -c1-600
bash tools/pmc_wide.sh r04w > $OUT/r04_pmcw.log 2>&1
