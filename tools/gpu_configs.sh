# The other BASELINE configs through bench.py (one GPU): configs[1] 100k Gaussians,
# one 800x800 camera (F = 0 and F = 32); configs[4] 1M Gaussians at 1920x1080,
# F = 32, 4 cameras per rank (the 8-GPU case runs the same per-rank work).
# One --full line per config (stages, roofline, the other call pattern) in $OUT/configs.jsonl.
set -o pipefail
R=$GRAFT_REPO_ROOT
cd $R
O=${OUT:-bench_out}
mkdir -p $O
rm -f $O/configs.jsonl
timeout -k 10 300 python bench.py --full --no-cpu-baseline --gaussians 100000 --cams 1 --features 0 --steps 20 --warmup 3 >> $O/configs.jsonl 2> $O/configs.err || exit 1
timeout -k 10 300 python bench.py --full --no-cpu-baseline --gaussians 100000 --cams 1 --features 32 --steps 20 --warmup 3 >> $O/configs.jsonl 2>> $O/configs.err || exit 2
timeout -k 10 300 python bench.py --full --no-cpu-baseline --gaussians 1000000 --width 1920 --height 1080 --cams 4 --features 32 --steps 5 --warmup 2 >> $O/configs.jsonl 2>> $O/configs.err || exit 3
