R=$GRAFT_REPO_ROOT
cd $R
bash tools/prof_run.sh cfg5 --mode bf16_1024 --conv-breakdown $R/gpurun_out/prof_cfg5/by_shape.csv > gpurun_out/prof_cfg5.log 2>&1
bash tools/traffic_run.sh cfg5 conv2d_mfma16 --mode bf16_1024 > gpurun_out/traffic_cfg5.log 2>&1
cd $R
OUT=$(python3 -c 'import sys; sys.path.insert(0, "tools"); import collect_profiles; print(collect_profiles.G)')   # the folder tools/collect_profiles.py reads
python bench.py --mode bf16_1024 --full > $OUT/bench_cfg5.json 2> $OUT/bench_cfg5.err
tail -1 gpurun_out/bench_cfg5.json | cut -c1-300
