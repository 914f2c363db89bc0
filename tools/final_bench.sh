#!/bin/bash
# Round numbers: the default bench with every leg (--full; --regions 0: the median of repeated regions) as the README quotes it,
# and the other workloads.  JSON lines land in $OUT (default bench_out/final/).
OUT=${OUT:-bench_out/final}
mkdir -p $OUT
python bench.py --full --regions 0 --steps 20 --warmup 5 > $OUT/bench_gowalla_steps20.json 2> $OUT/bench_gowalla_steps20.err
python bench.py --full --regions 0 > $OUT/bench_gowalla.json 2> $OUT/bench_gowalla.err
python bench.py --full --regions 0 --workload yelp2018 > $OUT/bench_lightgcn_yelp2018.json 2> $OUT/bench_lightgcn_yelp2018.err
python bench.py --full --regions 0 --workload ml10m --no-cpu-baseline > $OUT/bench_ml10m.json 2>/dev/null
python bench.py --full --regions 0 --workload addressa --no-cpu-baseline > $OUT/bench_addressa.json 2>/dev/null
python bench.py --full --regions 0 --train normalbce --no-cpu-baseline > $OUT/bench_gowalla_normalbce.json 2>/dev/null
python bench.py --full --regions 0 --no-defer --no-cpu-baseline > $OUT/bench_gowalla_nodefer.json 2>/dev/null
python bench.py --full --workload config4 --c4-lazy 1 --steps 40 --warmup 5 --regions 1 --no-eval --no-cpu-baseline > $OUT/bench_config4_1gpu_dense_adam.json 2>/dev/null
python bench.py --full --workload config4 --steps 256 --warmup 70 --regions 2 > $OUT/bench_config4_1gpu.json 2> $OUT/bench_config4_1gpu.err
MACR_DIST_BACKEND=gloo python bench.py --full --regions 0 --gpus 2 --steps 20 --warmup 5 --no-cpu-baseline --c4-users 2000000 --c4-items 200000 --c4-eval-users 20000 > $OUT/bench_gowalla_2ranks_gloo_one_gpu.json 2> $OUT/bench_gowalla_2ranks_gloo_one_gpu.err
tail -c 400 $OUT/bench_gowalla.json
