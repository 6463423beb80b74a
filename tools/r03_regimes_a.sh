#!/bin/bash
# Round 3, evidence run A: the regimes never measured -- crown-class (3.5 M triangles, textured, 1024 spp) and beyond the Infinity Cache (16 M triangles).
# usage: tools/r03_regimes_a.sh OUTDIR
cd "$(dirname "$0")/.."
out="${1:?usage: tools/r03_regimes_a.sh OUTDIR}"
mkdir -p "$out"
python3 bench.py --full --triangles 3500000 --materials textured --spp 1024 --steps 1 --warmup 1 --no-spp1024 --cpu-tiles 16 > "$out/bench_crown_class.json" 2> "$out/bench_crown_class.err" && \
python3 bench.py --full --triangles 16000000 --steps 1 --warmup 1 --no-spp1024 --cpu-tiles 16 > "$out/bench_16m.json" 2> "$out/bench_16m.err" && \
python3 -m pytest tests/test_gpu_wavefront.py -x -q -k "rt16m or rt1m" > "$out/pytest_16m.txt" 2>&1
echo "rc=$?"; tail -3 "$out"/*.err "$out/pytest_16m.txt"; cat "$out"/*.json
