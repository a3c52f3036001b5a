# training forward on fen_group_strip: parity (strip tests incl. the training saves, north-star
# training G10), then the stage-1 training leg with the strip forward on / off (same box)
export TMPDIR=/tmp
mkdir -p gpurun_out
timeout -k 10 600 python -u -m pytest tests/test_gpu_group_strip.py tests/test_gpu_train64.py -m gpu -v -s -x --timeout 300 --timeout-method thread > gpurun_out/st_tests.log 2>&1
rc=$?; echo "tests rc=$rc"; grep -E "passed|failed|Error|worst|max \|d\||training_saves" gpurun_out/st_tests.log | tail -14
[ $rc -eq 0 ] || exit 1
OUT=${FEN_OUT:-out}; mkdir -p "$OUT"     # the bench lines' folder
for rep in 1 2; do
  for v in 1 0; do
    FEN_GROUP_STRIP_TRAIN=$v timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-stress --no-perceptual --steps 10 --warmup 3 --train-steps 20 > "$OUT/stt_$v.json" 2> "$OUT/stt_$v.log"
    rc=$?; [ $rc -eq 0 ] || { echo "bench rc=$rc"; tail -5 "$OUT/stt_$v.log"; exit $rc; }
    python - "$v" "$OUT" <<'PY'
import json, sys
d = json.loads(open(f"{sys.argv[2]}/stt_{sys.argv[1]}.json").read().strip().splitlines()[-1])
t = d["train"]
print(f"strip_train={sys.argv[1]}  inference {d['value']:9.1f} img/s  train {t['ms_per_step']:7.3f} ms  loss {t['loss']:.6f}  gan {d.get('train_gan', {}).get('ms_per_step')}")
PY
  done
done
