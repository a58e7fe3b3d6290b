# round 6: register-resident weight fragments for the 8x8 convs -- parity, micro A/B, step A/B
set -o pipefail
R=$GRAFT_REPO_ROOT
cd $R
timeout -k 10 500 python -u -m pytest -x -q --timeout 200 --timeout-method thread -m gpu tests/test_gpu_kernels.py tests/test_gpu_trainer.py tests/test_gpu_fullsize.py > gpurun_out/r6_wreg_tests.txt 2>&1 || { echo TESTS_FAILED; tail -30 gpurun_out/r6_wreg_tests.txt; exit 1; }
tail -1 gpurun_out/r6_wreg_tests.txt
for i in 1 2; do for L in default nowreg; do
  if [ $L = default ]; then unset EBSDVAE_LIB; else export EBSDVAE_LIB=ebsd-vae_amd/lib/libebsdvae_$L.so; fi
  timeout -k 10 150 python3 tools/conv_micro.py --pieces 16 --warm 0.5 --only fwd128s8,dgrad128s8 2>&1 | grep -v amdgpu.ids | sed "s/^/$L /" || exit 1
  O=${O:-$(mktemp -d)}   # the bench lines go here
  timeout -k 10 200 python3 bench.py --full --no-cpu-baseline --strict-fp32-steps 0 --c4-batches 256 --c5-steps 0 --steps 30 > $O/wreg_$L.txt 2>/dev/null || exit 1
  echo "$L bench $(python3 -c "import json;d=json.loads(open('$O/wreg_$L.txt').read().splitlines()[-1]);print(d['ms_per_step'], d['c4_encoder_latents']['ms_per_batch'])")"
done; done
