cd $GRAFT_REPO_ROOT
export MSTTS_EXTRA_HIPCC_FLAGS="$1"
python -m multi_speaker_tts_amd.build > /dev/null 2>&1
mkdir -p bench_outputs
python bench.py --steps 6 --warmup 2 --full --no-cpu-baseline > bench_outputs/exp.json 2> bench_outputs/exp.err
tail -3 bench_outputs/exp.err
