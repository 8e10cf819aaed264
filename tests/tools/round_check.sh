set -o pipefail
out=${1:?usage: bash tests/tools/round_check.sh OUT_DIR}
mkdir -p "$out"
timeout -k 10 1000 python -m pytest tests -x -q -m gpu > "$out/round_gpu_tests.log" 2>&1; echo "gpu tests rc $?"; tail -5 "$out/round_gpu_tests.log"
timeout -k 10 600 python bench.py --full > "$out/round_bench.json" 2> "$out/round_bench.err"; echo "bench rc $?"; cut -c1-1500 "$out/round_bench.json"
