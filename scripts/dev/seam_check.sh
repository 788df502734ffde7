#!/bin/bash
# the seam after a change: its tests, a minute and a half of fuzz_seam, three warm calls + a traced one, the bench line
cd "$GRAFT_REPO_ROOT" || exit 1
export OUT=${OUT:-results}; out=$OUT  # OUT: the folder for results
mkdir -p $out
T=${1:-r07_seam}
python -m pytest tests/test_multi_gpu.py tests/test_cli.py tests/test_configs_gpu.py -m gpu -x -q -k "not whole_suite" 2>&1 | tail -5 > $out/${T}_pytest.txt
python scripts/fuzz_seam.py ${FUZZ_S:-90} 777 2>&1 | tail -4 > $out/${T}_fuzz.txt
bash scripts/dev/e2e_trace.sh > $out/${T}_e2e.txt 2>&1
python bench.py --full > $out/${T}_bench.json 2> $out/${T}_bench.err
tail -3 $out/${T}_pytest.txt; cat $out/${T}_fuzz.txt; cat $out/${T}_e2e.txt
