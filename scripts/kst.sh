#!/bin/bash
# kernel-trace statistics of the default bench step -> $OUT/<tag>_kstats.txt (OUT: the folder for results, default results/)
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
tag=${1:-x}; shift
out=${OUT:-results}
mkdir -p $out
rm -rf $out/prof_$tag
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -o k -- python3 bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-extra "$@" > $out/prof_$tag.log 2>&1
python3 scripts/kstats.py $out/prof_$tag > $out/${tag}_kstats.txt
head -12 $out/${tag}_kstats.txt
tail -1 $out/prof_$tag.log | cut -c1-400
