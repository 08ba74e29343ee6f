#!/bin/bash
# Same-box A/B of bench.py's headline between two source trees, each with its own build -- for changes that tools/ab_bench.sh
# cannot compare (two libraries under ONE tree's binding: a change that adds symbols to the binding cannot load the older library):
#   tools/ab_trees.sh <other tree, built> [rounds]
# prints "<side> <round> <bases classified per second> <ms per step>" for other, this, other, this ...; with AB_LINES=<file>
# every run's whole result line is appended to that file as "<side> <round> <json>" (kernel times, the byte form's leg)
OTHER=$1; N=${2:-5}
HERE=$(cd "$(dirname "$0")/.." && pwd)
for i in $(seq $N); do
  for side in other this; do
    dir=$HERE; [ $side = other ] && dir=$OTHER
    line=$(cd "$dir" && timeout -k 10 170 python bench.py --gpus 1 --steps 40 --warmup 5 2>/dev/null | tail -1) || exit 1
    [ -n "$AB_LINES" ] && echo "$side $i $line" >> "$AB_LINES"
    echo "$line" | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$side', $i, d['value'], d.get('ms_per_step'))" || exit 1
  done
done
