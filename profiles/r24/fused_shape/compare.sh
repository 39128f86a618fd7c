#!/bin/sh
# Builds shape_dump.cpp against the parent commit's csrc/ and against this tree's, with the
# sanitizers for the dump and at -O3 for the timing, compares the dumps and alternates the timed
# runs.  Usage: compare.sh [WORKDIR]   (from anywhere inside the repository)
set -e
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here" && git rev-parse --show-toplevel)
parent=${PARENT:-HEAD}
work=${1:-$(mktemp -d)}
cxx=${CXX:-g++}
mkdir -p "$work/parent"
(cd "$root" && git archive "$parent" distributed-learning_amd/csrc/launch.cpp \
    distributed-learning_amd/csrc/launch.h distributed-learning_amd/csrc/plan.cpp \
    distributed-learning_amd/csrc/plan.h include/dlamd.h) | tar -x -C "$work/parent"
for tree in parent new; do
    if [ $tree = parent ]; then src="$work/parent"; else src="$root"; fi
    c="$src/distributed-learning_amd/csrc"
    $cxx -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
        -I"$c" -I"$root/tests" "$here/shape_dump.cpp" "$c/launch.cpp" "$c/plan.cpp" \
        -o "$work/dump_$tree"
    $cxx -std=c++17 -O3 -Wall -I"$c" -I"$root/tests" "$here/shape_dump.cpp" "$c/launch.cpp" \
        "$c/plan.cpp" -o "$work/time_$tree"
    "$work/dump_$tree" > "$work/$tree.txt" 2> "$work/$tree.err"
    cat "$work/$tree.err"
done
cmp "$work/parent.txt" "$work/new.txt"
sha256sum "$work/parent.txt" "$work/new.txt"
wc -l < "$work/new.txt"
for round in sgd cheb track; do
    for i in 1 2 3 4 5 6 7; do
        for tree in parent new; do
            printf '%s ' $tree
            "$work/time_$tree" time $round 2000000
        done
    done
done
