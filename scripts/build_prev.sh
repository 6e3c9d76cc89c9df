#!/bin/bash
# Build the committed (HEAD, or REV=<rev>) library (kernels and host code) as sam2consensus_amd/libs2c_prev.so — the "before" side
# of an A/B on the GPU box (scripts/run.sh ab:WL with LIBS="libs2c.so libs2c_prev.so"): that revision's tree, by its own Makefile.
set -e
cd "$(dirname "$0")/.."
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
git archive "${REV:-HEAD}" | tar -x -C "$T"
make -C "$T" -j"${JOBS:-8}" OUT="$PWD/sam2consensus_amd/libs2c_prev.so" >"$T/make.log" 2>&1 || { tail -40 "$T/make.log"; exit 1; }
echo built sam2consensus_amd/libs2c_prev.so
