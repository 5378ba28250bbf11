#!/bin/bash
# The three measurements of DESIGN.md 4.12, each GPU step under its own time limit, chained: a step that fails, faults or runs out of
# time ends the script, and nothing more is started on the GPU.  Usage (from the repository root): profiles/microbench/kli_stage.sh [out]
out=${1:-/dev/stdout}
timeout -k 10 240 python profiles/microbench/kli_stage.py stage --atoms 86 --levels 17 >> "$out" &&
timeout -k 10 240 python profiles/microbench/kli_stage.py stage --atoms 2,4,10,12,18,20,30,36,38,48,54,56 --levels 14 >> "$out" &&
timeout -k 10 300 python profiles/microbench/kli_stage.py steps --levels 14 >> "$out"
