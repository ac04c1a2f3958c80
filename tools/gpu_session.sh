#!/bin/bash
# Session: the GPU suite and smoke() on HEAD.
cd "${GRAFT_REPO_ROOT:-/root/repo}"; export TMPDIR=/tmp; mkdir -p gpurun_out
O="${OUT_DIR:-out}"; mkdir -p "$O"  # (where the suite's log and the bench line go)
timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 200 --timeout-method thread > "$O/pytest_gpu.log" 2>&1
rc=$?; tail -4 "$O/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > gpurun_out/smoke.log 2>&1; rc=$?; tail -2 gpurun_out/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --gpus 1 --steps 20 --warmup 5 > "$O/bench_driver_head.json" 2> "$O/bench_driver_head.err" || exit 1
python -c "import json;d=json.load(open('$O/bench_driver_head.json'));print(d['ms_per_step'], d['value'])"
