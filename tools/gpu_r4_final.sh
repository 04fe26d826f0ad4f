#!/bin/bash
# Round 4, last visit: the whole GPU suite and the bench line on the final commit
ROOT="${GRAFT_REPO_ROOT:-/root/repo}"
cd "$ROOT"; mkdir -p gpurun_out/r4final; export TMPDIR=/tmp
O=gpurun_out/r4final
timeout 1500 python -m pytest tests -m gpu -q > $O/pytest_gpu.log 2>&1; echo "pytest exit $?"; tail -3 $O/pytest_gpu.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
( time timeout 1500 python bench.py --full > $O/bench.json 2> $O/bench.err ); echo "bench exit $?"; tail -c 200 $O/bench.json; echo
