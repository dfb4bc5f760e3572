#!/bin/bash
# One GPU session: parity tests (gpu marker), smoke(), then a full bench run (rooflines and CPU baselines).
# Each GPU step has its own time limit; the chain stops at the first failure.
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
LOGS=${LOGS:-logs}
mkdir -p $LOGS
timeout -k 10 ${TEST_TIMEOUT:-600} python -u -m pytest ${TESTS:-tests} -m gpu -x -v --timeout 120 --timeout-method thread -p no:cacheprovider > $LOGS/tests.log 2>&1 &&
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke()" > $LOGS/smoke.log 2>&1 &&
timeout -k 10 ${BENCH_TIMEOUT:-400} python -u bench.py ${BENCH_ARGS:---full} > $LOGS/bench.log 2>&1
