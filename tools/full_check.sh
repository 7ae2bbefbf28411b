cd $GRAFT_REPO_ROOT; export TMPDIR=/tmp
python -m pytest tests -x -q -m gpu 2>&1 | tail -4
python tools/time_gt_train.py 2>&1 | tail -3
python bench.py --full > /tmp/bench_full.json 2> /tmp/bench_full.err; tail -c 2500 /tmp/bench_full.json
