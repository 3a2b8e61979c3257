#!/usr/bin/env python
"""Records tests/golden/scratch_sizes.json: what every csd_*_bytes entry of the built library returns over the grid of
tests/test_scratch_sizes_host.py, with the commit it was recorded on.  No GPU.  Run it on the commit whose sizes are to be pinned (a
pull request that MEANS to change a size runs it on its own tree and says so); tests/test_scratch_sizes_host.py compares.

    python tools/make_scratch_sizes.py [--commit HASH]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None, help='hash to record (default: git rev-parse HEAD)')
    args = ap.parse_args()
    import test_scratch_sizes_host as t
    commit = args.commit or subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], text=True).strip()
    rec = t.scratch_sizes()
    rec['recorded_on_commit'] = commit
    path = os.path.join(ROOT, 'tests', 'golden', 'scratch_sizes.json')
    with open(path, 'w') as f:
        json.dump(rec, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    n = sum(len(v) for v in rec['operators'].values()) + sum(len(v) for v in rec['networks'].values() if v)
    print('%s: %d sizes on %s (%d bytes)' % (path, n, commit, os.path.getsize(path)))


if __name__ == '__main__':
    main()
