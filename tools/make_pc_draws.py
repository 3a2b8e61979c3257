#!/usr/bin/env python
"""Records tests/golden/pc_draws.json: the rows csd_pc_noise_draws of the built library returns (or 'refused') over the grid of
tests/test_pc_draws_host.py - rules, modes, step counts, batch sizes, four tiny handles.  No GPU.  A pull request that MEANS to change
a draw's place on the tape or its Philox stream runs it on its own tree and says so; tests/test_pc_draws_host.py compares, and holds
hand-written anchor rows beside the file.

    python tools/make_pc_draws.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'pc_draws.json'))
    args = ap.parse_args()
    import test_pc_draws_host as t
    rec = t.pc_draws()
    with open(args.out, 'w') as f:
        json.dump(rec, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    n = sum(len(v) for v in rec['draws'].values() if v != 'refused')
    print('%s: %d schedules, %d rows (%d bytes)' % (args.out, len(rec['draws']), n, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
