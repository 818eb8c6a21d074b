#!/usr/bin/env python
"""Write tests/match_assembly_expected.json: the pinned call of the match-assembly specification
(tests/match_assembly_oracle.py).

The call is a RECIPE (seed, the pair table ``PAIRS``) of ``tests/match_assembly_oracle.py`` - the inputs are regenerated
from it, bit for bit (pinned by their hashes) - and the recorded results are those of the numpy specification in that
module: the four counters per pair, the list offsets, the selection of pairs with too few matches, and hashes of the
integer outputs.  No arrays are stored.

Usage:  python tools/gen_golden_match_assembly.py [--out tests/match_assembly_expected.json]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.dont_write_bytecode = True
sys.path.insert(0, str(REPO / 'tests'))

import match_assembly_oracle as mao  # noqa: E402

SEED = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'match_assembly_expected.json'))
    args = ap.parse_args()
    call = mao.make_call(SEED)
    res = mao.assemble(**call)
    out = mao.record(SEED, call, res)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print('pairs', len(mao.PAIRS), 'keypoints', len(call['kp0']), len(call['kp1']), 'matches', out['offsets'][-1],
          'counts', out['counts'], 'few', out['few'][:out['n_few']])


if __name__ == '__main__':
    main()
