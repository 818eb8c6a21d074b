#!/usr/bin/env python
"""Write tests/fine_match_expected.json: the results of the fine-match specification (tests/fine_match_oracle.py, DESIGN
9.3p) on the pinned calls of tests/fine_match_cases.py, and its recorded margins.

The inputs are a RECIPE (seeds, shapes, kinds) - regenerated bit for bit and pinned by their hashes - and the recorded
results are, per call and capacity, the counters, the list offsets and a hash of every output of the specification.

One margin is MEASURED here and gated at four times its recorded value by tests/test_fine_match_cpu.py: ``head``, the
specification against a plain float64 restatement of the published head (``unfold``-style windows, ``einsum``,
``softmax(sim / sqrt(C))``, expectation, std) on pairs drawn with a seed.  The script ASSERTS that the match list, the
windows and the counters are EQUAL and records the largest difference of ``expec`` and of ``mkpts1``.

Usage:  python tools/gen_golden_fine_match.py [--out tests/fine_match_expected.json]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.dont_write_bytecode = True
sys.path.insert(0, str(REPO / 'tests'))

import fine_match_cases as fmc  # noqa: E402
import fine_match_oracle as fmo  # noqa: E402

HEAD_SEED = 11


def capacities(call):
    """Room for every match and two over; a cut in the middle of a pair; none."""
    total = fmc.matched_total(call)
    return [total + 2, max(total // 2, 1), 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'fine_match_expected.json'))
    args = ap.parse_args()
    calls = {}
    for name in fmc.SHAPES:
        call = fmc.make_call(name)
        calls[name] = dict(
            C=call['C'], W=call['W'], stride=call['stride'], matched=fmc.matched_total(call),
            inputs_sha256=dict(matches0=fmc.sha(call['matches0']), fine0=fmc.sha(call['fine0']), fine1=fmc.sha(call['fine1'])),
            results={str(cap): fmc.result_record(*fmc.expected(call, cap)) for cap in capacities(call)})
        print(name, calls[name]['matched'], {k: v['counts'] for k, v in calls[name]['results'].items()})
    head = []
    for k, shape in enumerate(fmc.HEAD_SHAPES):
        rec = fmc.head_compare(k, HEAD_SEED)
        assert rec['equal'], (shape, 'the list, the windows or the counters differ from the float64 restatement')
        head.append(dict(shape=[shape[0], shape[1], shape[2], list(shape[3]), list(shape[4])], seed=HEAD_SEED, **rec))
        print('head', shape, rec)
    out = dict(calls=calls, partials=fmo.PARTIALS, head=head,
               grids={str(W): [float(g) for g in fmo.grid(W)] for W in fmo.WINDOWS},
               statement=['the project\'s own statement, modelled on LoFTR\'s published fine matching; that code lives in '
                          'a third_party/ tree outside the reference checkout, so no parity with it is claimed'])
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
