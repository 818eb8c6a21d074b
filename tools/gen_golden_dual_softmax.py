#!/usr/bin/env python
"""Write tests/dual_softmax_expected.json: the results of the dual-softmax matcher's specification
(tests/dual_softmax_oracle.py) on the pinned calls of tests/dual_softmax_cases.py, and its recorded margins.

The inputs are a RECIPE (seeds, shapes, kinds) - regenerated bit for bit and pinned by their hashes - and the recorded
results are, per call and setting, the counters and a hash of every output of the specification.

Two margins are MEASURED here and gated at four times their recorded value by tests/test_dual_softmax_cpu.py:

* ``e_max_rel_err``: the specification's float32 exponential against float64 ``np.exp`` on ``dual_softmax_cases.e_sweep``;
* ``head``: the specification against a plain float64 restatement of the published head (``softmax(dim=1) *
  softmax(dim=2)``, ``> thr``, the border, the two ``== max`` tests) on calls drawn with a seed: the script takes, per
  shape, the FIRST seed at which the float64 program's own margins - best against second confidence per row and column,
  confidence against threshold - are all at least 1e-3 relative, ASSERTS that ``matches0`` and the counters are then
  EQUAL on every row, and records the seed, the margin and the error of the confidences.

Usage:  python tools/gen_golden_dual_softmax.py [--out tests/dual_softmax_expected.json]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.dont_write_bytecode = True
sys.path.insert(0, str(REPO / 'tests'))

import dual_softmax_cases as dsc  # noqa: E402
import dual_softmax_oracle as dso  # noqa: E402

MAX_SEEDS = 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'dual_softmax_expected.json'))
    args = ap.parse_args()
    calls = {}
    for name, kind in dsc.CALLS:
        call = dsc.make_call(name, kind)
        calls[f'{name}/{kind}'] = dict(
            D=call['D'], pairs=[list(q) for q in call['pairs']],
            inputs_sha256=dict(feat0=dsc.sha(call['feat0']), feat1=dsc.sha(call['feat1'])),
            results={dsc.setting_key(*s): dsc.result_record(dsc.expected(call, *s)) for s in dsc.SETTINGS})
    head = []
    for k, shape in enumerate(dsc.HEAD_SHAPES):
        for seed in range(MAX_SEEDS):
            rec = dsc.head_compare(k, seed)
            if rec['margin'] >= dsc.HEAD_MARGIN:
                break
        else:
            raise SystemExit(f'no seed below {MAX_SEEDS} gives shape {shape} its margins')
        assert rec['equal'], (shape, seed, 'matches0 or the counters differ from the float64 head')
        head.append(dict(shape=list(shape), seed=seed, **rec))
        print('head', shape, 'seed', seed, rec)
    inside, _ = dsc.e_sweep()
    out = dict(settings=[dsc.setting_key(*s) for s in dsc.SETTINGS], calls=calls, partials=dso.PARTIALS,
               e_cut=float(dso.E_CUT), q_min_log2=-62, e_max_rel_err=dsc.e_error(inside), head_margin=dsc.HEAD_MARGIN,
               head_rel_floor=dsc.HEAD_REL_FLOOR, head=head,
               statement=['the project\'s own statement, modelled on LoFTR\'s published coarse matching; that code lives '
                          'in a third_party/ tree outside the reference checkout, so no parity with it is claimed'])
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print('e_max_rel_err', out['e_max_rel_err'])
    for key, rec in calls.items():
        print(key, [r['counts'][-1] for r in rec['results'].values()][:1])


if __name__ == '__main__':
    main()
