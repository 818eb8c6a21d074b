#!/usr/bin/env python
"""Write tests/nn_match_expected.json: the results of the nearest-neighbour matcher's specification
(tests/nn_match_oracle.py) on the pinned calls of tests/nn_match_cases.py.

The inputs are a RECIPE (seeds, shapes, kinds) - regenerated bit for bit and pinned by their hashes - and the recorded
results are, per call and threshold setting, the counters and a hash of every output of the specification.

Where the reference snapshot exists (``oracle/_ref/``, placed by ``build()`` and kept out of git) the script also runs
the REFERENCE's own ``find_nn`` and ``mutual_check`` (``dloc/core/matchers/nearest_neighbor.py``; the two functions are
compiled from the file's syntax tree, so the ``dloc`` package and its third-party wrappers are never imported) on the
specification's float32 similarity of every pair, through torch on the CPU, and asserts that ``matches0`` and the bits
of ``matching_scores0`` agree

* on ALL rows of the unit-norm calls (no row may be excluded);
* on the grid calls, on the rows whose row maximum is attained once and whose matched column's maximum is attained
  once - torch's ``topk`` leaves a tied index open, the specification takes the lowest - with the excluded share
  recorded per call and held to at most 10 % of its rows.

Pairs the reference cannot run are counted as ``reference_cannot_run``: a side without rows, and a side of one row
under a ratio threshold (``topk(2)`` raises).  ``reference_checked`` says whether any of this happened; without the
snapshot the file is written from the specification alone and says so.

Usage:  python tools/gen_golden_nn_match.py [--out tests/nn_match_expected.json]
"""
import argparse
import ast
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
REF_FILE = REPO / 'oracle' / '_ref' / 'dloc' / 'core' / 'matchers' / 'nearest_neighbor.py'
sys.dont_write_bytecode = True
sys.path.insert(0, str(REPO / 'tests'))

import nn_match_cases as nmc  # noqa: E402
import nn_match_oracle as nmo  # noqa: E402

MAX_EXCLUDED_SHARE = {'unit': 0.0, 'grid': 0.10}


def load_reference(path=REF_FILE):
    """``(find_nn, mutual_check)`` of the reference, compiled from the two function definitions alone."""
    import torch
    tree = ast.parse(Path(path).read_text())
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ('find_nn', 'mutual_check')]
    assert len(wanted) == 2, [n.name for n in wanted]
    space = {'torch': torch}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), str(path), 'exec'), space)
    return space['find_nn'], space['mutual_check']


def attained_once(sim):
    """Per row of ``sim``: the row's maximum over the candidates is attained exactly once."""
    b1, i1, b2 = nmo.top2(sim)
    return (i1 >= 0) & (b2 < b1)


def compare_with_reference(ref, call, setting):
    """``(rows compared, rows excluded, pairs the reference cannot run)``; asserts agreement on the compared rows."""
    import torch
    find_nn, mutual_check = ref
    ratio, distance, mutual = setting
    compared = excluded = cannot = 0
    for p, sim in enumerate(call['sims']):
        K0, K1 = sim.shape
        if min(K0, K1) < (2 if ratio else 1):
            cannot += 1
            continue
        spec = nmo.match_similarity(sim, ratio, distance, mutual)
        t = torch.from_numpy(np.array(sim))[None]
        m0, s0 = find_nn(t, ratio, distance)
        if mutual:
            m1, _ = find_nn(t.transpose(1, 2), ratio, distance)
            m0 = mutual_check(m0, m1)
        m0, s0 = m0[0].numpy(), s0[0].numpy()
        assert s0.dtype == np.float32
        first, _ = nmo.find_nn(sim, ratio, distance)                # direction 0 before the mutual check
        column_once = attained_once(sim.T)
        covered = attained_once(sim) & np.where(first > -1, column_once[np.maximum(first, 0)], True)
        if call['kind'] == 'unit':
            assert covered.all(), (call['name'], p, 'a tied maximum in a unit-norm call')
        same = (m0 == spec['matches0']) & (s0.view(np.uint32) == spec['matching_scores0'].view(np.uint32))
        assert same[covered].all(), (call['name'], call['kind'], setting, p, np.nonzero(covered & ~same)[0][:8])
        compared += int(covered.sum())
        excluded += int((~covered).sum())
    return compared, excluded, cannot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'nn_match_expected.json'))
    args = ap.parse_args()
    have_reference = REF_FILE.is_file()
    ref = load_reference() if have_reference else None
    calls = {}
    for name, kind in nmc.CALLS:
        call = nmc.make_call(name, kind)
        rec = dict(D=call['D'], pairs=[list(q) for q in call['pairs']],
                   inputs_sha256=dict(desc0=nmc.sha(call['desc0']), desc1=nmc.sha(call['desc1'])), results={})
        compared = excluded = cannot = 0
        for setting in nmc.SETTINGS:
            rec['results'][nmc.setting_key(*setting)] = nmc.result_record(nmc.expected(call, *setting))
            if ref is not None:
                c, e, n = compare_with_reference(ref, call, setting)
                compared, excluded, cannot = compared + c, excluded + e, cannot + n
        if ref is not None:
            share = excluded / max(1, compared + excluded)
            assert share <= MAX_EXCLUDED_SHARE[kind], (name, kind, share)
            rec['reference'] = dict(rows_compared=compared, rows_excluded=excluded, excluded_share=share,
                                    reference_cannot_run=cannot)
        calls[f'{name}/{kind}'] = rec
    out = dict(settings=[nmc.setting_key(*s) for s in nmc.SETTINGS], max_excluded_share=MAX_EXCLUDED_SHARE,
               calls=calls, reference_checked=bool(have_reference),
               departures=['a tied maximum goes to the lowest index (torch.topk leaves it open)',
                           'a side of one row passes the ratio test (torch.topk(2) raises)'])
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    for key, rec in calls.items():
        print(key, rec.get('reference', 'specification only'))


if __name__ == '__main__':
    main()
