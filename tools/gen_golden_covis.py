#!/usr/bin/env python
"""Write tests/covis_expected.json: the pinned covis scenes and recall table.

The six scenes are RECIPES (kind, size, seed) of ``tests/covis_oracle.py`` - the inputs are regenerated from
them, bit for bit (pinned by the hashes of the two depth maps) - and the recorded results are those of the
float64 restatement in that module: boxes, valid, count, and the masks by hash.  Before anything is written this
script runs the REFERENCE's ``numpy_overlap_box`` (``src/datasets/utils.py``) on every scene and its ``_recalls`` /
``bbox_overlaps`` / ``bbox_oiou`` on the box table, and asserts that they give exactly the same boxes, masks, valid
flags, counts and recalls: the file holds the project's own numbers, checked against the reference.  Like
``oracle/gen_golden.py`` it reads the reference from the snapshot ``build()`` places in ``oracle/_ref/`` (kept out
of git) and runs only where that snapshot exists; ``cv2`` and ``h5py`` are empty stand-ins.

The reference is called with float64 COPIES of the float32 depth maps and float64 parameters, so its arithmetic
is float64 throughout whatever numpy's promotion rules are.  Every scene has a decision margin >=
``covis_oracle.MIN_MARGIN`` (asserted; a scene that fails is re-drawn, none is dropped).

Usage:  python tools/gen_golden_covis.py [--out tests/covis_expected.json]
"""
import argparse
import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
REF = REPO / 'oracle' / '_ref'
sys.dont_write_bytecode = True
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))

import covis_oracle as cvo  # noqa: E402

# (kind, H = W, seed): square maps only - that is where parity with the reference is claimed
SCENES = (('plane', 256, 1), ('plane', 320, 2), ('plane', 192, 3), ('no_overlap', 96, 4), ('behind', 128, 5),
          ('trunc', 160, 6))


def load_reference():
    from oracle.gen_golden import install_stubs
    install_stubs()                                   # cv2 among them
    sys.modules.setdefault('h5py', types.ModuleType('h5py'))
    sys.path.insert(0, str(REF))
    spec = importlib.util.spec_from_file_location('ref_datasets_utils', REF / 'src' / 'datasets' / 'utils.py')
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)
    from src.losses.utils import bbox_oiou, bbox_overlaps
    from src.utils.validation import _recalls
    return utils.numpy_overlap_box, _recalls, bbox_overlaps, bbox_oiou


def gen_scenes(numpy_overlap_box):
    out = []
    for kind, size, seed in SCENES:
        scene, mine = cvo.checked_scene(kind, size, size, seed)
        with np.errstate(all='ignore'):
            box1, mask1, box2, mask2, valid = numpy_overlap_box(*cvo.scene_args(scene))
        # the restatement's results ARE the reference's
        assert np.array_equal(np.asarray(box1, np.int64), mine['box1']) and np.array_equal(np.asarray(box2, np.int64), mine['box2'])
        assert bool(valid) == mine['valid'] and int((mask1 != 0).sum()) == mine['count']      # source pixels are distinct
        assert np.array_equal(mask1 != 0, mine['mask1'] != 0) and np.array_equal(mask2 != 0, mine['mask2'] != 0)
        rec = dict(kind=kind, size=size, seed=seed, depth1_sha256=cvo.sha(scene['depth1']),
                   depth2_sha256=cvo.sha(scene['depth2']), **cvo.result_record(mine))
        out.append(rec)
        print(kind, size, seed, rec['box1'], rec['box2'], rec['valid'], rec['count'], 'margin %.2e' % mine['margin'])
    return out


def gen_recalls(_recalls, bbox_overlaps, bbox_oiou):
    """A fixed table of ground-truth / predicted boxes (two per pair, some pairs with a zero ground-truth box,
    some IoUs exactly on a threshold) scored as ``evaluate_dummy`` scores them."""
    gt, pred = cvo.recall_table()
    thrs = np.arange(0.5, 0.96, 0.05)
    out = dict(thrs=[float(t) for t in thrs])
    tg, tp = torch.from_numpy(gt), torch.from_numpy(pred)
    for name, fn in (('iou', lambda a, b: bbox_overlaps(a, b, is_aligned=True)), ('oiou', bbox_oiou)):
        ious = np.array(list(fn(tg[0], tp[0]).numpy()) + list(fn(tg[1], tp[1]).numpy()))
        with np.errstate(all='ignore'):
            theirs = _recalls(np.array(ious), np.array(thrs))
        mine = cvo.recalls(cvo.box_scores(gt, pred, name == 'oiou'), thrs)
        assert np.array_equal(theirs, mine), (name, theirs, mine)
        out[f'{name}_recalls'] = [float(r) for r in mine]
        out[f'{name}_nansum'] = float(np.nansum(cvo.box_scores(gt, pred, name == 'oiou').astype(np.float64)))
        print(name, 'recalls', np.round(mine, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(REPO / 'tests' / 'covis_expected.json'))
    args = ap.parse_args()
    if not (REF / 'src' / 'datasets' / 'utils.py').is_file():
        sys.exit(f'no reference snapshot in {REF}: build() (oracle/ref_snapshot.py) makes it from a reference checkout')
    numpy_overlap_box, _recalls, bbox_overlaps, bbox_oiou = load_reference()
    rec = {'scenes': gen_scenes(numpy_overlap_box), 'recalls': gen_recalls(_recalls, bbox_overlaps, bbox_oiou)}
    Path(args.out).write_text(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
