"""Snapshot of the reference implementation's Python modules into ``oracle/_ref/`` (kept out of git).

``build()`` calls :func:`snapshot`; the golden generator (``oracle/gen_golden.py``) and
``tests/test_golden_regen_cpu.py`` read the reference from the snapshot only, so nothing in the
repository reaches outside it.  The upstream ImageMatching-OETR checkout is taken from
``$OETR_REFERENCE_DIR`` or, without it, from its usual place (``DEFAULT_SOURCE``).  Where no
checkout is readable the snapshot is simply not made, and the test that needs it skips.

The fixtures are torch-CPU results compared bit for bit, which holds on the kind of CPU that
produced them, not across processors: the snapshot records the CPU it was made on
(``FINGERPRINT``), and :func:`made_here` tells the test whether it runs on that CPU.

Usage:  python oracle/ref_snapshot.py [SOURCE]
"""
import json
import os
import shutil
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
DEST = REPO / 'oracle' / '_ref'
DEFAULT_SOURCE = Path('/root/reference')
MARKER = Path('src') / 'model.py'          # what makes a directory a reference checkout
FINGERPRINT = 'FINGERPRINT.json'


def source_dir():
    """The reference checkout to snapshot, or None when there is none readable."""
    src = Path(os.environ.get('OETR_REFERENCE_DIR') or DEFAULT_SOURCE)
    try:
        return src if (src / MARKER).is_file() and os.access(src / MARKER, os.R_OK) else None
    except OSError:
        return None


def fingerprint():
    """The CPU model and the ISA level torch's CPU kernels dispatch to on this machine."""
    import torch
    model = ''
    try:
        with open('/proc/cpuinfo') as f:
            model = next((line.split(':', 1)[1].strip() for line in f if line.startswith('model name')), '')
    except OSError:
        pass
    return {'cpu_model': model, 'torch_cpu_capability': torch.backends.cpu.get_cpu_capability()}


def available(dest=DEST):
    return (Path(dest) / MARKER).is_file()


def made_here(dest=DEST):
    """A snapshot exists and was made on a CPU like this one."""
    try:
        return available(dest) and json.loads((Path(dest) / FINGERPRINT).read_text()) == fingerprint()
    except (OSError, ValueError):
        return False


def snapshot(src=None, dest=DEST):
    """Copy every ``*.py`` file of the checkout into ``dest`` (layout kept; the old snapshot is
    replaced).  Returns ``dest``, or None when there is no checkout to copy from."""
    src = Path(src) if src else source_dir()
    if src is None or not (src / MARKER).is_file():
        return None
    dest = Path(dest)
    tmp = dest.with_name(dest.name + '.tmp')
    shutil.rmtree(tmp, ignore_errors=True)
    for path in sorted(src.rglob('*.py')):
        rel = path.relative_to(src)
        if any(part.startswith('.') for part in rel.parts):
            continue
        (tmp / rel).parent.mkdir(parents=True, exist_ok=True)
        shutil.copyfile(path, tmp / rel)
    (tmp / FINGERPRINT).write_text(json.dumps(fingerprint()))
    shutil.rmtree(dest, ignore_errors=True)
    tmp.rename(dest)
    return dest


if __name__ == '__main__':
    made = snapshot(sys.argv[1] if len(sys.argv) > 1 else None)
    print(made if made else 'no reference checkout found: nothing copied')
