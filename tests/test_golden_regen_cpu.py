"""The committed fixtures ARE what the reference produces: when ``build()`` has placed the
snapshot of the reference's Python modules in ``oracle/_ref/`` (``oracle/ref_snapshot.py``; made
only where a reference checkout is readable) the DEFAULT generator command
``python oracle/gen_golden.py --out <tmp>`` is re-run - importing the real reference from that
snapshot - and every family is compared bit for bit with ``tests/golden/``.  Bit-for-bit holds
on the kind of CPU that produced the fixtures: the test runs where the snapshot was made
(``ref_snapshot.made_here``: same CPU model and torch CPU dispatch level).

Pins the generator as well as the fixtures: round 2's default command overwrote
``train_forward.npz`` with different data (the neck family had loaded seeded neck weights
into the shared reference model first); ``gen_train_forward`` now gets a fresh model.
"""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / 'tests' / 'golden'
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))
from oracle import ref_snapshot  # noqa: E402

pytestmark = pytest.mark.skipif(not ref_snapshot.made_here(),
                                reason='needs the reference snapshot that build() places in oracle/_ref/, '
                                       'made on a CPU like this one')


@pytest.fixture(scope='module')
def regenerated(tmp_path_factory):
    out = tmp_path_factory.mktemp('golden_regen')
    proc = subprocess.run([sys.executable, str(REPO / 'oracle' / 'gen_golden.py'), '--out', str(out)],
                          capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return out


def test_default_command_regenerates_every_family(regenerated):
    made = sorted(p.name for p in regenerated.iterdir())
    committed = sorted(p.name for p in GOLDEN.iterdir())
    assert made == committed, (set(made) ^ set(committed))


def test_regenerated_fixtures_are_bit_identical(regenerated):
    for path in sorted(GOLDEN.glob('*.npz')):
        new, old = np.load(regenerated / path.name), np.load(path)
        assert sorted(new.files) == sorted(old.files), path.name
        for key in old.files:
            a, b = new[key], old[key]
            assert a.dtype == b.dtype and a.shape == b.shape, (path.name, key)
            assert a.tobytes() == b.tobytes(), f'{path.name}:{key} differs from the committed fixture'
    assert (regenerated / 'state_dict_keys.json').read_text() == (GOLDEN / 'state_dict_keys.json').read_text()
