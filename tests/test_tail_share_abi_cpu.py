"""CPU-only checks of the tail-sharing extension header (include/oetr_tail_share.h): the library exports what it
declares, the binding lists the same names, and a NULL handle is refused without a GPU."""
import re
from pathlib import Path

import imagematching_oetr_amd as pkg
from imagematching_oetr_amd import hip_engine

REPO = Path(__file__).resolve().parents[1]


def header_functions(name):
    text = (REPO / 'include' / name).read_text()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(oetr_[a-z_0-9]+)\s*\(', text)))


def test_header_exports_and_library_agree():
    lib = pkg.load_library()
    names = header_functions('oetr_tail_share.h')
    assert len(names) == 2 and set(names) == set(hip_engine.TAIL_SHARE_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/oetr_tail_share.h but not exported'
    assert not set(names) & set(hip_engine.EXPORTS)


def test_null_handle_is_refused():
    lib = pkg.load_library()
    assert lib.oetr_set_tail_share(None, 0) == 1 and b'NULL' in lib.oetr_last_error()
    assert lib.oetr_debug_encoder_grid(None) == -1
