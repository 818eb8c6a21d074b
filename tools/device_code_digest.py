#!/usr/bin/env python3
"""One line per kernel of the library's device code: `<sha256 of the kernel's text> <mangled name>`, sorted by name.
Two trees whose outputs are equal as files run the same instructions with the same registers, LDS and scratch.

    tools/device_code_digest.py                                  # every source of csrc/Makefile, its flags per file
    tools/device_code_digest.py --extra=-DOETR_SOAK_AMP=3 encoder   # the soak object
    tools/device_code_digest.py --csrc other/tree/imagematching_oetr_amd/csrc    # another checkout's sources

Each source is compiled device-only to assembly by csrc/Makefile's `asm` rule (so with exactly the flags its object
gets; no GPU needed, ~2 minutes).  A kernel's text is everything from its `<name>:` line to its `.Lfunc_end<N>:` line,
which includes its `.amdhsa_kernel` descriptor, with two things normalised that depend on the translation unit rather than on
the kernel: the `__hip_cuid_<hash>` symbol, and the function index in local labels (the order of emission)."""
import argparse
import hashlib
import re
import subprocess
import tempfile
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / 'imagematching_oetr_amd' / 'csrc'
LABEL = re.compile(r'\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+')


def kernels(asm):
    """{mangled name: normalised text} of every kernel in one assembly file."""
    asm = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_', asm)
    out = {}
    for name in re.findall(r'^\s*\.amdhsa_kernel (\S+)$', asm, re.M):
        body = re.search(r'^%s:.*?^\.Lfunc_end\d+:\n' % re.escape(name), asm, re.M | re.S).group(0)
        assert '.amdhsa_kernel ' + name in body, name           # the descriptor sits inside the function's text
        out[name] = LABEL.sub(r'.\1', body)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('sources', nargs='*', help='source names without .hip (default: all of the Makefile)')
    ap.add_argument('--extra', default='', help='extra compile flags, e.g. --extra=-DOETR_SOAK_AMP=3')
    ap.add_argument('--csrc', type=Path, default=CSRC, help='directory of the sources and their Makefile')
    args = ap.parse_args()
    csrc = args.csrc.resolve()
    digest = {}
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(['make', '-s', '-j16', '-C', tmp, '-f', str(csrc / 'Makefile'), f'VPATH={csrc}',
                        f'EXTRA={args.extra}'] + ([s + '.s' for s in args.sources] or ['asm']), check=True)
        for f in sorted(Path(tmp).glob('*.s')):
            for name, text in kernels(f.read_text()).items():
                assert name not in digest, name
                digest[name] = hashlib.sha256(text.encode()).hexdigest()
    for name in sorted(digest):
        print(digest[name], name)


if __name__ == '__main__':
    main()
