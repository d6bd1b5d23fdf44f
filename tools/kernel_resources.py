#!/usr/bin/env python3
"""Register and scratch use of the kernels of a built library, from the code objects' metadata notes.

    python tools/kernel_resources.py [LIB.so] [regex on the kernel name]

Every offload bundle of the library is unbundled (as tools/compare_device_code.py does) and the AMDGPU metadata note of
each code object is read with llvm-readelf: per kernel .vgpr_count, .agpr_count, .sgpr_count,
.private_segment_fixed_size (scratch bytes per lane) and .group_segment_fixed_size.  Resource counts only: no instruction
text is read.  alloc_vgprs() is what a wave of the kernel takes of a SIMD's 512 registers per lane: the request rounded
up to the allocation granule of 8.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from compare_device_code import LLVM, code_objects   # noqa: E402

KEYS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')
SIMD_VGPRS = 512
GRANULE = 8


def alloc_vgprs(res):
    n = res['.vgpr_count'] + res['.agpr_count']
    return (n + GRANULE - 1) // GRANULE * GRANULE


def kernel_resources(lib):
    """{mangled kernel name: {key: int}} for every kernel of `lib`."""
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            text = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], check=True, capture_output=True,
                                  text=True).stdout
            cur = None
            for line in text.splitlines():
                # a kernel's map is an item of amdhsa.kernels: '  - .agpr_count: 0', its other keys at '    .key: value'
                # (the keys of its arguments are nested deeper)
                m = re.match(r'^  (- | {2})(\.[a-z_]+):\s*(\S*)\s*$', line)
                if not m:
                    continue
                if m.group(1) == '- ':
                    cur = {}
                if cur is None:
                    continue
                if m.group(2) in KEYS:
                    cur[m.group(2)] = int(m.group(3))
                elif m.group(2) == '.name':
                    found[m.group(3).strip('\'"')] = cur
            os.remove(co)
    return found


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, '..', 'nfmc_amd', 'libnfmc_hip.so')
    pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else '.')
    res = kernel_resources(lib)
    names = sorted(res)
    shown = names
    if shutil.which('c++filt'):
        shown = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    for name, nice in sorted(zip(names, shown), key=lambda p: p[1]):
        if pat.search(nice) or pat.search(name):
            r = res[name]
            print('%-100s vgpr %3d (alloc %3d) agpr %d sgpr %3d scratch %d lds %d'
                  % (nice[:100], r['.vgpr_count'], alloc_vgprs(r), r['.agpr_count'], r['.sgpr_count'],
                     r['.private_segment_fixed_size'], r['.group_segment_fixed_size']))
