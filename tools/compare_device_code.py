#!/usr/bin/env python3
"""Did the kernels change?  Compares the gfx950 device code of two builds of the library, kernel by kernel.

    python tools/compare_device_code.py OLD.so NEW.so

Every offload bundle of both libraries is unbundled (clang-offload-bundler) and every kernel -- every symbol NAME with a
kernel descriptor NAME.kd -- is compared by (i) its mangled name, (ii) the 64 bytes of its descriptor, (iii) the
disassembly of its function (llvm-objdump, instruction addresses and encodings stripped).  Kernels may move between code
objects; names and bodies may not change.  One field of the descriptor is left out: KERNEL_CODE_ENTRY_BYTE_OFFSET
(bytes 16..23), the distance from the descriptor to the code, which says where the linker put the kernel and nothing
about it.  Exit status 0 when the name sets are identical and no kernel differs, 1 otherwise.
"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def code_objects(lib, tmp):
    """The gfx950 code objects of every bundle in `lib` (one bundle per translation unit), as files under tmp."""
    data = open(lib, 'rb').read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = []
    for i, s in enumerate(starts):
        bundle = os.path.join(tmp, '%s.%d.bundle' % (os.path.basename(lib), i))
        with open(bundle, 'wb') as fh:
            fh.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = bundle[:-7] + '.co'
        subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET,
                        '--input=' + bundle, '--output=' + co], check=True)
        os.remove(bundle)
        if os.path.getsize(co):
            out.append(co)
    return out


def descriptors(co):
    """{kernel name: its descriptor bytes without the entry offset} from the ELF symbol table of one code object."""
    d = open(co, 'rb').read()
    shoff, = struct.unpack_from('<Q', d, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', d, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', d, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for sec in secs:
        if sec[1] != 2:   # SHT_SYMTAB
            continue
        strtab = secs[sec[6]][4]
        for off in range(sec[4], sec[4] + sec[5], 24):
            name_off, _info, _other, shndx, value, size = struct.unpack_from('<IBBHQQ', d, off)
            name = d[strtab + name_off:d.index(b'\0', strtab + name_off)].decode()
            if name.endswith('.kd') and size == 64 and 0 < shndx < shnum:
                pos = secs[shndx][4] + value - secs[shndx][3]
                out[name[:-3]] = d[pos:pos + 16] + d[pos + 24:pos + 64]
    return out


def kernels(lib, tmp):
    """{kernel name: [(descriptor, sha256 of its disassembly), ...]} -- one entry per code object that holds it."""
    found = {}
    for co in code_objects(lib, tmp):
        kd = descriptors(co)
        text = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', co],
                              check=True, capture_output=True, text=True).stdout
        name, body = None, None
        for line in text.splitlines() + ['<>:']:
            m = re.match(r'^(?:[0-9a-f]+ )?<(.*)>:$', line)
            if m:
                if name in kd:
                    found.setdefault(name, []).append((kd.pop(name), body.hexdigest()))
                name, body = m.group(1), hashlib.sha256()
            elif body is not None:
                body.update(line.split('//')[0].strip().encode() + b'\n')
        assert not kd, 'descriptors without a function in %s: %s' % (co, sorted(kd)[:3])
        os.remove(co)
    return found


def main(old_lib, new_lib):
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(old_lib, tmp), kernels(new_lib, tmp)
    for n in sorted(set(old) - set(new)):
        print('only in OLD:', n)
    for n in sorted(set(new) - set(old)):
        print('only in NEW:', n)
    differ = [n for n in sorted(set(old) & set(new)) if sorted(old[n]) != sorted(new[n])]
    for n in differ:
        what = [w for i, w in enumerate(('descriptor', 'disassembly')) if sorted(c[i] for c in old[n]) != sorted(c[i] for c in new[n])]
        print('differs (%s; copies %d -> %d): %s' % (' and '.join(what) or 'copies', len(old[n]), len(new[n]), n))
    same_names = set(old) == set(new)
    print('%d kernels in OLD, %d in NEW, name sets %s; %d kernels compared, %d differing'
          % (len(old), len(new), 'identical' if same_names else 'DIFFERENT', len(set(old) & set(new)), len(differ)))
    return 0 if same_names and not differ else 1


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
