"""What the tests of more than one library read out of a built file: its exported symbols, what a public header declares, the kernel
descriptors of its gfx950 code objects and the no-scratch check on them."""
import os
import re
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exported(lib):
    """Sorted names of the functions ``lib`` defines and exports."""
    nm = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    return sorted(re.findall(r' T (\w+)$', nm, flags=re.M))


def declared(header):
    """Sorted names of the ``DAAM_API`` functions that ``include/<header>`` declares."""
    return sorted(re.findall(r'DAAM_API [\w \*]*?(daam_\w+)\(', open(os.path.join(ROOT, 'include', header)).read()))


def kernel_descriptors(lib):
    """{kernel name: its 64-byte kernel descriptor} of the gfx950 code objects in ``lib`` (the ``<name>.kd`` objects)."""
    data = open(lib, 'rb').read()
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    out = {}
    pos = data.find(magic)
    while pos >= 0:
        n, = struct.unpack_from('<Q', data, pos + len(magic))
        o = pos + len(magic) + 8
        for _ in range(n):
            off, size, ts = struct.unpack_from('<QQQ', data, o)
            o += 24
            triple = data[o:o + ts].decode()
            o += ts
            if 'gfx950' not in triple or not size:
                continue
            elf = data[pos + off:pos + off + size]
            shoff, = struct.unpack_from('<Q', elf, 0x28)
            shentsize, shnum, _ = struct.unpack_from('<HHH', elf, 0x3A)
            secs = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + i * shentsize) for i in range(shnum)]
            for (_, typ, _, _, soff, ssize, link, _, _, entsize) in secs:
                if typ != 2:                                     # SHT_SYMTAB
                    continue
                str_off = secs[link][4]
                for i in range(ssize // entsize):
                    name_i, _, _, shndx, value, osize = struct.unpack_from('<IBBHQQ', elf, soff + i * entsize)
                    end = elf.index(b'\0', str_off + name_i)
                    name = elf[str_off + name_i:end].decode()
                    if not name.endswith('.kd') or osize != 64 or shndx >= len(secs):
                        continue
                    sec = secs[shndx]
                    start = sec[4] + (value - sec[3])
                    out[name[:-3]] = elf[start:start + 64]
        pos = data.find(magic, pos + 1)
    return out


def assert_no_scratch(lib, names):
    """Private segment size 0 and the private-segment enable bit clear in the kernel descriptor of every kernel of ``names``."""
    kds = kernel_descriptors(lib)
    assert all(k in kds for k in names), sorted(set(names) - set(kds))
    for k in names:
        private, = struct.unpack_from('<I', kds[k], 4)
        _, rsrc2 = struct.unpack_from('<II', kds[k], 48)
        assert private == 0 and not (rsrc2 & 1), (k, private)
