"""Register, scratch and LDS budget of every ``tap_d64_kernel`` instance of the built library, read from the kernel descriptors
(DESIGN 3.1): the counted-wait step protocol must not cost the head_dim-64 tap its four waves per SIMD, nor a second workgroup per CU."""
import re
import struct

import pytest

from test_tap_walk_cpu import _kernel_descriptors

# (Q / K type, sums type, fast softmax, FULL64, waves, counted waits): the 18 instances of the protocol before and the head_dim < 64
# form, and the 12 counted-wait instances (every head_dim-64 one, four and eight waves)
_PAIRS = [('5InF16E', 'DF16_', 1), ('5InF16E', 'DF16_', 0), ('5InF16E', 'f', 1), ('5InF16E', 'f', 0), ('6InBF16E', 'NS_6bf16_tE', 1), ('6InBF16E', 'f', 1)]
INSTANCES = [(i, a, f, full, w, c) for (i, a, f) in _PAIRS for (full, w, c) in ((0, 4, 0), (1, 4, 0), (1, 8, 0), (1, 4, 1), (1, 8, 1))]
K_BUF, Q_TILE, PTRS = 80 * 128, 32 * 128, 64 * 2 * 8            # a K buffer, a wave's Q tile, the per-step tensor pointers

# machine code of the 12 counted-wait instances, (Q / K type, sums type, fast softmax, waves) -> fingerprint (the other 18 are in
# profiles/r06_counters.json, which tests/test_tap_walk_cpu.py checks)
COUNTED_SHAS = {('5InF16E', 'DF16_', 0, 4): 'd37c65c6f3b7', ('5InF16E', 'DF16_', 0, 8): 'f5c4476c9779',
                ('5InF16E', 'DF16_', 1, 4): '0d9d9c2154a1', ('5InF16E', 'DF16_', 1, 8): 'a1045eee27ba',
                ('5InF16E', 'f', 0, 4): 'd9c3ec096b35', ('5InF16E', 'f', 0, 8): '42ff7ba6ee83',
                ('5InF16E', 'f', 1, 4): '2a70c48669dd', ('5InF16E', 'f', 1, 8): '2f6562ed9a3f',
                ('6InBF16E', 'NS_6bf16_tE', 1, 4): 'c47e0e811c7f', ('6InBF16E', 'NS_6bf16_tE', 1, 8): '24b735e83473',
                ('6InBF16E', 'f', 1, 4): 'a55cd87df449', ('6InBF16E', 'f', 1, 8): '6cad80394276'}


def _name(i, a, f, full, w, c):
    return f'_ZN4daam14tap_d64_kernelINS_{i}{a}Lb{f}ELb{full}ELi{w}E{"Lb1E" if c else ""}EEvNS_9TapLaunchE'


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    lib = build.build(verbose=False)
    return _kernel_descriptors(lib), build.kernel_shas(lib)


def test_instances(built):
    kds, have = built
    names = {k for k in have if 'tap_d64_kernel' in k}
    assert names == {_name(*x) for x in INSTANCES} and names <= set(kds), sorted(names ^ {_name(*x) for x in INSTANCES})
    # the counted-wait instances are other machine code than their counterparts
    for (i, a, f, full, w, c) in INSTANCES:
        if c:
            assert have[_name(i, a, f, full, w, 1)] != have[_name(i, a, f, full, w, 0)]


@pytest.mark.parametrize('key', sorted(COUNTED_SHAS), ids=lambda x: '-'.join(str(v).strip('_E') for v in x))
def test_counted_fingerprint(built, key):
    """The machine code of every counted-wait instance is what it was before the tile moved to daam_tap_tile64.h."""
    _, have = built
    i, a, f, w = key
    assert have.get(_name(i, a, f, 1, w, 1)) == COUNTED_SHAS[key]


@pytest.mark.parametrize('inst', INSTANCES, ids=lambda x: '-'.join(str(v).strip('_E') for v in x))
def test_budget(built, inst):
    """Scratch 0 in every instance.  At most 128 VGPRs -- four waves per SIMD -- in every head_dim-64 (LDS-DMA) instance, which are the
    ones the step protocol concerns: both protocols, four and eight waves, all six type / softmax combinations; at most 104 in the
    fast-softmax fp16 / fp16 eight-wave instances (the headline launch).  The loop's LDS (K buffers + Q tiles + pointers) is 53 KiB
    for eight waves with 2-byte sums, under 69 KiB, two workgroups per CU.

    Two groups of instances are outside the 128 / 104 bound, in machine code that this protocol change leaves byte-identical (and
    that tests/test_tap_walk_cpu.py pins): the register-staged head_dim < 64 instances with f32 or bf16 sums are built for three
    waves per SIMD by their launch bounds (152 / 154 / 160 / 160 VGPRs) and are only checked for scratch; the strict-softmax fp16 /
    fp16 eight-wave instance has 125 VGPRs in either protocol (as before this change), so 104 is asserted for the fast softmax only."""
    kds, _ = built
    i, a, f, full, w, c = inst
    kd = kds[_name(*inst)]
    lds_static, private = struct.unpack_from('<II', kd, 0)
    rsrc1, rsrc2 = struct.unpack_from('<II', kd, 48)
    vgprs = ((rsrc1 & 0x3F) + 1) * 8
    print(inst, 'vgprs', vgprs, 'private', private)
    assert private == 0 and not (rsrc2 & 1), (inst, private)
    assert lds_static == 0                                      # all LDS is dynamic: the launcher sizes it (tap_d64_lds_bytes)
    loop = 2 * K_BUF + w * Q_TILE + PTRS
    two_byte_sums = a != 'f'
    stage = 77 * 32 * w * (2 if two_byte_sums else 4)
    lds = max(loop, stage + PTRS)
    if two_byte_sums and w == 8:
        assert lds == loop == 53 * 1024 and lds < 69 * 1024
    assert 2 * lds <= 160 * 1024                                # two workgroups per CU
    if full:
        limit = 104 if (i == '5InF16E' and a == 'DF16_' and w == 8 and f) else 128
        assert vgprs <= limit, (inst, vgprs, limit)
