"""Host-side checks of the window-walking tap kernel (``DAAM_TAP_WALK``): its instances in a fresh build, the machine
code of every kernel that was there before, its register / scratch budget as the code object states it, and the parked-context key.
The planner itself lives behind ``daam_ctx_create`` (which needs a device): tests/test_gpu_tap_walk.py drives it."""
import json
import os
import struct

import pytest

from _libcheck import kernel_descriptors as _kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the two tap_pair_kernel instances (not in profiles/r06_counters.json: they were never profiled)
PAIR_SHAS = {'_ZN4daam15tap_pair_kernelIDF16_Lb1EEEvNS_9TapLaunchE': '073238c22833',
             '_ZN4daam15tap_pair_kernelIDF16_Lb0EEEvNS_9TapLaunchE': 'd011f31fa1e0'}

# the six tap_walk_kernel instances (younger than profiles/r06_counters.json)
WALK_SHAS = {'_ZN4daam15tap_walk_kernelINS_5InF16EDF16_Lb0EEEvNS_10WalkLaunchE': 'd769333541c8',
             '_ZN4daam15tap_walk_kernelINS_5InF16EDF16_Lb1EEEvNS_10WalkLaunchE': '3b10c139e131',
             '_ZN4daam15tap_walk_kernelINS_5InF16EfLb0EEEvNS_10WalkLaunchE': '2a43ae6bbc85',
             '_ZN4daam15tap_walk_kernelINS_5InF16EfLb1EEEvNS_10WalkLaunchE': 'be9c10d5869c',
             '_ZN4daam15tap_walk_kernelINS_6InBF16ENS_6bf16_tELb1EEEvNS_10WalkLaunchE': 'f1aa0587245b',
             '_ZN4daam15tap_walk_kernelINS_6InBF16EfLb1EEEvNS_10WalkLaunchE': 'bf1fe237aa79'}


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    lib = build.build(verbose=False)
    return lib, build.kernel_shas(lib)


def test_walk_instances_and_untouched_kernels(built):
    _, have = built
    walk = {k: v for k, v in have.items() if 'tap_walk_kernel' in k}
    # fp16 Q / K with fp16 and f32 sums, fast and strict softmax; bf16 Q / K with bf16 and f32 sums (one softmax flavour)
    assert len(walk) == 6, sorted(walk)
    assert sum('InF16' in k for k in walk) == 4 and sum('InBF16' in k for k in walk) == 2
    others = {k: v for k, v in have.items() if k not in walk}
    assert len(set(walk.values())) == 6 and not set(walk.values()) & set(others.values())
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'r06_counters.json')))['kernel_shas']
    assert len(rec) == 132
    assert {k: have.get(k) for k in rec} == rec
    assert {k: have.get(k) for k in PAIR_SHAS} == PAIR_SHAS


@pytest.mark.parametrize('name', sorted(WALK_SHAS))
def test_walk_kernel_fingerprint(built, name):
    """The machine code of every tap_walk_kernel instance is what it was before the tile moved to daam_tap_tile64.h."""
    _, have = built
    assert have.get(name) == WALK_SHAS[name]


def test_walk_kernel_budget(built):
    """No scratch and at most 128 VGPRs (two eight-wave workgroups per CU = four waves per SIMD) in every instance, read from the
    kernel descriptors: private segment size, the private-segment enable bit and the granulated VGPR count (granule 8)."""
    lib, have = built
    kds = _kernel_descriptors(lib)
    walk = [k for k in have if 'tap_walk_kernel' in k]
    assert len(walk) == 6 and all(k in kds for k in walk), sorted(set(walk) - set(kds))
    for k in walk:
        private, = struct.unpack_from('<I', kds[k], 4)
        rsrc1, rsrc2 = struct.unpack_from('<II', kds[k], 48)
        vgprs = ((rsrc1 & 0x3F) + 1) * 8
        assert private == 0 and not (rsrc2 & 1), (k, private)
        assert vgprs <= 128, (k, vgprs)


def test_park_key_separates_the_switch(monkeypatch):
    """A context parked by an engine created without DAAM_TAP_WALK is not adopted by one created with it (the library reads the
    switch when it creates a context)."""
    from daam_amd import engine as E
    monkeypatch.setattr(E.nat, 'load', lambda: object())
    monkeypatch.delenv('DAAM_TAP_WALK', raising=False)
    eng = E.HeatMapEngine(2, defer_steps=4, reuse_context=True, time_bins=[0, 2])
    off = eng._park_key()
    monkeypatch.setenv('DAAM_TAP_WALK', '1')
    on = eng._park_key()
    monkeypatch.setenv('DAAM_TAP_WALK', '0')
    assert eng._park_key() == off and on != off
    assert on[-1] == 0 and on[-2] == (0, 2)                     # probes and window layout keep their places
