"""Host-side pieces of time-binned tracing: ``time_bins`` / ``time_bin`` validation, the window step counts, the C ABI
declaration and exports, the stale-library check, the library calls of a binned engine and the machine code of a fresh
build."""
import json
import os
import subprocess
import types

import pytest
import torch

from _fake_native import fake_engine  # noqa: F401 -- the recording stand-in of libdaam_hip (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_time_bins_validation():
    from daam_amd.engine import check_time_bins
    assert check_time_bins(None) is None
    assert check_time_bins([0]) == (0,)
    assert check_time_bins(range(50)) == tuple(range(50))
    assert check_time_bins((0, 2, 3)) == (0, 2, 3)
    for bad in ([], [1], [0, 0], [0, 3, 2], list(range(65)), [0, 1.5], 'abc', 5, [0, True]):
        with pytest.raises(ValueError):
            check_time_bins(bad)


def test_trace_rejects_bad_time_bins():
    import daam_amd
    from oracle import fake_diffusers as fd
    pipe = fd.make_pipe('sd15', mini=True)
    for bad in ([], [2, 3], [0, 5, 5], range(1, 10)):
        with pytest.raises(ValueError):
            daam_amd.trace(pipe, time_bins=bad)


def _bare(time_bins):
    from daam_amd.trace import DiffusionHeatMapHooker
    t = DiffusionHeatMapHooker.__new__(DiffusionHeatMapHooker)
    t.time_bins = None if time_bins is None else tuple(time_bins)
    t.last_prompts, t.last_prompt = ['a'], 'a'
    t.pipe = types.SimpleNamespace(tokenizer=None)
    return t


def test_time_bin_to_window_range():
    t = _bare([0, 2, 3, 10])
    assert t._bin_range(None) is None
    assert t._bin_range(0) == (0, 1) and t._bin_range(3) == (3, 4)
    assert t._bin_range(-1) == (3, 4) and t._bin_range(-4) == (0, 1)
    assert t._bin_range(slice(1, 3)) == (1, 3) and t._bin_range(slice(None)) == (0, 4)
    assert t._bin_range(slice(-2, None, 1)) == (2, 4) and t._bin_range(slice(2, 99)) == (2, 4)
    for bad in (4, -5, slice(2, 2), slice(3, 1), slice(0, 4, 2), slice('a', 2), 1.0, '1', True):
        with pytest.raises(ValueError):
            t._bin_range(bad)
    one = _bare(None)                                           # un-binned: the only window is 0
    assert one._bin_range(0) == (0, 1) and one._bin_range(-1) == (0, 1) and one._bin_range(slice(None)) == (0, 1)
    with pytest.raises(ValueError):
        one._bin_range(1)


def test_window_step_counts():
    from daam_amd.engine import window_steps
    assert window_steps((0, 2, 3), [6, 6]) == [2, 1, 3]
    assert window_steps((0, 2, 5), [3]) == [2, 1, 0]
    assert window_steps((0, 2, 3), [1, 6]) == [2, 1, 3]
    assert window_steps((0,), [4]) == [4]
    assert window_steps(tuple(range(50)), [50]) == [1] * 50
    assert window_steps((0, 10), []) == [0, 0]


def test_header_declares_time_bin_entry_points():
    from daam_amd import _native
    src = open(os.path.join(ROOT, 'include', 'daam_hip.h')).read()
    assert '#define DAAM_ABI_VERSION 6' in src and _native.ABI_VERSION == 6
    for decl in ('DAAM_API int daam_ctx_set_time_bins(DaamCtx* ctx, int n_bins, const int32_t* first_step);',
                 'DAAM_API int daam_tap_steps(DaamCtx* ctx, int layer, int* steps);',
                 'DAAM_API int daam_finalize_bins(DaamCtx* ctx, const int32_t* key_group, int n_groups, const int32_t* group_set,'):
        assert decl in src, decl
    for name in ('daam_ctx_set_time_bins', 'daam_tap_steps', 'daam_finalize_bins'):
        assert name in _native.EXPORTS


def test_fresh_build_exports_and_keeps_kernels():
    from daam_amd import build
    lib = build.build(verbose=False)
    out = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ('daam_ctx_set_time_bins', 'daam_tap_steps', 'daam_finalize_bins'):
        assert name in syms, name
    have = build.kernel_shas()
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'r06_counters.json')))['kernel_shas']
    assert {k: have.get(k) for k in rec} == rec
    assert sum('finalize_bin_sum_kernel' in k for k in have) == 3, [k for k in have if 'bin_sum' in k]


def test_load_rejects_library_without_new_symbol(tmp_path):
    """A library of the same ABI version that lacks an entry point of this build is stale: the same 'rebuild' message."""
    src = tmp_path / 'old.c'
    src.write_text('int daam_abi_version(void) { return 6; }\nconst char* daam_last_error(void) { return ""; }\n')
    lib = tmp_path / 'libold.so'
    subprocess.run(['cc', '-shared', '-fPIC', str(src), '-o', str(lib)], check=True)
    code = ('import daam_amd._native as n\n'
            'try:\n    n.load()\nexcept RuntimeError as e:\n    print("ERR", e)\n')
    env = dict(os.environ, DAAM_HIP_LIB=str(lib), PYTHONPATH=ROOT)
    out = subprocess.run(['python', '-c', code], capture_output=True, text=True, env=env, cwd=ROOT).stdout
    assert 'ERR' in out and 'rebuild' in out and 'daam_finalize_bins' in out, out


@pytest.mark.parametrize('recorder', ['c++', 'python'])
def test_binned_engine_sets_windows_before_configuring(fake_engine, monkeypatch, recorder):
    E, lib = fake_engine
    if recorder == 'python':
        monkeypatch.setenv('DAAM_NO_FASTPATH', '1')
    q, k = torch.zeros(2, 64, 16, dtype=torch.float16), torch.zeros(2, 77, 16, dtype=torch.float16)
    eng = E.HeatMapEngine(2, defer_steps=4, time_bins=[0, 3])
    for _ in range(5):
        for layer in (1, 0):
            eng.tap_qk(layer, q, k, 2, 0.35, 1)
    names = lib.names()
    assert names.count('daam_ctx_set_time_bins') == 1
    assert names.index('daam_ctx_set_time_bins') < names.index('daam_layer_configure')
    n, first = [c[1][1:] for c in lib.calls if c[0] == 'daam_ctx_set_time_bins'][0]
    assert n == 2 and list(first) == [0, 3]
    assert tuple(eng.acc[0].shape) == (2, 2, 77, 8, 8)          # [windows, heads, tokens, side, side]
    with pytest.raises(RuntimeError, match='raw_heat_maps'):
        list(eng.items())
    with pytest.raises(RuntimeError, match='update'):
        eng.add_map(1, 0, 0, torch.zeros(77, 8, 8, dtype=torch.float16))
    eng.close()
    plain = E.HeatMapEngine(2, defer_steps=4)
    before = len(lib.calls)
    for _ in range(5):
        for layer in (1, 0):
            plain.tap_qk(layer, q, k, 2, 0.35, 1)
    plain.global_heat_map()
    new = [c[0] for c in lib.calls[before:]]
    assert 'daam_ctx_set_time_bins' not in new and 'daam_tap_steps' not in new and 'daam_finalize_bins' not in new
    assert 'daam_finalize' in new and 'daam_finalize_prepare' in new
    assert tuple(plain.acc[0].shape) == (2, 77, 8, 8)
    plain.close()


def test_park_key_separates_window_layouts(fake_engine):
    E, lib = fake_engine
    q, k = torch.zeros(2, 64, 16, dtype=torch.float16), torch.zeros(2, 77, 16, dtype=torch.float16)
    a = E.HeatMapEngine(1, defer_steps=4, reuse_context=True, time_bins=[0, 2])
    a.tap_qk(0, q, k, 2, 0.35, 1)
    a.close()
    for bins in (None, [0, 3], [0]):
        b = E.HeatMapEngine(1, defer_steps=4, reuse_context=True, time_bins=bins)
        n = lib.names().count('daam_ctx_create')
        b.tap_qk(0, q, k, 2, 0.35, 1)
        assert lib.names().count('daam_ctx_create') == n + 1, bins        # another layout: never adopted
        b.close()
    c = E.HeatMapEngine(1, defer_steps=4, reuse_context=True, time_bins=(0, 2))
    n = lib.names().count('daam_ctx_create')
    c.tap_qk(0, q, k, 2, 0.35, 1)
    assert lib.names().count('daam_ctx_create') == n                      # the same layout: adopted
    c.close()
    E.release_parked_contexts()


def test_binned_finalize_routes_through_finalize_bins(fake_engine):
    E, lib = fake_engine
    q, k = torch.zeros(2, 64, 16, dtype=torch.float16), torch.zeros(2, 77, 16, dtype=torch.float16)
    eng = E.HeatMapEngine(1, defer_steps=4, time_bins=[0, 2, 4])
    for _ in range(5):
        eng.tap_qk(0, q, k, 2, 0.35, 1)
    eng.global_heat_map(bins=(1, 3), n_rows=9)
    call = [c for c in lib.calls if c[0] == 'daam_finalize_bins'][-1][1]
    assert call[2] == 1 and list(call[4]) == [1] and list(call[5]) == [3] and list(call[6]) == [9]
    assert 'daam_finalize_prepare' not in lib.names() and 'daam_finalize' not in lib.names()
    eng.time_heat_maps([(w, w + 1, 0) for w in range(3)] * 30, 1, [77])    # 90 groups: two calls of <= 64
    calls = [c for c in lib.calls if c[0] == 'daam_finalize_bins']
    assert [c[1][2] for c in calls[-2:]] == [64, 26]
    eng.close()


@pytest.mark.parametrize('how', ['clear', 'adopted'])
def test_windows_a_shorter_generation_does_not_reach_read_zero(fake_engine, how):
    """The buffers are kept across ``clear()`` (no views out) and across the adoption of a parked context, and ``daam_reset``
    zeroes nothing: the windows the next generation does not reach hold the previous one's sums until ``window_items`` zeroes
    them -- those windows only, for the touched layers only, once per reset, and never in a first generation."""
    E, lib = fake_engine
    q, k = torch.zeros(2, 64, 16, dtype=torch.float16), torch.zeros(2, 77, 16, dtype=torch.float16)

    def make():
        return E.HeatMapEngine(3, defer_steps=8, reuse_context=True, time_bins=[0, 2, 4])

    def taps(eng, counts):
        for s in range(max(counts)):
            for layer, n in enumerate(counts):
                if s < n:
                    eng.tap_qk(layer, q, k, 2, 0.35, 1)
    eng = make()
    taps(eng, (5, 5, 5))
    eng.flush()
    for buf in eng.acc.values():
        buf.fill_(7.0)                                          # what generation 1 left (the stand-in computes nothing)
    bufs = dict(eng.acc)
    if how == 'clear':
        eng.clear()
    else:
        eng.close()
        eng = make()
    taps(eng, (3, 1, 0))                                        # layer 0 reaches windows 0 and 1, layer 1 window 0, layer 2 none
    before = len(lib.calls)
    views = eng.window_items(2)
    assert all(eng.acc[layer] is bufs[layer] for layer in range(3))
    assert [c[0] for c in lib.calls[before:]].count('daam_tap_steps') == 2          # the two touched layers
    assert sorted(key[1] for key in views) == [0, 0, 1, 1]
    assert [bool((eng.acc[0][w] == 7.0).all()) for w in range(3)] == [True, True, False] and not bool(eng.acc[0][2].any())
    assert [bool((eng.acc[1][w] == 7.0).all()) for w in range(3)] == [True, False, False] and not bool(eng.acc[1][1:].any())
    assert bool((eng.acc[2] == 7.0).all())                       # not touched: not handed out, left to the library's finalize
    assert all(not bool(v.any()) for v in views.values())
    eng.acc[0][2].fill_(3.0)                                    # once per reset: what arrives later in the generation stays
    before = len(lib.calls)
    eng.window_items(2)
    assert 'daam_tap_steps' not in [c[0] for c in lib.calls[before:]] and bool((eng.acc[0][2] == 3.0).all())
    eng.close()
    E._PARKED.clear()
    first = E.HeatMapEngine(1, defer_steps=8, time_bins=[0, 2, 4])                   # a first generation: nothing to zero, nothing asked
    first.tap_qk(0, q, k, 2, 0.35, 1)
    before = len(lib.calls)
    first.window_items(1)
    assert 'daam_tap_steps' not in [c[0] for c in lib.calls[before:]]
    first.close()
