"""Non-square generations, host side: the size rule (``map_geometry``), the layer rule (``layer_geometry``), the argument checks of
``trace(pipe, height=, width=)`` and the additive C ABI (four ``*_rect`` entry points, ABI version unchanged)."""
import os
import re

import pytest
import torch

from conftest import ROOT
from daam_amd import _native
from daam_amd.engine import layer_geometry, map_geometry

RECT_SYMBOLS = ('daam_ctx_create_rect', 'daam_layer_configure_rect', 'daam_epilogue_normalize_rect', 'daam_word_heat_map_rect')


@pytest.mark.parametrize('args,want', [
    ((1024, 832, 1216), (52, 76)),
    ((512, 512, 768), (64, 96)),
    ((1024, 1024, 1024), (64, 64)),
    ((1024, 1216, 832), (76, 52)),
    ((768, 768, 768), (96, 96)),          # 96-cell pipelines (trace.py:32-33): cell = 8
    ((1024, 2048, 2048), (128, 128)),     # the limit itself
])
def test_map_geometry(args, want):
    assert map_geometry(*args) == want


@pytest.mark.parametrize('args,word', [
    ((1024, 840, 1216), '32'),            # height not a multiple of 2 * cell = 32
    ((1024, 832, 1200), '32'),            # width
    ((512, 520, 768), '16'),              # SD: 2 * cell = 16
    ((1024, 2080, 1024), '128'),          # 130 cells
    ((512, 512, 1040), '128'),            # 130 cells
    ((1024, 832.0, 1216), 'int'),
    ((1024, True, 1216), 'int'),
    ((1024, 0, 1216), 'int'),
    ((1024, -832, 1216), 'int'),
])
def test_map_geometry_refuses(args, word):
    with pytest.raises(ValueError, match=word):
        map_geometry(*args)


@pytest.mark.parametrize('out_hw,positions,want', [
    ((52, 76), 52 * 76, (1, 52, 76)),
    ((52, 76), 26 * 38, (2, 26, 38)),
    ((52, 76), 13 * 19, (4, 13, 19)),
    ((64, 96), 8 * 12, (8, 8, 12)),       # the gate (factor != 8) is the caller's
    ((12, 20), 6 * 10, (2, 6, 10)),
    ((64, 64), 32 * 32, (2, 32, 32)),
])
def test_layer_geometry(out_hw, positions, want):
    assert layer_geometry(*out_hw, positions) == want


@pytest.mark.parametrize('out_hw,positions', [
    ((52, 76), 7 * 10),                   # 52 x 76 // 70 = 56 -> factor 7: 52 % 7 != 0 (a UNet that rounds 6.5 x 9.5 up)
    ((52, 76), 27 * 38),                  # factor 1 but not the map's own size
    ((12, 20), 3 * 5 + 1),                # factor 3: 20 % 3 != 0
    ((12, 20), 12 * 20 * 4),              # more positions than map cells: factor 0
    ((12, 20), 0),
])
def test_layer_geometry_refuses(out_hw, positions):
    with pytest.raises(ValueError):
        layer_geometry(*out_hw, positions)


def test_rect_entry_points_are_declared_and_the_version_stays():
    src = open(os.path.join(ROOT, 'include', 'daam_hip.h')).read()
    assert '#define DAAM_ABI_VERSION 6' in src and _native.ABI_VERSION == 6
    for name in RECT_SYMBOLS:
        assert name in _native.EXPORTS, name
        assert re.search(r'DAAM_API int %s\(' % name, src), name
    for decl in ('DAAM_API int daam_ctx_create_rect(int max_layers, int tokens, int out_h, int out_w, int acc_dtype, DaamCtx** out);',
                 'DAAM_API int daam_layer_configure_rect(DaamCtx* ctx, int layer, int heads, int h, int w, int factor, void* acc);',
                 'DAAM_API int daam_epilogue_normalize_rect(float* maps, int n_rows, int h, int w, void* stream);'):
        assert decl in src, decl


def test_build_lists_the_rect_source():
    from daam_amd import build
    assert 'daam_finalize_rect.hip' in build.SOURCES and 'daam_fin_rect.h' in build.HEADERS


def _cpu_pipe():
    from oracle import fake_diffusers as fd
    return fd.make_pipe('sdxl', device='cpu', dtype=torch.float32, mini=True, identity_proj=True, tblocks_cap=1)


@pytest.mark.parametrize('kw,word', [
    (dict(height=832), 'both'),
    (dict(width=1216), 'both'),
    (dict(height=832.0, width=1216), 'int'),
    (dict(height='832', width=1216), 'int'),
    (dict(height=840, width=1216), '32'),
    (dict(height=832, width=4096), '128'),
    (dict(height=832, width=1216, time_bins=[0, 2]), 'time_bins'),
])
def test_trace_checks_height_and_width_at_construction(kw, word, tmp_path):
    import daam_amd
    with pytest.raises(ValueError, match=word):
        daam_amd.trace(_cpu_pipe(), data_dir=str(tmp_path), **kw)


def test_engine_geometry_without_a_device():
    """The engine's shape bookkeeping of a non-square map needs no GPU: sizes, the parked-context key, the exclusions."""
    from daam_amd.engine import HeatMapEngine
    eng = HeatMapEngine(2, out_hw=(52, 76))
    assert (eng.out_h, eng.out_w, eng.rect) == (52, 76, True)
    assert eng._side(26 * 38, 2) == (26, 38)
    with pytest.raises(ValueError):
        eng._side(26 * 38, 1)                  # the caller's factor is not the rule's
    with pytest.raises(ValueError):
        eng._side(7 * 10, 7)
    assert (52, 76) in eng._park_key()
    sq = HeatMapEngine(2, out_hw=(64, 64))
    default = HeatMapEngine(2, out_side=64)
    assert not sq.rect and sq._park_key() == default._park_key() and sq._side(1024, 2) == 32
    with pytest.raises(ValueError, match='time_bins'):
        HeatMapEngine(2, out_hw=(52, 76), time_bins=[0, 3])
