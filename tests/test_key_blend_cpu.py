"""Heat maps of weighted key sets without a GPU (the library itself: ``test_analysis_library_cpu.py``): the argument checks of
``daam_key_blend`` answer before any device call, the float64 reference of ``tests/_blend_domain.py`` agrees with the oracle and its
counted chain is pinned, and the engine and the trace hand ``daam_key_blend`` the weight table their arguments imply (a recording
stand-in below)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _blend_domain as bd
from _fake_native import fake_engine  # noqa: F401 -- the fixture
from oracle import heatmap_oracle as ho


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.ANALYSIS_OUT


def _raw(lib, a):
    return lib.daam_key_blend(a['keys'], a['n_keys'], a['dtype'], a['n_rows'], a['out_h'], a['out_w'], a['weights'], a['n_sets'], a['out'],
                              a['set_stride'], a['scratch'], a['scratch_bytes'], None)


def test_out_of_limits_arguments_are_refused_on_the_host(built):
    from daam_amd import _native as nat
    lib = nat.load_analysis()
    keys = (nat.KeyPlanes * 1)()
    buf = (ctypes.c_float * 64)()
    k, b = ctypes.addressof(keys), ctypes.addressof(buf)
    need = lib.daam_key_blend_scratch_bytes(1, 1, 1, 4, 4)
    assert need > 0
    good = dict(keys=k, n_keys=1, dtype=0, n_rows=1, out_h=4, out_w=4, weights=b, n_sets=1, out=b, set_stride=16, scratch=b, scratch_bytes=need)
    big = 1 << 40
    bad = [(dict(n_keys=0), 'keys'), (dict(n_keys=(1 << 20) + 1, scratch_bytes=big), 'keys'), (dict(n_sets=0), 'weight sets'),
           (dict(n_sets=9, scratch_bytes=big), 'weight sets'), (dict(out_h=0), 'output of'), (dict(out_h=129, scratch_bytes=big), 'output of'),
           (dict(out_w=0), 'output of'), (dict(out_w=129, scratch_bytes=big), 'output of'), (dict(n_rows=0), 'token rows'),
           (dict(dtype=3), 'dtype'), (dict(dtype=-1), 'dtype'), (dict(keys=None), 'NULL'), (dict(weights=None), 'NULL'),
           (dict(out=None), 'NULL'), (dict(scratch=None), 'NULL'), (dict(set_stride=15), 'set_stride'),
           (dict(n_rows=2, scratch_bytes=big), 'set_stride'), (dict(scratch_bytes=need - 1), 'scratch of'), (dict(scratch_bytes=0), 'scratch of')]
    for change, word in bad:
        rc = _raw(lib, dict(good, **change))
        assert rc == nat.E_INVALID, change
        assert word in lib.daam_analysis_last_error().decode(), (change, lib.daam_analysis_last_error().decode())
        with pytest.raises(nat.DaamError):
            nat.check_analysis(rc)


def test_scratch_bytes_is_monotone(built):
    from daam_amd import _native as nat
    size = nat.load_analysis().daam_key_blend_scratch_bytes
    assert size(1100, 1, 77, 64, 64) == 256 + bd.n_chunks(1100) * 77 * 64 * 64 * 4
    for bad in [(0, 1, 1, 4, 4), ((1 << 20) + 1, 1, 1, 4, 4), (1, 0, 1, 4, 4), (1, 9, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 1, 0, 4), (1, 1, 1, 4, 129)]:
        assert size(*bad) == 0, bad
    base = (40, 3, 7, 12, 20)
    for pos, values in enumerate([(1, 31, 32, 33, 64, 65, 1100, 1 << 20), range(1, 9), (1, 5, 77, 1000), (1, 12, 64, 128), (1, 20, 64, 128)]):
        last = 0
        for v in values:
            args = list(base)
            args[pos] = v
            assert size(*args) >= last > -1, (pos, v)
            last = size(*args)
            assert last > 0


def test_reference_agrees_with_the_oracle_and_the_chain_is_counted():
    rng = np.random.default_rng(2)
    planes = {(1, 0, 0): rng.standard_normal((5, 16, 16)).astype(np.float32), (2, 1, 0): rng.standard_normal((5, 8, 8)).astype(np.float32),
              (4, 2, 1): rng.standard_normal((5, 4, 4)).astype(np.float32)}
    w = np.full((1, 3), 1.0 / 3, np.float32)
    exact, bound = bd.reference([p[None] for p in planes.values()], w, 16, 16)
    want = ho.global_heat_map(planes.items(), 256, dtype=np.float64).reshape(5, -1)
    assert np.allclose(exact[0], want, rtol=0, atol=1e-6 * np.abs(want).max()) and (bound > 0).all()
    # weights are used as they are; windows are summed before the resize
    two = bd.reference([planes[(2, 1, 0)][None], planes[(4, 2, 1)][None]], np.float32([[2.0, -1.0], [0.0, 1.0]]), 16, 16)[0]
    a, b = (ho.global_heat_map([item], 256, dtype=np.float64).reshape(5, -1) for item in list(planes.items())[1:])
    assert np.allclose(two[0], 2 * a - b, atol=1e-9) and np.allclose(two[1], b, atol=1e-9)
    win = np.stack([planes[(2, 1, 0)], -0.5 * planes[(2, 1, 0)]])
    assert np.allclose(bd.reference([win], np.float32([[1.0]]), 16, 16)[0], bd.reference([0.5 * planes[(2, 1, 0)][None]], np.float32([[1.0]]), 16, 16)[0])
    # the chain the bound counts, for the key counts the device tests use: product + K + adds inside a chunk + the chunks
    c = bd.CHUNK
    assert c == 32 and [bd.n_chunks(n) for n in (1, c - 1, c, c + 1, 2 * c + 1, 1100)] == [1, 1, 1, 2, 3, 35]
    assert [bd.chain(n) for n in (1, c - 1, c, c + 1, 2 * c + 1, 1100)] == [3, 33, 34, 36, 37, 69]
    # the f32 restatement adds up, within the count
    k = np.abs(rng.standard_normal((2 * c + 1, 5, 12))).astype(np.float32)
    w = rng.standard_normal(2 * c + 1).astype(np.float32)
    w[c:2 * c] = 0.0
    like = bd.blend_like_kernel(k, w).astype(np.float64)
    exact = np.einsum('k,ktp->tp', w.astype(np.float64), k.astype(np.float64))
    assert (np.abs(like - exact) <= bd.chain(2 * c + 1) * 2.0 ** -24 * np.einsum('k,ktp->tp', np.abs(w), np.abs(k)).astype(np.float64)).all()
    assert np.array_equal(bd.blend_like_kernel(k[:3], np.float32([0, 2, 0])), (np.float32(2) * k[1]).astype(np.float32))


class FakeBlend:
    """Records every ``daam_key_blend`` call with its descriptors and its weight table decoded; returns 0."""

    def __init__(self):
        self.calls = []

    def daam_key_blend_scratch_bytes(self, n_keys, n_sets, n_rows, out_h, out_w):
        return 256 + bd.n_chunks(n_keys) * n_sets * n_rows * out_h * out_w * 4

    def daam_key_blend(self, keys, n_keys, dtype, n_rows, out_h, out_w, weights, n_sets, out, set_stride, scratch, scratch_bytes, stream):
        from daam_amd import _native as nat
        desc = [(d.base, d.win_stride, d.h, d.w, d.n_win) for d in (nat.KeyPlanes * n_keys).from_address(keys)]
        table = np.ctypeslib.as_array((ctypes.c_float * (n_sets * n_keys)).from_address(weights)).reshape(n_sets, n_keys).copy()
        self.calls.append(dict(keys=keys, desc=desc, dtype=dtype, n_rows=n_rows, out_hw=(out_h, out_w), weights=table, n_sets=n_sets, out=out,
                               set_stride=set_stride, scratch=scratch, scratch_bytes=scratch_bytes))
        return 0

    def daam_key_scores(self, keys, n_keys, *rest):
        self.calls.append(dict(keys=keys, n_keys=n_keys))
        return 0


def _tapped(E, time_bins=None, layers=(1, 0), batch=2):
    q, k = torch.zeros(batch, 64, 16, dtype=torch.float16), torch.zeros(batch, 77, 16, dtype=torch.float16)
    eng = E.HeatMapEngine(2, defer_steps=0, time_bins=time_bins)
    for layer in layers:
        eng.tap_qk(layer, q, k, 2, 0.35, 8)
    return eng


def test_engine_call(fake_engine, monkeypatch):
    E, lib = fake_engine
    fake = FakeBlend()
    monkeypatch.setattr(E.nat, 'load_analysis', lambda: fake)
    eng = _tapped(E)
    w = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    keys, maps = eng.key_blend(w, n_rows=5)
    assert keys == [(8, 0, 0), (8, 0, 1), (8, 1, 0), (8, 1, 1)] and maps.shape == (3, 5, 64, 64) and maps.dtype == torch.float32
    views = dict(eng.items())
    call = fake.calls[-1]
    assert [d[0] for d in call['desc']] == [views[k].data_ptr() for k in keys] and all(d[1:] == (0, 8, 8, 1) for d in call['desc'])
    assert (call['dtype'], call['n_rows'], call['out_hw'], call['n_sets'], call['set_stride']) == (0, 5, (64, 64), 3, 5 * 64 * 64)
    assert np.array_equal(call['weights'], w.numpy()) and call['out'] == maps.data_ptr()
    assert call['scratch'] == eng._blend_scratch.data_ptr() and call['scratch_bytes'] == eng._blend_scratch.numel() >= 256 + 3 * 5 * 64 * 64 * 4
    # the descriptors are key_scores': the same device tensor
    eng.key_scores(n_rows=5)
    assert fake.calls[-1]['keys'] == call['keys'] != 0
    # the scratch grows on demand and is kept
    grown = eng.key_blend(w)[1]
    assert grown.shape == (3, 77, 64, 64) and eng._blend_scratch.numel() >= 256 + 3 * 77 * 64 * 64 * 4
    held = eng._blend_scratch
    eng.key_blend(w, n_rows=5)
    assert eng._blend_scratch is held
    # G > 8: calls of 8 over the same descriptors, each writing its own slice of the one result
    n = len(fake.calls)
    w19 = torch.arange(19 * 4, dtype=torch.float32).reshape(19, 4)
    _, maps = eng.key_blend(w19, n_rows=2)
    assert maps.shape == (19, 2, 64, 64) and [c['n_sets'] for c in fake.calls[n:]] == [8, 8, 3]
    assert [c['out'] - maps.data_ptr() for c in fake.calls[n:]] == [0, 8 * 2 * 64 * 64 * 4, 16 * 2 * 64 * 64 * 4]
    assert np.array_equal(np.concatenate([c['weights'] for c in fake.calls[n:]]), w19.numpy())
    # filters, windows and errors are key_scores'
    assert eng.key_blend(torch.ones(1, 1), head_idx=1, layer_idx=1)[0] == [(8, 1, 1)]
    for bad in (torch.ones(1, 3), torch.ones(4), torch.ones(1, 4, dtype=torch.float64), torch.ones(0, 4)):
        with pytest.raises(ValueError, match=r'fp32 \[G, 4\].*got \(') as err:
            eng.key_blend(bad)
        assert str(tuple(bad.shape)) in str(err.value) and str(bad.dtype) in str(err.value)
    with pytest.raises(LookupError):
        eng.key_blend(torch.ones(1, 4), layer_idx=7)
    with pytest.raises(ValueError):
        eng.key_blend(torch.ones(1, 4), n_prompts=2, prompt=2)
    eng.close()
    eng = _tapped(E, time_bins=[0, 2, 4], layers=(0,))
    keys, _ = eng.key_blend(torch.ones(1, 2), bins=(1, 3))
    w1 = eng.window_items(1)
    assert fake.calls[-1]['desc'] == [(w1[k].data_ptr(), eng.acc[0].stride(0), 8, 8, 2) for k in keys]
    eng.close()


class _Tok:
    def tokenize(self, text):
        return text.split()


def _bare(eng, prompts=('a dog',)):
    from daam_amd.trace import DiffusionHeatMapHooker
    t = DiffusionHeatMapHooker.__new__(DiffusionHeatMapHooker)
    t.time_bins = None
    t.last_prompts, t.last_prompt = list(prompts), prompts[0]
    t.pipe = types.SimpleNamespace(tokenizer=_Tok())
    t.locator = types.SimpleNamespace(layer_names=['down.attn2', 'up.attn2'])
    t.engine = eng
    return t


def test_trace_builds_the_weight_table(fake_engine, monkeypatch):
    E, lib = fake_engine
    fake = FakeBlend()
    monkeypatch.setattr(E.nat, 'load_analysis', lambda: fake)
    eng = _tapped(E)
    tc = _bare(eng)                                             # key order: (8, 0, 0), (8, 0, 1), (8, 1, 0), (8, 1, 1)
    hm = tc.compute_key_heat_map([(8, 1, 0), (8, 0, 1)])
    assert hm.heat_maps.shape == (4, 64, 64) and hm.prompt == 'a dog'           # 'a dog' + 2 rows
    call = fake.calls[-1]
    assert call['n_rows'] == 4 and np.array_equal(call['weights'], np.float32([[0, 0.5, 0.5, 0]]))
    # given weights are used as they are; duplicates add; names are indices; (key, score) pairs are keys
    tc.compute_key_heat_map([(8, 'up.attn2', 1), (8, 0, 0), (8, 1, 1)], [2.0, -1.0, 0.25])
    assert np.array_equal(fake.calls[-1]['weights'], np.float32([[-1, 0, 0, 2.25]]))
    tc.compute_key_heat_map([((8, 'down.attn2', 1), 0.9), ((8, 1, 0), 0.1)], torch.tensor([3.0, 4.0]))
    assert np.array_equal(fake.calls[-1]['weights'], np.float32([[0, 3, 4, 0]]))
    tc.compute_key_heat_map(((8, 0, 0), (8, 0, 0)))              # a tuple of two keys; listed twice: 1/2 + 1/2
    assert np.array_equal(fake.calls[-1]['weights'], np.float32([[1, 0, 0, 0]]))
    # several selections: one call over the union, a zero column for every key nobody lists
    n = len(fake.calls)
    maps = tc.compute_key_heat_maps([[(8, 0, 1)], ([(8, 1, 1), (8, 0, 1)], [1.0, -1.0]), [((8, 0, 1), 7.0)]])
    assert len(fake.calls) == n + 1 and len(maps) == 3 and all(m.heat_maps.shape == (4, 64, 64) for m in maps)
    assert np.array_equal(fake.calls[-1]['weights'], np.float32([[0, 1, 0, 0], [0, -1, 0, 1], [0, 1, 0, 0]]))
    assert not fake.calls[-1]['weights'][:, [0, 2]].any()
    assert maps[1].heat_maps.data_ptr() - maps[0].heat_maps.data_ptr() == 4 * 64 * 64 * 4
    n = len(fake.calls)
    assert len(tc.compute_key_heat_maps([[(8, 0, g % 2)] for g in range(11)])) == 11
    assert [c['n_sets'] for c in fake.calls[n:]] == [8, 3]
    # errors: the key is named
    with pytest.raises(ValueError, match=r'\(8, 5, 0\).*not tapped'):
        tc.compute_key_heat_map([(8, 0, 0), (8, 5, 0)])
    with pytest.raises(ValueError, match=r'\(4, 0, 0\).*not tapped'):
        tc.compute_key_heat_map([(4, 0, 0)])
    with pytest.raises(ValueError, match="no layer named 'mid'"):
        tc.compute_key_heat_map([(8, 'mid', 0)])
    tc.locator.layer_names = ['attn-0', 'attn-0']               # the reference's names restart per block
    with pytest.raises(ValueError, match=r"layers \[0, 1\] share"):
        tc.compute_key_heat_map([(8, 'attn-0', 0)])
    with pytest.raises(ValueError, match='not tapped'):
        tc.compute_key_heat_map([(4, 'attn-0', 0)])
    with pytest.raises(ValueError, match='2 weights for 1 keys'):
        tc.compute_key_heat_map([(8, 0, 0)], [1.0, 2.0])
    with pytest.raises(ValueError, match='expected'):
        tc.compute_key_heat_map([(8, 0)])
    with pytest.raises(RuntimeError, match='No heat maps found'):
        tc.compute_key_heat_map([])
    with pytest.raises(RuntimeError, match='No heat maps found'):
        tc.compute_key_heat_maps([])
    eng.close()
    # a batch of prompts: prompt_idx is required, and heads count inside the prompt's block
    eng = _tapped(E, batch=4)
    tc = _bare(eng, prompts=('a dog', 'a big cat'))
    with pytest.raises(ValueError, match='prompt_idx'):
        tc.compute_key_heat_map([(8, 0, 0)])
    hm = tc.compute_key_heat_map([(8, 0, 1)], prompt_idx=1)
    views = dict(eng.items())
    call = fake.calls[-1]
    assert hm.heat_maps.shape[0] == 5 and hm.prompt == 'a big cat'
    assert [d[0] for d in call['desc']] == [views[(8, layer, 2 + h)].data_ptr() for layer in (0, 1) for h in (0, 1)]
    assert np.array_equal(call['weights'], np.float32([[0, 1, 0, 0]]))
    eng.close()


def test_index_of():
    from daam_amd import KeyCoattention, KeyScores
    keys = [(1, 0, 0), (1, 0, 1), (2, 3, 0)]
    ks = KeyScores(keys, torch.zeros(3, 1, 4), None, ['a', 'b', 'c', 'd'])
    ca = KeyCoattention(keys, torch.zeros(3, 4, 4), ['a', 'b', 'c', 'd'])
    for res in (ks, ca):
        assert res.index_of((2, 3, 0)) == 2 and res.index_of((2, 'd', 0)) == 2 and res.index_of(((1, 'a', 1), 0.5)) == 1
        with pytest.raises(ValueError, match='not among'):
            res.index_of((2, 3, 1))
        with pytest.raises(ValueError, match='no layer'):
            res.index_of((2, 'e', 0))
    twice = KeyScores(keys, torch.zeros(3, 1, 4), None, ['a', 'a', 'c', 'a'])    # names restart per block: the factor tells them apart
    assert twice.index_of((2, 'a', 0)) == 2 and twice.index_of((1, 'a', 1)) == 1
