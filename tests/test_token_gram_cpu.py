"""Token co-attention without a GPU (the library itself: ``test_analysis_library_cpu.py``): the argument checks of ``daam_token_gram``
answer before any device call, the engine hands it the descriptors of ``key_scores`` (a recording stand-in below), the
``KeyCoattention`` arithmetic, and the float64 reference and bound of ``tests/_gram_domain.py`` themselves."""
import ctypes

import numpy as np
import pytest
import torch

import _gram_domain as gd
from _fake_native import fake_engine  # noqa: F401 -- the fixture


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.ANALYSIS_OUT


def test_out_of_limits_arguments_are_refused_on_the_host(built):
    from daam_amd import _native as nat
    lib = nat.load_analysis()
    keys = (nat.KeyPlanes * 1)()
    gram = (ctypes.c_float * 16)()
    scratch = (ctypes.c_float * 16)()
    k, g, s = ctypes.addressof(keys), ctypes.addressof(gram), ctypes.addressof(scratch)
    good = dict(keys=k, n_keys=1, dtype=0, n_rows=2, gram=g, scratch=s, scratch_bytes=16)
    bad = [dict(n_keys=0), dict(n_keys=-1), dict(n_keys=(1 << 20) + 1, scratch_bytes=1 << 40), dict(n_rows=0), dict(n_rows=97, scratch_bytes=1 << 20),
           dict(dtype=3), dict(dtype=-1), dict(keys=None), dict(gram=None), dict(scratch=None), dict(scratch_bytes=15), dict(scratch_bytes=0)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.daam_token_gram(a['keys'], a['n_keys'], a['dtype'], a['n_rows'], a['gram'], a['scratch'], a['scratch_bytes'], None)
        assert rc == nat.E_INVALID, change
        assert lib.daam_analysis_last_error().decode(), change
        with pytest.raises(nat.DaamError):
            nat.check_analysis(rc)


def test_scratch_bytes_is_monotone(built):
    from daam_amd import _native as nat
    size = nat.load_analysis().daam_token_gram_scratch_bytes
    assert size(1, 1, 1) == 4 and size(1100, 77, 4096) == 1100 * 4 * 77 * 77 * 4
    assert size(1, 96, 1024) == size(1, 96, 1) and size(1, 96, 1025) == 2 * size(1, 96, 1024)
    assert size(1, 96, 128 * 128) == 16 * 96 * 96 * 4 == size(1, 96, 1 << 30)
    for bad in [(0, 1, 1), (1, 0, 1), (1, 97, 1), (1, 1, 0), ((1 << 20) + 1, 1, 1)]:
        assert size(*bad) == 0, bad
    last = 0
    for hw in (1, 60, 1024, 1025, 4096, 4097, 16384):
        assert size(7, 33, hw) >= last
        last = size(7, 33, hw)
    assert all(size(n + 1, 33, 4096) > size(n, 33, 4096) for n in (1, 7, 1099))
    assert all(size(7, r + 1, 4096) > size(7, r, 4096) for r in (1, 32, 95))


class FakeGram:
    """Records every ``daam_token_gram`` call with its descriptors decoded, and where ``daam_key_scores`` was given its own; returns 0."""

    def __init__(self):
        self.calls = []

    def daam_token_gram_scratch_bytes(self, n_keys, n_rows, max_hw):
        return n_keys * -(-max_hw // 1024) * n_rows * n_rows * 4 if 1 <= n_rows <= 96 else 0

    def daam_token_gram(self, keys, n_keys, dtype, n_rows, gram, scratch, scratch_bytes, stream):
        from daam_amd import _native as nat
        desc = [(d.base, d.win_stride, d.h, d.w, d.n_win) for d in (nat.KeyPlanes * n_keys).from_address(keys)]
        self.calls.append(dict(keys=keys, desc=desc, dtype=dtype, n_rows=n_rows, gram=gram, scratch=scratch, scratch_bytes=scratch_bytes))
        return 0

    def daam_key_scores(self, keys, n_keys, dtype, n_rows, out_h, out_w, footprint, n_masks, scores, stream):
        self.calls.append(dict(keys=keys, n_keys=n_keys))
        return 0


def _tapped(E, time_bins=None, layers=(1, 0), batch=2):
    q, k = torch.zeros(batch, 64, 16, dtype=torch.float16), torch.zeros(batch, 77, 16, dtype=torch.float16)
    eng = E.HeatMapEngine(2, defer_steps=0, time_bins=time_bins)
    for layer in layers:
        eng.tap_qk(layer, q, k, 2, 0.35, 8)
    return eng


def test_engine_descriptors_are_those_of_key_scores(fake_engine, monkeypatch):
    E, lib = fake_engine
    fake = FakeGram()
    monkeypatch.setattr(E.nat, 'load_analysis', lambda: fake)
    eng = _tapped(E)
    keys, gram = eng.token_gram(n_rows=5)
    assert keys == [(8, 0, 0), (8, 0, 1), (8, 1, 0), (8, 1, 1)] and gram.shape == (4, 5, 5) and gram.dtype == torch.float32
    views = dict(eng.items())
    call = fake.calls[-1]
    assert [d[0] for d in call['desc']] == [views[k].data_ptr() for k in keys]
    assert all(d[1:] == (0, 8, 8, 1) for d in call['desc'])
    assert (call['dtype'], call['n_rows'], call['gram']) == (0, 5, gram.data_ptr())
    assert call['scratch_bytes'] >= 4 * 5 * 5 * 4 and call['scratch'] == eng._gram_scratch.data_ptr()
    held = eng._gram_scratch.data_ptr()
    assert eng.token_gram(n_rows=500)[1].shape == (4, 77, 77)   # the crop is 1 .. tokens; the scratch has grown
    assert eng._gram_scratch.numel() >= 4 * 77 * 77 * 4
    grown = eng._gram_scratch
    eng.token_gram(n_rows=5)
    assert eng._gram_scratch is grown and held is not None      # ... and is kept
    # the selection and its cache are key_scores': one library, one preamble, the same descriptors on the device
    eng.key_scores(n_rows=5)
    eng.token_gram(n_rows=5)
    assert fake.calls[-1]['keys'] == fake.calls[-2]['keys'] != 0 and fake.calls[-2]['n_keys'] == len(fake.calls[-1]['desc']) == 4
    assert eng.token_gram(head_idx=1, layer_idx=1)[0] == [(8, 1, 1)]
    n = len(eng._ks_cache)
    eng.token_gram(head_idx=1, layer_idx=1)
    assert len(eng._ks_cache) == n
    with pytest.raises(LookupError):
        eng.token_gram(layer_idx=7)
    with pytest.raises(LookupError):
        E.HeatMapEngine(2).token_gram()
    with pytest.raises(ValueError):
        eng.token_gram(n_prompts=2, prompt=2)
    eng.close()
    eng = _tapped(E, time_bins=[0, 2, 4], layers=(0,))
    keys, _ = eng.token_gram(bins=(1, 3))
    w1 = eng.window_items(1)
    stride = eng.acc[0].stride(0)
    assert fake.calls[-1]['desc'] == [(w1[k].data_ptr(), stride, 8, 8, 2) for k in keys]
    eng.close()


class _Tok:
    def tokenize(self, text):
        return text.split()


def _merge(tok, prompt, word, idx, *a):
    """A stand-in for ``compute_token_merge_indices``: 'big dog' style words own several rows; ``word_idx`` picks an occurrence."""
    words = prompt.split()
    at = [i for i, w in enumerate(words) if w == word]
    if not at:
        raise ValueError(word)
    first = at[0 if idx is None else idx]
    return ([1 + first, 2 + first] if word == 'dog' else [1 + first]), first


def test_key_coattention_algebra(monkeypatch):
    from daam_amd import KeyCoattention, coattention
    monkeypatch.setattr(coattention, 'compute_token_merge_indices', _merge)
    rng = np.random.default_rng(4)
    keys = [(1, 0, 0), (1, 0, 1), (2, 3, 0), (2, 3, 1), (2, 3, 2)]
    planes = rng.random((5, 7, 24))                              # [K, rows, hw] float64
    planes[:, 6] = 0.0                                           # a row of zeros
    planes[1] = planes[3]                                        # a tie between keys 1 and 3
    gram = torch.from_numpy(planes @ planes.transpose(0, 2, 1)).float()
    ca = KeyCoattention(keys, gram, ['down', 'l1', 'l2', 'up'], _Tok(), 'a dog x cat and cat')
    # cosine: the definition, and the zero row is 0 rather than NaN
    cos = ca.cosine()
    assert np.allclose(cos.numpy(), gd.cosine(gram.double().numpy()), atol=1e-6)
    assert torch.isfinite(cos).all() and float(cos[:, 6].abs().max()) == 0.0 and float(cos[:, :, 6].abs().max()) == 0.0
    assert torch.equal(ca.mean(), cos.mean(dim=0))
    # block means against explicitly merged word maps, float64: 'dog' owns rows 2, 3; 'cat' row 4 (or 6 with word_idx)
    got = ca.of('dog', 'cat').double().numpy()
    want = np.array([gd.word_cosine(planes[k], [2, 3], [4]) for k in range(5)])
    assert np.abs(got - want).max() <= 1e-6
    got = ca.of('dog', 'cat', word_idx_b=1).double().numpy()     # the second 'cat': row 6, all zeros
    assert got.shape == (5,) and np.abs(got).max() == 0.0
    assert np.abs(ca.of('dog', 'dog').numpy() - 1.0).max() <= 1e-6
    # top_keys: order, ties keep the key order, layer names
    col = ca.of('dog', 'cat')
    top = ca.top_keys('dog', 'cat', k=5)
    order = torch.sort(col, descending=True, stable=True).indices.tolist()
    assert [k for k, _ in top] == [(keys[i][0], ca.layer_names[keys[i][1]], keys[i][2]) for i in order]
    assert order.index(1) + 1 == order.index(3) and top[0][1] == float(col[order[0]])
    low = ca.top_keys('dog', 'cat', k=2, largest=False)
    assert [v for _, v in low] == sorted(col.tolist())[:2]
    # by_layer / by_head: KeyScores' shape
    layers, by_layer = ca.by_layer()
    assert layers == [0, 3] and by_layer.shape == (2, 7, 7) and torch.equal(by_layer[1], cos[2:].mean(dim=0))
    heads, by_head = ca.by_head('dog', 'cat')
    assert heads == [0, 1, 2] and by_head.shape == (3,) and torch.equal(by_head[0], col[[0, 2]].mean(dim=0))
    assert ca.by_layer('dog', 'cat')[1].shape == (2,) and ca.by_head()[1].shape == (3, 7, 7)
    with pytest.raises(ValueError):
        ca.by_layer('dog')
    assert ca.cpu().keys == keys and ca.cpu().layer_names == ca.layer_names and torch.equal(ca.cpu().gram, gram)


def test_domain_reference_and_bound():
    rng = np.random.default_rng(6)
    win = rng.standard_normal((3, 9, 60)).astype(np.float32)
    exact, bnd = gd.reference(win, True)
    assert np.allclose(exact, np.einsum('wip,vjp->ij', win.astype(np.float64), win.astype(np.float64)), rtol=1e-12, atol=1e-12)
    assert (bnd > 0).all() and np.array_equal(exact, exact.T)
    one, bnd1 = gd.reference(win[:1], False)
    assert np.allclose(one, np.einsum('ip,jp->ij', win[0].astype(np.float64), win[0].astype(np.float64)), rtol=1e-12, atol=1e-12)
    # the counted chain: as long as the kernel's, per path
    assert gd.chain(1, False) == 32 + 2 and gd.chain(1024, False) == 256 + 2 and gd.chain(4096, False) == 256 + 2 + 3
    assert gd.chain(60, True) == 16 + 2 and gd.chain(1024, True) == 256 + 2 and gd.chain(128 * 128, True) == 256 + 2 + 15
    assert gd.chain(1056, False) == 256 + 2 + 1 and gd.n_chunks(1024) == 1 and gd.n_chunks(1025) == 2
    # the bound scales with hw: the same rows tiled four times have four times the products and a chain at least as long
    _, small = gd.reference(np.abs(win[:1, :, :32]), False)
    _, large = gd.reference(np.tile(np.abs(win[:1, :, :32]), (1, 1, 40)), False)
    assert (large >= 40 * small).all()
    # the windows' term is there
    _, no_win = gd.reference(win.sum(axis=0, dtype=np.float64)[None], True)
    assert (bnd > no_win).all()
    assert gd.worst_ratio(exact.astype(np.float32), exact, bnd, 'float64 rounded to f32') <= 1.0
