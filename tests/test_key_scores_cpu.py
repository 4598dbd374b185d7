"""Head analysis without a GPU (the library itself: ``test_analysis_library_cpu.py``): the argument checks of ``daam_key_scores``
answer before any device call, one error buffer serves the library's three calls, the float64 reference of
``tests/_key_scores_domain.py`` agrees with the oracle, the engine hands ``daam_key_scores`` the descriptors the views imply (a
recording stand-in below), and the ``KeyScores`` algebra."""
import ctypes

import numpy as np
import pytest
import torch

import _key_scores_domain as kd
from _fake_native import fake_engine  # noqa: F401 -- the fixture
from oracle import heatmap_oracle as ho


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.ANALYSIS_OUT


def test_out_of_limits_arguments_are_refused_on_the_host(built):
    from daam_amd import _native as nat
    lib = nat.load_analysis()
    keys = (nat.KeyPlanes * 1)()
    scores = (ctypes.c_float * 8)()
    fp = (ctypes.c_float * 16)()
    k, s, f = ctypes.addressof(keys), ctypes.addressof(scores), ctypes.addressof(fp)
    good = dict(keys=k, n_keys=1, dtype=0, n_rows=1, out_h=4, out_w=4, footprint=f, n_masks=1, scores=s)
    bad = [dict(n_keys=0), dict(n_keys=(1 << 20) + 1), dict(n_masks=-1), dict(n_masks=33), dict(out_h=0), dict(out_h=129), dict(out_w=0),
           dict(out_w=129), dict(n_rows=0), dict(dtype=3), dict(dtype=-1), dict(keys=None), dict(scores=None), dict(footprint=None),
           dict(n_masks=0)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.daam_key_scores(a['keys'], a['n_keys'], a['dtype'], a['n_rows'], a['out_h'], a['out_w'], a['footprint'], a['n_masks'],
                                 a['scores'], None)
        assert rc == nat.E_INVALID, change
        assert lib.daam_analysis_last_error().decode(), change
        with pytest.raises(nat.DaamError):
            nat.check_analysis(rc)


def test_one_error_buffer_serves_both_calls(built):
    """A rejected ``daam_token_gram`` or ``daam_key_blend`` and then a rejected ``daam_key_scores`` on one thread: the message is the
    second call's."""
    from daam_amd import _native as nat
    lib = nat.load_analysis()
    keys = (nat.KeyPlanes * 1)()
    out = (ctypes.c_float * 16)()
    k, o = ctypes.addressof(keys), ctypes.addressof(out)
    assert lib.daam_token_gram(k, 1, 0, 97, o, o, 1 << 20, None) == nat.E_INVALID
    first = lib.daam_analysis_last_error().decode()
    assert '97 token rows' in first
    assert lib.daam_key_scores(k, 1, 0, 1, 4, 4, None, 33, o, None) == nat.E_INVALID
    second = lib.daam_analysis_last_error().decode()
    assert '33 masks' in second and '97' not in second
    assert lib.daam_key_blend(k, 1, 0, 1, 4, 4, o, 9, o, 16, o, 1 << 20, None) == nat.E_INVALID
    first = lib.daam_analysis_last_error().decode()
    assert '9 weight sets' in first and 'masks' not in first
    assert lib.daam_key_scores(k, 1, 0, 1, 4, 4, None, 33, o, None) == nat.E_INVALID
    second = lib.daam_analysis_last_error().decode()
    assert '33 masks' in second and 'weight sets' not in second
    # the checks the three calls share are reported in the same words
    assert lib.daam_token_gram(k, 0, 0, 2, o, o, 64, None) == nat.E_INVALID
    words = lib.daam_analysis_last_error().decode()
    assert lib.daam_key_scores(k, 0, 0, 1, 4, 4, None, 0, o, None) == nat.E_INVALID
    assert words and lib.daam_analysis_last_error().decode() == words
    assert lib.daam_key_blend(k, 0, 0, 1, 4, 4, o, 1, o, 16, o, 1 << 20, None) == nat.E_INVALID
    assert lib.daam_analysis_last_error().decode() == words


def test_reference_agrees_with_the_oracle_on_squares():
    rng = np.random.default_rng(2)
    planes = {(1, 0, 0): rng.standard_normal((5, 16, 16)).astype(np.float32), (2, 1, 0): rng.standard_normal((5, 8, 8)).astype(np.float32),
              (4, 2, 1): rng.standard_normal((5, 4, 4)).astype(np.float32)}
    fp = rng.standard_normal((3, 16, 16)).astype(np.float32)
    exact = [kd.reference(p[None], 16, 16, fp)[0] for p in planes.values()]
    want = fp.reshape(3, -1).astype(np.float64) @ ho.global_heat_map(planes.items(), 256, dtype=np.float64).reshape(5, -1).T
    assert np.allclose(np.mean(exact, axis=0), want, rtol=0, atol=1e-5 * np.abs(want).max())
    for key, p in planes.items():                               # ... and key by key
        one = fp.reshape(3, -1).astype(np.float64) @ ho.global_heat_map([(key, p)], 256, dtype=np.float64).reshape(5, -1).T
        assert np.allclose(kd.reference(p[None], 16, 16, fp)[0], one, rtol=0, atol=1e-5 * np.abs(one).max())
    # windows are summed before the resize; the total mass is the all-ones footprint
    two = np.stack([planes[(2, 1, 0)], -0.5 * planes[(2, 1, 0)]])
    assert np.allclose(kd.reference(two, 16, 16, None)[0], kd.reference(0.5 * planes[(2, 1, 0)][None], 16, 16, np.ones((1, 16, 16)))[0])
    # the tree the bound counts: as long as the kernel's, and it adds up
    assert kd.reduction_chain(64 * 64) == 16 + 8 and kd.reduction_chain(12 * 20) == 1 + 8
    prod = rng.standard_normal(12 * 20).astype(np.float32)
    assert abs(float(kd.reduce_like_kernel(prod)) - prod.astype(np.float64).sum()) <= kd.reduction_chain(240) * 2.0 ** -24 * np.abs(prod).sum()


class FakeAnalysis:
    """Records every ``daam_key_scores`` call with its descriptors decoded; returns 0."""

    def __init__(self):
        self.calls = []

    def daam_key_scores(self, keys, n_keys, dtype, n_rows, out_h, out_w, footprint, n_masks, scores, stream):
        from daam_amd import _native as nat
        desc = [(d.base, d.win_stride, d.h, d.w, d.n_win) for d in (nat.KeyPlanes * n_keys).from_address(keys)]
        self.calls.append(dict(desc=desc, dtype=dtype, n_rows=n_rows, out=(out_h, out_w), footprint=footprint, n_masks=n_masks, scores=scores))
        return 0


def _tapped(E, time_bins=None, layers=(1, 0), batch=2):
    q, k = torch.zeros(batch, 64, 16, dtype=torch.float16), torch.zeros(batch, 77, 16, dtype=torch.float16)
    eng = E.HeatMapEngine(2, defer_steps=0, time_bins=time_bins)
    for layer in layers:
        eng.tap_qk(layer, q, k, 2, 0.35, 8)
    return eng


def test_engine_descriptors(fake_engine, monkeypatch):
    E, lib = fake_engine
    fake = FakeAnalysis()
    monkeypatch.setattr(E.nat, 'load_analysis', lambda: fake)
    eng = _tapped(E)
    keys, scores = eng.key_scores(n_rows=5)
    # the library's key order is by slot, not by first update (layer 1 was tapped first)
    assert keys == [(8, 0, 0), (8, 0, 1), (8, 1, 0), (8, 1, 1)] and scores.shape == (4, 1, 5)
    views = dict(eng.items())
    call = fake.calls[-1]
    assert [d[0] for d in call['desc']] == [views[k].data_ptr() for k in keys]
    assert all(d[1:] == (0, 8, 8, 1) for d in call['desc'])
    assert (call['dtype'], call['n_rows'], call['out'], call['footprint'], call['n_masks']) == (0, 5, (64, 64), None, 0)
    assert call['scores'] == scores.data_ptr()
    assert eng.key_scores(n_rows=500)[1].shape[2] == 77         # the crop is 1 .. tokens
    # filters, and the descriptor tensor is cached per selection
    assert eng.key_scores(head_idx=1, layer_idx=1)[0] == [(8, 1, 1)]
    assert len(eng._ks_cache) == 2
    eng.key_scores(head_idx=1, layer_idx=1)
    assert len(eng._ks_cache) == 2
    with pytest.raises(LookupError):
        eng.key_scores(layer_idx=7)
    with pytest.raises(LookupError):
        E.HeatMapEngine(2).key_scores()
    # 70 footprints: chunks of 32, 32, 6 over the same descriptors
    fp = torch.zeros(70, 64, 64)
    n = len(fake.calls)
    _, scores = eng.key_scores(fp, n_rows=3)
    assert scores.shape == (4, 70, 3)
    assert [c['n_masks'] for c in fake.calls[n:]] == [32, 32, 6]
    assert [c['footprint'] - fp.data_ptr() for c in fake.calls[n:]] == [0, 32 * 64 * 64 * 4, 64 * 64 * 64 * 4]
    with pytest.raises(ValueError):
        eng.key_scores(torch.zeros(2, 32, 32))
    eng.close()


def test_engine_descriptors_of_prompt_blocks_and_windows(fake_engine, monkeypatch):
    E, lib = fake_engine
    fake = FakeAnalysis()
    monkeypatch.setattr(E.nat, 'load_analysis', lambda: fake)
    eng = _tapped(E, batch=4)                                    # [uncond x 2 ; cond x 2]: 4 kept entries, 2 per prompt
    views = dict(eng.items())
    keys, _ = eng.key_scores(n_prompts=2, prompt=1)
    assert keys == [(8, 0, 0), (8, 0, 1), (8, 1, 0), (8, 1, 1)]  # heads count inside the prompt's block
    assert [d[0] for d in fake.calls[-1]['desc']] == [views[(8, layer, 2 + h)].data_ptr() for layer in (0, 1) for h in (0, 1)]
    assert eng.key_scores(n_prompts=2, prompt=0, head_idx=1)[0] == [(8, 0, 1), (8, 1, 1)]
    with pytest.raises(ValueError):
        eng.key_scores(n_prompts=2, prompt=2)
    eng.close()
    eng = _tapped(E, time_bins=[0, 2, 4], layers=(0,))
    keys, _ = eng.key_scores(bins=(1, 3))
    w1 = eng.window_items(1)
    stride = eng.acc[0].stride(0)
    assert stride == 2 * 77 * 64
    assert fake.calls[-1]['desc'] == [(w1[k].data_ptr(), stride, 8, 8, 2) for k in keys]
    eng.key_scores()                                             # the whole generation: every window
    assert [d[1:] for d in fake.calls[-1]['desc']] == [(stride, 8, 8, 3)] * 2
    eng.key_scores(bins=(2, 3))
    assert [d[1:] for d in fake.calls[-1]['desc']] == [(0, 8, 8, 1)] * 2
    eng.close()


class _Tok:
    def tokenize(self, text):
        return text.split()


def test_key_scores_algebra(monkeypatch):
    from daam_amd import KeyScores, heatmap
    monkeypatch.setattr(heatmap, 'compute_token_merge_indices', lambda tok, prompt, word, idx, *a: ([1 + prompt.split().index(word)], idx))
    keys = [(1, 0, 0), (1, 0, 1), (2, 3, 0), (2, 3, 1), (2, 3, 2)]
    scores = torch.arange(5 * 2 * 4, dtype=torch.float32).reshape(5, 2, 4)
    scores[1] = scores[3]                                        # a tie between keys 1 and 3
    ks = KeyScores(keys, scores, torch.tensor([3, 4], dtype=torch.int32), ['a', 'b', 'c', 'd'], _Tok(), 'a dog')
    assert torch.equal(ks.mean(), scores.mean(dim=0))
    assert torch.equal(ks.word_scores('dog'), scores[:, :, 2])
    top = ks.top_keys('dog', region=1, k=3)
    assert [k for k, _ in top] == [(2, 3, 2), (1, 0, 1), (2, 3, 1)]            # the tie keeps the key order
    assert top[0][1] == float(scores[4, 1, 2])
    layers, by_layer = ks.by_layer()
    assert layers == [0, 3] and torch.equal(by_layer[0], scores[:2].mean(dim=0)) and torch.equal(by_layer[1], scores[2:].mean(dim=0))
    heads, by_head = ks.by_head()
    assert heads == [0, 1, 2] and torch.equal(by_head[2], scores[4]) and torch.equal(by_head[0], scores[[0, 2]].mean(dim=0))
    assert ks.cpu().keys == keys and ks.cpu().layer_names == ['a', 'b', 'c', 'd']
