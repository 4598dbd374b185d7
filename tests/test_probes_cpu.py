"""Host-side pieces of probe tracing (open-vocabulary heat maps): argument checks, the probe encoding, the probe rows, the probe
key-group table, and the deferred launch's extra chains, on a recording stand-in of the library."""
import types

import numpy as np
import pytest
import torch

from _fake_native import fake_engine  # noqa: F401 -- the recording stand-in of libdaam_hip (fixture)


def _pipe():
    from oracle import fake_diffusers as fd
    return fd.make_pipe('sd15', mini=True)


def test_probe_validation():
    from daam_amd.engine import check_probes
    assert check_probes(None) is None
    assert check_probes(['a cat']) == ('a cat',)
    assert check_probes(('a', 'b', 'c')) == ('a', 'b', 'c')
    assert len(check_probes(['x'] * 8)) == 8
    for bad in ([], ['x'] * 9, 'a cat', [1], ['a', None], 5):
        with pytest.raises(ValueError):
            check_probes(bad)
    with pytest.raises(ValueError, match='time_bins'):
        check_probes(['a cat'], time_bins=[0, 2])


def test_trace_rejects_bad_probe_arguments(tmp_path):
    import daam_amd
    pipe = _pipe()
    emb = torch.zeros(2, 77, 16)
    for kw in (dict(probes=[]), dict(probes=['x'] * 9), dict(probes=['a cat'], time_bins=[0, 2]),
               dict(probes=['a cat', 'grass'], probe_embeds=torch.zeros(3, 77, 16)),     # count mismatch
               dict(probes=['a cat', 'grass'], probe_embeds=torch.zeros(2, 76, 16)),     # not 77 tokens
               dict(probes=['a cat', 'grass'], probe_embeds=torch.zeros(2, 77)),         # not [P, 77, C]
               dict(probe_embeds=emb),                                                   # embeddings without names
               dict(probes=['a cat'], probe_embeds=emb[:1], save_heads=True, data_dir=str(tmp_path))):
        with pytest.raises(ValueError):
            daam_amd.trace(pipe, **kw)


class _Encoder:
    """``encode_prompt`` of a stand-in pipeline: SD's 2-tuple or SDXL's 4-tuple, conditional embedding first."""

    def __init__(self, n_out, width=24):
        self.n_out, self.width, self.calls = n_out, width, []
        self.device = torch.device('cpu')

    def encode_prompt(self, prompt, prompt_2=None, device=None, num_images_per_prompt=1, do_classifier_free_guidance=True,
                      negative_prompt=None):
        self.calls.append((prompt, prompt_2, device, num_images_per_prompt, do_classifier_free_guidance))
        cond = torch.full((num_images_per_prompt, 77, self.width), float(len(prompt)))
        rest = [torch.zeros(1, 77, self.width), torch.zeros(1, 5), torch.zeros(1, 5)]
        return (cond, *rest[:self.n_out - 1])


@pytest.mark.parametrize('n_out', [2, 4], ids=['sd_2tuple', 'sdxl_4tuple'])
def test_encode_prompt_takes_the_conditional_embedding(n_out):
    from daam_amd.trace import _probe_embeddings
    enc = _Encoder(n_out)
    emb = _probe_embeddings(enc, ('a cat', 'green grass'))
    assert tuple(emb.shape) == (2, 77, 24)
    assert float(emb[0, 0, 0]) == len('a cat') and float(emb[1, 3, 7]) == len('green grass')
    assert [c[0] for c in enc.calls] == ['a cat', 'green grass']
    for _, prompt_2, device, k, cfg in enc.calls:                 # encoded once each: one image, no guidance, SDXL's prompt_2 untouched
        assert prompt_2 is None and device == enc.device and k == 1 and cfg is False
    given = torch.ones(2, 77, 8)
    assert _probe_embeddings(enc, ('a', 'b'), given) is given and len(enc.calls) == 2
    with pytest.raises(ValueError, match='probe_embeds'):
        _probe_embeddings(types.SimpleNamespace(), ('a',))          # no encode_prompt: the caller must pass embeddings


def test_probe_rows_and_groups():
    """A probe map keeps ``len(tokenize(probe)) + 2`` rows and is labelled with the probe; the maps of all probes come from one
    engine call with groups = probes x prompts."""
    from daam_amd.trace import DiffusionHeatMapHooker
    from oracle import fake_diffusers as fd
    t = DiffusionHeatMapHooker.__new__(DiffusionHeatMapHooker)
    t.probes = ('a cat', 'green grass growing', 'x')
    t.pipe = types.SimpleNamespace(tokenizer=fd.FakeTokenizer())
    calls = []

    class _Eng:
        def probe_heat_maps(self, probes, n_prompts, n_rows, **kw):
            calls.append((list(probes), n_prompts, list(n_rows)))
            out = torch.zeros(len(probes) * n_prompts, 77, 4, 4)
            for g in range(out.shape[0]):
                out[g] = g
            return out
    t.engine = _Eng()
    for n_prompts in (1, 2):
        t.last_prompts = ['a dog'] if n_prompts == 1 else ['a dog', 'a bird']
        t.last_prompt = 'a dog'
        calls.clear()
        maps = t.compute_probe_heat_maps(prompt_idx=None if n_prompts == 1 else 1)
        assert calls == [([0, 1, 2], n_prompts, [4, 6, 3])]            # 'growing' is two sub-word pieces
        assert [m.prompt for m in maps] == list(t.probes)
        assert [m.heat_maps.shape[0] for m in maps] == [4, 6, 3]
        assert [float(m.heat_maps[0, 0, 0]) for m in maps] == [p * n_prompts + (n_prompts - 1) for p in range(3)]
        calls.clear()
        one = t.compute_probe_heat_map(-1, prompt_idx=0 if n_prompts == 2 else None)
        assert calls == [([2], n_prompts, [3])] and one.prompt == 'x' and one.heat_maps.shape[0] == 3
    every = t.compute_probe_heat_maps()                                   # two prompts, no prompt_idx: [probe][prompt]
    assert len(every) == 3 and all(len(row) == 2 for row in every)
    with pytest.raises(ValueError, match='prompt_idx'):
        t.compute_probe_heat_map(0)
    for bad in (3, -4, 1.0, True):
        with pytest.raises(ValueError):
            t.compute_probe_heat_map(bad, prompt_idx=0)
    t.probes = None
    with pytest.raises(ValueError, match='no probes'):
        t.compute_probe_heat_maps()


def test_probe_key_group_table():
    from daam_amd.engine import probe_key_groups, prompt_key_groups
    # two generation layers (4 and 2 kept heads) and two probes; the probes' slots come after the generation's keys
    layout = [(0, 0, 12, 1, 4), (0, 1, 16, 2, 2), (1, 0, 18, 1, 4), (1, 1, 22, 2, 2)]
    total = 24
    one = probe_key_groups(layout, total, 2, 1)
    assert one == [-1] * 12 + [0] * 6 + [1] * 6                           # the generation's keys are never selected
    two = probe_key_groups(layout, total, 2, 2)                            # batched: [cond x N] blocks of each slot
    assert two == [-1] * 12 + [0, 0, 1, 1, 0, 1] + [2, 2, 3, 3, 2, 3]
    # the same grouping as the generation's own table of each slot
    gen = prompt_key_groups([(0, 12, 1, 4), (1, 16, 2, 2)], total, 2)
    assert [g for g in gen if g >= 0] == [0, 0, 1, 1, 0, 1]
    assert probe_key_groups(layout, total, 2, 2, head_idx=1) == [-1] * 12 + [-1, 0, -1, 1, -1, -1] + [-1, 2, -1, 3, -1, -1]
    assert probe_key_groups(layout, total, 2, 1, layer_idx=1) == [-1] * 16 + [0] * 2 + [-1] * 4 + [1] * 2
    assert probe_key_groups(layout, total, 2, 1, factors=[1]) == [-1] * 12 + [0] * 4 + [-1] * 2 + [1] * 4 + [-1] * 2


@pytest.mark.parametrize('recorder', ['c++', 'python'])
@pytest.mark.parametrize('n_probes', [1, 3])
def test_deferred_launch_adds_probe_chains(fake_engine, monkeypatch, recorder, n_probes):
    from daam_amd import _native as nat
    E, lib = fake_engine
    if recorder == 'python':
        monkeypatch.setenv('DAAM_NO_FASTPATH', '1')
    q = [torch.zeros(2, 64, 16, dtype=torch.float16) for _ in range(3)]
    k = torch.zeros(2, 77, 16, dtype=torch.float16)
    eng = E.HeatMapEngine(2, defer_steps=8, n_probes=n_probes)
    keys = {layer: torch.zeros(n_probes, 77, 16, dtype=torch.float16) for layer in (0, 1)}
    for layer, kk in keys.items():
        eng.set_probe_keys(layer, kk)
    held = []
    for step in range(3):
        for layer in (1, 0):
            eng.tap_qk(layer, q[step], k, 2, 0.25, 1)
        held.append(eng._fast.held_bytes() if eng._fast is not None else eng._held)
    assert held[1] == 2 * held[0]                                       # the probes hold no Q / K of their own
    creates = [c[1] for c in lib.calls if c[0] == 'daam_ctx_create']
    assert creates[0][0] == 2 * (1 + n_probes)                          # one slot per layer and per (probe, layer)
    configured = sorted(c[1][1] for c in lib.calls if c[0] == 'daam_layer_configure')
    assert configured == sorted(range(2 * (1 + n_probes)))
    eng.flush()
    (ent,) = lib.enqueued
    gen, rest = ent[:6], ent[6:]
    assert [e[0] for e in gen] == [1, 0, 1, 0, 1, 0]
    assert len(rest) == 6 * n_probes
    for p in range(n_probes):
        part = rest[6 * p:6 * p + 6]
        assert [e[0] for e in part] == [(1 + p) * 2 + layer for layer in (1, 0, 1, 0, 1, 0)]
        assert [e[1] for e in part] == [e[1] for e in gen]              # the generation's Q, step by step
        for (layer, _, kp, desc), g in zip(part, gen):
            kk = keys[layer - (1 + p) * 2]
            assert kp == kk.data_ptr() + p * 77 * 16 * 2
            want = nat.QKDesc.from_buffer_copy(g[3])
            want.k_stride_b = 0                                          # one probe key for every kept batch entry
            assert desc == bytes(want)
    assert eng._park_key()[-1] == n_probes
    eng.close()


def test_no_probes_launch_is_unchanged(fake_engine):
    E, lib = fake_engine
    q, k = torch.zeros(2, 64, 16, dtype=torch.float16), torch.zeros(2, 77, 16, dtype=torch.float16)
    eng = E.HeatMapEngine(2, defer_steps=8)
    for _ in range(2):
        for layer in (1, 0):
            eng.tap_qk(layer, q, k, 2, 0.25, 1)
    eng.flush()
    assert [e[0] for e in lib.enqueued[0]] == [1, 0, 1, 0]
    assert [c[1][0] for c in lib.calls if c[0] == 'daam_ctx_create'] == [2]
    eng.close()


def test_probe_keys_must_match(fake_engine):
    E, lib = fake_engine
    eng = E.HeatMapEngine(2, defer_steps=8, n_probes=2)
    with pytest.raises(ValueError):
        eng.set_probe_keys(0, torch.zeros(3, 77, 16))
    with pytest.raises(ValueError):
        E.HeatMapEngine(2, n_probes=9)
    with pytest.raises(ValueError):
        E.HeatMapEngine(2, n_probes=1, time_bins=[0, 2])
    eng.close()
