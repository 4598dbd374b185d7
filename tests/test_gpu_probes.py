"""Open-vocabulary heat maps (``trace(..., probes=[...])``): each probe's sums against a generation whose context IS the probe
(the stand-in UNet's hidden states do not depend on the context, so the queries are the same) on every tap route, the generation
itself unchanged, probe maps against the oracle, batched prompts, word lookup, and the SDXL-1024 stack against the reference's
processor."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fake_diffusers as fd
from oracle import heatmap_oracle as ho

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
STEPS = 3
PROBES = ['a cat', 'green grass growing', 'one small red bird']


class _Crop(torch.nn.Module):
    """``norm_cross`` of the stand-in layers: the first ``width`` channels of the encoder states, so that one probe embedding feeds
    layers of different widths (identity projections make each layer's key width its inner width)."""

    def __init__(self, width):
        super().__init__()
        self.width = width

    def forward(self, e):
        return e[..., :self.width].contiguous()


def _crop_layers(pipe) -> int:
    widths = []
    for spec in pipe.unet.execution_order():
        spec.module.norm_cross = _Crop(spec.module.to_v.in_features)
        widths.append(spec.module.to_v.in_features)
    return max(widths)


def _pipe(kind, dtype):
    if kind == 'sdxl64':                       # head_dim 64, fp16 sums: generation and probe chains pair up on tap_pair_kernel
        pipe = fd.make_pipe('sdxl', device=DEV, dtype=dtype, seed=5, mini=True, identity_proj=True, dim_head=64, heads_scale=0.2,
                            tblocks_cap=1)
    elif kind == 'sd15_full':                    # head_dim 40 / 80 / 160: the slab, chunked and wide kernels
        pipe = fd.make_pipe('sd15', device=DEV, dtype=dtype, seed=5, mini=False, identity_proj=True)
    else:
        unet = dict(dim_head=16, heads_scale=0.2, tblocks_cap=1) if kind == 'sdxl' else dict(dim_head=16)
        pipe = fd.make_pipe(kind, device=DEV, dtype=dtype, seed=5, mini=True, identity_proj=True, **unet)
    return pipe, _crop_layers(pipe)


def _embeds(n, width, dtype, seed=11):
    g = torch.Generator(device='cpu').manual_seed(seed)
    e = torch.randn(n, 77, width, generator=g)
    e[:, 0] *= 3.0
    return e.to(dtype).to(DEV)


def _swapped(pipe, emb_row):
    """The pipe's context replaced by one probe embedding (every batch row)."""
    pipe.context = lambda i, spec: emb_row[None].expand(pipe.batch, 77, emb_row.shape[-1]).contiguous()


def _restore(pipe):
    pipe.__dict__.pop('context', None)


def _set_env(monkeypatch, env):
    monkeypatch.setenv('DAAM_NO_CTX_POOL', '1')                  # a fresh context reads the route switches
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# (name, pipe kind, dtype, trace kwargs, environment, reference kwargs, reference environment, kernel the probes' taps ran on)
ROUTES = [
    ('pair', 'sdxl64', torch.float16, {}, dict(DAAM_TAP_PAIR='1'), None, None, 'tap_pair_kernel'),
    ('pair_off', 'sdxl64', torch.float16, {}, {}, None, None, 'tap_d64_kernel'),            # the default: separate chains
    ('pair_split', 'sdxl64', torch.float16, {}, dict(DAAM_TAP_PAIR='1', DAAM_DEFER_BYTES='1'), None, None, 'tap_pair_kernel'),
    ('pair_acc32', 'sdxl64', torch.float16, dict(accumulate='float32'), dict(DAAM_TAP_PAIR='1'), None, None, 'tap_d64_kernel'),
    ('d64', 'sdxl', torch.float16, {}, {}, None, None, 'tap_d64_kernel'),
    ('slab', 'sd15_full', torch.float16, {}, {}, None, None, 'tap_slab_kernel'),
    ('chunk_f16', 'sd15_full', torch.float16, {}, dict(DAAM_TAP_SLAB='0'), None, None, 'tap_chunk_kernel'),
    ('chunk_bf16', 'sd15_full', torch.bfloat16, {}, {}, None, None, 'tap_chunk_kernel'),
    ('wide', 'sd15_full', torch.float16, {}, dict(DAAM_TAP_SLAB='0', DAAM_TAP_CHUNKED='0'), None, None, 'tap_wide_kernel'),
    ('mfma', 'sdxl', torch.float16, {}, dict(DAAM_NO_D64='1'), None, None, 'tap_mfma_kernel'),
    ('any_shape', 'sdxl', torch.float32, {}, {}, None, None, 'tap_generic_kernel'),
    ('attend', 'sdxl', torch.float16, dict(defer_steps=0), {}, None, None, 'tap_d64_kernel'),
    ('no_attend', 'sdxl', torch.float16, {}, dict(DAAM_NO_ATTEND='1'), None, None, 'tap_d64_kernel'),
    # the materialised route taps its probes with daam_tap_qk on the same Q: the reference is the immediate stand-alone tap
    ('probs', 'sdxl', torch.float16, dict(tap='probs'), {}, dict(defer_steps=0), dict(DAAM_NO_ATTEND='1'), 'tap_d64_kernel'),
    ('split_launch', 'sdxl', torch.float16, {}, dict(DAAM_DEFER_BYTES='1'), None, None, 'tap_d64_kernel'),
    ('acc32', 'sdxl', torch.float16, dict(accumulate='float32'), {}, None, None, 'tap_d64_kernel'),
]


@pytest.mark.parametrize('n_probes', [1, 2, 3])
@pytest.mark.parametrize('route', ROUTES, ids=[r[0] for r in ROUTES])
def test_probe_equals_swapped_context_generation(route, n_probes, monkeypatch):
    import daam_amd
    name, kind, dtype, kw, env, ref_kw, ref_env, kernel = route
    _set_env(monkeypatch, env)
    pipe, width = _pipe(kind, dtype)
    emb = _embeds(n_probes, width, dtype)
    probes = PROBES[:n_probes]
    prompt = 'a dog on a bench'
    pipe.keep_outputs = True
    # the generation without probes
    with daam_amd.trace(pipe, **kw) as tc:
        pipe(prompt, num_inference_steps=STEPS)
        plain_outs = [o.clone() for o in pipe.last_outputs]
        plain_raw = {k: v.clone() for k, v in tc.all_heat_maps}
        plain_map = tc.compute_global_heat_map().heat_maps.clone()
        plain_kernels = tc.engine.last_kernels(0)
    # the same generation with probes
    with daam_amd.trace(pipe, probes=probes, probe_embeds=emb, **kw) as tc:
        pipe(prompt, num_inference_steps=STEPS)
        outs = [o.clone() for o in pipe.last_outputs]
        launches = tc.engine.last_flush()['launches']
        got = [{k: v.clone() for k, v in tc.raw_probe_heat_maps(p).items()} for p in range(n_probes)]
        names = tc.engine.last_kernels(0)
        if not kw and name not in ('no_attend', 'split_launch', 'pair_split'):
            assert tc.engine.last_flush()['launches'] == launches + 1      # generation and probes: one tap launch
        gen_raw = {k: v.clone() for k, v in tc.all_heat_maps}
        gen_map = tc.compute_global_heat_map().heat_maps
        maps = tc.compute_probe_heat_maps()
        assert 'grouped' in tc.engine.last_kernels(1) or n_probes == 1
        one = [tc.compute_probe_heat_map(p).heat_maps for p in range(n_probes)]
    pipe.keep_outputs = False
    assert kernel in names.split('+'), names
    assert 'tap_pair_kernel' not in plain_kernels                   # without probes no two chains share a Q
    if kernel == 'tap_pair_kernel':                                  # generation + probe 0, probe 1 + probe 2: an even P leaves one chain alone
        assert ('tap_d64_kernel' in names.split('+')) == (n_probes % 2 == 0), names
    else:
        assert 'tap_pair_kernel' not in names
        assert kernel in plain_kernels.split('+') or name in ('attend', 'probs'), plain_kernels
    # the generation does not change
    assert all(torch.equal(a, b) for a, b in zip(outs, plain_outs))
    assert list(gen_raw) == list(plain_raw) and all(torch.equal(gen_raw[k], v) for k, v in plain_raw.items())
    # the same finalize calls on the same sums; their f32 atomics may add the chunks in another order from call to call
    assert (gen_map - plain_map).abs().max().item() <= 1e-6
    # each probe: the generation of the swapped context, bit for bit
    _set_env(monkeypatch, ref_env or {})
    for p in range(n_probes):
        _swapped(pipe, emb[p])
        try:
            with daam_amd.trace(pipe, **(kw if ref_kw is None else ref_kw)) as tc:
                pipe(prompt, num_inference_steps=STEPS)
                want = {k: v.clone() for k, v in tc.all_heat_maps}
                want_map = tc.compute_global_heat_map(prompt=probes[p]).heat_maps
        finally:
            _restore(pipe)
        assert list(got[p]) == list(want)
        for key, v in want.items():
            assert torch.equal(got[p][key], v), (name, p, key)
        assert maps[p].prompt == probes[p] and maps[p].heat_maps.shape == want_map.shape
        assert (maps[p].heat_maps - want_map).abs().max().item() <= 1e-6
        assert (one[p] - want_map).abs().max().item() <= 1e-6


def _replay(cpu, emb_row, steps, dtype):
    """Numpy oracle of a generation whose context is ``emb_row`` (the probe), on the CPU twin of the pipe."""
    np_dtype = {torch.float16: np.float16, torch.float32: np.float32}[dtype]
    raw = ho.RawMaps(np_dtype)
    modules, _ = ho.locate(cpu.unet)
    index_of = {id(m): i for i, m in enumerate(modules)}
    lat = ho.latent_hw_for(cpu.unet.config.sample_size, cpu.vae_scale_factor)
    order = cpu.unet.execution_order()
    with torch.no_grad():
        for step in steps:
            for i, spec in enumerate(order):
                li = index_of.get(id(spec.module))
                if li is None:
                    continue
                a = spec.module
                ctx = emb_row[None].expand(cpu.batch, 77, emb_row.shape[-1])[..., :a.to_v.in_features]
                q = a.head_to_batch_dim(a.to_q(cpu.hidden_states(i, spec, step))).cpu().numpy()
                k = a.head_to_batch_dim(a.to_k(ctx.contiguous())).cpu().numpy()
                ho.tap(raw, li, q, k, a.scale, lat, np_dtype)
    return raw, lat


@pytest.mark.parametrize('kind', ['sd15', 'sdxl'])
@pytest.mark.parametrize('dtype,tol', [(torch.float16, 1e-3), (torch.float32, 2e-6)], ids=['f16', 'f32'])
def test_probe_maps_against_oracle(kind, dtype, tol):
    import daam_amd
    pipe, width = _pipe(kind, dtype)
    unet = dict(dim_head=16, heads_scale=0.2, tblocks_cap=1) if kind == 'sdxl' else dict(dim_head=16)
    cpu = fd.make_pipe(kind, device='cpu', dtype=dtype, seed=5, mini=True, identity_proj=True, **unet)
    emb = _embeds(2, width, dtype)
    with daam_amd.trace(pipe, probes=PROBES[:2], probe_embeds=emb) as tc:
        pipe('a dog on a bench', num_inference_steps=STEPS)
        got = [m.heat_maps.cpu().numpy() for m in tc.compute_probe_heat_maps()]
        got_norm = tc.compute_probe_heat_map(1, normalize=True).heat_maps.cpu().numpy()
        got_layer = tc.compute_probe_heat_map(0, layer_idx=1).heat_maps.cpu().numpy()
    for p in range(2):
        raw, lat = _replay(cpu, emb[p].cpu(), range(STEPS), dtype)
        n_rows = len(cpu.tokenizer.tokenize(PROBES[p])) + 2
        want = ho.global_heat_map(list(raw), lat, n_rows=n_rows)
        scale = max(1.0, float(np.abs(want).max())) if dtype is torch.float32 else 1.0
        assert got[p].shape == want.shape
        assert np.abs(got[p] - want).max() <= tol * scale, (p, np.abs(got[p] - want).max())
        if p == 1:
            want_norm = ho.global_heat_map(list(raw), lat, n_rows=n_rows, normalize=True)
            assert np.abs(got_norm - want_norm).max() <= tol * max(1.0, float(np.abs(want_norm).max()))
        else:
            want_layer = ho.global_heat_map([kv for kv in raw if kv[0][1] == 1], lat, n_rows=n_rows)
            assert np.abs(got_layer - want_layer).max() <= tol * scale


def _mp():
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import test_gpu_multi_prompt as mp
    return mp


@pytest.mark.parametrize('kind', ['sd15', 'sdxl'])
@pytest.mark.parametrize('route', [dict(), dict(defer_steps=0), dict(tap='probs')], ids=['deferred', 'immediate', 'probs'])
def test_batched_prompts_probe_maps(kind, route):
    """N = 2 prompts x k = 2 images: each prompt's probe maps equal those of its single-prompt generation."""
    import daam_amd
    mp = _mp()
    pipe = mp._pipe(kind, torch.float16)
    width = _crop_layers(pipe)
    emb = _embeds(2, width, torch.float16)
    prompts = mp.PROMPTS[:2]
    want = []
    for prompt in prompts:
        with daam_amd.trace(pipe, probes=PROBES[:2], probe_embeds=emb, **route) as tc:
            pipe(prompt, num_inference_steps=STEPS, num_images_per_prompt=2)
            want.append([m.heat_maps.clone() for m in tc.compute_probe_heat_maps()])
    with daam_amd.trace(pipe, batch_prompts=True, probes=PROBES[:2], probe_embeds=emb, **route) as tc:
        pipe(prompts, num_inference_steps=STEPS, num_images_per_prompt=2)
        every = tc.compute_probe_heat_maps()
        assert len(every) == 2 and all(len(row) == 2 for row in every)
        for p in range(2):
            for i in range(2):
                assert (every[p][i].heat_maps - want[i][p]).abs().max().item() <= 1e-6, (p, i)
                one = tc.compute_probe_heat_map(p, prompt_idx=i).heat_maps
                assert (one - want[i][p]).abs().max().item() <= 1e-6
        with pytest.raises(ValueError, match='prompt_idx'):
            tc.compute_probe_heat_map(0)


def test_word_lookup_and_encode_prompt():
    """A probe's words are looked up in the probe's map; on the generation's own map the same word raises as before.  Without
    probe_embeds the probes go through the pipeline's encode_prompt."""
    import daam_amd
    pipe, width = _pipe('sdxl', torch.float16)
    table = {p: _embeds(1, width, torch.float16, seed=20 + i)[0] for i, p in enumerate(PROBES)}
    seen = []

    def encode_prompt(prompt, prompt_2=None, device=None, num_images_per_prompt=1, do_classifier_free_guidance=True):
        seen.append((prompt, num_images_per_prompt, do_classifier_free_guidance))
        e = table[prompt][None]
        return e, torch.zeros_like(e), torch.zeros(1, 8), torch.zeros(1, 8)      # SDXL's 4-tuple
    pipe.encode_prompt = encode_prompt
    with daam_amd.trace(pipe, probes=['a cat', 'green grass growing']) as tc:
        out = pipe('a dog on a bench', num_inference_steps=STEPS)
        assert seen == [('a cat', 1, False), ('green grass growing', 1, False)]
        cat = tc.compute_probe_heat_map(0)
        word = cat.compute_word_heat_map('cat')
        assert word.heatmap.shape == (64, 64) and bool(torch.isfinite(word.heatmap).all())
        grass = tc.compute_probe_heat_map(1).compute_word_heat_map('growing')      # a word of two sub-word pieces
        assert grass.heatmap.shape == (64, 64)
        with pytest.raises(Exception):
            tc.compute_global_heat_map().compute_word_heat_map('cat')
        with_embeds = tc.compute_probe_heat_maps()
    with daam_amd.trace(pipe, probes=['a cat', 'green grass growing'],
                        probe_embeds=torch.stack([table['a cat'], table['green grass growing']])) as tc:
        pipe('a dog on a bench', num_inference_steps=STEPS)
        again = tc.compute_probe_heat_maps()
    for a, b in zip(with_embeds, again):
        assert (a.heat_maps - b.heat_maps).abs().max().item() <= 1e-6
    assert out.images


def _integration():
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import test_gpu_integration as gi
    return gi


def test_full_size_sdxl_two_probes_against_reference_processor(monkeypatch):
    """SDXL-1024 x 50 steps with 2 probes (one tap launch for generation and probes) against the reference's processor restated in
    torch on the swapped context, within the bound of tests/test_gpu_integration.py (global maps <= 1e-3 max-abs).  The generation and
    probe 0 run paired on tap_pair_kernel, probe 1 alone on tap_d64_kernel, side by side in the one launch."""
    import daam_amd
    monkeypatch.setenv('DAAM_NO_CTX_POOL', '1')
    monkeypatch.setenv('DAAM_TAP_PAIR', '1')
    gi = _integration()
    pipe = fd.make_pipe('sdxl', device=DEV, dtype=torch.float16, batch=2, seed=3, mini=False, identity_proj=False)
    gi._resident_inputs(pipe, n_sets=4)
    context = pipe.context
    g = torch.Generator(device=DEV).manual_seed(9)
    emb = torch.randn(2, 77, pipe.unet.cross_dim, generator=g, device=DEV, dtype=torch.float16) * 3.0
    emb[:, 0] *= 3.0
    probes = ['a photo of a cat', 'green grass']
    steps = 50
    with daam_amd.trace(pipe, probes=probes, probe_embeds=emb) as tc:
        pipe('a photo of a monkey riding a bicycle', num_inference_steps=steps)
        maps = [m.heat_maps.clone() for m in tc.compute_probe_heat_maps()]
        flush = tc.engine.last_flush()
        assert flush['kernels'] == 2 and flush['max_steps'] == steps, flush          # generation + probe 0 paired, probe 1 alone
        assert sorted(tc.engine.last_kernels(0).split('+')) == ['tap_d64_kernel', 'tap_pair_kernel'], tc.engine.last_kernels(0)
    errs = []
    for p in range(2):
        pipe.context = lambda i, spec, e=emb[p]: e[None].expand(pipe.batch, 77, e.shape[-1])
        try:
            ref = gi._reference_generation(pipe, probes[p], steps, 4096)
        finally:
            pipe.context = context
        assert maps[p].shape == ref['glob'].shape
        errs.append((maps[p] - ref['glob']).abs().max().item())
    gi._report('sdxl1024_probes', dict(config='SDXL-1024 stack, fp16, 2 probes, %d steps' % steps, probe_global_max_abs=errs))
    assert max(errs) <= 1e-3, errs
