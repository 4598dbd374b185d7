"""Per-prompt heat maps from one batched generation: ``daam_finalize_groups`` against per-group ``daam_finalize`` calls for
every finalize class, and ``trace(..., batch_prompts=True)`` against one single-prompt generation per prompt."""
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import fake_diffusers as fd
from oracle import heatmap_oracle as ho

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _dev(a, dtype):
    if dtype is ho.BF16:
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('sides', [(32, 64), (16, 32, 64), (128, 64), (24, 48, 96), (32,)])
@pytest.mark.parametrize('acc', ['float16', 'float32', 'bfloat16'])
def test_finalize_groups_matches_per_group_finalize(sides, acc):
    """Uneven groups, per-group n_rows with sentinel rows left untouched, one launch per class whatever N is."""
    import ctypes
    from daam_amd import _native as nat
    from daam_amd.engine import HeatMapEngine
    rng = np.random.default_rng(len(sides) * 31 + sides[0])
    out_side = 96 if 96 in sides else 64
    heads = 6
    eng = HeatMapEngine(len(sides), tokens=77, out_side=out_side, accumulate='float32' if acc == 'float32' else 'exact')
    np_dt = ho.BF16 if acc == 'bfloat16' else acc
    for layer, side in enumerate(sides):
        planes = rng.standard_normal((2 * heads, side * side, 77)).astype(np.float32) * 3
        planes = ho.round_bf16(planes) if acc == 'bfloat16' else planes.astype(acc)
        eng.tap_probs(layer, _dev(planes, np_dt), factor=out_side // side if side <= out_side else 0)
    lib, stream, plane = eng.lib, eng.stream, out_side * out_side
    total = heads * len(sides)
    names_seen = set()
    for n in (1, 2, 3, 4):
        groups = rng.integers(-1, n, total)
        groups[:n] = np.arange(n)                                # every group has a key
        rows = [int(r) for r in rng.integers(1, 78, n)]
        buf = torch.full((n, 77, out_side, out_side), -123.0, device=DEV)
        nat.check(lib.daam_finalize_groups(eng.ctx, (ctypes.c_int32 * total)(*groups.tolist()), n, (ctypes.c_int32 * n)(*rows),
                                           buf.data_ptr(), 77 * plane, stream))
        names = eng.last_kernels(1)
        for g in range(n):
            want = torch.full((77, out_side, out_side), -123.0, device=DEV)
            mask = (ctypes.c_uint8 * total)(*(groups == g).astype(np.uint8).tolist())
            nat.check(lib.daam_finalize(eng.ctx, mask, rows[g], want.data_ptr(), stream))
            np.testing.assert_allclose(buf[g, :rows[g]].cpu().numpy(), want[:rows[g]].cpu().numpy(), rtol=0, atol=1e-6,
                                       err_msg=f'{sides} {acc} n={n} group {g}')
            assert bool((buf[g, rows[g]:] == -123.0).all())
        if n > 1:
            parts = re.split(r'\+(?![^<]*>)', names)            # '+' between kernels, not inside <...>
            assert len(parts) == len(set(parts)) and all('grouped' in p for p in parts), names
            names_seen.add(names)
    assert len(names_seen) == 1, names_seen                      # the same launches for N = 2, 3, 4
    # an empty group, a bad group index
    groups = np.zeros(total, np.int32)
    rc = lib.daam_finalize_groups(eng.ctx, (ctypes.c_int32 * total)(*groups.tolist()), 2, (ctypes.c_int32 * 2)(77, 77),
                                  buf.data_ptr(), 77 * plane, stream)
    assert rc == nat.E_NOMAPS
    groups[0] = 5
    rc = lib.daam_finalize_groups(eng.ctx, (ctypes.c_int32 * total)(*groups.tolist()), 2, (ctypes.c_int32 * 2)(77, 77),
                                  buf.data_ptr(), 77 * plane, stream)
    assert rc == nat.E_INVALID
    eng.close()


class _PerPrompt:
    """Hidden states / contexts drawn from a generator seeded by (prompt text, CFG half, image, layer, step), in the diffusers CFG
    layout [uncond x N*k ; cond x N*k] (prompt p's k images in rows p*k ... of each half): N single-prompt generations and one
    N-prompt generation see the same per-prompt Q / K.  ``encode_prompt`` takes the arguments of diffusers' SD pipeline
    (positionally, as its ``__call__`` passes them), and every sample gets its own image."""
    prompts = ['']
    k = 1
    told = None                         # (images per prompt, guidance) passed to encode_prompt instead of the real ones

    def encode_prompt(self, prompt, device, num_images_per_prompt, do_classifier_free_guidance, negative_prompt=None):
        self.encoded = (num_images_per_prompt, do_classifier_free_guidance)

    def _rows(self, key, shape):
        out = []
        for half in (0, 1):
            for p in self.prompts:
                for j in range(self.k):
                    g = torch.Generator(device='cpu')
                    g.manual_seed(zlib.crc32(f'{p}|{half}|{j}|{key}'.encode()) & 0x7FFFFFFF)
                    out.append(torch.randn(*shape, generator=g))
        return torch.stack(out)

    def hidden_states(self, i, spec, step):
        return self._rows((1, i, step), (spec.res * spec.res, spec.query_dim)).to(self.dtype).to(self.device)

    def context(self, i, spec):
        c = self._rows((2, i), (77, spec.module.to_v.in_features))
        c[:, 0, :] *= self.sos_gain
        return c.to(self.dtype).to(self.device)

    def __call__(self, prompt, num_inference_steps=5, num_images_per_prompt=1, **kw):
        # diffusers' order: check_inputs, then encode_prompt, then the denoising loop
        self.prompts = [prompt] if isinstance(prompt, str) else list(prompt)
        self.k = num_images_per_prompt
        self.batch = 2 * len(self.prompts) * self.k
        self.check_inputs(prompt, 512, 512, 1)
        told_k, told_cfg = self.told or (num_images_per_prompt, True)
        self.encode_prompt(prompt, self.device, told_k, told_cfg)
        with torch.no_grad():
            for step in range(num_inference_steps):
                self.unet(self.hidden_states, self.context, step, self.mask_fn)
        return self._finish([f'image-of:{p}#{j}' for p in self.prompts for j in range(self.k)])


class _SD(_PerPrompt, fd.StableDiffusionPipeline):
    pass


class _SDXL(_PerPrompt, fd.StableDiffusionXLPipeline):
    pass


def _pipe(kind, dtype, mini=True):
    unet = {} if not mini else dict(dim_head=16, heads_scale=0.2, tblocks_cap=1) if kind == 'sdxl' else dict(dim_head=16)
    base = fd.make_pipe(kind, device=DEV, dtype=dtype, seed=5, mini=mini, identity_proj=True, **unet)
    pipe = (_SDXL if kind == 'sdxl' else _SD)(base.unet, device=DEV, dtype=dtype)
    pipe.seed = 5
    return pipe


PROMPTS = ['a dog', 'a cat on a red mat', 'three small birds sitting on one long wire']


@pytest.mark.parametrize('kind', ['sd15', 'sdxl'])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize('route', [dict(), dict(defer_steps=0), dict(tap='probs'), dict(accumulate='float32')])
def test_batched_equals_sequential(kind, dtype, route):
    import daam_amd
    pipe = _pipe(kind, dtype)
    single_raw, single_maps = [], []
    for p in PROMPTS:
        with daam_amd.trace(pipe, **route) as tc:
            pipe(p, num_inference_steps=3)
            single_raw.append({k: v.clone() for k, v in tc.all_heat_maps})
            single_maps.append(tc.compute_global_heat_map().heat_maps.clone())
    with daam_amd.trace(pipe, batch_prompts=True, **route) as tc:
        pipe(PROMPTS, num_inference_steps=3)
        assert tc.last_prompts == PROMPTS and tc.last_prompt == PROMPTS[0]
        raw = {k: v for k, v in tc.all_heat_maps}
        maps = tc.compute_global_heat_maps()
        with pytest.raises(ValueError, match='prompt_idx'):
            tc.compute_global_heat_map()
        with pytest.raises(ValueError, match='out of range'):
            tc.compute_global_heat_map(prompt_idx=3)
        one = tc.compute_global_heat_map(prompt_idx=1).heat_maps
        heads = {}
        for (f, layer, h) in raw:
            heads[layer] = max(heads.get(layer, 0), h + 1)
        n = len(PROMPTS)
        for p in range(n):
            for (f, layer, h), v in single_raw[p].items():
                H = heads[layer] // n
                assert torch.equal(raw[(f, layer, p * H + h)], v), (p, f, layer, h)
            assert maps[p].heat_maps.shape == single_maps[p].shape
            assert (maps[p].heat_maps - single_maps[p]).abs().max().item() <= 1e-6
        assert (one - maps[1].heat_maps).abs().max().item() <= 1e-6    # another finalize: f32 atomics in another order
        # filters: per prompt, as on the single-prompt trace
        layer0 = min(heads)
        filt = tc.compute_global_heat_maps(layer_idx=layer0, head_idx=1)
    for p, prompt in enumerate(PROMPTS):
        with daam_amd.trace(pipe, **route) as tc:
            pipe(prompt, num_inference_steps=3)
            want = tc.compute_global_heat_map(layer_idx=layer0, head_idx=1).heat_maps
        assert (filt[p].heat_maps - want).abs().max().item() <= 1e-6


def test_single_prompt_batched_trace_is_a_no_op_and_default_still_refuses():
    import daam_amd
    pipe = _pipe('sd15', torch.float16)
    with daam_amd.trace(pipe) as tc:
        pipe('a dog', num_inference_steps=2)
        a = tc.compute_global_heat_map().heat_maps.clone()
        with pytest.raises(ValueError, match='Only single prompt'):
            pipe(['a', 'b'])
    with daam_amd.trace(pipe, batch_prompts=True) as tc:
        pipe(['a dog'], num_inference_steps=2)
        b = tc.compute_global_heat_map().heat_maps
        c = tc.compute_global_heat_map(prompt_idx=0).heat_maps
        d = tc.compute_global_heat_maps()[0].heat_maps
    assert (a - b).abs().max().item() <= 1e-6 and (a - c).abs().max().item() <= 1e-6
    assert (a - d).abs().max().item() <= 1e-6


def test_batch_that_does_not_divide_raises():
    import daam_amd
    pipe = fd.make_pipe('sd15', device=DEV, dtype=torch.float16, batch=2, seed=5, mini=True, identity_proj=True, dim_head=16)
    with daam_amd.trace(pipe, batch_prompts=True):
        with pytest.raises(ValueError, match='does not divide'):
            pipe(['a', 'b', 'c'], num_inference_steps=1)


def test_trace_prompts_in_calls_of_two():
    from daam_amd.distributed import trace_prompts
    pipe = _pipe('sd15', torch.float16)
    prompts = PROMPTS + ['one more prompt here']
    a, rows_a = trace_prompts(pipe, prompts, num_inference_steps=2)
    b, rows_b = trace_prompts(pipe, prompts, num_inference_steps=2, prompts_per_call=2)
    assert rows_a == rows_b and a.shape == b.shape
    for i, r in enumerate(rows_a):
        assert (a[i, :r] - b[i, :r]).abs().max().item() <= 1e-6


def _run(pipe, prompts, k, trace_kw, steps=2, names=None):
    """One generation under a trace: ({key: raw sums}, [maps per prompt], [(f, layer, head_idx=1 maps)], the trace)."""
    import daam_amd
    tc = daam_amd.trace(pipe, batch_prompts=not isinstance(prompts, str), **trace_kw)
    if names is not None:                                       # what every immediate tap / attend call launched
        eng = tc.engine
        for attr in ('tap_qk', 'attend'):
            fn = getattr(eng, attr)

            def wrapped(*a, _fn=fn, **kw):
                r = _fn(*a, **kw)
                names.add(eng.last_kernels(0))
                return r
            setattr(eng, attr, wrapped)
    with tc:
        pipe(prompts, num_inference_steps=steps, num_images_per_prompt=k)
        if names is not None:
            tc.engine.flush()
            names.add(tc.engine.last_kernels(0))
        raw = {key: v.clone() for key, v in tc.all_heat_maps}
        if isinstance(prompts, str):
            maps = [tc.compute_global_heat_map().heat_maps.clone()]
            filt = [tc.compute_global_heat_map(head_idx=1, factors=[2, 4]).heat_maps.clone()]
        else:
            maps = [m.heat_maps.clone() for m in tc.compute_global_heat_maps()]
            filt = [m.heat_maps.clone() for m in tc.compute_global_heat_maps(head_idx=1, factors=[2, 4])]
    return raw, maps, filt, tc


def _check_batched_vs_sequential(pipe, prompts, k, trace_kw, what, steps=2):
    names = set()
    raw, maps, filt, tc = _run(pipe, prompts, k, trace_kw, steps, names)
    n = len(prompts)
    heads = {}
    for (f, layer, h) in raw:
        heads[layer] = max(heads.get(layer, 0), h + 1)
    for p, prompt in enumerate(prompts):
        s_raw, s_maps, s_filt, _ = _run(pipe, prompt, k, trace_kw, steps)
        assert len(s_raw) * n == len(raw)
        for (f, layer, h), v in s_raw.items():
            block = heads[layer] // n                            # k * H keys per prompt
            assert torch.equal(raw[(f, layer, p * block + h)], v), (what, p, f, layer, h)
        for got, want in ((maps[p], s_maps[0]), (filt[p], s_filt[0])):
            assert got.shape == want.shape
            assert (got - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item()), (what, p)
    return names, tc


# every tap route at B = 2 * N * k: (id, pipe kind, mini, dtype, trace kwargs, environment, kernel the batched run must launch)
ROUTES = [
    ('d64', 'sdxl', True, torch.float16, {}, {}, 'tap_d64_kernel'),
    ('slab', 'sd15', False, torch.float16, {}, {}, 'tap_slab_kernel'),
    ('chunk', 'sd15', False, torch.float16, {}, {'DAAM_TAP_SLAB': '0'}, 'tap_chunk_kernel'),
    ('chunk_bf16', 'sd15', False, torch.bfloat16, {}, {}, 'tap_chunk_kernel'),
    ('wide', 'sd15', False, torch.float16, dict(defer_steps=0), {'DAAM_NO_ATTEND': '1'}, 'tap_wide_kernel'),
    ('mfma', 'sd15', True, torch.float16, {}, {'DAAM_NO_D64': '1'}, 'tap_mfma_kernel'),
    ('generic', 'sd15', True, torch.float16, {}, {'DAAM_FORCE_GENERIC': '1'}, 'tap_generic_kernel'),
    ('attend_fused', 'sd15', False, torch.float16, dict(defer_steps=0), {}, None),
    ('probs', 'sd15', False, torch.float16, dict(tap='probs'), {}, None),
    ('defer_bytes_split', 'sd15', False, torch.float16, {}, {'DAAM_DEFER_BYTES': str(8 << 20)}, None),
]


@pytest.mark.parametrize('n,k', [(3, 1), (2, 2), (4, 1)])
@pytest.mark.parametrize('route', ROUTES, ids=[r[0] for r in ROUTES])
def test_tap_routes_batched_equals_sequential(route, n, k, monkeypatch):
    """Raw sums of prompt p's keys bit-identical to its single-prompt run, maps (also with head_idx / factor filters) within the
    f32-atomics noise, on every tap route -- and the batched run really launched the route's kernel."""
    what, kind, mini, dtype, trace_kw, env, kernel = route
    monkeypatch.setenv('DAAM_NO_CTX_POOL', '1')                 # a fresh context reads the route switches
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    pipe = _pipe(kind, dtype, mini=mini)
    names, _ = _check_batched_vs_sequential(pipe, PROMPTS_4[:n], k, trace_kw, what)
    if kernel is not None:
        assert any(kernel in s for s in names), (what, names)


PROMPTS_4 = ['a dog', 'a cat on a red mat', 'three small birds sitting on one long wire', 'rain']


def test_save_and_load_heads_batched(tmp_path, monkeypatch):
    """save_heads / load_heads at B = 2 * N: the saved batched generation equals the sequential runs, and loading it back
    reproduces its sums bit for bit."""
    monkeypatch.setenv('DAAM_NO_CTX_POOL', '1')
    pipe = _pipe('sd15', torch.float16)
    prompts = PROMPTS_4[:3]
    _check_batched_vs_sequential(pipe, prompts, 1, dict(save_heads=True, data_dir=str(tmp_path / 's')), 'save_heads')
    saved, maps, _, _ = _run(pipe, prompts, 1, dict(save_heads=True, data_dir=str(tmp_path / 'b')))
    loaded, lmaps, _, _ = _run(pipe, prompts, 1, dict(load_heads=True, data_dir=str(tmp_path / 'b')))
    assert list(saved) == list(loaded)
    for key in saved:
        assert torch.equal(saved[key], loaded[key]), key
    for a, b in zip(maps, lmaps):
        assert (a - b).abs().max().item() <= 1e-6


def test_images_per_prompt_encode_prompt_and_to_experiment(tmp_path):
    """k = 2 images per prompt, told through encode_prompt: the key blocks are k*H wide, head_idx counts inside the block
    (image 0's head), to_experiment(prompt_idx) exports the prompt's text, map and first image (p * k); a batch that contradicts
    encode_prompt is refused."""
    import daam_amd
    pipe = _pipe('sd15', torch.float16)
    prompts = PROMPTS_4[:2]
    with daam_amd.trace(pipe, batch_prompts=True) as tc:
        pipe(prompts, num_inference_steps=2, num_images_per_prompt=2)
        assert tc._encode_args == (2, True)
        assert len(tc.last_images) == 4
        exp = tc.to_experiment(str(tmp_path), prompt_idx=1)
        assert exp.prompt == prompts[1] and exp.image == f'image-of:{prompts[1]}#0'
        want = tc.compute_global_heat_map(prompt_idx=1).heat_maps
        assert (exp.global_heat_map - want).abs().max().item() <= 1e-6
        # prompt= relabels AND crops, as on a single prompt
        short = tc.compute_global_heat_map(prompt='x', prompt_idx=1)
        assert short.prompt == 'x' and short.heat_maps.shape[0] == len(pipe.tokenizer.tokenize('x')) + 2
        assert (short.heat_maps - want[:short.heat_maps.shape[0]]).abs().max().item() <= 1e-6
        with pytest.raises(ValueError, match='prompt_idx'):      # without prompt_idx: as before, and N > 1 needs one
            tc.to_experiment(str(tmp_path))

    pipe.told = (1, True)                                        # says k = 1 but runs k = 2
    with daam_amd.trace(pipe, batch_prompts=True):
        with pytest.raises(ValueError, match='images per prompt'):
            pipe(prompts, num_inference_steps=1, num_images_per_prompt=2)
    pipe.told = (1, False)                                       # no guidance: the kept half would split the prompts
    with daam_amd.trace(pipe, batch_prompts=True):
        with pytest.raises(ValueError, match='without classifier-free guidance'):
            pipe(prompts, num_inference_steps=1)


def test_reference_golden_two_prompts():
    """sd15_b4_f32 (batch 4, recorded by the unmodified reference) traced as TWO prompts of different lengths: the raw keys are
    the golden's, and each prompt's map -- also with factor / layer / head filters -- is the oracle's global heat map over that
    prompt's heads [p*H, (p+1)*H) of the replayed generation, cropped to the prompt's own rows."""
    import daam_amd
    from conftest import golden_pipe, load_golden
    from oracle.make_golden import SAMPLE_TOKENS
    z, meta = load_golden('sd15_b4_f32')
    pipe = golden_pipe(meta, device=DEV)
    prompts = ['a dog', 'a cat sitting on a red mat by the door']
    cpu_pipe = golden_pipe(meta, device='cpu')
    raw = ho.replay_generation(cpu_pipe, meta['steps'], torch.float32)
    lat = ho.latent_hw_for(cpu_pipe.unet.config.sample_size, cpu_pipe.vae_scale_factor)
    kept = {}
    for (f, layer, h), _ in raw:
        kept[layer] = max(kept.get(layer, 0), h + 1)
    with daam_amd.trace(pipe, batch_prompts=True) as tc:
        pipe(prompts, num_inference_steps=meta['steps'])
        items = list(tc.all_heat_maps)
        np.testing.assert_array_equal(np.asarray([key for key, _ in items], dtype=np.int32), z['keys'])
        for sid in z['raw_sample_ids']:
            got = items[int(sid)][1][SAMPLE_TOKENS].float().cpu().numpy()
            np.testing.assert_allclose(got, z[f'raw_{int(sid)}'], rtol=0, atol=2e-6)
        layer0 = sorted(kept)[1]
        for kw in (dict(), dict(factors=[2, 4]), dict(layer_idx=layer0), dict(head_idx=1)):
            maps = tc.compute_global_heat_maps(**kw)
            for p, prompt in enumerate(prompts):
                mine = []
                for (f, layer, h), v in raw:
                    H = kept[layer] // 2
                    if p * H <= h < (p + 1) * H:
                        mine.append(((f, layer, h - p * H), v))
                n_rows = len(cpu_pipe.tokenizer.tokenize(prompt)) + 2
                want = ho.global_heat_map(mine, lat, n_rows=n_rows, **kw)
                got = maps[p].heat_maps.cpu().numpy()
                assert got.shape == want.shape, (p, kw)
                assert np.abs(got - want).max() <= 1e-3, (p, kw)


def test_single_prompt_without_guidance_is_a_no_op():
    """batch_prompts=True with one prompt and no CFG (batch 1, the sd15_nocfg_f32 golden) behaves as the default trace."""
    import daam_amd
    from conftest import golden_pipe, load_golden
    z, meta = load_golden('sd15_nocfg_f32')
    pipe = golden_pipe(meta, device=DEV)
    with daam_amd.trace(pipe) as tc:
        pipe(meta['prompt'], num_inference_steps=meta['steps'])
        a = tc.compute_global_heat_map().heat_maps.clone()
    with daam_amd.trace(pipe, batch_prompts=True) as tc:
        pipe(meta['prompt'], num_inference_steps=meta['steps'])
        b = tc.compute_global_heat_map().heat_maps
        c = tc.compute_global_heat_maps()[0].heat_maps
    assert (a - b).abs().max().item() <= 1e-6 and (a - c).abs().max().item() <= 1e-6
    np.testing.assert_allclose(b.cpu().numpy(), z['global_default'], rtol=0, atol=1e-5 * max(1.0, float(np.abs(z['global_default']).max())))


def test_trace_prompts_with_seeds_in_calls_of_two():
    """prompts_per_call with seeds: one generator per prompt, handed over as a list."""
    from daam_amd.distributed import trace_prompts
    pipe = _pipe('sd15', torch.float16)
    seen = []
    orig = type(pipe).__call__

    def spy(self, prompt, generator=None, **kw):
        seen.append(generator)
        return orig(self, prompt, **kw)
    pipe.__class__ = type('Spy', (type(pipe),), {'__call__': spy})
    a, rows_a = trace_prompts(pipe, PROMPTS_4, seeds=[1, 2, 3, 4], num_inference_steps=2)
    b, rows_b = trace_prompts(pipe, PROMPTS_4, seeds=[1, 2, 3, 4], num_inference_steps=2, prompts_per_call=2)
    assert all(isinstance(g, torch.Generator) for g in seen[:4])
    assert all(isinstance(g, list) and len(g) == 2 for g in seen[4:]) and len(seen) == 6
    assert rows_a == rows_b
    for i, r in enumerate(rows_a):
        assert (a[i, :r] - b[i, :r]).abs().max().item() <= 1e-6
