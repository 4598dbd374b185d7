"""Time-resolved heat maps (``trace(..., time_bins=...)``): every window's sums against a generation that ran only that
window's steps, window ranges against the oracle, the raw ``daam_finalize_bins`` ABI against numpy, the launch structure at
full size, batched prompts x windows and the edge cases."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fake_diffusers as fd
from oracle import heatmap_oracle as ho

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = [0, 2, 3]                      # windows of 2, 1 and 3 steps of a 6-step generation
STEPS = 6


def _pipe(kind, dtype):
    unet = dict(dim_head=16, heads_scale=0.2, tblocks_cap=1) if kind == 'sdxl' else dict(dim_head=16)
    return fd.make_pipe(kind, device=DEV, dtype=dtype, seed=5, mini=True, identity_proj=True, **unet)


def _run_steps(pipe, prompt, steps):
    """``pipe(prompt)`` restricted to the denoising steps ``steps`` (same per-step inputs as the full generation)."""
    pipe.check_inputs(prompt, 512, 512, 1)
    with torch.no_grad():
        for step in steps:
            pipe.unet(pipe.hidden_states, pipe.context, step, pipe.mask_fn)
    return pipe._finish('image-of:' + prompt)


def _windows(bins, steps):
    return [list(range(b, bins[i + 1] if i + 1 < len(bins) else steps)) for i, b in enumerate(bins)]


ROUTES = [('deferred', {}, {}), ('immediate', dict(defer_steps=0), {}), ('no_attend', {}, dict(DAAM_NO_ATTEND='1')),
          ('probs', dict(tap='probs'), {}), ('acc32', dict(accumulate='float32'), {}),
          ('split_launch', {}, dict(DAAM_DEFER_BYTES='1')), ('save_heads', dict(save_heads=True), {})]


@pytest.mark.parametrize('kind', ['sd15', 'sdxl'])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32], ids=['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('route', ROUTES, ids=[r[0] for r in ROUTES])
def test_window_equals_restricted_generation(kind, dtype, route, monkeypatch, tmp_path):
    import daam_amd
    name, kw, env = route
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name == 'save_heads':
        kw = dict(kw, data_dir=str(tmp_path))
    pipe = _pipe(kind, dtype)
    prompt = 'a dog on a mat'
    want_raw, want_maps, want_names = [], [], []
    for steps in _windows(BINS, STEPS):
        with daam_amd.trace(pipe, **kw) as tc:
            _run_steps(pipe, prompt, steps)
            want_raw.append({k: v.clone() for k, v in tc.all_heat_maps})
            want_maps.append(tc.compute_global_heat_map().heat_maps.clone())
            want_names.append(tc.engine.last_kernels(0))
    with daam_amd.trace(pipe, time_bins=BINS, **kw) as tc:
        pipe(prompt, num_inference_steps=STEPS)
        launches = tc.engine.last_flush()['launches']                      # the deferred taps are still recorded
        assert tc.time_bin_steps() == [2, 1, 3]
        if name == 'deferred':
            assert tc.engine.last_flush()['launches'] == launches + 1          # one tap launch for all windows
        if name in ('deferred', 'acc32', 'split_launch'):
            assert tc.engine.last_kernels(0) == want_names[-1] and want_names[-1].startswith('tap_'), tc.engine.last_kernels(0)
        with pytest.raises(RuntimeError, match='raw_heat_maps'):
            list(tc.all_heat_maps)
        per_window = tc.compute_time_heat_maps()
        for w in range(len(BINS)):
            raw = tc.raw_heat_maps(w)
            assert list(raw) == list(want_raw[w])
            for key, v in want_raw[w].items():
                assert torch.equal(raw[key], v), (w, key)
            got = tc.compute_global_heat_map(time_bin=w).heat_maps
            assert got.shape == want_maps[w].shape
            assert (got - want_maps[w]).abs().max().item() <= 1e-6
            assert (per_window[w].heat_maps - want_maps[w]).abs().max().item() <= 1e-6


def test_one_window_is_the_default_trace():
    import daam_amd
    pipe = _pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe) as tc:
        pipe('a dog', num_inference_steps=4)
        want_raw = {k: v.clone() for k, v in tc.all_heat_maps}
        want = tc.compute_global_heat_map().heat_maps.clone()
    with daam_amd.trace(pipe, time_bins=[0]) as tc:
        pipe('a dog', num_inference_steps=4)
        raw = tc.raw_heat_maps(0)
        assert list(raw) == list(want_raw) and all(torch.equal(raw[k], v) for k, v in want_raw.items())
        # the same finalize calls as the default trace; its f32 atomics may add the chunks in another order from call to call
        assert (tc.compute_global_heat_map().heat_maps - want).abs().max().item() <= 1e-6
        assert (tc.compute_global_heat_map(time_bin=0).heat_maps - want).abs().max().item() <= 1e-6
        assert 'bin_sum' not in tc.engine.last_kernels(1)
        assert tc.time_bin_steps() == [4]


def _replay_steps(cpu, steps, dtype, acc_dtype):
    np_dtype = {torch.float16: np.float16, torch.float32: np.float32, torch.bfloat16: ho.BF16}[dtype]
    as_np = (lambda t: t.detach().float().cpu().numpy()) if ho.is_bf16(np_dtype) else (lambda t: t.detach().cpu().numpy())
    raw = ho.RawMaps(np_dtype if acc_dtype is None else acc_dtype)
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
                q = as_np(a.head_to_batch_dim(a.to_q(cpu.hidden_states(i, spec, step))))
                k = as_np(a.head_to_batch_dim(a.to_k(cpu.context(i, spec))))
                ho.tap(raw, li, q, k, a.scale, lat, np_dtype, upcast_attention=getattr(a, 'upcast_attention', False))
    return raw


@pytest.mark.parametrize('kind', ['sd15', 'sdxl'])
@pytest.mark.parametrize('dtype,acc,tol', [(torch.float32, 'exact', 2e-6), (torch.float16, 'exact', 1e-3),
                                           (torch.bfloat16, 'exact', 8e-3), (torch.float16, 'float32', 1e-3)],
                         ids=['f32', 'f16', 'bf16', 'f16_acc32'])
def test_ranges_against_oracle(kind, dtype, acc, tol):
    import daam_amd
    pipe = _pipe(kind, dtype)
    unet_kw = dict(dim_head=16, heads_scale=0.2, tblocks_cap=1) if kind == 'sdxl' else dict(dim_head=16)
    prompt = 'a cat on a red mat'
    cpu = fd.make_pipe(kind, device='cpu', dtype=dtype, seed=5, mini=True, identity_proj=True, **unet_kw)
    lat = ho.latent_hw_for(cpu.unet.config.sample_size, cpu.vae_scale_factor)
    n_rows = len(cpu.tokenizer.tokenize(prompt)) + 2
    acc_np = np.float32 if acc == 'float32' else None
    with daam_amd.trace(pipe, time_bins=BINS, accumulate=acc) as tc:
        pipe(prompt, num_inference_steps=STEPS)
        rng = tc.compute_global_heat_map(time_bin=slice(1, 3)).heat_maps.cpu().numpy()
        whole = tc.compute_global_heat_map().heat_maps.cpu().numpy()
        assert 'finalize_bin_sum_kernel' in tc.engine.last_kernels(1)
        whole2 = tc.compute_global_heat_map(time_bin=slice(None)).heat_maps.cpu().numpy()
    with daam_amd.trace(pipe, accumulate=acc) as tc:
        pipe(prompt, num_inference_steps=STEPS)
        plain = tc.compute_global_heat_map().heat_maps.cpu().numpy()
    for got, steps in ((rng, range(2, STEPS)), (whole, range(STEPS)), (whole2, range(STEPS))):
        want = ho.global_heat_map(list(_replay_steps(cpu, steps, dtype, acc_np)), lat, n_rows=n_rows)
        scale = max(1.0, float(np.abs(want).max())) if dtype is torch.float32 else 1.0
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= tol * scale, (steps, np.abs(got - want).max())
    scale = max(1.0, float(np.abs(plain).max())) if dtype is torch.float32 else 1.0
    assert np.abs(whole - plain).max() <= tol * scale


def _np_bicubic_clamp_mean(planes_by_key, out_side):
    """planes_by_key: list of [rows, s, s] f64 window sums -> the oracle's bicubic / clamp / mean (f32)."""
    total = None
    for p in planes_by_key:
        up = np.maximum(ho.bicubic_resize(p.astype(np.float32), out_side, np.float32), 0)
        total = up if total is None else total + up
    return total * np.float32(1.0 / len(planes_by_key))


@pytest.mark.parametrize('acc', ['float16', 'bfloat16', 'float32'])
def test_finalize_bins_abi_against_numpy(acc):
    from daam_amd import _native as nat
    from daam_amd.engine import HeatMapEngine
    code = {'float16': nat.DAAM_F16, 'bfloat16': nat.DAAM_BF16, 'float32': nat.DAAM_F32}[acc]
    tdt = {'float16': torch.float16, 'bfloat16': torch.bfloat16, 'float32': torch.float32}[acc]
    sides, heads, out_side, nb = [16, 32, 64, 128], 3, 64, 5
    lib = nat.load()
    ctx = nat.c_void_p()
    nat.check(lib.daam_ctx_create(len(sides), 77, out_side, code, nat.byref(ctx)))
    try:
        nat.check(lib.daam_ctx_set_time_bins(ctx, nb, (ctypes.c_int32 * nb)(0, 1, 3, 4, 9)))
        rng = np.random.default_rng(7)
        bufs, host = [], []
        for li, side in enumerate(sides):
            h = rng.random((nb, heads, 77, side, side)).astype(np.float32) * 4 - 0.5
            t = torch.from_numpy(h).to(DEV).to(tdt)
            host.append(t.float().cpu().numpy().astype(np.float64))
            bufs.append(t)
            nat.check(lib.daam_layer_configure(ctx, li, heads, side, out_side // side if side <= out_side else 0, t.data_ptr()))
        total = heads * len(sides)
        key_at = [(li, h) for li in range(len(sides)) for h in range(heads)]
        plane = 77 * out_side * out_side
        cases = [
            # (key set per key, groups: (set, b0, b1, rows))
            ([0] * total, [(0, 0, 5, 77)]),
            ([0] * total, [(0, 1, 3, 12), (0, 4, 5, 77), (0, 0, 2, 5)]),
            ([k % 2 for k in range(total)], [(0, 2, 5, 30), (1, 0, 1, 77), (1, 1, 4, 9)]),
            ([k % 3 - 1 for k in range(total)], [(0, 3, 4, 40), (1, 0, 5, 20)]),
            ([0] * total, [(0, b, b + 1, 33) for b in range(nb)]),                   # single windows: no reduction
        ]
        stream = torch.cuda.current_stream().cuda_stream
        for kg, groups in cases:
            n = len(groups)
            out = torch.full((n, 77, out_side, out_side), -7.0, device=DEV)
            i32 = ctypes.c_int32
            nat.check(lib.daam_finalize_bins(ctx, (i32 * total)(*kg), n, (i32 * n)(*[g[0] for g in groups]),
                                             (i32 * n)(*[g[1] for g in groups]), (i32 * n)(*[g[2] for g in groups]),
                                             (i32 * n)(*[g[3] for g in groups]), out.data_ptr(), plane, stream))
            got = out.cpu().numpy()
            for gi, (st, b0, b1, rows) in enumerate(groups):
                keys = [key_at[i] for i in range(total) if kg[i] == st]
                want = _np_bicubic_clamp_mean([host[li][b0:b1, h, :rows].sum(0) for li, h in keys], out_side)
                err = np.abs(got[gi, :rows] - want).max()
                assert err <= 2e-6 * max(1.0, float(np.abs(want).max())), (acc, kg[:6], groups[gi], err)
                assert (got[gi, rows:] == -7.0).all()                           # sentinel rows untouched
        # errors
        i32 = ctypes.c_int32
        bad = lib.daam_finalize_bins(ctx, (i32 * total)(*[0] * total), 1, None, (i32 * 1)(2), (i32 * 1)(2), (i32 * 1)(77),
                                     out.data_ptr(), plane, stream)
        assert bad == nat.E_INVALID
        bad = lib.daam_finalize_bins(ctx, (i32 * total)(*[-1] * total), 1, None, (i32 * 1)(0), (i32 * 1)(1), (i32 * 1)(77),
                                     out.data_ptr(), plane, stream)
        assert bad == nat.E_NOMAPS
        assert lib.daam_layer_touch(ctx, 0, stream) == nat.E_UNSUPPORTED
        acc_p, nbytes = ctypes.c_void_p(), ctypes.c_size_t()
        nat.check(lib.daam_layer_acc(ctx, 1, ctypes.byref(acc_p), ctypes.byref(nbytes)))
        assert acc_p.value == bufs[1].data_ptr() and nbytes.value == bufs[1].numel() * bufs[1].element_size()
    finally:
        lib.daam_ctx_destroy(ctx)


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


@pytest.mark.parametrize('kind,latent,bins', [('sdxl', 128, list(range(0, 50, 5))), ('sdxl', 128, list(range(50))),
                                              ('sd15', 64, list(range(0, 50, 5)))], ids=['sdxl_10', 'sdxl_50', 'sd15_10'])
def test_full_size_one_launch(kind, latent, bins):
    from daam_amd.engine import HeatMapEngine
    bench = _bench()
    layers = bench.topology(kind, latent)
    sets = bench.make_inputs(layers, 5, DEV, seed=3)
    calls = bench.call_lists(layers, sets, latent // 2 if kind == 'sdxl' else latent)
    n_layers = max(l[0] for l in layers) + 1
    steps = 50

    def run(time_bins, step_list):
        eng = HeatMapEngine(n_layers, tokens=77, out_side=64, defer_steps=64, time_bins=time_bins)
        eng.clear()
        for t in step_list:
            for a in calls[t % len(calls)]:
                eng.tap_qk(*a)
        n0 = eng.last_flush()['launches']
        eng.flush()
        return eng, eng.last_flush()['launches'] - n0, eng.last_kernels(0)
    eng, launches, names = run(bins, range(steps))
    plain, plain_launches, plain_names = run(None, range(steps))
    assert launches == 1 and plain_launches == 1 and names == plain_names, (names, plain_names)
    assert names == ('tap_d64_kernel' if kind == 'sdxl' else 'tap_slab_kernel')
    width = bins[1] - bins[0]
    assert eng.window_steps() == [width] * len(bins)
    plain.close()
    for w in (1, len(bins) - 1):
        ref, _, _ = run(None, range(bins[w], bins[w] + width))
        got = eng.window_items(w)
        for key, v in ref.items():
            assert torch.equal(got[key], v), (w, key)
        ref.close()
    eng.close()


def _mp():
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import test_gpu_multi_prompt as mp
    return mp


def _run_prompt_steps(pipe, prompt, steps):
    """The multi-prompt test pipeline (per-prompt inputs) restricted to the denoising steps ``steps``."""
    pipe.prompts = [prompt] if isinstance(prompt, str) else list(prompt)
    pipe.k = 1
    pipe.batch = 2 * len(pipe.prompts)
    pipe.check_inputs(prompt, 512, 512, 1)
    pipe.encode_prompt(prompt, pipe.device, 1, True)
    with torch.no_grad():
        for step in steps:
            pipe.unet(pipe.hidden_states, pipe.context, step, pipe.mask_fn)


@pytest.mark.parametrize('kind', ['sd15', 'sdxl'])
def test_batched_prompts_by_windows(kind):
    import daam_amd
    mp = _mp()
    pipe = mp._pipe(kind, torch.float16)
    prompts = mp.PROMPTS
    want = []                                                   # [prompt][window]: single-prompt restricted generations
    for p in prompts:
        row = []
        for steps in _windows(BINS, STEPS):
            with daam_amd.trace(pipe) as tc:
                _run_prompt_steps(pipe, p, steps)
                row.append(tc.compute_global_heat_map().heat_maps.clone())
        want.append(row)
    with daam_amd.trace(pipe, batch_prompts=True, time_bins=BINS) as tc:
        pipe(prompts, num_inference_steps=STEPS)
        assert tc.time_bin_steps() == [2, 1, 3]
        for b in range(len(BINS)):
            maps = tc.compute_global_heat_maps(time_bin=b)
            for p in range(len(prompts)):
                assert (maps[p].heat_maps - want[p][b]).abs().max().item() <= 1e-6, (b, p)
            one = tc.compute_global_heat_map(prompt_idx=1, time_bin=b).heat_maps
            assert (one - want[1][b]).abs().max().item() <= 1e-6
        for p in range(len(prompts)):
            per_window = tc.compute_time_heat_maps(prompt_idx=p)
            for b in range(len(BINS)):
                assert per_window[b].prompt == prompts[p]
                assert (per_window[b].heat_maps - want[p][b]).abs().max().item() <= 1e-6, (b, p)
        every = tc.compute_time_heat_maps()
        assert len(every) == len(BINS) and all(len(e) == len(prompts) for e in every)
        assert (every[2][2].heat_maps - want[2][2]).abs().max().item() <= 1e-6


def test_empty_window_parking_and_experiment(tmp_path):
    import daam_amd
    pipe = _pipe('sdxl', torch.float16)
    prompt = 'a dog on a mat'
    with daam_amd.trace(pipe) as tc:                            # un-binned first: its context is parked afterwards
        pipe(prompt, num_inference_steps=3)
        plain3 = tc.compute_global_heat_map().heat_maps.clone()
    with daam_amd.trace(pipe, time_bins=[0, 2, 5]) as tc:       # 3 steps: window 2 gets none
        pipe(prompt, num_inference_steps=3)
        assert tc.time_bin_steps() == [2, 1, 0]
        maps = tc.compute_time_heat_maps()
        assert maps[2] is None and maps[0] is not None and maps[1] is not None
        with pytest.raises(RuntimeError, match='window.*2'):
            tc.compute_global_heat_map(time_bin=2)
        with pytest.raises(RuntimeError, match='window.*2'):
            tc.compute_global_heat_map(time_bin=-1)
        with pytest.raises(ValueError):
            tc.compute_global_heat_map(time_bin=3)
        with pytest.raises(ValueError):
            tc.compute_global_heat_map(time_bin=slice(2, 1))
        with pytest.raises(RuntimeError, match='update'):
            tc.all_heat_maps.update(1, 0, 0, torch.zeros(77, 8, 8, device=DEV, dtype=torch.float16))
        whole = tc.compute_global_heat_map().heat_maps
        assert (whole - plain3).abs().max().item() <= 1e-3
        first = tc.compute_global_heat_map(time_bin=slice(0, 2)).heat_maps
        assert (first - plain3).abs().max().item() <= 1e-3
        exp = tc.to_experiment(str(tmp_path), time_bin=0)
        assert (exp.global_heat_map.to(DEV) - maps[0].heat_maps).abs().max().item() <= 1e-6
    with daam_amd.trace(pipe) as tc:                            # and back: the binned context is not adopted here
        pipe(prompt, num_inference_steps=3)
        again = tc.compute_global_heat_map().heat_maps
        assert (again - plain3).abs().max().item() <= 1e-6
        assert len(list(tc.all_heat_maps)) > 0
    with daam_amd.trace(pipe, time_bins=[0, 2, 5]) as tc:       # a parked binned context adopted by the same layout
        pipe(prompt, num_inference_steps=3)
        assert (tc.compute_time_heat_maps()[0].heat_maps - maps[0].heat_maps).abs().max().item() <= 1e-6
