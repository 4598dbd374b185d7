"""``DAAM_TAP_WALK=1``: the window-walking tap kernel (``tap_walk_kernel``) against the default per-window chains of
``tap_d64_kernel`` -- every window's raw sums bit for bit, the kernel names, the launch count, and the routes around it (strict
softmax, a window cut by a launch boundary, batched prompts, a second generation, uneven window counts, a head_dim-40 layer in
the launch, the finalize on top of the sums, the full SDXL-1024 size)."""
import os
import sys

import pytest
import torch

from oracle import fake_diffusers as fd

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 6
HEADS = 2
PAIRS = [(torch.float16, 'exact'), (torch.float16, 'float32'), (torch.bfloat16, 'exact'), (torch.bfloat16, 'float32')]
PAIR_IDS = ['f16_f16', 'f16_f32', 'bf16_bf16', 'bf16_f32']


def _inputs(layers, steps, dtype, seed=3, batch=2):
    """[step][layer] = (q [batch, hw, heads * d], k [batch, 77, heads * d]); ``layers`` = [(side, head_dim)]."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(steps):
        cur = []
        for side, d in layers:
            q = torch.randn(batch, side * side, HEADS * d, generator=g, device=DEV, dtype=dtype)
            k = torch.randn(batch, 77, HEADS * d, generator=g, device=DEV, dtype=dtype)
            k[:, 0, :] *= 3.0
            cur.append((q, k))
        out.append(cur)
    return out


def _switch(monkeypatch, on, **env):
    if on:
        monkeypatch.setenv('DAAM_TAP_WALK', '1')
    else:
        monkeypatch.delenv('DAAM_TAP_WALK', raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _engine(n_layers, acc, bins):
    from daam_amd.engine import HeatMapEngine
    return HeatMapEngine(n_layers, tokens=77, out_side=64, defer_steps=64, accumulate=acc, time_bins=bins)


def _generate(eng, layers, inputs, schedule=None, flush_after=()):
    """Tap ``inputs`` step by step; ``schedule[step]`` = the layers tapped at that step (default: all); an explicit launch after
    the steps in ``flush_after``.  Returns (launches of the final flush, its kernel names)."""
    for t, cur in enumerate(inputs):
        for li, ((side, d), (q, k)) in enumerate(zip(layers, cur)):
            if schedule is None or li in schedule[t]:
                eng.tap_qk(li, q, k, HEADS, d ** -0.5, 64 // side)
        if t in flush_after:
            eng.flush()
    n0 = eng.last_flush()['launches']
    eng.flush()
    return eng.last_flush()['launches'] - n0, eng.last_kernels(0)


def _windows(eng, n):
    return [{key: v.clone() for key, v in eng.window_items(w).items()} for w in range(n)]


def _compare(got, want):
    assert len(got) == len(want)
    for w, (a, b) in enumerate(zip(got, want)):
        assert list(a) == list(b) and len(a) > 0
        for key in b:
            assert torch.equal(a[key], b[key]), (w, key)


def _both(monkeypatch, layers, dtype, acc, bins, env=None, **kw):
    """The same generation with the switch unset and set: ((windows, launches, names) off, the same on)."""
    inputs = _inputs(layers, STEPS, dtype)
    res = []
    for on in (False, True):
        _switch(monkeypatch, on, **(env or {}))
        eng = _engine(len(layers), acc, bins)
        launches, names = _generate(eng, layers, inputs, **kw)
        res.append((_windows(eng, len(bins)), launches, names))
        eng.close()
    return res


@pytest.mark.parametrize('side', [16, 24], ids=['hw256', 'hw576'])          # one exact tile; 2.25 tiles (a partial tile, waves outside)
@pytest.mark.parametrize('bins', [[0, 2, 3], list(range(STEPS))], ids=['bins023', 'per_step'])
@pytest.mark.parametrize('dtype,acc', PAIRS, ids=PAIR_IDS)
def test_walk_equals_per_window_chains(monkeypatch, dtype, acc, bins, side):
    layers = [(side, 64), (side, 64)]
    (want, off_launches, off_names), (got, launches, names) = _both(monkeypatch, layers, dtype, acc, bins)
    assert names == 'tap_walk_kernel' and launches == 1, (names, launches)
    assert off_names == 'tap_d64_kernel' and off_launches == 1, (off_names, off_launches)
    _compare(got, want)


@pytest.mark.parametrize('acc', ['exact', 'float32'])
def test_strict_exp(monkeypatch, acc):
    layers = [(24, 64), (16, 64)]
    (want, _, off_names), (got, launches, names) = _both(monkeypatch, layers, torch.float16, acc, [0, 2, 3],
                                                         env=dict(DAAM_STRICT_EXP='1'))
    assert names == 'tap_walk_kernel' and launches == 1 and off_names == 'tap_d64_kernel', (names, off_names)
    _compare(got, want)


@pytest.mark.parametrize('dtype,acc', PAIRS, ids=PAIR_IDS)
def test_window_cut_by_a_launch_boundary(monkeypatch, dtype, acc):
    """A launch after step 0: window 0 (steps 0, 1) is the non-fresh first window of the second launch's entries."""
    layers = [(24, 64), (16, 64)]
    (want, _, off_names), (got, launches, names) = _both(monkeypatch, layers, dtype, acc, [0, 2, 3], flush_after=(0,))
    assert names == 'tap_walk_kernel' and launches == 1 and off_names == 'tap_d64_kernel', (names, off_names)
    _compare(got, want)


def _mini_sdxl(dtype, per_prompt=False):
    """The mini SDXL pipe of tests/test_gpu_time_bins.py, with the head_dim (64) the walk kernel is for."""
    base = fd.make_pipe('sdxl', device=DEV, dtype=dtype, seed=5, mini=True, identity_proj=True, dim_head=64, heads_scale=0.2,
                        tblocks_cap=1)
    if not per_prompt:
        return base
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import test_gpu_multi_prompt as mp
    pipe = mp._SDXL(base.unet, device=DEV, dtype=dtype)
    pipe.seed = 5
    return pipe


def _traced(monkeypatch, on, pipe, prompt, bins, env=None, **kw):
    import daam_amd
    _switch(monkeypatch, on, **(env or {}))
    names = set()
    with daam_amd.trace(pipe, time_bins=bins, **kw) as tc:
        pipe(prompt, num_inference_steps=STEPS)
        raws = [{key: v.clone() for key, v in tc.raw_heat_maps(w).items()} for w in range(len(bins))]
        names.add(tc.engine.last_kernels(0))
    return raws, names


def test_defer_bytes_split_through_trace(monkeypatch):
    """DAAM_DEFER_BYTES=1: a launch at every step boundary, so every window is split over launches and every sum but a window's
    first is added to what is there; a launch then holds one window per layer and the planner leaves it on tap_d64_kernel."""
    pipe = _mini_sdxl(torch.float16)
    env = dict(DAAM_DEFER_BYTES='1')
    want, off_names = _traced(monkeypatch, False, pipe, 'a dog on a mat', [0, 2, 3], env)
    got, names = _traced(monkeypatch, True, pipe, 'a dog on a mat', [0, 2, 3], env)
    assert names == off_names == {'tap_d64_kernel'}, (names, off_names)
    _compare(got, want)


def test_batched_prompts(monkeypatch):
    pipe = _mini_sdxl(torch.float16, per_prompt=True)
    prompts = ['a dog', 'a cat on a red mat']
    want, off_names = _traced(monkeypatch, False, pipe, prompts, [0, 2, 3], batch_prompts=True)
    got, names = _traced(monkeypatch, True, pipe, prompts, [0, 2, 3], batch_prompts=True)
    assert names == {'tap_walk_kernel'} and off_names == {'tap_d64_kernel'}, (names, off_names)
    _compare(got, want)


def test_second_generation_after_clear(monkeypatch):
    """Lazy zeroing: after clear() the windows are fresh again and the first generation's sums are overwritten, not added to."""
    layers = [(24, 64), (16, 64)]
    bins = [0, 2, 3]
    first, second = _inputs(layers, STEPS, torch.float16, seed=3), _inputs(layers, STEPS, torch.float16, seed=4)
    res = []
    for on in (False, True):
        _switch(monkeypatch, on)
        eng = _engine(len(layers), 'exact', bins)
        _generate(eng, layers, first)
        eng.clear()
        launches, names = _generate(eng, layers, second)
        res.append((_windows(eng, len(bins)), launches, names))
        eng.close()
    (want, _, off_names), (got, launches, names) = res
    assert names == 'tap_walk_kernel' and launches == 1 and off_names == 'tap_d64_kernel'
    _compare(got, want)
    _switch(monkeypatch, False)
    eng = _engine(len(layers), 'exact', bins)                   # and the second generation alone gives the same sums
    _generate(eng, layers, second)
    _compare(got, _windows(eng, len(bins)))
    eng.close()


def test_one_layer_with_one_window_beside_one_with_several(monkeypatch):
    """Layer 1 is tapped at steps 0 and 1 only (window 0): a walk of length one in the same launch as layer 0's three windows."""
    layers = [(24, 64), (16, 64)]
    schedule = [{0, 1}, {0, 1}] + [{0}] * (STEPS - 2)
    (want, _, off_names), (got, launches, names) = _both(monkeypatch, layers, torch.float16, 'exact', [0, 2, 3], schedule=schedule)
    assert names == 'tap_walk_kernel' and launches == 1 and off_names == 'tap_d64_kernel', (names, off_names)
    _compare(got[:1], want[:1])
    for w in (1, 2):                                            # layer 1 has no sums there
        for key in want[w]:
            if key[1] == 0:
                assert torch.equal(got[w][key], want[w][key]), (w, key)


def test_head_dim_40_layer_keeps_the_launch_on_its_kernel(monkeypatch):
    """A head_dim-40 layer makes the launch a zero-padded four-wave tap_d64_kernel launch: not the eight-wave form, so no walk."""
    layers = [(16, 64), (16, 40)]
    (want, _, off_names), (got, launches, names) = _both(monkeypatch, layers, torch.float16, 'exact', [0, 2, 3])
    assert names == off_names and 'tap_walk_kernel' not in names and launches == 1, (names, off_names)
    _compare(got, want)


def test_finalize_on_walk_sums(monkeypatch):
    layers = [(16, 64), (32, 64)]
    bins = [0, 2, 3]
    inputs = _inputs(layers, STEPS, torch.float16)
    maps = []
    for on in (False, True):
        _switch(monkeypatch, on)
        eng = _engine(len(layers), 'exact', bins)
        _, names = _generate(eng, layers, inputs)
        assert names == ('tap_walk_kernel' if on else 'tap_d64_kernel')
        maps.append((eng.global_heat_map(bins=(1, 2)).clone(), eng.global_heat_map(bins=(1, 3)).clone(),
                     eng.global_heat_map().clone()))
        eng.close()
    for a, b in zip(*maps):
        # the finalize's f32 atomics may add the chunks in another order from call to call: the existing tests' bound
        assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-6


def test_full_size_per_step_windows(monkeypatch):
    """SDXL-1024 topology, 50 steps, one window per step: one launch of tap_walk_kernel, windows bit-identical to single-step runs."""
    from daam_amd.engine import HeatMapEngine
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    layers = bench.topology('sdxl', 128)
    sets = bench.make_inputs(layers, 5, DEV, seed=3)
    calls = bench.call_lists(layers, sets, 64)
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
    _switch(monkeypatch, True)
    eng, launches, names = run(list(range(steps)), range(steps))
    assert launches == 1 and names == 'tap_walk_kernel', (launches, names)
    assert eng.window_steps() == [1] * steps
    _switch(monkeypatch, False)
    for w in (1, steps - 1):
        ref, _, ref_names = run(None, [w])
        assert ref_names == 'tap_d64_kernel'
        got = eng.window_items(w)
        for key, v in ref.items():
            assert torch.equal(got[key], v), (w, key)
        ref.close()
    eng.close()
