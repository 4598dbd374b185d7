"""``daam_token_gram`` (libdaam_analysis.so) on the device: the raw C ABI against the float64 reference and the counted bound of
``tests/_gram_domain.py`` -- exact small-integer data first, which is what catches a permuted MFMA fragment --, its determinism
promises, then ``HeatMapEngine.token_gram`` / ``compute_key_coattention`` / ``GlobalHeatMap.coattention`` on traced generations."""
import functools

import numpy as np
import pytest
import torch

import _gram_domain as gd
from oracle import heatmap_oracle as ho

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TORCH_DT = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
CODE = {'f16': 0, 'f32': 1, 'bf16': 2}
SENTINEL = -12345.0
TAIL = 2                                      # poisoned rows behind the token rows of every plane set
SHAPES = ((1, 1), (3, 5), (6, 10), (16, 16), (26, 38), (32, 32), (32, 33), (64, 64))     # (128, 128): one key only, below
ROWS = (1, 5, 31, 32, 33, 64, 77, 96)


def _lib():
    from daam_amd import _native as nat
    return nat, nat.load_analysis()


def _as_np(t):
    return ho.round_bf16(t.float().numpy()) if t.dtype == torch.bfloat16 else t.numpy()


@functools.lru_cache(maxsize=None)
def _values(kind, dt, n_win, n_rows, hw, seed):
    """[n_win, n_rows, hw] CPU tensor of ``dt``.  ``ints``: values in {0, 1, 2} (every Gram entry is an integer below 2^24);
    ``sums``: what running sums look like ([0, 64]) with zeros, fp16 subnormals (f16) and a row of zeros mixed in; ``signed``: mixed
    signs up to 2^15 (the f32 path)."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'ints':
        return torch.randint(0, 3, (n_win, n_rows, hw), generator=g).to(TORCH_DT[dt])
    if kind == 'signed':
        v = torch.randn(n_win, n_rows, hw, generator=g) * torch.tensor([1.0, 300.0, 2.0 ** 13])[torch.randint(0, 3, (n_rows, 1), generator=g)]
        return v.clamp(-2.0 ** 15, 2.0 ** 15).to(TORCH_DT[dt])
    v = torch.rand(n_win, n_rows, hw, generator=g) * 64.0 / n_win
    pick = torch.rand(n_win, n_rows, hw, generator=g)
    v[pick < 0.2] = 0.0
    if dt == 'f16':
        sub = torch.randint(1, 1024, (n_win, n_rows, hw), generator=g).float() * 2.0 ** -24
        v = torch.where((pick >= 0.2) & (pick < 0.4), sub, v)
    v[:, n_rows // 2] = 0.0                                      # a row of zeros
    return v.to(TORCH_DT[dt])


def _key(values, off, n_rows):
    """One key on the device: a flat buffer of NaN with the planes of each window written at ``off`` elements from its (256-byte
    aligned) start, ``TAIL`` rows of NaN behind the token rows, and a window stride that is no multiple of 8 elements."""
    nat, _ = _lib()
    n_win, rows, hw = values.shape
    assert rows == n_rows
    stride = (n_rows + TAIL) * hw + 3
    buf = torch.full((off + n_win * stride + 8,), float('nan'), dtype=values.dtype)
    for wi in range(n_win):
        buf[off + wi * stride: off + wi * stride + n_rows * hw] = values[wi].reshape(-1)
    dev = buf.to(DEV)
    return dev, (dev.data_ptr() + off * dev.element_size(), stride)


def _call(descs, dt, n_rows, max_hw, extra_scratch=0):
    """``descs``: [(base, win_stride, h, w, n_win)] -> gram [n_keys, n_rows, n_rows] on the device."""
    nat, lib = _lib()
    arr = (nat.KeyPlanes * len(descs))(*[nat.KeyPlanes(base=b, win_stride=s, h=h, w=w, n_win=n, pad=0) for b, s, h, w, n in descs])
    desc = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    need = lib.daam_token_gram_scratch_bytes(len(descs), n_rows, max_hw) + extra_scratch
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    gram = torch.full((len(descs), n_rows, n_rows), SENTINEL, dtype=torch.float32, device=DEV)
    nat.check_analysis(lib.daam_token_gram(desc.data_ptr(), len(descs), CODE[dt], n_rows, gram.data_ptr(), scratch.data_ptr(), need,
                                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return gram


def _run(kind, dt, n_win, n_rows, shapes, off, label, exact_bits=False):
    """Every shape of ``shapes`` as one key of one call; returns ``(gram, descs, buffers)`` after holding each key to the reference."""
    vals = [_values(kind, dt, n_win, n_rows, h * w, 17 + 3 * i) for i, (h, w) in enumerate(shapes)]
    keep, descs = [], []
    for v, (h, w) in zip(vals, shapes):
        dev, (base, stride) = _key(v, off, n_rows)
        keep.append(dev)
        descs.append((base, stride, h, w, n_win))
    got = _call(descs, dt, n_rows, max(h * w for h, w in shapes))
    host = got.cpu().numpy()
    assert host.shape == (len(shapes), n_rows, n_rows)
    assert np.isfinite(host).all() and not (host == SENTINEL).any()      # overwritten in full; no poisoned row or tail reached it
    assert torch.equal(got, got.transpose(1, 2))                          # symmetric bit for bit
    wide = dt == 'f32' or n_win > 1
    worst = 0.0
    for i, v in enumerate(vals):
        exact, bnd = gd.reference(_as_np(v), wide)
        if exact_bits:
            assert np.array_equal(host[i].astype(np.float64), exact), (label, shapes[i])
        else:
            worst = max(worst, gd.worst_ratio(host[i], exact, bnd, f'{label} {shapes[i]}'))
    assert worst <= 1.0, worst
    return got, descs, keep


# ---- exact small integers: a wrong k order, a swapped C/D map or a lost k-step cannot hide -------------------------------------
@pytest.mark.parametrize('n_rows', ROWS)
def test_exact_integers_every_row_count(n_rows):
    _run('ints', 'f16', 1, n_rows, SHAPES, 0, f'ints f16 rows {n_rows}', exact_bits=True)


@pytest.mark.parametrize('dt,n_win,n_rows,off', [('bf16', 1, 77, 0), ('f32', 1, 77, 0), ('f16', 1, 33, 1), ('bf16', 1, 96, 1), ('f32', 1, 5, 1),
                                                 ('f16', 2, 77, 0), ('bf16', 3, 33, 1), ('f32', 3, 64, 0)])
def test_exact_integers_every_dtype_window_and_alignment(dt, n_win, n_rows, off):
    _run('ints', dt, n_win, n_rows, SHAPES, off, f'ints {dt} win {n_win} rows {n_rows} off {off}', exact_bits=True)


@pytest.mark.parametrize('dt,n_win', [('f16', 1), ('bf16', 1), ('f32', 1), ('f16', 2)])
def test_exact_integers_128(dt, n_win):
    _run('ints', dt, n_win, 77 if dt == 'f16' else 33, ((128, 128),), 0, f'ints 128x128 {dt} win {n_win}', exact_bits=True)


# ---- the counted bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt,n_win,n_rows,off', [('f16', 1, 77, 0), ('f16', 1, 31, 1), ('bf16', 1, 77, 0), ('bf16', 1, 64, 1), ('f32', 1, 77, 0),
                                                 ('f32', 1, 32, 1), ('f16', 2, 77, 0), ('f16', 3, 5, 1), ('bf16', 2, 96, 1), ('bf16', 3, 77, 0),
                                                 ('f32', 2, 33, 1), ('f32', 3, 77, 0)])
def test_sums_within_the_counted_bound(dt, n_win, n_rows, off):
    _run('sums', dt, n_win, n_rows, SHAPES, off, f'sums {dt} win {n_win} rows {n_rows} off {off}')


@pytest.mark.parametrize('dt,n_win', [('f32', 1), ('f32', 3), ('f16', 2), ('bf16', 3)])
def test_mixed_signs_on_the_f32_path(dt, n_win):
    _run('signed', dt, n_win, 77, SHAPES, 1, f'signed {dt} win {n_win}')


@pytest.mark.parametrize('dt,n_win', [('f16', 1), ('f32', 1), ('bf16', 2)])
def test_128_within_the_counted_bound(dt, n_win):
    _run('sums', dt, n_win, 77, ((128, 128),), 0, f'sums 128x128 {dt} win {n_win}')


def test_zero_row_has_cosine_zero():
    got, _, _ = _run('sums', 'f16', 1, 5, ((6, 10), (32, 33)), 0, 'zero row')
    from daam_amd import KeyCoattention
    cos = KeyCoattention([(1, 0, 0), (1, 0, 1)], got).cosine()
    assert torch.isfinite(cos).all() and float(got[:, 2].abs().max()) == 0.0 and float(cos[:, 2].abs().max()) == 0.0


# ---- properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt,n_win', [('f16', 1), ('bf16', 3), ('f32', 1)])
def test_deterministic_and_independent_of_the_other_keys(dt, n_win):
    every, descs, keep = _run('sums', dt, n_win, 77, SHAPES, 1, f'mixed {dt} win {n_win}')
    hw = max(h * w for _, _, h, w, _ in descs)
    assert torch.equal(every, _call(descs, dt, 77, hw))                               # across two runs
    for i in range(len(descs)):                                                       # alone versus among all keys
        assert torch.equal(_call(descs[i:i + 1], dt, 77, descs[i][2] * descs[i][3])[0], every[i]), SHAPES[i]
    assert torch.equal(_call(descs[::-1], dt, 77, hw), every.flip(0))                 # ... in another order
    assert torch.equal(_call(descs, dt, 77, 128 * 128, extra_scratch=12345), every)   # ... and with more scratch than needed
    # where a plane starts: the same values at an aligned base take the 16-byte pieces
    vals = [_values('sums', dt, n_win, 77, h * w, 17 + 3 * i) for i, (h, w) in enumerate(SHAPES)]
    moved = [_key(v, 0, 77) for v in vals]
    aligned = [(base, stride, h, w, n_win) for (_, (base, stride)), (h, w) in zip(moved, SHAPES)]
    assert all(d[0] % 16 == 0 for d in aligned) and all(d[0] % 16 != 0 for d in descs)
    assert torch.equal(_call(aligned, dt, 77, hw), every)


def test_bad_descriptors_are_nan_with_correct_neighbours():
    every, descs, keep = _run('sums', 'f16', 1, 33, SHAPES, 0, 'neighbours')
    bad = list(descs)
    bad[1] = (descs[1][0], 0, 0, 5, 1)                            # h = 0
    bad[4] = (descs[4][0], 0, 26, 38, 0)                          # n_win = 0
    bad[6] = (descs[6][0], 0, 32, 129, 1)                         # w past 128
    got = _call(bad, 'f16', 33, 64 * 64)
    for i in range(len(bad)):
        if i in (1, 4, 6):
            assert torch.isnan(got[i]).all(), i
        else:
            assert torch.equal(got[i], every[i]), i
    # a key of more pixels than the scratch was sized for is not read either
    small = _call(descs, 'f16', 33, 32 * 32)
    assert torch.isnan(small[6]).all() and torch.isnan(small[7]).all() and torch.equal(small[:6], every[:6])


# ---- HeatMapEngine.token_gram -----------------------------------------------------------------------------------------------------
PROMPT = 'a cat and a dog'
STEPS = 3


def _hold(got, windows, dt, label):
    """``got`` [rows, rows] tensor against the planes ``windows`` [n_win, >= rows, h, w] the views show."""
    rows = got.shape[0]
    w = _as_np(windows[:, :rows].reshape(windows.shape[0], rows, -1).cpu())
    exact, bnd = gd.reference(w, dt == torch.float32 or windows.shape[0] > 1)
    assert torch.equal(got, got.T)
    return gd.worst_ratio(got.cpu().numpy(), exact, bnd, label)


def _hold_keys(eng, keys, gram, views, n_win, label, block=0):
    """Every key of ``keys`` against ``views``: {(factor, layer, head in the buffer): [n_win, tokens, h, w]}; ``block``: heads in
    front of the prompt's block."""
    assert gram.shape[0] == len(keys) and len(keys) > 0
    worst = 0.0
    for i, (factor, layer, head) in enumerate(keys):
        worst = max(worst, _hold(gram[i], views[(factor, layer, head + block(layer) if callable(block) else head)], eng.acc_dtype,
                                 f'{label} key {(factor, layer, head)}'))
    assert worst <= 1.0, worst


@pytest.mark.parametrize('kind,dtype,acc', [('sd15', torch.float16, 'exact'), ('sdxl', torch.bfloat16, 'exact'), ('sdxl', torch.float16, 'float32'),
                                            ('sd15', torch.bfloat16, 'float32')])
def test_engine_token_gram(kind, dtype, acc):
    import daam_amd
    import test_gpu_time_bins as tb
    pipe = tb._pipe(kind, dtype)
    with daam_amd.trace(pipe, accumulate=acc) as tc:
        pipe(PROMPT, num_inference_steps=STEPS)
        eng = tc.engine
        views = {k: v[None] for k, v in eng.items()}
        keys, gram = eng.token_gram()
        assert gram.shape == (len(keys), eng.tokens, eng.tokens) and gram.dtype == torch.float32 and gram.is_cuda
        assert keys == eng.key_scores()[0]                       # the key order of key_scores
        _hold_keys(eng, keys, gram, views, 1, f'engine {kind} {dtype} {acc}')
        # the crop and the filters
        keys5, gram5 = eng.token_gram(n_rows=5)
        assert keys5 == keys and torch.equal(gram5, gram[:, :5, :5])
        for sel in (dict(head_idx=1), dict(layer_idx=keys[-1][1]), dict(factors=[keys[0][0]]), dict(head_idx=0, layer_idx=keys[0][1])):
            want = eng.key_scores(**sel)[0]
            got_keys, got = eng.token_gram(n_rows=7, **sel)
            assert got_keys == want and 0 < len(want) < len(keys)
            assert torch.equal(got, torch.stack([gram[keys.index(k), :7, :7] for k in want]))
        with pytest.raises(LookupError):
            eng.token_gram(layer_idx=10 ** 6)


def test_engine_token_gram_of_time_windows():
    import daam_amd
    import test_gpu_time_bins as tb
    pipe = tb._pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe, time_bins=[0, 1, 2, 50]) as tc:   # the last window receives no step
        pipe(PROMPT, num_inference_steps=2)
        eng = tc.engine
        windows = [eng.window_items(w) for w in range(4)]
        stack = {k: torch.stack([w[k] for w in windows]) for k in windows[0]}
        for b0, b1 in ((0, 1), (1, 2), (0, 2), (0, 4), (1, 3)):
            keys, gram = eng.token_gram(n_rows=9, bins=(b0, b1))
            _hold_keys(eng, keys, gram, {k: v[b0:b1] for k, v in stack.items()}, b1 - b0, f'windows {b0}:{b1}')
        keys, gram = eng.token_gram(n_rows=9, bins=(3, 4))       # a window that received no step: all zeros
        assert float(gram.abs().max()) == 0.0
        whole, _ = eng.token_gram(n_rows=9), None
        assert torch.equal(whole[1], eng.token_gram(n_rows=9, bins=(0, 4))[1])


def test_engine_token_gram_of_a_batch_of_prompts():
    import daam_amd
    import test_gpu_multi_prompt as mp
    pipe = mp._pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe, batch_prompts=True) as tc:
        pipe(mp.PROMPTS, num_inference_steps=STEPS)
        eng, n = tc.engine, len(mp.PROMPTS)
        views = {k: v[None] for k, v in eng.items()}
        heads = {layer: len([1 for _, l_, _ in views if l_ == layer]) // n for _, layer, _ in views}
        for p in range(n):
            keys, gram = eng.token_gram(n_rows=11, n_prompts=n, prompt=p)
            assert keys == eng.key_scores(n_prompts=n, prompt=p)[0]
            _hold_keys(eng, keys, gram, views, 1, f'prompt {p}', block=lambda layer, p=p: p * heads[layer])
        with pytest.raises(ValueError):
            eng.token_gram(n_prompts=n, prompt=n)


def test_engine_token_gram_rectangular():
    """``out_hw = (6, 10)`` with 6 x 10 and 3 x 5 layers: 60 and 15 pixels, no multiple of 8 -- the element-by-element path."""
    from daam_amd import engine as E
    eng = E.HeatMapEngine(2, out_hw=(6, 10), defer_steps=0)
    g = torch.Generator().manual_seed(8)
    for layer, (hw, factor) in enumerate(((60, 1), (15, 2))):
        q = torch.randn(4, hw, 16, generator=g).to(torch.float16).to(DEV)
        k = torch.randn(4, 77, 16, generator=g).to(torch.float16).to(DEV)
        for _ in range(2):
            eng.tap_qk(layer, q, k, 2, 0.25, factor)
    views = {k: v[None] for k, v in eng.items()}
    assert sorted({tuple(v.shape[-2:]) for v in views.values()}) == [(3, 5), (6, 10)]
    keys, gram = eng.token_gram()
    assert len(keys) == len(views) and float(gram.abs().max()) > 0
    _hold_keys(eng, keys, gram, views, 1, 'rect 6x10')
    with pytest.raises(LookupError):
        eng.token_gram(factors=[64])
    eng.close()


# ---- through daam_amd.trace -----------------------------------------------------------------------------------------------------
def _merged_cosines(ca, views, block=0):
    """Per key of ``ca`` the cosine of the 'dog' and 'cat' word maps merged explicitly from the key's raw planes, float64."""
    from daam_amd.utils import compute_token_merge_indices
    dog, _ = compute_token_merge_indices(ca.tokenizer, ca.prompt, 'dog', None)
    cat, _ = compute_token_merge_indices(ca.tokenizer, ca.prompt, 'cat', None)
    rows = ca.gram.shape[1]
    out = []
    for factor, layer, head in ca.keys:
        planes = views[(factor, layer, head + (block(layer) if callable(block) else 0))].double().sum(dim=0)[:rows]
        out.append(gd.word_cosine(planes.reshape(rows, -1).cpu().numpy(), dog, cat))
    return np.array(out)


def _cos_tol(ca, views, n_win, block=0):
    """What the Gram's bound allows the word cosine: the three block means are each within the mean of their elements' bounds, and
    cos = ab / sqrt(aa bb) moves by at most e_ab / sqrt(aa bb) + |cos| (e_aa / aa + e_bb / bb) / 2 to first order; twice that, plus
    the f32 the result is returned in."""
    from daam_amd.utils import compute_token_merge_indices
    dog = list(compute_token_merge_indices(ca.tokenizer, ca.prompt, 'dog', None)[0])
    cat = list(compute_token_merge_indices(ca.tokenizer, ca.prompt, 'cat', None)[0])
    rows = ca.gram.shape[1]
    tol = []
    for factor, layer, head in ca.keys:
        v = views[(factor, layer, head + (block(layer) if callable(block) else 0))]
        w = _as_np(v[:, :rows].reshape(v.shape[0], rows, -1).cpu())
        exact, bnd = gd.reference(w, v.dtype == torch.float32 or n_win > 1)

        tol.append(_pair_tol(exact, bnd, dog, cat))
    return np.array(tol)


def _pair_tol(exact, bnd, rows_a, rows_b):
    def mean(m, r, c):
        return m[np.ix_(list(r), list(c))].mean()
    ab, aa, bb = mean(exact, rows_a, rows_b), mean(exact, rows_a, rows_a), mean(exact, rows_b, rows_b)
    e_ab, e_aa, e_bb = mean(bnd, rows_a, rows_b), mean(bnd, rows_a, rows_a), mean(bnd, rows_b, rows_b)
    cos = ab / np.sqrt(aa * bb)
    return 2.0 * (e_ab / np.sqrt(aa * bb) + abs(cos) * (e_aa / aa + e_bb / bb) / 2) + 2.0 ** -23


def test_trace_coattention_of_two_words():
    import daam_amd
    import test_gpu_time_bins as tb
    pipe = tb._pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe) as tc:
        pipe(PROMPT, num_inference_steps=STEPS)
        views = {k: v[None] for k, v in tc.all_heat_maps}
        ca = tc.compute_key_coattention()
        assert isinstance(ca, daam_amd.KeyCoattention) and ca.keys == tc.compute_key_scores().keys
        rows = len(pipe.tokenizer.tokenize(PROMPT)) + 2
        assert ca.gram.shape == (len(ca.keys), rows, rows)
        got = ca.of('dog', 'cat').double().cpu().numpy()
        want, tol = _merged_cosines(ca, views), _cos_tol(ca, views, 1)
        print(f'coattention of dog, cat: worst |err| / tol = {float((np.abs(got - want) / tol).max()):.4f}')
        assert (np.abs(got - want) <= tol).all()
        assert np.abs(ca.of('dog', 'dog').cpu().numpy() - 1.0).max() <= 1e-5
        top = ca.top_keys('dog', 'cat', k=3)
        assert len(top) == 3 and top[0][1] == float(ca.of('dog', 'cat').max()) and top[0][0][1] in tc.layer_names
        assert ca.mean().shape == (rows, rows) and ca.by_layer()[1].shape[1:] == (rows, rows)
        assert ca.cpu().gram.device.type == 'cpu'
        one = tc.compute_key_coattention(head_idx=1, layer_idx=ca.keys[-1][1])
        assert one.keys == [k for k in ca.keys if k[1] == ca.keys[-1][1] and k[2] == 1]
        # the global map's own Gram, through the same library call
        ghm = tc.compute_global_heat_map()
        co = ghm.coattention()
        exact, bnd = gd.reference(ghm.heat_maps.reshape(1, rows, -1).cpu().numpy(), True)
        assert co.shape == (rows, rows) and gd.worst_ratio(co.cpu().numpy(), exact, bnd, 'global map') <= 1.0
        planes = ghm.heat_maps.reshape(rows, -1).cpu().numpy()
        from daam_amd.utils import compute_token_merge_indices
        dog, cat = (compute_token_merge_indices(pipe.tokenizer, PROMPT, w, None)[0] for w in ('dog', 'cat'))
        assert abs(ghm.word_cosine('dog', 'cat') - gd.word_cosine(planes, dog, cat)) <= _pair_tol(exact, bnd, dog, cat)
        # the error strings of compute_key_scores for the same misuse
        for bad in (dict(layer_idx=10 ** 6), dict(prompt_idx=3), dict(time_bin=1), dict(time_bin=slice(0, 1, 2)), dict(factors=5)):
            with pytest.raises(Exception) as mine:
                tc.compute_key_coattention(**bad)
            with pytest.raises(Exception) as theirs:
                tc.compute_key_scores(**bad)
            assert type(mine.value) is type(theirs.value) and str(mine.value) == str(theirs.value), bad


def test_trace_coattention_of_time_windows_and_prompts():
    import daam_amd
    import test_gpu_multi_prompt as mp
    import test_gpu_time_bins as tb
    pipe = tb._pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe, time_bins=[0, 1]) as tc:
        pipe(PROMPT, num_inference_steps=STEPS)
        windows = [tc.raw_heat_maps(w) for w in range(2)]
        stack = {k: torch.stack([w[k] for w in windows]) for k in windows[0]}
        for time_bin, lo, hi in ((slice(0, 2), 0, 2), (1, 1, 2), (None, 0, 2)):
            ca = tc.compute_key_coattention(time_bin=time_bin)
            views = {k: v[lo:hi] for k, v in stack.items()}
            got = ca.of('dog', 'cat').double().cpu().numpy()
            want, tol = _merged_cosines(ca, views), _cos_tol(ca, views, hi - lo)
            print(f'coattention time_bin {time_bin}: worst |err| / tol = {float((np.abs(got - want) / tol).max()):.4f}')
            assert (np.abs(got - want) <= tol).all(), time_bin
        with pytest.raises(Exception) as mine:
            tc.compute_key_coattention(time_bin=5)
        with pytest.raises(Exception) as theirs:
            tc.compute_key_scores(time_bin=5)
        assert type(mine.value) is type(theirs.value) and str(mine.value) == str(theirs.value)
    pipe = mp._pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe, batch_prompts=True) as tc:
        pipe(['a cat and a dog', 'a dog', 'a cat sat by a dog'], num_inference_steps=STEPS)
        views = {k: v[None] for k, v in tc.all_heat_maps}
        heads = {layer: len([1 for _, l_, _ in views if l_ == layer]) // 3 for _, layer, _ in views}
        ca = tc.compute_key_coattention(prompt_idx=2)
        assert ca.prompt == 'a cat sat by a dog' and ca.gram.shape[1] == len(pipe.tokenizer.tokenize(ca.prompt)) + 2
        block = lambda layer: 2 * heads[layer]                   # noqa: E731
        got = ca.of('dog', 'cat').double().cpu().numpy()
        want, tol = _merged_cosines(ca, views, block), _cos_tol(ca, views, 1, block)
        assert (np.abs(got - want) <= tol).all()
        with pytest.raises(ValueError, match='prompt_idx'):
            tc.compute_key_coattention()
