"""``daam_key_blend`` (libdaam_analysis.so) on the device: the raw C ABI on signed random planes against the float64 reference and the
counted bound of ``tests/_blend_domain.py``, the zero-weight and bad-descriptor rules, its determinism promises, and
``compute_key_heat_map`` / ``compute_key_heat_maps`` on traced generations against float64 of the raw running sums."""
import functools

import numpy as np
import pytest
import torch

import _blend_domain as bd
from oracle import heatmap_oracle as ho

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOKENS, TAIL = 77, 2                          # token rows, rows behind the tokens that are always poison
TORCH_DT = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
CODE = {'f16': 0, 'f32': 1, 'bf16': 2}
SENTINEL = -12345.0
PAD = 4                                       # elements between two sets of the output: set_stride = rows * cells + PAD


def _lib():
    from daam_amd import _native as nat
    return nat, nat.load_analysis()


def _as_np(t):
    return ho.round_bf16(t.float().numpy()) if t.dtype == torch.bfloat16 else t.numpy()


@functools.lru_cache(maxsize=None)
def _key(index, h, w, n_win, dt, out_h, out_w):
    """Key ``index``: ``(sums [n_win, TOKENS, h, w] CPU tensor of dt, K [TOKENS, cells] float64, e [TOKENS])`` -- signed values, so
    the clamp matters; the reference is computed once per key at 77 rows (a row's map and error know no other row)."""
    g = torch.Generator().manual_seed(1000 * index + 10 * h + w + n_win)
    sums = (torch.randn(n_win, TOKENS, h, w, generator=g) * 3.0).to(TORCH_DT[dt])
    k, rowmax = bd.clamped64(_as_np(sums), out_h, out_w)
    return sums, k, bd.row_error(rowmax, n_win)


def _keys(specs, dt, out_h, out_w):
    return [_key(i, h, w, n_win, dt, out_h, out_w) for i, (h, w, n_win) in enumerate(specs)]


def _upload(keys, n_rows, misalign):
    """The sums on the device, NaN from row ``n_rows`` on and around every buffer (what nobody may read), and the descriptors.
    ``misalign``: every base sits one element behind a 16-byte boundary."""
    nat, _ = _lib()
    bufs, desc = [], []
    for sums, _, _ in keys:
        n_win, _, h, w = sums.shape
        flat = torch.full((n_win * (TOKENS + TAIL) * h * w + 16,), float('nan'), dtype=sums.dtype)
        at = 9 if misalign else 8
        view = flat[at:at + n_win * (TOKENS + TAIL) * h * w].view(n_win, TOKENS + TAIL, h, w)
        view[:, :n_rows] = sums[:, :n_rows]
        flat = flat.to(DEV)
        bufs.append(flat)
        base = flat.data_ptr() + at * flat.element_size()
        assert (base % 16 != 0) == bool(misalign)
        desc.append(nat.KeyPlanes(base=base, win_stride=(TOKENS + TAIL) * h * w, h=h, w=w, n_win=n_win, pad=0))
    return bufs, desc


def _call(desc, dt, n_rows, out_h, out_w, weights, extra_scratch=0):
    """-> out [n_sets, n_rows, cells] on the device; the gaps between the sets must come back untouched."""
    nat, lib = _lib()
    arr = (nat.KeyPlanes * len(desc))(*desc)
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    w = torch.as_tensor(weights, dtype=torch.float32).contiguous().to(DEV)
    n_sets, cells = w.shape[0], out_h * out_w
    need = lib.daam_key_blend_scratch_bytes(len(desc), n_sets, n_rows, out_h, out_w)
    assert need > 0
    scratch = torch.full((need + extra_scratch,), 0xA5, dtype=torch.uint8, device=DEV)
    stride = n_rows * cells + PAD
    out = torch.full((n_sets, stride), SENTINEL, dtype=torch.float32, device=DEV)
    nat.check_analysis(lib.daam_key_blend(dev.data_ptr(), len(desc), CODE[dt], n_rows, out_h, out_w, w.data_ptr(), n_sets, out.data_ptr(),
                                       stride, scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (out[:, n_rows * cells:] == SENTINEL).all()
    return out[:, :n_rows * cells].reshape(n_sets, n_rows, cells)


def _weights(n_sets, n_keys, seed=0):
    """Mixed signs with zeros sprinkled in; with more than one chunk, set 1 weighs nothing in chunk 1 and the last set weighs only
    the last key (one chunk for the join)."""
    rng = np.random.default_rng([seed, n_sets, n_keys])
    w = rng.standard_normal((n_sets, n_keys)).astype(np.float32)
    w[rng.random((n_sets, n_keys)) < 0.3] = 0.0
    w[0, 0] = 0.75
    if n_keys > bd.CHUNK and n_sets > 1:
        w[1, bd.CHUNK:2 * bd.CHUNK] = 0.0
        w[-1, :-1] = 0.0
        w[-1, -1] = -1.5
    return w


def _check(specs, dt, n_rows, out_h, out_w, n_sets, misalign, label):
    keys = _keys(specs, dt, out_h, out_w)
    w = _weights(n_sets, len(keys))
    bufs, desc = _upload(keys, n_rows, misalign)
    got = _call(desc, dt, n_rows, out_h, out_w, w).cpu().numpy()
    assert np.isfinite(got).all() and not (got == SENTINEL).any()       # fully overwritten; no poisoned row reached a result
    exact, bound = bd.blend64(np.stack([k[:n_rows] for _, k, _ in keys]), np.stack([e[:n_rows] for _, _, e in keys]), w)
    worst = bd.worst_ratio(got, exact, bound, f'blend {label}')
    assert worst <= 1.0, worst
    return got


def _mixed(n_keys):
    """x4, x2, x1 and x0.5 of a 16 x 16 output in turn, with 1, 2 and 3 windows."""
    sizes = ((4, 4), (8, 8), (16, 16), (32, 32))
    return tuple(sizes[i % 4] + (1 + i % 3,) for i in range(n_keys))


C = bd.CHUNK


@pytest.mark.parametrize('dt,n_rows,n_sets,n_keys,misalign', [
    ('f16', 77, 8, 2 * C + 1, True), ('bf16', 5, 3, C + 1, False), ('f32', 1, 1, 1, True), ('f16', 5, 1, C - 1, False),
    ('bf16', 77, 3, C, True), ('f32', 77, 8, C + 1, False), ('f32', 5, 3, 2 * C + 1, True), ('f16', 1, 8, C, False)])
def test_mixed_sizes_16(dt, n_rows, n_sets, n_keys, misalign):
    _check(_mixed(n_keys), dt, n_rows, 16, 16, n_sets, misalign, f'16x16 {dt} rows {n_rows} sets {n_sets} keys {n_keys} off {int(misalign)}')


RECT = ((3, 5, 1), (6, 10, 2), (12, 20, 3), (6, 10, 1), (12, 20, 1), (3, 5, 3))


@pytest.mark.parametrize('dt,n_rows,n_sets', [('f16', 77, 3), ('bf16', 5, 8), ('f32', 1, 1)])
def test_rectangular(dt, n_rows, n_sets):
    _check(RECT, dt, n_rows, 12, 20, n_sets, dt == 'f16', f'12x20 {dt} rows {n_rows} sets {n_sets}')


def test_real_class_64():
    _check(((32, 32, 1), (16, 16, 1), (32, 32, 1), (16, 16, 1), (32, 32, 1)), 'f16', 77, 64, 64, 3, False, '64x64 f16')


def test_real_class_128():
    _check(((64, 64, 1), (64, 64, 1)), 'f16', 5, 128, 128, 2, False, '128x128 f16')


def test_a_zero_weight_is_no_contribution():
    """A key of NaN planes: the sets that weigh it 0 are the bits of the call without it, the set that weighs it is NaN."""
    for n_keys in (5, C + 4):
        keys = _keys(_mixed(n_keys), 'f16', 16, 16)
        bufs, desc = _upload(keys, 5, False)
        bufs[2].fill_(float('nan'))
        w = _weights(3, n_keys, seed=1)
        w[:, 2] = (0.0, 0.5, -0.0)
        got = _call(desc, 'f16', 5, 16, 16, w)
        assert torch.isfinite(got[0]).all() and torch.isnan(got[1]).all() and torch.isfinite(got[2]).all()
        without = _call(desc[:2] + desc[3:], 'f16', 5, 16, 16, np.delete(w, 2, axis=1)[[0, 2]]) if n_keys <= C else None
        if without is not None:                                  # (the same chunk either way: the same order of additions)
            assert torch.equal(got[[0, 2]], without)
        # ... and weighed 0 by every set it reaches nobody
        w[1, 2] = 0.0
        assert torch.isfinite(_call(desc, 'f16', 5, 16, 16, w)).all()


def test_a_bad_descriptor_is_nan_in_the_sets_that_weigh_it():
    nat, _ = _lib()
    keys = _keys(_mixed(C + 4), 'f16', 16, 16)
    bufs, desc = _upload(keys, 5, False)
    good = list(desc)
    desc[C + 1] = nat.KeyPlanes(base=desc[C + 1].base, win_stride=0, h=0, w=16, n_win=1, pad=0)
    w = _weights(4, C + 4, seed=2)
    w[:, C + 1] = (0.0, 1.0, 0.0, -2.0)
    got = _call(desc, 'f16', 5, 16, 16, w)
    assert [bool(torch.isnan(got[g]).all()) for g in range(4)] == [False, True, False, True]
    assert torch.isfinite(got[[0, 2]]).all() and torch.equal(got[[0, 2]], _call(good, 'f16', 5, 16, 16, w)[[0, 2]])


def test_bit_identical_again_alone_cropped_and_with_more_scratch():
    n_keys = 2 * C + 1
    keys = _keys(_mixed(n_keys), 'f16', 16, 16)
    w = _weights(8, n_keys)
    bufs, desc = _upload(keys, TOKENS, True)
    every = _call(desc, 'f16', TOKENS, 16, 16, w)
    assert torch.equal(every, _call(desc, 'f16', TOKENS, 16, 16, w))                       # across two calls
    for g in (0, 1, 7):                                                                    # alone versus among eight
        assert torch.equal(_call(desc, 'f16', TOKENS, 16, 16, w[g:g + 1])[0], every[g]), g
    bufs5, desc5 = _upload(keys, 5, True)                                                  # rows 5.. are poison here
    assert torch.equal(_call(desc5, 'f16', 5, 16, 16, w), every[:, :5])                    # n_rows = 5 versus the first 5 of 77
    assert torch.equal(_call(desc, 'f16', TOKENS, 16, 16, w, extra_scratch=4096 + 12), every)
    bufs0, desc0 = _upload(keys, TOKENS, False)                                            # ... and where a plane starts in memory
    assert torch.equal(_call(desc0, 'f16', TOKENS, 16, 16, w), every)
    # the f32 restatement of the add order on the exact maps rounded to f32: it and the kernel are each within the bound of float64
    k64, e64 = np.stack([k for _, k, _ in keys]), np.stack([e for _, _, e in keys])
    exact, bound = bd.blend64(k64, e64, w)
    for g in (0, 7):
        like = bd.blend_like_kernel(k64.astype(np.float32), w[g]).astype(np.float64)
        assert (np.abs(like - exact[g]) <= bound[g]).all(), g
        assert (np.abs(every[g].cpu().numpy().astype(np.float64) - like) <= 2 * bound[g]).all(), g


def test_a_refused_call_then_the_three_calls_on_one_handle():
    """One library, one error buffer: a ``daam_key_blend`` refused on the host (``set_stride`` one short) leaves the handle good for
    a blend of two chunks (the join runs) within the bound, and for ``daam_key_scores`` and ``daam_token_gram`` on the same keys."""
    nat, lib = _lib()
    n_keys, n_rows, out_h, out_w = C + 1, 2, 8, 8
    keys = _keys(((4, 4, 1),) * n_keys, 'f16', out_h, out_w)
    w = _weights(2, n_keys, seed=3)
    w[:, 3] = 0.0
    bufs, desc = _upload(keys, n_rows, False)
    dev = torch.frombuffer(bytearray(bytes((nat.KeyPlanes * n_keys)(*desc))), dtype=torch.uint8).to(DEV)
    wd = torch.as_tensor(w).to(DEV)
    need = lib.daam_key_blend_scratch_bytes(n_keys, 2, n_rows, out_h, out_w)
    scratch = torch.empty(max(need, lib.daam_token_gram_scratch_bytes(n_keys, n_rows, 16)), dtype=torch.uint8, device=DEV)
    out = torch.full((2, n_rows * out_h * out_w), SENTINEL, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.daam_key_blend(dev.data_ptr(), n_keys, CODE['f16'], n_rows, out_h, out_w, wd.data_ptr(), 2, out.data_ptr(),
                            n_rows * out_h * out_w - 1, scratch.data_ptr(), scratch.numel(), stream)
    assert rc == nat.E_INVALID and 'set_stride' in lib.daam_analysis_last_error().decode()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                               # refused before any launch
    got = _call(desc, 'f16', n_rows, out_h, out_w, w).cpu().numpy()
    exact, bound = bd.blend64(np.stack([k[:n_rows] for _, k, _ in keys]), np.stack([e[:n_rows] for _, _, e in keys]), w)
    assert np.isfinite(got).all() and bd.worst_ratio(got, exact, bound, 'blend after a refused call') <= 1.0
    scores = torch.empty(n_keys, 1, n_rows, dtype=torch.float32, device=DEV)
    gram = torch.empty(n_keys, n_rows, n_rows, dtype=torch.float32, device=DEV)
    assert lib.daam_key_scores(dev.data_ptr(), n_keys, CODE['f16'], n_rows, out_h, out_w, None, 0, scores.data_ptr(), stream) == 0
    assert lib.daam_token_gram(dev.data_ptr(), n_keys, CODE['f16'], n_rows, gram.data_ptr(), scratch.data_ptr(), scratch.numel(), stream) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(scores).all() and torch.isfinite(gram).all()


# ---- through daam_amd.trace ------------------------------------------------------------------------------------------------------
PROMPT = 'a cat and a dog'
STEPS = 3


def _check_trace(tc, raw, n_win, n_prompts=1, prompt_idx=None, **kw):
    """``raw``: {(factor, layer, head): [n_win, 77, h, w] tensor} of the sums behind the selection."""
    out_h, out_w = tc.engine.out_h, tc.engine.out_w
    sel = dict(kw) if prompt_idx is None else dict(kw, prompt_idx=prompt_idx)
    keys = tc.compute_key_scores(**sel).keys
    p = prompt_idx or 0
    ghm = tc.compute_global_heat_map(**sel)
    rows = ghm.heat_maps.shape[0]

    def windows_of(key):
        factor, layer, head = key
        block = len([1 for _, l_, _ in raw if l_ == layer]) // n_prompts
        return _as_np(raw[(factor, layer, p * block + head)][:, :rows].cpu())

    k, e = bd.key_maps([windows_of(key) for key in keys], out_h, out_w)
    n = len(keys)
    assert n > 3
    # every key at 1 / K: trace.py:116-126 itself -- the blend within its bound, the finalize within its documented class, each of
    # the same float64
    uniform = np.full((1, n), 1.0 / n, np.float32)
    exact, bound = bd.blend64(k, e, uniform)
    got = tc.compute_key_heat_map(keys, **sel).heat_maps
    assert got.shape == (rows, out_h, out_w) and got.dtype == torch.float32
    assert bd.worst_ratio(got.reshape(1, rows, -1).cpu().numpy(), exact, bound, f'trace all {n} keys') <= 1.0
    fin = np.abs(ghm.heat_maps.reshape(rows, -1).cpu().numpy().astype(np.float64) - exact[0]).max(axis=1)
    fin_bound = 2.0 ** -19 * np.abs(exact[0]).max(axis=1) + 2.0 ** -23
    print(f'finalize of the same keys: worst err_t / class = {float((fin / fin_bound).max()):.4f}')
    assert (fin <= fin_bound).all()
    # two keys, weights (2, -1): heads A minus heads B; by layer name and as (key, score) pairs
    pair = [keys[0], keys[-1]]
    exact, bound = bd.blend64(k[[0, n - 1]], e[[0, n - 1]], np.float32([[2.0, -1.0]]))
    two = tc.compute_key_heat_map(pair, [2.0, -1.0], **sel).heat_maps
    assert bd.worst_ratio(two.reshape(1, rows, -1).cpu().numpy(), exact, bound, 'trace two keys (2, -1)') <= 1.0
    assert float(two.min()) < 0
    def by_name(key):                                            # the reference's names restart per block: the factor must tell them apart
        same = [k_ for k_ in keys if (k_[0], tc.layer_names[k_[1]], k_[2]) == (key[0], tc.layer_names[key[1]], key[2])]
        return (key[0], tc.layer_names[key[1]] if len(same) == 1 else key[1], key[2])

    named = [(by_name(key), 0.0) for key in pair]
    assert torch.equal(tc.compute_key_heat_map(named, [2.0, -1.0], **sel).heat_maps, two)
    # three selections from one pass: the bits of three calls
    sels = [keys, (pair, [2.0, -1.0]), keys[1:3]]
    many = tc.compute_key_heat_maps(sels, **sel)
    assert torch.equal(many[0].heat_maps, got) and torch.equal(many[1].heat_maps, two)
    assert torch.equal(many[2].heat_maps, tc.compute_key_heat_map(keys[1:3], **sel).heat_maps)
    return keys


def test_traced_generation_and_time_windows():
    import daam_amd
    import test_gpu_time_bins as tb
    pipe = tb._pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe) as tc:
        pipe(PROMPT, num_inference_steps=STEPS)
        raw = {k: v[None] for k, v in tc.all_heat_maps}
        keys = _check_trace(tc, raw, 1)
        ks = tc.compute_key_scores()
        top = ks.top_keys('dog', k=3)
        assert [ks.index_of(pair) for pair in top] == [keys.index(key) for key, _ in top]
        norm = tc.compute_key_heat_map(top, normalize=True).heat_maps
        assert norm.shape == tc.compute_global_heat_map().heat_maps.shape and torch.isfinite(norm).all()
        with pytest.raises(ValueError, match='not tapped'):
            tc.compute_key_heat_map([(1, 10 ** 6, 0)])
        with pytest.raises(RuntimeError, match='No heat maps'):
            tc.compute_key_heat_map([])
    with daam_amd.trace(pipe, time_bins=[0, 1]) as tc:
        pipe(PROMPT, num_inference_steps=STEPS)
        windows = [tc.raw_heat_maps(w) for w in range(2)]
        raw = {k: torch.stack([w[k] for w in windows]) for k in windows[0]}
        _check_trace(tc, raw, 2, time_bin=slice(0, 2))
        _check_trace(tc, {k: v[1:] for k, v in raw.items()}, 1, time_bin=1)


def test_traced_rectangular_generation():
    import daam_amd
    import test_gpu_rect as gr
    pipe, _ = gr._rect_pipe(batch=2)
    with daam_amd.trace(pipe, height=16 * gr.OUT_H, width=16 * gr.OUT_W) as tc:
        pipe(PROMPT, num_inference_steps=STEPS)
        _check_trace(tc, {k: v[None] for k, v in tc.all_heat_maps}, 1)


def test_traced_batch_of_prompts():
    import daam_amd
    import test_gpu_multi_prompt as mp
    pipe = mp._pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe, batch_prompts=True) as tc:
        pipe(mp.PROMPTS, num_inference_steps=STEPS)
        raw = {k: v[None] for k, v in tc.all_heat_maps}
        _check_trace(tc, raw, 1, n_prompts=len(mp.PROMPTS), prompt_idx=1)
        with pytest.raises(ValueError, match='prompt_idx'):
            tc.compute_key_heat_map([(1, 0, 0)])
