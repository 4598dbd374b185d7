"""``daam_key_scores`` (libdaam_analysis.so) on the device: the raw C ABI on signed random planes against the float64 reference and
the derived bound of ``tests/_key_scores_domain.py``, its determinism promises, and ``compute_key_scores`` on traced generations
against the route it replaces (``compute_global_heat_map(head_idx=, layer_idx=)`` + ``attribute``)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _key_scores_domain as kd
from oracle import heatmap_oracle as ho

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOKENS, HEADS, TAIL = 77, 2, 2                # token rows, heads per layer, rows behind the tokens that are always poison
TORCH_DT = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
CODE = {'f16': 0, 'f32': 1, 'bf16': 2}
SENTINEL = -12345.0


def _lib():
    from daam_amd import _native as nat
    return nat, nat.load_analysis()


@functools.lru_cache(maxsize=None)
def _sums(layers, dt, n_win):
    """Per layer one buffer [n_win, HEADS, TOKENS + TAIL, h, w] of signed values (so the clamp matters), as a CPU tensor of ``dt``.
    The window stride is HEADS * (TOKENS + TAIL) planes: not a plane, not a head."""
    g = torch.Generator().manual_seed(11 + 7 * n_win + len(layers))
    return tuple((torch.randn(n_win, HEADS, TOKENS + TAIL, h, w, generator=g) * 3.0).to(TORCH_DT[dt]) for h, w in layers)


@functools.lru_cache(maxsize=None)
def _footprints(out_h, out_w, n_masks):
    """``n_masks - 1`` footprints of random masks at 3x the map size (``daam_region_scores`` without maps: negative lobes) and one of
    all ones, fp32 on the device."""
    from daam_amd import engine
    g = torch.Generator().manual_seed(5 + n_masks)
    parts = [torch.ones(1, out_h, out_w, dtype=torch.float32, device=DEV)]
    if n_masks > 1:
        big_h, big_w = 3 * out_h, 3 * out_w
        masks = (torch.rand(n_masks - 1, big_h, big_w, generator=g) < 0.01).to(torch.uint8)
        for m in range(n_masks - 1):                             # ... and a box each: the cells around its edge take negative weight
            y, x = int(torch.randint(0, big_h // 2, (1,), generator=g)), int(torch.randint(0, big_w // 2, (1,), generator=g))
            masks[m, y:y + big_h // 3, x:x + big_w // 3] = 1
        _, _, fp = engine.region_scores(None, masks.to(DEV), map_hw=(out_h, out_w))
        assert float(fp.min()) < 0
        parts.insert(0, fp)
    return torch.cat(parts).contiguous()


def _device_planes(layers, dt, n_win, n_rows):
    """The sums on the device with NaN planes from row ``n_rows`` on (rows nobody may read), and the key descriptors."""
    nat, _ = _lib()
    bufs, keys = [], []
    for buf in _sums(layers, dt, n_win):
        dev = buf.clone()
        dev[:, :, n_rows:] = float('nan')
        dev = dev.to(DEV)
        bufs.append(dev)
        for head in range(HEADS):
            keys.append(nat.KeyPlanes(base=dev[0, head].data_ptr(), win_stride=dev.stride(0), h=dev.shape[-2], w=dev.shape[-1],
                                      n_win=n_win, pad=0))
    return bufs, keys


def _call(keys, dt, n_rows, out_h, out_w, footprint):
    nat, lib = _lib()
    arr = (nat.KeyPlanes * len(keys))(*keys)
    desc = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    m = 0 if footprint is None else footprint.shape[0]
    scores = torch.full((len(keys), max(m, 1), n_rows), SENTINEL, dtype=torch.float32, device=DEV)
    nat.check_analysis(lib.daam_key_scores(desc.data_ptr(), len(keys), CODE[dt], n_rows, out_h, out_w,
                                           None if footprint is None else footprint.data_ptr(), m, scores.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return scores


def _as_np(t):
    return ho.round_bf16(t.float().numpy()) if t.dtype == torch.bfloat16 else t.numpy()


def _check(layers, dt, n_win, n_rows, out_h, out_w, n_masks, label):
    fp = _footprints(out_h, out_w, n_masks) if n_masks else None
    bufs, keys = _device_planes(layers, dt, n_win, n_rows)
    got = _call(keys, dt, n_rows, out_h, out_w, fp).cpu().numpy()
    assert got.shape == (len(keys), max(n_masks, 1), n_rows)
    assert np.isfinite(got).all() and not (got == SENTINEL).any()       # fully overwritten; no poisoned row reached a result
    fp_np = None if fp is None else fp.cpu().numpy()
    worst = 0.0
    for li, buf in enumerate(_sums(layers, dt, n_win)):
        for head in range(HEADS):
            exact, bnd = kd.reference(_as_np(buf[:, head, :n_rows]), out_h, out_w, fp_np)
            worst = max(worst, kd.worst_ratio(got[li * HEADS + head], exact, bnd, f'{label} layer {li} head {head}'))
    assert worst <= 1.0, worst
    return got, keys, bufs


SQUARE = ((16, 16), (8, 8), (4, 4))           # x1, x2, x4 in one call
RECT = ((12, 20), (6, 10), (3, 5))            # a 6 x 10 f16 plane is 120 bytes: the second head is not 16-byte aligned


@pytest.mark.parametrize('dt,n_rows,n_masks,n_win', [('f16', 77, 3, 1), ('bf16', 5, 32, 3), ('f32', 1, 0, 1), ('f32', 77, 1, 3),
                                                     ('bf16', 77, 0, 1), ('f16', 5, 1, 3)])
def test_square_x1_x2_x4(dt, n_rows, n_masks, n_win):
    _check(SQUARE, dt, n_win, n_rows, 16, 16, n_masks, f'16x16 {dt} rows {n_rows} masks {n_masks} win {n_win}')


@pytest.mark.parametrize('dt,n_rows,n_masks,n_win', [('f16', 77, 3, 3), ('bf16', 5, 1, 1), ('f32', 77, 32, 1), ('f16', 1, 0, 1)])
def test_rectangular_and_unaligned(dt, n_rows, n_masks, n_win):
    _check(RECT, dt, n_win, n_rows, 12, 20, n_masks, f'12x20 {dt} rows {n_rows} masks {n_masks} win {n_win}')


@pytest.mark.parametrize('dt,n_masks,n_win', [('f16', 3, 1), ('f32', 1, 3), ('bf16', 0, 1)])
def test_half_size_output(dt, n_masks, n_win):
    """x0.5: more cells than the output, the kernel's gather path."""
    _check(((16, 16),), dt, n_win, 77, 8, 8, n_masks, f'8x8 from 16x16 {dt} masks {n_masks} win {n_win}')


def test_real_class_64():
    _check(((32, 32), (64, 64)), 'f16', 1, 77, 64, 64, 32, '64x64 f16 32 masks')


def test_128():
    _check(((128, 128), (64, 64)), 'f16', 1, 5, 128, 128, 3, '128x128 f16 3 masks')


def test_total_mass_equals_all_ones_footprint_bit_for_bit():
    """``n_masks == 0`` runs the same fused multiply-adds with f = 1 on the same tree: the bits of an all-ones footprint."""
    bufs, keys = _device_planes(SQUARE, 'f16', 1, 77)
    ones = torch.ones(1, 16, 16, dtype=torch.float32, device=DEV)
    assert torch.equal(_call(keys, 'f16', 77, 16, 16, None), _call(keys, 'f16', 77, 16, 16, ones))


def test_bit_identical_alone_cropped_and_again():
    fp = _footprints(16, 16, 3)
    bufs, keys = _device_planes(SQUARE, 'f16', 3, 77)
    every = _call(keys, 'f16', 77, 16, 16, fp)
    assert torch.equal(every, _call(keys, 'f16', 77, 16, 16, fp))                   # across two runs
    for i in (0, 3, 5):                                                             # alone versus among all keys
        assert torch.equal(_call(keys[i:i + 1], 'f16', 77, 16, 16, fp)[0], every[i]), i
    bufs5, keys5 = _device_planes(SQUARE, 'f16', 3, 5)                              # rows 5.. are poison here
    assert torch.equal(_call(keys5, 'f16', 5, 16, 16, fp), every[:, :, :5])         # n_rows = 5 versus the first 5 of 77
    one = _call(keys, 'f16', 77, 16, 16, fp[:1])                                    # ... and the other masks of the call
    assert torch.equal(one[:, 0], every[:, 0])


def test_bad_key_on_the_device_is_nan_not_a_read():
    nat, _ = _lib()
    bufs, keys = _device_planes(SQUARE, 'f16', 1, 5)
    keys[1] = nat.KeyPlanes(base=keys[1].base, win_stride=0, h=129, w=16, n_win=1, pad=0)
    got = _call(keys, 'f16', 5, 16, 16, None)
    assert torch.isnan(got[1]).all() and torch.isfinite(got[0]).all() and torch.isfinite(got[2:]).all()


# ---- through daam_amd.trace ------------------------------------------------------------------------------------------------------
PROMPT = 'a cat and a dog'
STEPS = 3


def _route_bound(fp, k_map, rowmax, n_win, extra_adds=0):
    """The bound of one route from its own f32 map ``k_map`` [rows, cells] (within ``e_t`` of the exact one, which is added to
    ``|K|``): finalize + region dots, or key scores -- both are a bicubic of the 2^-19 class and a dot whose chain is at most
    ``reduction_chain``; ``extra_adds``: further f32 additions per map element (the finalize's sum over N keys and its 1 / N)."""
    f = np.abs(fp.reshape(fp.shape[0], -1).astype(np.float64))
    e = kd.row_error(rowmax, n_win) + extra_adds * 2.0 ** -24 * np.abs(k_map).max(axis=1)
    c = 2 + kd.reduction_chain(f.shape[1])
    return f.sum(axis=1)[:, None] * e[None, :] + c * 2.0 ** -24 * (f @ (np.abs(k_map) + e[:, None]).T)


def _check_trace(tc, raw, n_win, n_prompts=1, prompt_idx=None, **kw):
    """``raw``: {(factor, layer, head): [n_win, 77, h, w] tensor} of the sums behind the selection."""
    g = torch.Generator().manual_seed(3)
    out_h, out_w = tc.engine.out_h, tc.engine.out_w
    masks = (torch.rand(3, 3 * out_h, 3 * out_w, generator=g) < 0.4).to(torch.uint8).to(DEV)
    sel = dict(kw) if prompt_idx is None else dict(kw, prompt_idx=prompt_idx)
    ghm = tc.compute_global_heat_map(**sel)
    att = ghm.attribute(masks)
    ks = tc.compute_key_scores(att, **sel)                       # the attribution's footprint is reused
    ks2 = tc.compute_key_scores(masks, **sel)                    # ... and is what the masks give
    assert torch.equal(ks.scores, ks2.scores) and torch.equal(ks2.area, att.area)
    rows = ghm.heat_maps.shape[0]
    assert ks.scores.shape == (len(ks.keys), 3, rows) and len(ks.keys) > 3
    fp = att.footprint.cpu().numpy()
    p = prompt_idx or 0

    def rowmax_of(key):
        factor, layer, head = key
        block = len([1 for f_, l_, _ in raw if l_ == layer]) // n_prompts
        planes = raw[(factor, layer, p * block + head)].double().cumsum(dim=0)
        return planes.abs().amax(dim=(0, 2, 3))[:rows].cpu().numpy()

    # three sampled keys against the route this replaces
    for i in (0, len(ks.keys) // 2, len(ks.keys) - 1):
        factor, layer, head = ks.keys[i]
        one = tc.compute_global_heat_map(head_idx=head, layer_idx=layer, **sel)
        want = one.attribute(masks).scores.cpu().numpy().astype(np.float64)
        k_map = one.heat_maps.reshape(rows, -1).cpu().numpy().astype(np.float64)
        tol = _route_bound(fp, k_map, rowmax_of(ks.keys[i]), n_win, extra_adds=1) + _route_bound(fp, k_map, rowmax_of(ks.keys[i]), n_win)
        err = np.abs(ks.scores[i].cpu().numpy().astype(np.float64) - want)
        print(f'key_scores trace key {ks.keys[i]}: worst |err| / tol = {float((err / tol).max()):.4f}')
        assert (err <= tol).all(), ks.keys[i]
    # the mean over keys against the global map's attribution: every key's bound averaged, the finalize's sum over N keys and the
    # N + 1 roundings of torch's mean on this side
    n = len(ks.keys)
    rowmax = np.mean([rowmax_of(key) for key in ks.keys], axis=0)
    g_map = ghm.heat_maps.reshape(rows, -1).cpu().numpy().astype(np.float64)
    tol = _route_bound(fp, g_map, rowmax, n_win, extra_adds=n + 1) + _route_bound(fp, g_map, rowmax, n_win) \
        + (n + 1) * 2.0 ** -24 * ks.scores.abs().mean(dim=0).cpu().numpy().astype(np.float64)
    err = np.abs(ks.mean().cpu().numpy().astype(np.float64) - att.scores.cpu().numpy().astype(np.float64))
    print(f'key_scores trace mean over {n} keys: worst |err| / tol = {float((err / tol).max()):.4f}')
    assert (err <= tol).all()
    return ks


def test_traced_generation_and_time_windows():
    import daam_amd
    import test_gpu_time_bins as tb
    pipe = tb._pipe('sdxl', torch.float16)
    with daam_amd.trace(pipe) as tc:
        pipe(PROMPT, num_inference_steps=STEPS)
        raw = {k: v[None] for k, v in tc.all_heat_maps}
        ks = _check_trace(tc, raw, 1)
        total = tc.compute_key_scores()
        assert total.scores.shape == (len(ks.keys), 1, ks.scores.shape[2]) and total.area is None and total.keys == ks.keys
        word = ks.word_scores('dog')
        assert word.shape == (len(ks.keys), 3) and [k for k, _ in ks.top_keys('dog', region=1, k=4)][0] in ks.keys
        with pytest.raises(RuntimeError):
            tc.compute_key_scores(layer_idx=10 ** 6)
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
            tc.compute_key_scores()
