"""The life of a layer's running sums across launches, resets and kernels: ``Layer::dirty`` / ``Layer::zero_pending`` on the host
(daam_amd/csrc/daam_ctx.h) decide whether a tap launch overwrites the sums (``fresh``) or adds to them, and who zeroes a buffer that
``daam_reset`` only marked.  Every scenario holds the sums to the numpy oracle of exactly the steps they should hold:

  A  two launches into one sum, no reset between them: the second takes every kernel's non-fresh branch
  B  a generation, ``daam_reset``, a SHORTER generation of OTHER data: the fresh branch must overwrite (the buffers are not the
     ``torch.zeros`` of a first generation), a finalize afterwards must leave the new sums alone (every tap kind clears
     ``zero_pending``)
  C  a layer that is reset and not tapped again contributes zeros to a finalize and reads zero afterwards
  D  two DIFFERENT consumers on one layer's sums after ``clear()``: probabilities, the any-shape kernel, the fused tap of
     ``daam_attend``, an immediate and a deferred tap, a plane added by hand
  E  time windows: a second generation that is shorter than the first, per layer -- the windows it does not reach must read zero
     through ``window_items`` (they are owed a zeroing that only a finalize would settle; the engine zeroes them itself)

Data: two sets X and Y of other seeds whose K start-of-sequence row grows by other ladders (X: 1.0, 1.5, 2.0, ...; Y: 1.25, 1.5,
1.75, ...): no sum of Y steps is within tolerance of a sum of X steps, of X + Y, or of twice itself.  Generation 1 (X) always has more
steps than generation 2 (Y).  The per-pixel sum over the tokens of a running sum is its number of steps (each step's probabilities
sum to one), within ``steps * 77 * half_ulp`` as in ``test_gpu_layouts._check_sane``: a stale or a doubled row shows there on its own.
Tolerances: sums -- ``test_gpu_layouts.test_contiguous_baseline_vs_oracle`` with ``steps`` = the steps of the sum; maps -- the end-to-end
bounds of ``test_gpu_parity._global_tol`` (f32 2e-6 of the largest value, fp16 1e-3, bf16 8e-3).  Every launch's kernel name and block
size is asserted (``test_gpu_layouts._expected``), so that no scenario passes on another route.  Shapes: batch 2, hw 576 (partial
tiles, waves outside the tile, the slab's tail entry) and 256, at most 5 steps per generation."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import heatmap_oracle as ho
from test_gpu_layouts import BATCH, DEV, HWS, MODES, ROUTES, ROUTE_MODES, _bits, _configure, _expected, _last_launch, _qk_desc, _raw_engine
from test_gpu_parity import _dev, _engine, _oracle_steps, _qk, _to_bh

# D and E drive the engine: what daam_last_kernels / daam_last_launch report after each of its launches.  A deferred launch of
# head_dim-64 layers alone takes the eight-wave form (512), an immediate tap four waves (256); the any-shape kernel, the
# probabilities kernel and daam_attend (fused tap) run 256-thread workgroups.  daam_tap_probs and daam_attend report their block
# size but leave the kernel NAME of the last tap launch in place: their launches are told apart by what only they can produce
# (the attention output against the oracle; sums that are bit-equal to the oracle's adds).

pytestmark = pytest.mark.gpu

N_DATA = 5
GAINS = {'X': [1.0 + 0.5 * s for s in range(N_DATA)], 'Y': [1.25 + 0.25 * s for s in range(N_DATA)]}
SEEDS = {'X': 1000, 'Y': 2000}
WALK_BINS = [0, 2, 4]
# the pair kernel (tests/test_gpu_tap_plan.py 'pair_*'): DAAM_TAP_PAIR=1, two head_dim-64 layers on the same Q, the second with one K
PAIR = dict(d=64, heads=2, deferred=True, env=dict(DAAM_TAP_PAIR='1'), kernel=('tap_pair_kernel', 512), modes=('f16_exact',), pair=True)
CASES = ROUTE_MODES + [('pair', 'f16_exact')]
# B: (steps of generation 1, of generation 2).  With the windows [0, 2, 4] a generation of two steps stays in window 0 and the planner
# leaves a launch of one window per layer on tap_d64_kernel (asserted): the walk route also runs 5 and 3 steps, so that generation 2
# overwrites through tap_walk_kernel (windows 0 and 1) and leaves window 2 behind
B_CASES = [(r, m, 3, 2) for r, m in CASES] + [('walk', m, 5, 3) for m in ROUTES['walk']['modes']]


def _route(route):
    return PAIR if route == 'pair' else ROUTES[route]


def _kernel(route):
    return PAIR['kernel'] if route == 'pair' else _expected(route, 'L0')


_data_cache, _oracle_cache = {}, {}


def _data(name, hw, heads, d, np_dt):
    """N_DATA steps [(q, k)] of data set ``name`` (numpy, in the pipeline dtype)."""
    key = (name, hw, heads, d, str(np_dt))
    if key not in _data_cache:
        rng = np.random.default_rng(SEEDS[name] + hw + 7 * d + heads)
        _data_cache[key] = [_qk(rng, BATCH, heads, hw, d, np_dt, sos_gain=g) for g in GAINS[name]]
    return _data_cache[key]


def _oracle(name, hw, heads, d, mode, first, end, fixed_k=False):
    """float64 oracle sums [kept heads, 77, side, side] of the steps [first, end) of data set ``name`` in order, summed in the sum
    dtype of ``mode``; ``fixed_k``: every step against the K of step 0 (the pair's second chain)."""
    np_dt, _, accumulate, _ = MODES[mode]
    key = (name, hw, heads, d, str(np_dt), accumulate, first, end, fixed_k)
    if key not in _oracle_cache:
        data = _data(name, hw, heads, d, np_dt)
        qs = [q for q, _ in data[first:end]]
        ks = [data[0][1] if fixed_k else k for _, k in data[first:end]]
        acc_np = np.float32 if accumulate == 'float32' else np_dt
        _oracle_cache[key] = _oracle_steps(qs, ks, heads, d ** -0.5, np_dt, acc_np).astype(np.float64)
    return _oracle_cache[key]


def _half_ulp(mode):
    return 2.0 ** -8 if mode.startswith('bf16') else 2.0 ** -11          # of a probability <= 1


def _sum_tol(mode, want, steps):
    """test_contiguous_baseline_vs_oracle's bound for a sum of ``steps`` steps."""
    accumulate = MODES[mode][2]
    if mode == 'f32':
        return 2e-6 * max(1.0, np.abs(want).max())
    if accumulate == 'exact':
        return 2 * _half_ulp(mode) * max(1.0, want.max())               # 1 ulp of the largest running sum
    return steps * _half_ulp(mode)                                      # one flipped probability ulp per step


def _map_tol(mode, want):
    """test_gpu_parity._global_tol by pipeline dtype (the f32 one relative to the largest value, as its callers apply it)."""
    if mode == 'f32':
        return 2e-6 * max(1.0, float(np.abs(want).max()))
    return 8e-3 if mode.startswith('bf16') else 1e-3


def _check_sums(got, want, mode, steps, what):
    """``got`` (a CPU tensor) against the oracle ``want`` of a sum of ``steps`` steps, and its token sums against ``steps``."""
    got = got.float().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), what
    err, tol = np.abs(got - want).max(), _sum_tol(mode, want, steps)
    print(f'{what}: max-abs {err:.3e} (tolerance {tol:.3e})')
    assert err <= tol, f'{what}: max-abs {err} > {tol}'
    np.testing.assert_allclose(got.sum(-3), steps, atol=steps * 77 * _half_ulp(mode), err_msg=f'{what}: token sums')
    return err


def _oracle_map(planes):
    """The oracle's global heat map (64 x 64) of ``planes`` = one [kept heads, 77, side, side] array per layer."""
    raw = [((1, layer, h), p[h].astype(np.float32)) for layer, p in enumerate(planes) for h in range(p.shape[0])]
    return ho.global_heat_map(raw, 64 * 64)


class _T:
    """A contiguous device tensor [BATCH, rows, heads * d] as ``_qk_desc`` reads a placed one."""

    def __init__(self, t, d):
        self.t, self.ptr, self.strides = t, t.data_ptr(), (t.stride(0), d, t.stride(1))


class _Raw:
    """One native context of ``route`` / ``mode`` at ``hw`` through the C ABI: launches with the kernel name and block size asserted."""

    def __init__(self, monkeypatch, route, mode, hw):
        from daam_amd import _native as nat
        self.nat, self.route, self.mode, self.hw = nat, route, mode, hw
        r = self.r = _route(route)
        self.np_dt, self.dtype, accumulate, env = MODES[mode]
        _configure(monkeypatch, dict(r['env'], **env))
        self.bins = WALK_BINS if 'bins' in r else None
        self.n_layers = 2 if r.get('pair') else 1
        if r.get('pair'):
            self.eng = _layers_engine(self.dtype, accumulate, [int(math.isqrt(hw))] * 2, r['heads'])
        else:
            self.eng = _raw_engine(self.dtype, accumulate, r['heads'], hw, self.bins)
        self.keep = []                                        # a launch reads the tensors: alive until the context goes
        self.desc = None

    def steps(self, name, first, end):
        """Device steps [first, end) of data set ``name``: per step one (q, k) per layer (the pair: layer 1 on layer 0's Q and the
        K of the set's step 0)."""
        r = self.r
        data = [(_T(_dev(q, self.np_dt), r['d']), _T(_dev(k, self.np_dt), r['d'])) for q, k in _data(name, self.hw, r['heads'], r['d'], self.np_dt)]
        self.keep.append(data)
        return [[(q, k)] + ([(q, data[0][1])] if r.get('pair') else []) for q, k in data[first:end]]

    def launch(self, steps, expect=None):
        """The deferred routes: every step recorded, one flush; the immediate ones: one call per step."""
        nat, eng, r = self.nat, self.eng, self.r
        for per_layer in steps:
            for layer, (q, k) in enumerate(per_layer):
                if self.desc is None:
                    self.desc = _qk_desc(nat, self.dtype, r['heads'], self.hw, r['d'], q, k)
                if r['deferred']:
                    nat.check(eng.lib.daam_tap_qk_enqueue(eng.ctx, layer, q.ptr, k.ptr, ctypes.byref(self.desc)))
                else:
                    nat.check(eng.lib.daam_tap_qk(eng.ctx, layer, q.ptr, k.ptr, ctypes.byref(self.desc), eng.stream))
                    assert _last_launch(nat, eng) == (expect or _kernel(self.route)), (self.route, _last_launch(nat, eng))
        if r['deferred']:
            nat.check(eng.lib.daam_tap_flush(eng.ctx, eng.stream))
            assert _last_launch(nat, eng) == (expect or _kernel(self.route)), (self.route, _last_launch(nat, eng))

    def reset(self):
        self.nat.check(self.eng.lib.daam_reset(self.eng.ctx, self.eng.stream))

    def sums(self):
        torch.cuda.synchronize()
        return [self.eng.acc[layer].clone().cpu() for layer in range(self.n_layers)]

    def finalize(self):
        out = torch.full((77, 64, 64), -5.0, device=DEV)
        self.nat.check(self.eng.lib.daam_finalize(self.eng.ctx, None, 77, out.data_ptr(), self.eng.stream))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def close(self):
        torch.cuda.synchronize()
        self.eng.close()


def _layers_engine(dtype, accumulate, sides, heads, bins=None):
    """``test_gpu_layouts._raw_engine`` with one layer per entry of ``sides``."""
    eng = _engine(n_layers=len(sides), accumulate=accumulate, defer_steps=0, time_bins=bins)
    eng._require_device(torch.empty(1, device=DEV))
    eng._ensure_ctx(dtype)
    for layer, side in enumerate(sides):
        eng._ensure_layer(layer, BATCH * heads - (BATCH * heads) // 2, side, 1)
        eng._touch(layer)
    return eng


def _windows_of(n):
    """Steps [0, n) by window of WALK_BINS: [(first, end)] (empty windows: first == end)."""
    ends = WALK_BINS[1:] + [max(n, WALK_BINS[-1])]
    return [(min(b, n), min(e, n)) for b, e in zip(WALK_BINS, ends)]


def _want(run, name, n):
    """Per layer: the oracle of the steps [0, n) of ``name`` as ``run``'s buffers are laid out (a binned context: one sum per
    window, zeros where no step fell), and the steps of every sum."""
    r = run.r
    out, counts = [], None
    for layer in range(run.n_layers):
        args = (name, run.hw, r['heads'], r['d'], run.mode)
        if run.bins is None:
            out.append(_oracle(*args, 0, n, fixed_k=layer == 1))
            counts = n
        else:
            wins = _windows_of(n)
            full = _oracle(*args, 0, 1)
            out.append(np.stack([_oracle(*args, a, b) if b > a else np.zeros_like(full) for a, b in wins]))
            counts = [b - a for a, b in wins]
    return out, counts


def _check_run(run, got, want, counts, what):
    worst = 0.0
    for layer, (g, w) in enumerate(zip(got, want)):
        if run.bins is None:
            worst = max(worst, _check_sums(g, w, run.mode, counts, f'{what} layer {layer}'))
        else:
            for win, n in enumerate(counts):
                if n:
                    worst = max(worst, _check_sums(g[win], w[win], run.mode, n, f'{what} layer {layer} window {win}'))
    return worst


# ---- A: two launches into one sum ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', HWS)
@pytest.mark.parametrize('route,mode', CASES)
def test_a_second_launch_adds_to_the_first(route, mode, hw, monkeypatch):
    """Launch 1 = Y[0:2], launch 2 = Y[2:4], no reset between them.  Walk: windows [0, 2, 4], launch 1 = steps 0..2, launch 2 = steps
    3..4: window 1 is cut by the launch boundary and continues non-fresh while window 2 starts fresh in the same launch."""
    run = _Raw(monkeypatch, route, mode, hw)
    cut, n = (3, 5) if run.bins else (2, 4)
    steps = run.steps('Y', 0, n)
    run.launch(steps[:cut])
    run.launch(steps[cut:])
    got = run.sums()
    run.close()
    want, counts = _want(run, 'Y', n)
    _check_run(run, got, want, counts, f'A {route} {mode} hw {hw}')


# ---- B: reset, then a shorter generation of other data --------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', HWS)
@pytest.mark.parametrize('route,mode,n1,n2', B_CASES)
def test_b_generation_after_reset_overwrites(route, mode, n1, n2, hw, monkeypatch):
    """X[0:n1], daam_reset, Y[0:n2] (the immediate routes: the second call reads what the first overwrote).  The sums equal those of
    the same generation 2 on a new context bit for bit and the oracle of Y alone; daam_finalize leaves them bit-unchanged and gives the
    oracle's map of Y's sums.  A binned context: the windows generation 2 did not reach are owed a zeroing that the C ABI settles in
    the finalize (the engine's views: scenario E) -- they are compared after it, and must then read zero."""
    what = f'B {route} {mode} hw {hw} {n1}+{n2}'
    run = _Raw(monkeypatch, route, mode, hw)
    reached = [b > a for a, b in _windows_of(n2)] if run.bins else None
    second = _kernel(route)
    if run.bins and sum(reached) == 1:
        second = ('tap_d64_kernel', 512)                      # one window per layer in the launch: no walk (tap_plan 'walk_single_window')
    run.launch(run.steps('X', 0, n1))
    first = run.sums()
    assert all(float(t.float().abs().max()) > 0 for t in first)
    run.reset()
    run.launch(run.steps('Y', 0, n2), second)
    got = run.sums()
    fresh_run = _Raw(monkeypatch, route, mode, hw)
    fresh_run.launch(fresh_run.steps('Y', 0, n2), second)
    fresh = fresh_run.sums()
    fresh_run.close()

    def live(t):
        return t if reached is None else t[torch.tensor(reached)]
    for layer, (a, b) in enumerate(zip(got, fresh)):
        differ = _bits(live(a)) != _bits(live(b))
        assert not differ.any(), f'{what} layer {layer}: {int(differ.sum())} of {differ.numel()} sums differ from a new context'
    want, counts = _want(run, 'Y', n2)
    _check_run(run, got, want, counts, what)
    gm = run.finalize()
    after = run.sums()
    run.close()
    for layer, (a, b, f) in enumerate(zip(after, got, fresh)):
        assert torch.equal(_bits(live(a)), _bits(live(b))), f'{what} layer {layer}: the finalize changed the sums'
        assert torch.equal(_bits(a), _bits(f)), f'{what} layer {layer}: a window generation 2 did not reach is not zero after the finalize'
    want_map = _oracle_map([w.sum(0) if run.bins else w for w in want])
    err, tol = float(np.abs(gm - want_map).max()), _map_tol(mode, want_map)
    print(f'{what}: map max-abs {err:.3e} (tolerance {tol:.3e})')
    assert err <= tol, f'{what}: map max-abs {err} > {tol}'


# ---- C: a layer reset and not tapped again -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['finalize', 'finalize_groups'])
def test_c_layer_not_tapped_after_reset_counts_as_zero(entry, monkeypatch):
    """Layers of sides 24 and 16 (head_dim 64), both tapped with X[0:3]; reset; Y[0:2] on layer 0 only; a finalize over both layers.
    daam_finalize on fp16 sums; daam_finalize_groups (two groups: head 0 / head 1 of both layers) on f32 sums."""
    from daam_amd import _native as nat
    mode = 'f16_exact' if entry == 'finalize' else 'f16_f32acc'
    np_dt, dtype, accumulate, _ = MODES[mode]
    heads, d, sides = 2, 64, [24, 16]
    _configure(monkeypatch, {})
    eng = _layers_engine(dtype, accumulate, sides, heads)
    keep = []

    def tap(name, first, end, layers):
        for s in range(first, end):
            for layer in layers:
                hw = sides[layer] ** 2
                q, k = (_T(_dev(x, np_dt), d) for x in _data(name, hw, heads, d, np_dt)[s])
                keep.append((q, k))
                desc = _qk_desc(nat, dtype, heads, hw, d, q, k)
                nat.check(eng.lib.daam_tap_qk_enqueue(eng.ctx, layer, q.ptr, k.ptr, ctypes.byref(desc)))
        nat.check(eng.lib.daam_tap_flush(eng.ctx, eng.stream))
        assert _last_launch(nat, eng) == ('tap_d64_kernel', 512)
    tap('X', 0, 3, (0, 1))
    torch.cuda.synchronize()
    assert float(eng.acc[1].float().abs().max()) > 0
    nat.check(eng.lib.daam_reset(eng.ctx, eng.stream))
    tap('Y', 0, 2, (0,))
    torch.cuda.synchronize()
    before = eng.acc[0].clone()
    y0 = _oracle('Y', 576, heads, d, mode, 0, 2)
    _check_sums(before.cpu(), y0, mode, 2, f'C {entry} layer 0')
    zeros = np.zeros((heads, 77, 16, 16))
    if entry == 'finalize':
        out = torch.full((77, 64, 64), -5.0, device=DEV)
        nat.check(eng.lib.daam_finalize(eng.ctx, None, 77, out.data_ptr(), eng.stream))
        want = [_oracle_map([y0, zeros])]
        got = [out]
    else:
        out = torch.full((2, 77, 64, 64), -5.0, device=DEV)
        i32 = ctypes.c_int32
        nat.check(eng.lib.daam_finalize_groups(eng.ctx, (i32 * 4)(0, 1, 0, 1), 2, (i32 * 2)(77, 77), out.data_ptr(), 77 * 64 * 64, eng.stream))
        want = [_oracle_map([y0[g:g + 1], zeros[g:g + 1]]) for g in range(2)]
        got = [out[0], out[1]]
    torch.cuda.synchronize()
    for g, (a, w) in enumerate(zip(got, want)):
        err, tol = float(np.abs(a.cpu().numpy() - w).max()), _map_tol(mode, w)
        print(f'C {entry} group {g}: map max-abs {err:.3e} (tolerance {tol:.3e})')
        assert err <= tol, (entry, g, err)
    assert not bool(eng.acc[1].any()), 'the layer that was not tapped again does not read zero after the finalize'
    assert torch.equal(_bits(eng.acc[0]), _bits(before)), 'the finalize changed the sums of the layer that was tapped'
    eng.close()


# ---- D: mixed consumers of one layer's sums --------------------------------------------------------------------------------------------
# (first operation, second operation) of generation 2: every kind once in each place, never beside itself.  'generic' is the immediate tap
# of a context created under DAAM_FORCE_GENERIC=1 (the switch is read then), where 'qk' / 'deferred' would be the same kernel: its
# partners are the kernels the switch leaves alone.
D_SEQUENCES = [('probs', 'qk'), ('generic', 'attend'), ('attend', 'deferred'), ('qk', 'add_map'), ('deferred', 'probs'), ('add_map', 'generic')]


@pytest.mark.parametrize('hw', [256, 576])
@pytest.mark.parametrize('accumulate', ['exact', 'float32'])
@pytest.mark.parametrize('ops', D_SEQUENCES, ids=['+'.join(s) for s in D_SEQUENCES])
def test_d_mixed_consumers(ops, accumulate, hw, monkeypatch):
    """Generation 1: three deferred steps of X, launched; clear() with no views out (the buffer is kept and owed a zeroing).
    Generation 2: two operations of different kinds on Y's steps 0 and 1 -- the second reads sums another kernel wrote, the first
    must overwrite or zero what generation 1 left."""
    heads, d, side = 2, 64, int(math.isqrt(hw))
    mode = 'f16_exact' if accumulate == 'exact' else 'f16_f32acc'
    scale = d ** -0.5
    generic = 'generic' in ops
    _configure(monkeypatch, dict(DAAM_FORCE_GENERIC='1') if generic else {})
    monkeypatch.setenv('DAAM_NO_FASTPATH', '1')               # the Python recorder: the test switches between deferred and immediate taps
    eng = _engine(n_layers=1, accumulate=accumulate, defer_steps=4)

    def deferred(on):
        eng.flush()
        eng.defer_steps = 4 if on else 0
        eng._set_window(eng.defer_steps)
    x = [(_dev(q), _dev(k)) for q, k in _data('X', hw, heads, d, np.float16)[:3]]
    for q, k in x:
        eng.tap_qk(0, q, k, heads, scale, 1)
    eng.flush()
    from daam_amd import _native as nat
    qk_deferred = ('tap_generic_kernel', 256) if generic else ('tap_d64_kernel', 512)
    qk_immediate = ('tap_generic_kernel', 256) if generic else ('tap_d64_kernel', 256)
    assert _last_launch(nat, eng) == qk_deferred, _last_launch(nat, eng)
    torch.cuda.synchronize()
    assert float(eng.acc[0].float().abs().max()) > 0
    eng.clear()
    acc_np = np.float32 if accumulate == 'float32' else np.float16
    raw = ho.RawMaps(acc_np)
    rng = np.random.default_rng(hw + len(ops[0]))
    y = _data('Y', hw, heads, d, np.float16)
    keep, n_taps, planes = [], 0, False
    for step, op in enumerate(ops):
        q_np, k_np = y[step]
        q, k = _dev(q_np), _dev(k_np)
        keep.append((q, k))
        if op == 'add_map':
            plane = (rng.random((77, side, side)) * 0.5).astype(np.float16)
            torch.cuda.synchronize()
            base = eng.acc[0].clone() if step else torch.zeros_like(eng.acc[0])
            deferred(False)
            eng.add_map(1, 0, 1, _dev(plane))
            raw.update(1, 0, 1, plane)
            if not step:
                raw.update(1, 0, 0, np.zeros_like(plane))    # (the oracle keeps no key it has not seen; the layer has both heads)
                raw.maps = {key: raw.maps[key] for key in sorted(raw.maps)}
            torch.cuda.synchronize()
            base[1] += _dev(plane).to(base.dtype)
            assert torch.equal(_bits(eng.acc[0]), _bits(base)), f'{ops}: the plane did not arrive exactly (on zeros, if it came first)'
            planes = True
            continue
        n_taps += 1
        if op == 'probs':
            probs = ho.attention_probs(_to_bh(q_np, heads), _to_bh(k_np, heads), scale, np.float16)
            ho.tap(raw, 0, None, None, scale, latent_hw=hw, pipe_dtype=np.float16, probs=probs)
            torch.cuda.synchronize()
            base = (eng.acc[0].clone() if step else torch.zeros_like(eng.acc[0])).cpu()
            eng.tap_probs(0, _dev(probs), 1)
            assert _last_launch(nat, eng)[1] == 256
            # the probabilities kernel adds the given numbers in the sum dtype: exactly base + unravel(probs), which no softmax kernel
            # reproduces bit for bit on its own logits
            torch.cuda.synchronize()
            added = base + torch.from_numpy(ho.unravel(probs)).to(base.dtype)
            assert torch.equal(_bits(eng.acc[0].cpu()), _bits(added)), f'{ops}: tap_probs did not add exactly the given probabilities'
            continue
        ho.tap(raw, 0, _to_bh(q_np, heads), _to_bh(k_np, heads), scale, latent_hw=hw, pipe_dtype=np.float16)
        if op == 'attend':
            deferred(False)
            v_np = rng.standard_normal(k_np.shape).astype(np.float16)
            v = _dev(v_np)
            keep.append(v)
            out = eng.attend(0, q, k, v, heads, scale, 1, tapped=True)
            assert out is not None and _last_launch(nat, eng)[1] == 256
            # the fused kernel is the one that writes the attention output: test_gpu_layouts.test_attend_baseline_matches_reference's bound
            want_out = ho.batch_to_head_dim(ho.attention_output(_to_bh(q_np, heads), _to_bh(k_np, heads), _to_bh(v_np, heads), scale, np.float16),
                                            heads).astype(np.float32)
            err = float(np.abs(out.float().cpu().numpy() - want_out).max())
            assert err <= 2e-3 * float(np.abs(want_out).max()), f'{ops}: attend output max-abs {err}'
        elif op == 'deferred':
            deferred(True)
            eng.tap_qk(0, q, k, heads, scale, 1)
            eng.flush()
            assert _last_launch(nat, eng) == qk_deferred, _last_launch(nat, eng)
        else:                                                  # 'qk' / 'generic': an immediate tap
            deferred(False)
            eng.tap_qk(0, q, k, heads, scale, 1)
            assert _last_launch(nat, eng) == qk_immediate, _last_launch(nat, eng)
    torch.cuda.synchronize()
    got = eng.acc[0].clone().cpu()
    want = np.stack([raw.maps[(1, 0, h)] for h in range(heads)]).astype(np.float64)
    what = f'D {"+".join(ops)} {accumulate} hw {hw}'
    g64 = got.float().numpy().astype(np.float64)
    err, tol = np.abs(g64 - want).max(), _sum_tol(mode, want, n_taps)
    print(f'{what}: max-abs {err:.3e} (tolerance {tol:.3e})')
    assert err <= tol, f'{what}: max-abs {err} > {tol}'
    if not planes:
        np.testing.assert_allclose(g64.sum(-3), n_taps, atol=n_taps * 77 * _half_ulp(mode), err_msg=f'{what}: token sums')
    gm = eng.global_heat_map().cpu().numpy()
    torch.cuda.synchronize()
    assert torch.equal(_bits(eng.acc[0].cpu()), _bits(got)), f'{what}: the finalize changed the sums'
    want_map = _oracle_map([want])
    err, tol = float(np.abs(gm - want_map).max()), _map_tol(mode, want_map)
    print(f'{what}: map max-abs {err:.3e} (tolerance {tol:.3e})')
    assert err <= tol, f'{what}: map max-abs {err} > {tol}'
    eng.close()


# ---- E: time windows and a shorter second generation ----------------------------------------------------------------------------------
@pytest.mark.parametrize('reuse', [False, True], ids=['clear', 'adopted'])
@pytest.mark.parametrize('walk', ['0', '1'])
def test_e_windows_a_shorter_generation_does_not_reach(walk, reuse, monkeypatch):
    """Windows [0, 2, 4], head_dim-64 layers of sides 24 and 16.  Generation 1: 5 steps of X on both, launched; clear() with no views
    out -- or close() and a second engine that adopts the parked context.  Generation 2: 3 steps of Y on layer 0, 1 on layer 1.  What
    ``window_items`` hands out is generation 2's: window 2 of layer 0 and windows 1, 2 of layer 1 read exactly zero."""
    from daam_amd import _native as nat
    from daam_amd import engine as E
    heads, d, sides, mode = 2, 64, [24, 16], 'f16_exact'
    scale = d ** -0.5
    _configure(monkeypatch, dict(DAAM_TAP_WALK=walk))
    name = 'tap_walk_kernel' if walk == '1' else 'tap_d64_kernel'

    def make():
        return _engine(n_layers=2, accumulate='exact', defer_steps=8, time_bins=WALK_BINS, reuse_context=reuse)

    def generation(eng, data, counts):
        keep = []
        for s in range(max(counts)):
            for layer, n in enumerate(counts):
                if s < n:
                    q, k = (_dev(t) for t in _data(data, sides[layer] ** 2, heads, d, np.float16)[s])
                    keep.append((q, k))
                    eng.tap_qk(layer, q, k, heads, scale, 1)
        eng.flush()
        assert _last_launch(nat, eng) == (name, 512), _last_launch(nat, eng)
        torch.cuda.synchronize()
    eng = make()
    generation(eng, 'X', (5, 5))
    assert all(float(eng.acc[layer][2].float().abs().max()) > 0 for layer in (0, 1))
    if reuse:
        ctx = eng.ctx.value
        eng.close()
        eng = make()
    else:
        eng.clear()
    counts = (3, 1)
    generation(eng, 'Y', counts)
    if reuse:
        assert eng.ctx.value == ctx, 'the parked context was not adopted'
    assert eng.window_steps() == [2, 1, 0]
    want = []                                                 # [window][layer]: float64 sums, or None where the layer has no step
    for a, b in zip(WALK_BINS, WALK_BINS[1:] + [N_DATA]):
        want.append([_oracle('Y', sides[layer] ** 2, heads, d, mode, a, min(b, n)) if min(b, n) > a else None
                     for layer, n in enumerate(counts)])
    steps_in = [[max(0, min(b, n) - a) for n in counts] for a, b in zip(WALK_BINS, WALK_BINS[1:] + [N_DATA])]
    for w in range(3):
        items = eng.window_items(w)
        torch.cuda.synchronize()
        assert list(items) == [(1, layer, h) for layer in (0, 1) for h in range(heads)]
        for layer in (0, 1):
            got = torch.stack([items[(1, layer, h)] for h in range(heads)]).cpu()
            if want[w][layer] is None:
                assert not bool(got.any()), f'E walk={walk} window {w} layer {layer}: {int((got != 0).sum())} stale sums'
            else:
                _check_sums(got, want[w][layer], mode, steps_in[w][layer], f'E walk={walk} window {w} layer {layer}')

    def planes(w0, w1):
        out = []
        for layer in (0, 1):
            total = np.zeros((heads, 77, sides[layer], sides[layer]))
            for w in range(w0, w1):
                if want[w][layer] is not None:
                    total = total + want[w][layer]
            out.append(total)
        return out
    for bins in [(0, 1), (1, 2), (2, 3), None]:
        gm = eng.global_heat_map(bins=bins).cpu().numpy()
        want_map = _oracle_map(planes(*(bins or (0, 3))))
        err, tol = float(np.abs(gm - want_map).max()), _map_tol(mode, want_map)
        print(f'E walk={walk} bins {bins}: map max-abs {err:.3e} (tolerance {tol:.3e})')
        assert err <= tol, (bins, err)
    eng.close()
    E.release_parked_contexts()
