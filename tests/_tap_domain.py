"""Shared by ``test_tap_domain_cpu.py`` and ``test_gpu_tap_domain.py``: the tap's own running sums held to the float64 softmax PER
PROBABILITY, on the rows of ``tests/_attend_domain.py`` (``ad.build``, unchanged), and the numpy emulation and mutants that show what
the bound catches.

Inputs.  Q / K are multiples of 1/4, so every f32 logit is the same number in any summation order.  Pixel p has kind ``ad.KINDS[p %
13]``: ``spread`` rows (77 probabilities of about 1e-2), ``tie2`` rows, and ``gap8`` .. ``gap20`` rows, on which one designed token
sits 8 / 12 / 16 / 20 nats above 76 minor tokens that differ from each other: minor probabilities that are fp16 normals (3e-4), a
hundred fp16-subnormal ulps (6e-6), a few subnormal ulps (1e-7), and zero after the rounding.  The designed token rotates over
tokens 0 / 5 / 41 / 76 with the step: over a few steps one sum element of those four tokens receives a probability near 1 and
probabilities near 1e-7 (the fp16 absorption case, in the reference's order), and the other 73 tokens' elements stay minor throughout.

Reference.  Per step the logits as the pipeline forms them (``sd.rounded_logits``: f32 accumulation, the scale in f32, one rounding
to the pipeline dtype, none with ``round_logits = 0``) and ``p64``, their float64 softmax, left unrounded.  ``A_s = sum_{i<=s} p64_i``.

Bound, per sum element, from the number formats only (``E_0 = 0``; ``u(x) = sd.ulp_of(x, dtype)``, for fp16 the subnormal spacing
2^-24 below 2^-14):

  f32 sums             E_s = E_{s-1} + u(p64_s) + 2^-24 A_s
                       one ulp on each probability (what the project allows a correct softmax: ``sd.output_slack``) and the f32 add
  fp16 / bf16 sums     E_s = E_{s-1} + u(p64_s) + u(A_s + E_{s-1} + u(p64_s)) / 2
                       the last term: the rounding of the add at the largest value the sum can have there
  f32 pipeline         E_s = E_{s-1} + c 2^-24 p64_s + 2^-24 A_s                      (``any_shape_f32``: nothing is rounded to 16 bits)

``c``, in units of 2^-24 relative (half an f32 ulp), read off ``tap_generic_kernel`` (daam_amd/csrc/daam_kernels.hip); p = e_t / sum:

  76          the 77-term f32 sum: 19 adds per thread and 3 across the four token chunks, each rounded relative to a partial sum that
              is no larger than the total (76 covers every order)
  2 + 2       ``expf``: one ulp on the numerator, one ulp on every term of the denominator
  2           the division (one ulp; half of it where the compiler's correctly rounded division is on)
  2 * spread  ``logit - m`` is one f32 subtraction: its rounding, at most 2^-24 |x_t - m| in nats, is a relative error of e_t; once on
              the numerator, once (as a weighted mean over the terms) on the denominator.  ``spread`` = the row's max - min logit,
              at most twice its largest |logit|.  (``expf`` itself forms ``x log2 e`` in two pieces: no further argument rounding.)

so ``c = 82 + 2 spread`` per row: 82 .. 130 on these inputs (spreads up to 24 nats).  It is a worst case over 80 roundings; the rows
here have ``x_t - m`` exact, and the kernel measures 0.12 of the bound (LABNOTES R8.9).

Rounding bias.  A conversion that truncates stays inside one ulp, so the bound cannot see it.  On the runs with f32 sums, over the
elements of ``spread`` pixels whose p64_s >= 2^-14 at every step (normal in fp16: the ulp follows the value):

  | mean( (got - A_n) / sum_s u(p64_s) ) | <= 0.05       over N >= 4096 elements (asserted, not skipped)

Round-to-nearest leaves errors uniform in +-1/2 ulp: the mean of N of them has sigma = 0.289 / sqrt(N) <= 0.0045, so 0.05 is ten
sigma; truncation gives -0.5.  Not extended to the gap kinds: their minor probabilities cluster, and the reference's own mean
reaches 0.14 there.

Mutants (``MUTANTS``), applied to the emulation (``sd.emulate_fast_probs`` plus the sum in the sum dtype):

  flush       fp16 probabilities below 2^-14 become 0 (a conversion, a packed add or the f32 widening that drops subnormals)
  truncate    the conversion to the pipeline dtype rounds toward zero (bf16 is narrowed by hand on gfx950)
  swap        two minor tokens (``SWAP``) exchanged on the gap rows
  padding     three extra exp(0) terms in the row sum (the padding slots 77..79 un-masked; their K rows are zero)
  exp_rounded the exponential rounded to the pipeline dtype before the sum"""
import numpy as np

import _attend_domain as ad
import _softmax_domain as sd
from oracle import heatmap_oracle as ho

TOKENS = ad.TOKENS
NORMAL_MIN = 2.0 ** -14                              # smallest fp16 normal
BIAS_LIMIT, BIAS_MIN_COUNT = 0.05, 4096
MUTANTS = ('flush', 'truncate', 'swap', 'padding', 'exp_rounded')
SWAP = (10, 11)                                      # two tokens that are never the designed one
C_FIXED = 76 + 2 + 2 + 2                             # f32 pipeline: sum, expf twice, division (module docstring)


def sum_dtype(np_dt, accumulate):
    """numpy dtype of the running sums: the pipeline dtype (``exact``) or float32."""
    return np.float32 if accumulate == 'float32' else np_dt


def is_f32(dt):
    return not ho.is_bf16(dt) and np.dtype(dt) == np.float32


def kept_logits(steps, heads, scale, np_dt, upcast=False):
    """[steps, kept heads, hw, 77] float32: the logits of the half the tap keeps, as the pipeline forms them."""
    return np.stack([sd.rounded_logits(sd.kept(sd.to_bh(np.asarray(q, np.float32), heads)), sd.kept(sd.to_bh(np.asarray(k, np.float32), heads)),
                                       scale, np_dt, upcast) for q, k in steps])


def softmax64(logits):
    """float64 softmax of the given logits, unrounded."""
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def per_token(x):
    """[..., hw, 77] -> [..., 77, hw]: the layout of the running sums."""
    return np.ascontiguousarray(np.swapaxes(x, -1, -2))


def reference(steps, heads, scale, np_dt, acc_np, upcast=False):
    """``dict(logits, p64 [steps, kept heads, hw, 77], want = A_n and bound = E_n [kept heads, 77, hw])``."""
    logits = kept_logits(steps, heads, scale, np_dt, upcast)
    p64 = softmax64(logits)
    want, bnd = bound(p64, logits, np_dt, acc_np)
    return dict(logits=logits, p64=p64, want=per_token(want), bound=per_token(bnd))


def windows(ref, np_dt, acc_np):
    """The same steps judged as one-step sums (time windows of one step each): ``want`` / ``bound`` [steps, kept heads, 77, hw]."""
    parts = [bound(ref['p64'][s:s + 1], ref['logits'][s:s + 1], np_dt, acc_np) for s in range(len(ref['p64']))]
    return dict(logits=ref['logits'], p64=ref['p64'], want=np.stack([per_token(a) for a, _ in parts]),
                bound=np.stack([per_token(e) for _, e in parts]))


def bound(p64, logits, np_dt, acc_np):
    """``(A_n, E_n)`` [kept heads, hw, 77] of the module docstring for probabilities ``p64`` [steps, ...]."""
    a, e = np.zeros(p64.shape[1:]), np.zeros(p64.shape[1:])
    for p, x in zip(p64, logits):
        a = a + p
        if is_f32(np_dt):
            x = np.asarray(x, np.float64)
            c = C_FIXED + 2.0 * (x.max(-1, keepdims=True) - x.min(-1, keepdims=True))
            e = e + c * 2.0 ** -24 * p + 2.0 ** -24 * a
        elif is_f32(acc_np):
            e = e + sd.ulp_of(p, np_dt) + 2.0 ** -24 * a
        else:
            t = e + sd.ulp_of(p, np_dt)
            e = t + 0.5 * sd.ulp_of(a + t, np_dt)
    return a, e


def worst_by_kind(got, ref, names):
    """``{kind: (worst |got - A_n| / E_n, (head, pixel, token))}`` of sums [kept heads, 77, hw] (leading window axes are folded into
    the heads') against ``reference``'s or ``windows``' dict."""
    got = np.asarray(got, np.float64).reshape(ref['want'].shape)
    ratio = (np.abs(got - ref['want']) / ref['bound']).reshape(-1, TOKENS, len(names))
    out = {}
    for kind in ad.KIND_NAMES:
        sel = names == kind
        if sel.any():
            part = np.where(sel[None, None, :], ratio, -1.0)
            h, t, p = np.unravel_index(int(part.argmax()), part.shape)
            out[kind] = (float(part[h, t, p]), (int(h), int(p), int(t)))
    return out


def report(worst):
    return ', '.join(f'{kind} {r:.3f} (head {h} pixel {p} token {t})' for kind, (r, (h, p, t)) in worst.items())


def assert_inside_bound(got, ref, names, what):
    """Every element within E_n of A_n; prints the worst ratio per kind."""
    got = np.asarray(got, np.float64)
    assert got.size == ref['want'].size, (what, got.shape, ref['want'].shape)
    assert np.isfinite(got).all(), f'{what}: {int((~np.isfinite(got)).sum())} non-finite sums'
    worst = worst_by_kind(got, ref, names)
    print(f'{what}: worst |got - A_n| / E_n per kind -- {report(worst)}')
    assert set(worst) == set(ad.KIND_NAMES), (what, sorted(worst))
    bad = {kind: (round(r, 3), at) for kind, (r, at) in worst.items() if not r <= 1.0}
    assert not bad, f'{what}: outside the bound at (head, pixel, token) -- {bad}'
    return worst


def bias_terms(got, p64, names, np_dt):
    """``(got - A_n) / sum_s u(p64_s)`` of the elements the bias rule covers, 1-D.  ``got`` [kept heads, 77, hw], ``p64`` [steps, kept
    heads, hw, 77]."""
    got = np.asarray(got, np.float64).reshape(p64.shape[1], TOKENS, p64.shape[2])
    sel = per_token((p64.min(0) >= NORMAL_MIN) & (names == 'spread')[None, :, None])
    return ((got - per_token(p64.sum(0))) / per_token(sd.ulp_of(p64, np_dt).sum(0)))[sel]


def bias(got, ref, names, np_dt, per_window=False):
    """``(mean, N)`` of the bias rule; ``per_window``: ``got`` [steps, kept heads, 77, hw] holds one-step sums, pooled."""
    if per_window:
        terms = np.concatenate([bias_terms(g, ref['p64'][s:s + 1], names, np_dt) for s, g in enumerate(np.asarray(got, np.float64))])
    else:
        terms = bias_terms(got, ref['p64'], names, np_dt)
    return float(terms.mean()), int(terms.size)


def assert_unbiased(got, ref, names, np_dt, what, per_window=False):
    mean, count = bias(got, ref, names, np_dt, per_window)
    print(f'{what}: rounding bias {mean:+.4f} ulp over {count} elements (limit {BIAS_LIMIT})')
    assert count >= BIAS_MIN_COUNT, f'{what}: only {count} elements carry the bias rule'
    assert abs(mean) <= BIAS_LIMIT, f'{what}: mean error {mean:+.4f} ulp over {count} elements: the conversion does not round to nearest'
    return mean, count


# ---- the literal oracle, the emulation and its mutants ---------------------------------------------------------------------------
def oracle_sums(steps, heads, scale, np_dt, acc_np, upcast=False):
    """``ho.tap`` into ``ho.RawMaps``: [kept heads, 77, hw] float64."""
    raw = ho.RawMaps(acc_np)
    for q, k in steps:
        ho.tap(raw, 0, sd.to_bh(np.asarray(q, np.float32), heads), sd.to_bh(np.asarray(k, np.float32), heads), scale, latent_hw=q.shape[1],
               pipe_dtype=np_dt, upcast_attention=upcast)
    return np.stack([v for _, v in raw]).astype(np.float64).reshape(len(raw), TOKENS, -1)


def _toward_zero(x, np_dt):
    x = np.asarray(x, np.float32)
    if ho.is_bf16(np_dt):
        return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r = x.astype(np.float16)
    return np.where(np.abs(r.astype(np.float32)) > np.abs(x), np.nextafter(r, np.float16(0)), r).astype(np.float32)


def emulated_probs(logits, np_dt, mutant=None, gap_rows=None):
    """``sd.emulate_fast_probs`` with the mutants' hooks (``mutant=None`` is that function, bit for bit); float32 [..., hw, 77]."""
    assert mutant is None or mutant in MUTANTS, mutant
    L = float(np.float32(1.44269502162933349609375))
    x = np.asarray(logits, np.float64)
    nml = np.float32(-x.max(-1, keepdims=True) * L).astype(np.float64)
    e = np.exp2((x * L + nml).astype(np.float32).astype(np.float64)).astype(np.float32)
    if mutant == 'exp_rounded':
        e = sd._round(e, np_dt).astype(np.float32)
    tot = e.sum(-1, keepdims=True, dtype=np.float32)
    if mutant == 'padding':                                   # logit 0 in the slots of tokens 77..79
        tot = tot + np.float32(3) * np.exp2(nml).astype(np.float32)
    p = e * (np.float32(1) / tot)
    p = _toward_zero(p, np_dt) if mutant == 'truncate' else sd._round(p, np_dt).astype(np.float32)
    if mutant == 'flush' and not ho.is_bf16(np_dt):
        p = np.where(p < NORMAL_MIN, np.float32(0), p)
    if mutant == 'swap':
        a, b = SWAP
        q = p.copy()
        q[..., gap_rows, a], q[..., gap_rows, b] = p[..., gap_rows, b], p[..., gap_rows, a]
        p = q
    return p


def emulated_sums(logits_steps, np_dt, acc_np, names, mutant=None):
    """The emulation's running sums [kept heads, 77, hw] float64: one add per step in the sum dtype (heatmap.py:156)."""
    gap_rows = np.isin(names, list(ad.GAPS))
    total = None
    for logits in logits_steps:
        p = per_token(emulated_probs(logits, np_dt, mutant, gap_rows))
        if is_f32(acc_np):
            total = p if total is None else total + p
        elif ho.is_bf16(acc_np):
            total = p if total is None else ho.round_bf16(total + p)
        else:
            total = p.astype(np.float16) if total is None else total + p.astype(np.float16)
    return np.asarray(total, np.float64)


def old_tolerance(np_dt, acc_np, want, steps):
    """What tests/test_gpu_parity.py::test_tap_qk_vs_oracle accepts: ``2 half_ulp max(1, max want)`` resp. ``steps half_ulp``."""
    half_ulp = 2.0 ** -8 if ho.is_bf16(np_dt) else 2.0 ** -11
    return steps * half_ulp if is_f32(acc_np) else 2 * half_ulp * max(1.0, float(np.max(want)))
