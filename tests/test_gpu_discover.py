"""``libdaam_discover.so`` (include/daam_discover.h) on the device: the four entry points through ctypes on guarded
buffers -- 0xA5 guards, outputs pre-filled with NaN bytes, inputs unchanged afterwards, two runs bit-identical -- held to the float64
restatements of ``_discover_domain`` inside the bounds derived there, and ``SelfAffinity.discover`` end to end on the planted
affinities and behind the stand-in pipelines.  A missing library is a failure.  Figures are printed before they are asserted
(``pytest -s``).

A tile of D is 64 x 64 and a chunk 32 cells: A, B = 1, 3, 63, 65, 130 sit inside one tile, on either side of its edge and across three;
N = 1, 7, 64, 65, 257, 1024 are below a chunk, a whole number of chunks and one cell more, with the float4 loads (N a multiple of 4) and
the scalar ones."""
import numpy as np
import pytest
import torch

import _discover_domain as DD
from oracle import fake_diffusers as fd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


class Buf:
    """``n_bytes`` on the device at ``offset`` bytes past 16-byte alignment between two guards of 0xA5, holding ``array`` or 0xFF."""

    def __init__(self, array=None, n_bytes=None, offset=0):
        self.n = int(array.nbytes if array is not None else n_bytes)
        self.raw = torch.full((GUARD + 16 + max(self.n, 1) + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.start = GUARD + (-(self.raw.data_ptr() + GUARD) % 16) + offset
        if array is not None:
            flat = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(DEV)
            self.raw[self.start:self.start + self.n] = flat
        else:
            self.raw[self.start:self.start + self.n] = 0xFF
        self.before = self.raw.clone()

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.start

    def get(self, dtype, shape):
        return self.raw[self.start:self.start + self.n].cpu().numpy().view(dtype).reshape(shape).copy()

    def intact(self):
        return bool((self.raw[:self.start] == 0xA5).all()) and bool((self.raw[self.start + self.n:] == 0xA5).all())

    def unchanged(self):
        return torch.equal(self.raw, self.before)


def _run(fn, inputs, outputs, args):
    """One call on the current stream; every guard intact, every input unchanged."""
    from daam_amd import _native as nat
    lib = nat.load_discover()
    nat.check_discover(getattr(lib, 'daam_discover_' + fn)(*args, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert all(b.intact() for b in inputs + outputs), 'a guard was written'
    assert all(b.unchanged() for b in inputs), 'an input changed'


def _worst(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / bound).max())
    print(f'\n{name}: worst error {err.max():.3e}, worst device error / bound {ratio:.3f}')
    return err, ratio


# ---- prepare ---------------------------------------------------------------------------------------------------------------------------
def prepare_raw(buf, stride, r, n):
    src = Buf(buf, offset=4)
    p, l = Buf(n_bytes=4 * r * n, offset=8), Buf(n_bytes=4 * r * n, offset=12)
    assert np.isnan(p.get(np.float32, -1)).all()
    _run('prepare', [src], [p, l], (src.ptr, stride, r, n, p.ptr, l.ptr))
    return p.get(np.float32, (r, n)), l.get(np.float32, (r, n))


@pytest.mark.parametrize('case', DD.PREPARE_CASES, ids=DD.case_id)
def test_prepare_is_within_the_bound(case):
    r, n, kind = case
    buf, stride = DD.prepare_inputs(case)
    p, l = prepare_raw(buf, stride, r, n)
    again = prepare_raw(buf, stride, r, n)
    assert np.array_equal(p.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(l.view(np.uint32), again[1].view(np.uint32)), 'a second run'
    want_p, want_l = DD.prepare64(buf[:, :n])
    bound_p, bound_l = DD.prepare_bounds(buf[:, :n])
    err_p, ratio_p = _worst(f'prepare P {DD.case_id(case)}', p, want_p, bound_p)
    err_l, ratio_l = _worst(f'prepare L {DD.case_id(case)}', l, want_l, bound_l)
    assert np.isfinite(p).all() and np.isfinite(l).all() and (err_p <= bound_p).all() and (err_l <= bound_l).all(), (ratio_p, ratio_l)
    if kind == 'zero_row':
        assert (p[r // 2] == 0).all() and (l[r // 2] == np.float32(DD.LN_EPS)).all()
    if kind == 'one_cell':
        assert np.array_equal(p, (buf[:, :n] != 0).astype(np.float32)) and set(np.unique(l)) <= {np.float32(0), np.float32(DD.LN_EPS)}


# ---- pair_kl ---------------------------------------------------------------------------------------------------------------------------
def pair_kl_raw(pa, la, pb, lb, same):
    a, b, n = pa.shape[0], pb.shape[0], pa.shape[1]
    ins = [Buf(pa), Buf(la)]
    ins += ins if same else [Buf(pb), Buf(lb, offset=0 if n % 8 else 4)]       # an operand off 16 bytes takes the scalar loads
    d = Buf(n_bytes=4 * a * b, offset=4)
    _run('pair_kl', ins[:2] if same else ins, [d], (ins[0].ptr, ins[1].ptr, a, ins[2].ptr, ins[3].ptr, b, n, d.ptr))
    return d.get(np.float32, (a, b))


@pytest.mark.parametrize('case', DD.PAIR_CASES, ids=DD.case_id)
def test_pair_kl_is_within_the_bound(case):
    a, b, n, regime = case
    pa, la, pb, lb = DD.pair_inputs(case)
    got = pair_kl_raw(pa, la, pb, lb, regime == 'self')
    assert np.array_equal(got.view(np.uint32), pair_kl_raw(pa, la, pb, lb, regime == 'self').view(np.uint32)), 'a second run'
    want, bound = DD.pair_kl64(pa, la, pb, lb), DD.pair_kl_bound(pa, la, pb, lb)
    err, ratio = _worst(f'pair_kl {DD.case_id(case)} (largest D {want.max():.3e})', got, want, bound)
    assert got.shape == (a, b) and np.isfinite(got).all() and (got >= 0).all() and (err <= bound).all(), f'{ratio:.3f} of the bound'
    if regime == 'self':
        assert (np.diag(got) == 0).all() and np.array_equal(got.view(np.uint32), got.T.copy().view(np.uint32)), 'exactly 0 on the diagonal, bitwise symmetric'
    if regime == 'near':
        assert want.max() < 1e-5 and (err <= 1e-3 * want + 2.0 ** -125).all(), 'D ~ 1e-6 is resolved to a part in a thousand'


# ---- merge -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', DD.MERGE_CASES, ids=DD.case_id)
def test_merge_is_within_the_bound(case):
    k, r, n = case
    p, member = DD.merge_inputs(case)
    runs = []
    for _ in range(2):
        ins = [Buf(p, offset=4), Buf(member, offset=1)]
        out, cnt = Buf(n_bytes=4 * k * n, offset=8), Buf(n_bytes=4 * k, offset=4)
        _run('merge', ins, [out, cnt], (ins[0].ptr, r, n, ins[1].ptr, k, out.ptr, cnt.ptr))
        runs.append((out.get(np.float32, (k, n)), cnt.get(np.int32, (k,))))
    (got, got_cnt), again = runs
    assert np.array_equal(got.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(got_cnt, again[1]), 'a second run'
    want, want_cnt = DD.merge64(p, member)
    err, ratio = _worst(f'merge {DD.case_id(case)}', got, want, DD.merge_bound(p, member))
    assert np.array_equal(got_cnt, want_cnt) and (err <= DD.merge_bound(p, member)).all(), f'{ratio:.3f} of the bound'
    assert (got[want_cnt == 0] == 0).all()
    if k > 2:
        assert np.array_equal(got[2], p[r // 2]), 'a single member is copied'


# ---- labels ----------------------------------------------------------------------------------------------------------------------------
def labels_raw(props, out_h, out_w, values=True):
    k, h, w = props.shape
    src = Buf(props, offset=4)
    lab, val = Buf(n_bytes=out_h * out_w, offset=3), Buf(n_bytes=4 * out_h * out_w, offset=4)
    _run('labels', [src], [lab, val], (src.ptr, k, h, w, out_h, out_w, lab.ptr, val.ptr if values else None))
    if not values:
        assert val.unchanged()
    return lab.get(np.uint8, (out_h, out_w)), val.get(np.float32, (out_h, out_w))


@pytest.mark.parametrize('case', DD.LABEL_CASES, ids=DD.case_id)
def test_labels_match_float64_where_the_margin_is_clear(case):
    k, (h, w), (out_h, out_w), kind = case
    props = DD.label_inputs(case)
    got, val = labels_raw(props, out_h, out_w)
    again = labels_raw(props, out_h, out_w, values=False)[0]
    assert np.array_equal(got, again), 'a second run, without the values'
    want, want_val, decided = DD.labels64(props, out_h, out_w)
    left_out = int((~decided).sum())
    print(f'\nlabels {DD.case_id(case)}: {left_out} of {out_h * out_w} pixels left out, {int((got != want)[decided].sum())} decided pixels differ, '
          f'worst value error / bound {float(np.abs(val - want_val).max() / max(DD.labels_bound(props), 2.0 ** -149)):.3f}')
    assert left_out <= 0.01 * out_h * out_w
    assert np.array_equal(got[decided], want[decided]) and (got < k).all()
    assert (np.abs(val - want_val) <= DD.labels_bound(props)).all()
    if (out_h, out_w) == (h, w):
        assert np.array_equal(got, props.argmax(axis=0)) and np.array_equal(val, props.max(axis=0)), 'a plain argmax'
    # among the candidates within the bound: the device names one of them
    v = DD.resize64(props, out_h, out_w)
    picked = np.take_along_axis(v, got[None].astype(np.int64), axis=0)[0]
    assert (v.max(axis=0) - picked <= 2 * DD.labels_bound(props)).all()


def test_a_tie_goes_to_the_lowest_index():
    props = DD.label_inputs((7, (5, 7), (5, 7), 'plateaus'))
    for size in ((5, 7), (10, 14), (37, 53)):
        single = labels_raw(props, *size)[0]
        double = labels_raw(np.concatenate([props, props]), *size)[0]              # every proposal twice: the same bits, exact ties
        assert (double < 7).all() and np.array_equal(double, single)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('segments,grid', DD.PLANTED, ids=[f'S{s}-{g[0]}x{g[1]}' for s, g in DD.PLANTED])
def test_discover_recovers_the_planted_partition(segments, grid):
    import daam_amd
    sums, truth = DD.planted(segments, grid)
    aff = daam_amd.SelfAffinity(torch.from_numpy(sums).to(DEV), grid, 1, 1)
    found = aff.discover(anchors=grid, threshold=DD.THRESHOLD, iterations=3)
    labels = found.labels.cpu().numpy()
    assert found.n == segments and labels.shape == grid and DD.same_partition(labels, truth)
    assert np.array_equal(labels, DD.discover64(sums, grid, anchors=grid, threshold=DD.THRESHOLD, iterations=3)[0])
    assert found.areas.tolist() == np.bincount(truth.reshape(-1)).tolist() and bool((found.masks.sum(0) == 1).all())
    big = aff.discover(anchors=grid, threshold=DD.THRESHOLD, iterations=3, size=(37, 53))
    assert big.labels.shape == (37, 53) and big.n == segments and big.labels.device.type == 'cuda'


def test_names_and_word_masks_on_planted_segments():
    import daam_amd
    from daam_amd.utils import compute_token_merge_indices
    grid = (16, 16)
    sums, truth = DD.planted(3, grid)
    found = daam_amd.SelfAffinity(torch.from_numpy(sums).to(DEV), grid, 1, 1).discover(anchors=grid, threshold=DD.THRESHOLD)
    tok, words = fd.FakeTokenizer(), ['monkey', 'bicycle', 'photo']
    maps = np.zeros((13, *grid), np.float32)
    for seg, word in enumerate(words[:2]):                    # 'photo' owns nothing; segment 2 has no word
        for i in compute_token_merge_indices(tok, PROMPT, word, None)[0]:
            maps[i] = truth == seg
    ghm = daam_amd.GlobalHeatMap(tok, PROMPT, torch.from_numpy(maps).to(DEV))
    labels = found.labels.cpu().numpy()
    seg_of = [int(labels[truth == s][0]) for s in range(3)]
    names = found.names(ghm, words)
    assert [names[s] for s in seg_of] == ['monkey', 'bicycle', None]
    wm = found.word_masks(ghm, words)
    assert wm.dtype == torch.uint8 and tuple(wm.shape) == (3, *grid) and wm.device.type == 'cuda'
    wm = wm.cpu().numpy()
    assert np.array_equal(wm[0], truth == 0) and np.array_equal(wm[1], truth == 1) and not wm[2].any()
    overlaps = daam_amd.mask_overlap_matrix(found.word_masks(ghm, words), torch.from_numpy((truth[None] == np.arange(3)[:, None, None]).astype(np.uint8)).to(DEV))
    assert overlaps is not None


def _composes(aff, size):
    found = aff.discover(anchors=4, size=size)
    assert tuple(found.labels.shape) == size and found.labels.dtype == torch.uint8 and found.n >= 1
    assert bool((found.masks.sum(0) == 1).all()) and int(found.areas.sum()) == size[0] * size[1]
    assert tuple(found.proposals.shape) == (found.n, *aff.grid)


def test_it_composes_with_trace():
    import daam_amd
    from test_self_affinity_cpu import add_attn1
    pipe = fd.make_pipe('sd15', device=DEV, dtype=torch.float16, batch=2, seed=3, mini=True, identity_proj=True, dim_head=40, latent_size=8)
    add_attn1(pipe)
    with daam_amd.trace(pipe, height=64, width=64, self_affinity=True) as tc:
        pipe(PROMPT, num_inference_steps=2)
        aff = tc.compute_self_affinity()
    _composes(aff, (48, 40))


def test_it_composes_with_trace_joint():
    import daam_amd
    import _mmdit_standin as M
    pipe = M.make_pipe(device=DEV, dtype=torch.float16, seed=3)
    with daam_amd.trace_joint(pipe, self_affinity=True) as tc:
        pipe(PROMPT, num_inference_steps=2)
        aff = tc.compute_self_affinity()
    _composes(aff, (48, 40))
