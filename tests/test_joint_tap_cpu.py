"""The joint-attention tap (include/daam_joint_tap.h) without a GPU: ``libdaam_joint.so`` builds by the side libraries'
recipe beside their tables, exports what its header declares and the binding names; the header is C99; no kernel has scratch; every
argument the header rules out is refused before any HIP call; the float64 reference has the properties the contract states, the f32
emulation is inside the bound on every case of the device test and the mutants are outside it; and the Python layer
(``trace_joint``, ``engine.JointTapState``) on a numpy stand-in of the library.  The kernels run in ``test_gpu_joint_tap.py``."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import _joint_domain as J
import _libcheck as LC
import _mmdit_standin as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
N_KERNELS = 8                       # statistics and text columns for 2 dtypes x 2 head dims
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build_joint(verbose=False)
    return build.JOINT_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_joint()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_joint.so' and not build.joint_stale()
    assert build.JOINT_SOURCES == ['daam_joint_tap.hip'] and build.JOINT.name == 'joint'
    exported = LC.exported(built)
    assert exported == LC.declared('daam_joint_tap.h') == sorted(nat.JOINT_EXPORTS) and len(exported) == 4
    assert lib.daam_joint_tap_abi_version() == 1 == nat.JOINT_ABI_VERSION and nat.JOINT_LIBRARY.env == 'DAAM_JOINT_LIB'
    assert len(lib.daam_joint_tap_accumulate.argtypes) == 27
    names = list(build.kernel_shas(built))
    assert len(names) == N_KERNELS and sum('joint_stats_kernel' in n for n in names) == 4 and sum('joint_text_kernel' in n for n in names) == 4


def test_the_tables_of_the_other_libraries_are_as_they_were():
    from daam_amd import _native as nat, build
    assert [lib.name for lib in build.SIDE_LIBRARIES] == ['analysis', 'eval', 'locate', 'components', 'refine', 'selfaff']
    assert build.JOINT not in build.SIDE_LIBRARIES and nat.JOINT_LIBRARY not in nat.LIBRARIES and len(nat.LIBRARIES) == 7
    assert 'daam_joint_tap.hip' not in build.SOURCES and not any('joint' in h for h in build.HEADERS)
    others = [lib.file for lib in nat.LIBRARIES] + [os.path.basename(lib.out) for lib in build.SIDE_LIBRARIES]
    stems = {f[len('libdaam_'):-len('.so')] for f in others}
    for name in ('daam_joint_tap.hip', 'daam_joint_tap.h', 'libdaam_joint.so'):
        assert not any(stem in os.path.splitext(name)[0] for stem in stems), name


def test_build_joint_is_the_side_recipe(monkeypatch):
    from daam_amd import build
    ran = []
    monkeypatch.setattr(build.subprocess, 'run', lambda cmd, check: ran.append(cmd))
    assert build.build_joint(force=True, verbose=False) == build.JOINT_LIB
    src = os.path.join(build.HERE, 'csrc', 'daam_joint_tap.hip')
    assert ran == [[build.hipcc(), *build.HIPCC_FLAGS, src, '-o', build.JOINT_LIB]]
    ran.clear()
    build.build(force=True, verbose=False)
    assert not any('joint' in ' '.join(cmd) for cmd in ran), 'build() makes the libraries of its tables alone'


def test_joint_tap_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_joint_tap.h"\nint main(void) { return DAAM_JOINT_TAP_ABI_VERSION == 1 && '
                   'sizeof(&daam_joint_tap_accumulate) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)


def test_no_kernel_has_scratch(built):
    from daam_amd import build
    names = list(build.kernel_shas(built))
    LC.assert_no_scratch(built, names)
    kds = LC.kernel_descriptors(built)
    for k in names:
        group, = struct.unpack_from('<I', kds[k], 0)
        assert 0 < group <= 64 * 1024, (k, group)


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
def _accumulate(lib, **over):
    """A call that is in range but for ``over``; pointers are small fake addresses (nothing is dereferenced)."""
    row = 8 * 64
    a = dict(q=0x100000, kt=0x200000, ki=0x300000, dtype=0, batch=2, heads=8, P=96, T=77, Pk=96, d=64, qs=(96 * row, 64, row),
             ts=(77 * row, 64, row), its=(96 * row, 64, row), scale=0.125, weight=1.0, accumulate=0, sums=0x1000000, stride_h=0, ws=0x2000000,
             ws_bytes=None, stream=None)
    a.update(over)
    if a['ws_bytes'] is None:
        a['ws_bytes'] = lib.daam_joint_tap_workspace(a['batch'], a['heads'], a['P']) or 1 << 20
    rc = lib.daam_joint_tap_accumulate(a['q'], a['kt'], a['ki'], a['dtype'], a['batch'], a['heads'], a['P'], a['T'], a['Pk'], a['d'], *a['qs'],
                                       *a['ts'], *a['its'], a['scale'], a['weight'], a['accumulate'], a['sums'], a['stride_h'], a['ws'],
                                       a['ws_bytes'], a['stream'])
    return rc, lib.daam_joint_tap_last_error().decode()


ROW = 8 * 64
BAD = {
    'f32 inputs': dict(dtype=1), 'dtype 3': dict(dtype=3), 'batch 0': dict(batch=0), 'heads 0': dict(heads=0), '4097 slices': dict(batch=4097, heads=1),
    'P 0': dict(P=0), 'P 16385': dict(P=16385), 'T 0': dict(T=0), 'T 513': dict(T=513), 'Pk -1': dict(Pk=-1), 'Pk 16385': dict(Pk=16385),
    'd 40': dict(d=40), 'd 80': dict(d=80), 'd 160': dict(d=160), 'd 0': dict(d=0), 'd 256': dict(d=256), 'scale 0': dict(scale=0.0),
    'scale -1': dict(scale=-1.0), 'scale inf': dict(scale=math.inf), 'scale nan': dict(scale=math.nan), 'weight inf': dict(weight=math.inf),
    'weight nan': dict(weight=math.nan), 'NULL q': dict(q=None), 'NULL k_txt': dict(kt=None), 'NULL k_img with Pk > 0': dict(ki=None),
    'NULL sums': dict(sums=None), 'NULL workspace': dict(ws=None), 'q off 16 bytes': dict(q=0x100008), 'k_txt off 16 bytes': dict(kt=0x200002),
    'k_img off 16 bytes': dict(ki=0x300004), 'sums off 4 bytes': dict(sums=0x1000002), 'workspace off 8 bytes': dict(ws=0x2000004),
    'row stride not 8': dict(qs=(96 * ROW, 64, ROW + 4)), 'head stride not 8': dict(ts=(77 * ROW, 60, ROW)),
    'batch stride not 8': dict(its=(96 * ROW + 4, 64, ROW)), 'negative stride': dict(ts=(-8, 64, ROW)), 'q row stride below d': dict(qs=(96 * 32, 64, 32)),
    'k_txt row stride below d': dict(ts=(77 * 32, 64, 32)), 'k_img row stride below d': dict(its=(96 * 32, 64, 32)),
    'plane stride below T P': dict(stride_h=77 * 96 - 1), 'negative plane stride': dict(stride_h=-77 * 96),
    'short workspace': dict(ws_bytes=8 * 16 * 128 - 8), 'sums in the workspace': dict(sums=0x2000000 + 64),
    'a later plane in the workspace': dict(sums=0x2000000 - 4 * 7 * 77 * 96 - 64, stride_h=77 * 96),
}
# The inside of every limit.  A call that passes the checks would launch, so each of these carries ONE fault that a later range check
# catches (a workspace eight bytes short): a message about the workspace shows that the limit under test let the call through.
INSIDE = {
    'P 1': dict(P=1), 'P 16384': dict(P=16384), 'T 1': dict(T=1), 'T 512': dict(T=512), 'Pk 0': dict(Pk=0), 'Pk 0 with NULL k_img': dict(Pk=0, ki=None),
    'Pk 0 with wild k_img strides': dict(Pk=0, ki=0x300004, its=(0, 0, 0)), 'Pk 16384': dict(Pk=16384), '4096 slices': dict(batch=64, heads=64),
    'one slice': dict(batch=1, heads=1), 'bf16': dict(dtype=2), 'd 128': dict(d=128, qs=(96 * 1024, 128, 1024), ts=(77 * 1024, 128, 1024), its=(96 * 1024, 128, 1024)),
    'packed layout': dict(qs=(8 * 96 * 64, 96 * 64, 64), ts=(8 * 77 * 64, 77 * 64, 64), its=(8 * 96 * 64, 96 * 64, 64)),
    'zero batch stride': dict(ts=(0, 64, ROW)), 'tiny scale': dict(scale=1e-30), 'huge scale': dict(scale=1e30), 'weight 0': dict(weight=0.0),
    'negative weight': dict(weight=-3.5), 'accumulate 1': dict(accumulate=1), 'a plane per head': dict(stride_h=77 * 96),
    'planes apart': dict(stride_h=77 * 96 + 5),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _accumulate(lib, **BAD[what])
    assert rc == E_INVALID and msg.startswith('joint_tap_accumulate: '), (what, rc, msg)


@pytest.mark.parametrize('what', sorted(INSIDE))
def test_inside_every_limit_reaches_the_workspace_check(lib, what):
    over = dict(INSIDE[what])
    shape = dict(batch=2, heads=8, P=96)
    shape.update({k: v for k, v in over.items() if k in shape})
    need = lib.daam_joint_tap_workspace(shape['batch'], shape['heads'], shape['P'])
    assert need > 0
    rc, msg = _accumulate(lib, **dict(over, ws_bytes=need - 8))
    assert rc == E_INVALID and msg.startswith('joint_tap_accumulate: workspace of'), (what, rc, msg)


def test_workspace_sizes_agree_with_the_stand_in(lib):
    fake = J.FakeJointLib()
    for args in [(1, 1, 1), (2, 3, 128), (2, 3, 129), (64, 64, 16384), (1, 24, 4096), (0, 1, 5), (1, 0, 5), (65, 64, 5), (1, 1, 0), (1, 1, 16385)]:
        got = lib.daam_joint_tap_workspace(*args)
        assert got == fake.daam_joint_tap_workspace(*args) and got % 8 == 0, args


# ---- reference, emulation, bound -------------------------------------------------------------------------------------------------------
def test_the_reference_is_the_text_block_of_one_softmax():
    q, kt, ki, scale = J.inputs('small', 2, 3, 65, 77, 65, 64, 'f16', seed=1)
    one, heads = J.reference_sums([(q, kt, ki, scale, 1.0)]), J.reference_sums([(q, kt, ki, scale, 1.0)], per_head=True)
    assert one.shape == (77, 65) and heads.shape == (3, 77, 65) and np.allclose(heads.sum(axis=0), one, rtol=1e-13, atol=0)
    share = J.image_share(q, kt, ki, scale)
    assert 0.2 < share < 0.8 and np.all(one.sum(axis=0) <= 6 * (1 - share) + 1e-12)      # a cell's text mass is what the image keys leave
    # the order of the keys is immaterial; Pk = 0 is the UNet's softmax; a zero Q gives 1 / (T + Pk) per slice
    perm = np.random.default_rng(0).permutation(65)
    assert np.allclose(J.reference_sums([(q, kt, ki[:, :, perm], scale, 1.0)]), one, rtol=1e-12, atol=0)
    assert np.allclose(J.reference_sums([(q, kt, ki[:, :, :0], scale, 1.0)]), J.reference_text_only(q, kt, scale), rtol=1e-14, atol=0)
    assert np.allclose(J.reference_sums([(0 * q, kt, ki, scale, 1.0)]), 6 / (77 + 65), rtol=1e-14, atol=0)
    # chained calls: fma(weight, acc, previous)
    two = J.reference_sums([(q, kt, ki, scale, 0.5), (q, kt, ki, scale, -0.25)])
    assert np.allclose(two, 0.25 * one, rtol=1e-13, atol=0)


@pytest.mark.parametrize('case', J.CASES, ids=[J.case_id(c) for c in J.CASES])
def test_the_emulation_is_inside_the_bound(case):
    q, kt, ki, scale = J.case_inputs(case)
    calls = [(q, kt, ki, scale, 1.0)]
    got, want, bound = J.emulate_sums(calls, case[7]), J.reference_sums(calls, case[7]), J.sums_bound(calls, case[7])
    err = np.abs(got.astype(np.float64) - want)
    assert got.shape == want.shape == bound.shape and np.isfinite(got).all() and (err <= bound).all(), float((err / bound).max())
    assert bound.max() <= 1e-2 * max(1.0, want.max()), 'the bound says something'


def test_the_case_table_meets_what_it_promises():
    assert 72 <= len(J.CASES) <= 90
    for col, values in ((0, J.PS), (1, J.TS), (5, J.SLICES), (6, J.LAYOUTS), (7, (False, True)), (8, J.REGIMES)):
        for v in values:
            assert {(c[3], c[4]) for c in J.CASES if c[col] == v} == {(d, t) for d in J.HEAD_DIMS for t in ('f16', 'bf16')}, (col, v)
    assert sum(c[2] == 0 for c in J.CASES) == 2 and sum(c[2] == 200 and c[0] == 65 for c in J.CASES) == 2


def _applies(mutant, case):
    P, T, Pk, d, dtype, (batch, heads), layout, per_head, regime = case
    if mutant == 'no_image_keys':
        return Pk >= 5
    if mutant == 'no_scale':
        return regime != 'zero_q'
    if mutant == 'padded_keys':
        return (T + Pk) % 32 != 0 and (T % 32 != 0 or Pk % 32 != 0)
    if mutant == 'neighbour_stats':
        return P > 1 and regime != 'zero_q'
    if mutant == 'packed_head_stride':
        return layout == 'interleaved' and heads > 1 and P > 1 and regime != 'zero_q'
    return per_head and heads > 1                   # all_to_plane0


@pytest.mark.parametrize('mutant', J.MUTANTS)
def test_mutants_fall_outside_the_bound(mutant):
    """Every mutant leaves the bound on at least one listed case -- here: on EVERY listed case it can show on in the regime 'small'
    (where no probability is tiny), by a wide margin."""
    cases = [c for c in J.CASES if _applies(mutant, c) and c[8] == 'small']
    assert cases, mutant
    for case in cases:
        q, kt, ki, scale = J.case_inputs(case)
        calls = [(q, kt, ki, scale, 1.0)]
        got, want, bound = J.emulate_sums(calls, case[7], mutant=mutant), J.reference_sums(calls, case[7]), J.sums_bound(calls, case[7])
        worst = float((np.abs(got.astype(np.float64) - want) / bound).max())
        assert worst > 50, (mutant, J.case_id(case), worst)


def test_the_decisive_mutant_where_the_image_keys_hold_a_clear_share():
    """Image keys left out of the denominator (the UNet softmax): in these cases the image keys hold between a tenth and nearly all of
    every row's mass, and the mutant's planes are wrong by that factor -- thousands of bounds."""
    seen = 0
    for case in J.CASES:
        if case[2] < 63 or case[8] not in ('small', 'outlier'):
            continue
        q, kt, ki, scale = J.case_inputs(case)
        share = J.image_share(q, kt, ki, scale)
        assert share > 0.1, (J.case_id(case), share)
        calls = [(q, kt, ki, scale, 1.0)]
        got, want, bound = J.emulate_sums(calls, case[7], mutant='no_image_keys'), J.reference_sums(calls, case[7]), J.sums_bound(calls, case[7])
        assert float((np.abs(got - want) / bound).max()) > 1000, J.case_id(case)
        seen += 1
    assert seen >= 12


def test_two_calls_chain_inside_the_bound_and_the_prior_is_carried():
    q1, kt1, ki1, scale = J.inputs('small', 1, 3, 65, 77, 65, 64, 'f16', seed=1)
    q2, kt2, ki2, _ = J.inputs('outlier', 1, 3, 65, 77, 65, 64, 'f16', seed=2)
    for per_head in (False, True):
        for w1, w2 in ((1.0, 1.0), (0.5, -0.25)):
            calls = [(q1, kt1, ki1, scale, w1), (q2, kt2, ki2, scale, w2)]
            got, want, bound = J.emulate_sums(calls, per_head), J.reference_sums(calls, per_head), J.sums_bound(calls, per_head)
            assert (np.abs(got - want) <= bound).all()
            first = J.sums_bound(calls[:1], per_head)
            assert (bound > first).all()


# ---- the Python layer on a numpy stand-in of the library -------------------------------------------------------------------------------
@pytest.fixture
def fakes(monkeypatch):
    E, lib = J.install(monkeypatch.setattr)
    return E, lib


def _reference_of(calls, per_head=False):
    return J.reference_sums([(q, kt, ki, scale, 1.0) for q, kt, ki, scale in calls], per_head)


@pytest.mark.parametrize('batch,per_head', [(2, False), (2, True), (1, False)])
def test_trace_joint_taps_the_kept_half_and_leaves_the_model_alone(fakes, batch, per_head):
    import daam_amd
    E, lib = fakes
    steps = 2
    pipe = M.make_pipe(seed=3, batch=batch)
    recorded = M.record(pipe)
    pipe(PROMPT, num_inference_steps=steps)
    plain = [o.clone() for o in pipe.outputs]
    processors = [b.attn.processor for b in pipe.transformer.transformer_blocks]
    M.record(pipe, on=False)
    with daam_amd.trace_joint(pipe, per_head=per_head) as tc:
        assert tc.state is None and not lib.calls, 'nothing is allocated before a call is tapped'
        pipe(PROMPT, num_inference_steps=steps)
        assert all(torch.equal(a, b) for a, b in zip(plain, pipe.outputs)), 'the traced generation is bit-identical'
        raw, ghm = tc.raw_heat_maps(), tc.compute_global_heat_map()
        state = tc.state
        if per_head:
            head_maps = tc.compute_head_heat_maps()
    assert [b.attn.processor for b in pipe.transformer.transformer_blocks] == processors, 'unhooked'
    kept = batch - batch // 2
    T = M.CLIP_ROWS + M.T5_ROWS
    assert len(recorded) == 3 * steps == len(lib.calls) == state.calls and state.slices == 3 * steps * kept * 2
    assert all(c[1:7] == (kept, 2, 64, T, 64, 64) for c in lib.calls) and [c[10] for c in lib.calls] == [0] + [1] * (3 * steps - 1)
    assert all(c[11] == (T * 64 if per_head else 0) for c in lib.calls)
    assert all(r[0].shape[0] == kept for r in recorded), 'the stand-in records the conditional half'
    want = _reference_of(recorded)
    bound = J.sums_bound([(q, kt, ki, scale, 1.0) for q, kt, ki, scale in recorded])
    assert raw.shape == (T, 8, 8) and raw.dtype == torch.float32
    assert (np.abs(raw.numpy().reshape(T, 64) - want) <= bound).all(), 'the kept half, through the strides of the projections'
    assert ghm.heat_maps.shape == (77, 8, 8) and ghm.prompt == PROMPT and ghm.tokenizer is pipe.tokenizer
    assert torch.allclose(ghm.heat_maps, raw[:77] / state.slices, rtol=1e-6, atol=0)
    if per_head:
        assert head_maps.shape == (2, T, 8, 8) and state.sums.shape == (2, T, 64)
        assert torch.allclose(head_maps.sum(0) * (state.slices // 2), raw, rtol=1e-5, atol=0)
    else:
        with pytest.raises(ValueError, match='per_head'):
            tc.compute_head_heat_maps()


def test_a_second_generation_starts_over_other_sizes_and_masked_calls(fakes):
    import daam_amd
    E, lib = fakes
    pipe = M.make_pipe(seed=4)
    with daam_amd.trace_joint(pipe, height=96, width=160) as tc:
        assert tc.grid == (6, 10)
        with pytest.raises(RuntimeError, match='No heat maps'):
            tc.compute_global_heat_map()
        pipe(PROMPT, num_inference_steps=1)                                  # the default 8 x 8 generation: 64 cells, not 60
        assert not lib.calls, 'a call of another query length is not tapped'
        pipe(PROMPT, num_inference_steps=1, height=96, width=160)
        assert len(lib.calls) == 3 and lib.calls[0][3] == 60 and lib.calls[0][10] == 0
        first = tc.raw_heat_maps().clone()
        assert first.shape == (96, 6, 10)
        pipe('another prompt', num_inference_steps=1, height=96, width=160)
        assert len(lib.calls) == 6 and lib.calls[3][10] == 0 and tc.state.calls == 3, 'a new generation overwrites'
        assert torch.equal(tc.raw_heat_maps(), first) and tc.last_prompt == 'another prompt'
        pipe.mask_fn = lambda n: torch.zeros(n, n, dtype=pipe.dtype)
        pipe(PROMPT, num_inference_steps=1, height=96, width=160)
        assert len(lib.calls) == 6, 'a masked call is not tapped'
        with pytest.raises(ValueError, match='single prompt'):
            pipe([PROMPT, PROMPT], num_inference_steps=1)


def test_norms_are_skipped_where_none_and_self_attention_calls_are_not_tapped(fakes):
    import daam_amd
    E, lib = fakes
    pipe = M.make_pipe(seed=5, blocks=2)
    blocks = pipe.transformer.transformer_blocks
    assert blocks[0].attn.norm_q is not None and blocks[1].attn.norm_q is None and blocks[1].attn.norm_added_k is None
    hidden = pipe._randn(2, 64, 128, key=1)
    with daam_amd.trace_joint(pipe) as tc:
        with torch.no_grad():
            out = blocks[0].attn(hidden)                                      # no encoder_hidden_states
        assert not lib.calls and torch.is_tensor(out)
    for kw in (dict(height=100), dict(width=72)):
        with pytest.raises(ValueError, match='16-pixel cells'):
            daam_amd.trace_joint(pipe, **kw)


def test_trace_joint_refuses_what_it_cannot_trace(fakes):
    import daam_amd
    from oracle import fake_diffusers as fd
    with pytest.raises(ValueError, match='transformer'):
        daam_amd.trace_joint(fd.make_pipe('sd15', mini=True))
    with pytest.raises(ValueError, match='fp16 or bf16'):
        daam_amd.trace_joint(M.make_pipe(dtype=torch.float32))
    with pytest.raises(ValueError, match='head dim 32'):
        daam_amd.trace_joint(M.make_pipe(dim_head=32))
    daam_amd.trace_joint(M.make_pipe(dim_head=128, heads=1, blocks=1))
    assert 'trace_joint' in daam_amd.__all__ if hasattr(daam_amd, '__all__') else hasattr(daam_amd, 'trace_joint')


def test_joint_tap_state_holds_the_header_limits(fakes):
    E, lib = fakes
    for bad in (dict(h=0, w=4, tokens=77), dict(h=129, w=128, tokens=77), dict(h=8, w=8, tokens=0), dict(h=8, w=8, tokens=513)):
        with pytest.raises(ValueError):
            E.JointTapState(**bad)
    state = E.JointTapState(2, 3, 5)
    x = lambda rows, ch=128, dt=torch.bfloat16: torch.zeros(1, rows, ch, dtype=dt)
    with pytest.raises(ValueError, match='joint tap'):
        state.tap(x(7), x(5), x(6), 2, 0.125)                                # 7 queries on 6 cells
    with pytest.raises(ValueError, match='joint tap'):
        state.tap(x(6), x(4), x(6), 2, 0.125)                                # 4 tokens, not 5
    with pytest.raises(ValueError, match='head dim'):
        state.tap(x(6), x(5), x(6), 4, 0.125)
    with pytest.raises(RuntimeError, match='fp16 or bf16'):
        state.tap(x(6, dt=torch.float32), x(5, dt=torch.float32), x(6, dt=torch.float32), 2, 0.125)
    assert state.sums is None and not lib.calls
    state.tap(x(6), x(5), x(0), 2, 0.125)                                    # no image keys: the text-only softmax
    assert lib.calls[0][3:6] == (6, 5, 0) and torch.allclose(state.sums, torch.full((5, 6), 2 / 5))
