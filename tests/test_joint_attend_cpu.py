"""The fused joint attention (include/daam_joint_attend.h) without a GPU: ``libdaam_jointattend.so`` builds by the side
libraries' recipe beside their tables, exports what its header declares and the binding names; the header is C99; no kernel has
scratch; the other libraries' kernels do not move; every argument the header rules out is refused before any HIP call; the f32
emulation is inside the bound and the mutants are outside it; and the Python layer (``trace_joint(attend=True)``,
``engine.JointAttendState``, ``JointTapState.tap_from_stats``) on stand-ins of the libraries.  The kernels run in
``test_gpu_joint_attend.py``."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import _joint_attend_domain as A
import _joint_domain as J
import _libcheck as LC
import _mmdit_standin as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
N_KERNELS = 8                       # the forward and the text kernel for 2 dtypes x 2 head dims
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'
WIDE = 8.0                          # a mutant that can show on a case is at least this many bounds away


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    others = {lib.name: build.kernel_shas(lib.out) for lib in (build.JOINT, build.JOINT_AFFINITY) if os.path.exists(lib.out)}
    build.build_joint_attend(verbose=False)
    return build.JOINT_ATTEND_LIB, others


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_joint_attend()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    path, others = built
    assert os.path.exists(path) and os.path.basename(path) == 'libdaam_jointattend.so' and not build.joint_attend_stale()
    assert build.JOINT_ATTEND_SOURCES == ['daam_joint_attend.hip'] and build.JOINT_ATTEND.name == 'jointattend'
    exported = LC.exported(path)
    assert exported == LC.declared('daam_joint_attend.h') == sorted(nat.JOINT_ATTEND_EXPORTS)
    assert exported == ['daam_joint_attend_abi_version', 'daam_joint_attend_forward', 'daam_joint_attend_last_error',
                        'daam_joint_attend_stats_bytes', 'daam_joint_attend_text']
    assert lib.daam_joint_attend_abi_version() == 1 == nat.JOINT_ATTEND_ABI_VERSION
    assert nat.JOINT_ATTEND_LIBRARY.env == 'DAAM_JOINT_ATTEND_LIB' and len(lib.daam_joint_attend_text.argtypes) == 22
    assert nat.load_joint_attend.__name__ == 'load_joint_attend' and nat.check_joint_attend.__name__ == 'check_joint_attend'
    names = list(build.kernel_shas(path))
    assert len(names) == N_KERNELS and sum('joint_attend_kernel' in n for n in names) == 4
    assert sum('joint_attend_text_kernel' in n for n in names) == 4
    for other in (build.JOINT, build.JOINT_AFFINITY):
        if other.name in others:
            assert build.kernel_shas(other.out) == others[other.name], 'the build moved another library\'s kernels'


def test_the_record_stands_outside_the_tables(monkeypatch):
    from daam_amd import _native as nat, build
    assert build.JOINT_ATTEND not in build.SIDE_LIBRARIES and isinstance(build.JOINT_ATTEND, build.SideLibrary)
    assert nat.JOINT_ATTEND_LIBRARY not in nat.LIBRARIES and isinstance(nat.JOINT_ATTEND_LIBRARY, nat.Library)
    assert 'daam_joint_attend.hip' not in build.SOURCES and not any('joint' in h for h in build.HEADERS)
    assert build.joint_attend_stale.func is build.side_stale and build.build_joint_attend.func is build.build_side
    assert build.joint_attend_stale.args == build.build_joint_attend.args == (build.JOINT_ATTEND,)
    text = open(os.path.join(build.HERE, 'csrc', 'daam_joint_attend.hip')).read()
    assert [line for line in text.splitlines() if line.startswith('#include "')] == ['#include "../../include/daam_joint_attend.h"']
    tap = open(os.path.join(build.HERE, 'csrc', 'daam_rowsoftmax32.h')).read()
    term = 'return __fmaf_rn(__builtin_amdgcn_exp2f(__fmaf_rn(x, c, st.x)), st.y, acc);'
    assert term in tap and term in text, 'add_prob is the text kernel\'s expression term for term'
    ran = []
    monkeypatch.setattr(build.subprocess, 'run', lambda cmd, check: ran.append(cmd))
    assert build.build_joint_attend(force=True, verbose=False) == build.JOINT_ATTEND_LIB
    assert ran == [[build.hipcc(), *build.HIPCC_FLAGS, os.path.join(build.HERE, 'csrc', 'daam_joint_attend.hip'), '-o', build.JOINT_ATTEND_LIB]]
    ran.clear()
    build.build(force=True, verbose=False)
    assert not any('joint' in ' '.join(cmd) for cmd in ran), 'build() makes the libraries of its tables alone'


def test_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_joint_attend.h"\nint main(void) { return DAAM_JOINT_ATTEND_ABI_VERSION == 1 && '
                   'sizeof(&daam_joint_attend_forward) && sizeof(&daam_joint_attend_text) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)


def test_no_kernel_has_scratch(built):
    from daam_amd import build
    names = list(build.kernel_shas(built[0]))
    LC.assert_no_scratch(built[0], names)
    kds = LC.kernel_descriptors(built[0])
    for k in names:
        group, = struct.unpack_from('<I', kds[k], 0)
        assert 0 < group <= 64 * 1024, (k, group)


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
ROW = 8 * 64
IMG, TXT = (96 * ROW, 64, ROW), (80 * ROW, 64, ROW)
PTRS = dict(qi=0x1000000, ki=0x2000000, vi=0x3000000, qt=0x4000000, kt=0x5000000, vt=0x6000000, oi=0x7000000, ot=0x8000000)


def _forward(lib, **over):
    """A call that is in range but for ``over``; pointers are fake addresses 16 MB apart (nothing is dereferenced)."""
    a = dict(PTRS, dtype=0, batch=2, heads=8, P=96, T=80, d=64, qi_st=IMG, ki_st=IMG, vi_st=IMG, qt_st=TXT, kt_st=TXT, vt_st=TXT, oi_st=IMG,
             ot_st=TXT, scale=0.125, stats=0x9000000, stats_bytes=None, arrays=True)
    a.update(over)
    if a['stats_bytes'] is None:
        a['stats_bytes'] = lib.daam_joint_attend_stats_bytes(a['batch'], a['heads'], a['P']) or 1 << 20
    arr = lambda *names: (ctypes.c_int64 * (3 * len(names)))(*[v for n in names for v in a[n + '_st']]) if a['arrays'] else None
    rc = lib.daam_joint_attend_forward(a['qi'], a['ki'], a['vi'], a['qt'], a['kt'], a['vt'], a['oi'], a['ot'], a['dtype'], a['batch'], a['heads'],
                                       a['P'], a['T'], a['d'], arr('qi', 'ki', 'vi'), arr('qt', 'kt', 'vt'), arr('oi', 'ot'), a['scale'],
                                       a['stats'], a['stats_bytes'], None)
    return rc, lib.daam_joint_attend_last_error().decode()


def _text(lib, **over):
    a = dict(q=0x1000000, kt=0x5000000, stats=0x9000000, stats_bytes=None, dtype=0, batch=2, heads=8, P=96, T=80, d=64, qs=IMG, ks=TXT,
             scale=0.125, weight=1.0, accumulate=0, sums=0xA000000, stride=0)
    a.update(over)
    if a['stats_bytes'] is None:
        a['stats_bytes'] = lib.daam_joint_attend_stats_bytes(a['batch'], a['heads'], a['P']) or 1 << 20
    rc = lib.daam_joint_attend_text(a['q'], a['kt'], a['stats'], a['stats_bytes'], a['dtype'], a['batch'], a['heads'], a['P'], a['T'], a['d'],
                                    *a['qs'], *a['ks'], a['scale'], a['weight'], a['accumulate'], a['sums'], a['stride'], None)
    return rc, lib.daam_joint_attend_last_error().decode()


COMMON = {
    'f32 inputs': (dict(dtype=1), 'dtype'), 'batch 0': (dict(batch=0), 'slices'), 'heads 0': (dict(heads=0), 'slices'),
    '4097 slices': (dict(batch=4097, heads=1), 'slices'), 'P 0': (dict(P=0), 'P 0'), 'P 16385': (dict(P=16385), 'P 16385'),
    'T 0': (dict(T=0), 'T 0'), 'T 513': (dict(T=513), 'T 513'), 'd 40': (dict(d=40), 'head dim 40'), 'd 256': (dict(d=256), 'head dim 256'),
    'scale 0': (dict(scale=0.0), 'scale'), 'scale -1': (dict(scale=-1.0), 'scale'), 'scale inf': (dict(scale=math.inf), 'scale'),
    'scale nan': (dict(scale=math.nan), 'scale'), 'stats off 8 bytes': (dict(stats=0x9000004), '8-byte'),
    'short stats': (dict(stats_bytes=8 * 16 * 128 - 8), 'stats of'),
}
BAD_FORWARD = dict(COMMON, **{
    **{f'NULL {n}': ({n: None}, 'NULL') for n in PTRS}, 'NULL strides': (dict(arrays=False), 'NULL'),
    **{f'{n} off 16 bytes': ({n: PTRS[n] + 8}, '16-byte') for n in PTRS},
    'row stride not 8': (dict(vi_st=(96 * ROW, 64, ROW + 4)), 'stride'), 'head stride not 8': (dict(kt_st=(80 * ROW, 60, ROW)), 'stride'),
    'negative stride': (dict(qt_st=(-8, 64, ROW)), 'stride'), 'v row stride below d': (dict(vi_st=(96 * 32, 64, 32)), 'below the head dim'),
    'out row stride below d': (dict(ot_st=(80 * 32, 64, 32)), 'below the head dim'),
    'out heads share rows': (dict(oi_st=(96 * ROW, 0, ROW)), 'share elements'),
    'out row 1 of head 0 is row 0 of head 1': (dict(oi_st=(96 * ROW, 64, 64)), 'share elements'),
    'out rows of a head run into the next head': (dict(ot_st=(8 * 80 * 64, 79 * 64, 64)), 'share elements'),
    'out batch entries share rows': (dict(oi_st=(95 * ROW, 64, ROW)), 'batch entries would share'),
    'stats inside out_img': (dict(stats=PTRS['oi'] + 64), 'stats overlap out_img'),
    'out_txt inside stats': (dict(ot=0x9000000 + 8 * 16 * 128 - 16), 'stats overlap out_txt'),
    'stats over v_txt': (dict(stats=PTRS['vt'] + 8), 'stats overlap v_txt'),
    'out_img over q_img': (dict(oi=PTRS['qi'] + 16), 'out_img overlaps q_img'), 'outputs overlap': (dict(ot=PTRS['oi'] + 32), 'out_img overlaps out_txt'),
})
BAD_TEXT = dict(COMMON, **{
    'weight inf': (dict(weight=math.inf), 'weight'), 'weight nan': (dict(weight=math.nan), 'weight'), 'NULL q': (dict(q=None), 'NULL'),
    'NULL k_txt': (dict(kt=None), 'NULL'), 'NULL stats': (dict(stats=None), 'NULL'), 'NULL sums': (dict(sums=None), 'NULL'),
    'q off 16 bytes': (dict(q=0x1000008), '16-byte'), 'sums off 4 bytes': (dict(sums=0xA000002), '4-byte'),
    'row stride not 8': (dict(qs=(96 * ROW, 64, ROW + 4)), 'stride'), 'k row stride below d': (dict(ks=(80 * 32, 64, 32)), 'below the head dim'),
    'plane stride short': (dict(stride=96 * 80 - 1), 'sums_stride_h'), 'stats inside sums': (dict(stats=0xA000000 + 64), 'stats overlap sums'),
    'sums inside stats': (dict(sums=0x9000000 + 8 * 16 * 128 - 4), 'stats overlap sums'),
})


@pytest.mark.parametrize('what', sorted(BAD_FORWARD))
def test_forward_refuses_before_any_hip_call(lib, what):
    over, word = BAD_FORWARD[what]
    rc, msg = _forward(lib, **over)
    assert rc == E_INVALID and msg.startswith('joint_attend_forward: ') and word in msg, (what, rc, msg)


@pytest.mark.parametrize('what', sorted(BAD_TEXT))
def test_text_refuses_before_any_hip_call(lib, what):
    over, word = BAD_TEXT[what]
    rc, msg = _text(lib, **over)
    assert rc == E_INVALID and msg.startswith('joint_attend_text: ') and word in msg, (what, rc, msg)


def test_stats_bytes_are_the_layout_of_the_affinity(lib):
    fake = A.FakeJointAttendLib()
    for args in [(1, 1, 1), (2, 3, 128), (2, 3, 129), (64, 64, 16384), (1, 24, 4096), (0, 1, 5), (1, 0, 5), (65, 64, 5), (1, 1, 0), (1, 1, 16385)]:
        assert lib.daam_joint_attend_stats_bytes(*args) == fake.daam_joint_attend_stats_bytes(*args), args
    assert lib.daam_joint_attend_stats_bytes(2, 3, 129) == 8 * 6 * 256


# ---- the arithmetic: emulation and mutants against the bound ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def references():
    """Per case: inputs, float64 outputs and their bounds, computed once."""
    out = {}
    for case in A.CASES:
        inp = A.case_inputs(case)
        want_i, want_t, _ = A.reference(inp)
        out[case] = (inp, want_i, want_t, *A.out_bound(inp))
    return out


@pytest.mark.parametrize('case', A.CASES, ids=[A.case_id(c) for c in A.CASES])
def test_the_emulation_is_inside_the_bounds(references, case):
    inp, want_i, want_t, bound_i, bound_t = references[case]
    got_i, got_t, stats = A.emulate(inp)
    s_bound, s_want = A.stats_bound(inp)
    ratios = (A.worst(got_i, want_i, bound_i), A.worst(got_t, want_t, bound_t), A.worst(A.stats_probabilities(inp, stats), s_want, s_bound))
    calls = A.tap_calls(inp)
    planes = A.emulate_text(inp, stats, per_head=True)
    ratios += (A.worst(planes, J.reference_sums(calls, True), J.sums_bound(calls, True)),)
    print(f'\n{A.case_id(case)}: emulation / bound: out_img {ratios[0]:.3f} out_txt {ratios[1]:.3f} statistics {ratios[2]:.3f} planes {ratios[3]:.3f}')
    assert np.isfinite(got_i).all() and np.isfinite(got_t).all() and max(ratios) <= 1.0, ratios


@pytest.mark.parametrize('mutant', A.MUTANTS[:-1])
def test_forward_mutants_fall_outside_the_bound(references, mutant):
    shown = 0
    for case in A.CASES:
        if not A.shows(mutant, case):
            continue
        inp, want_i, want_t, bound_i, bound_t = references[case]
        with np.errstate(all='ignore'):
            got_i, got_t, _ = A.emulate(inp, mutant)
            ratio = max(A.worst(np.nan_to_num(got_i, nan=np.inf), want_i, bound_i), A.worst(np.nan_to_num(got_t, nan=np.inf), want_t, bound_t))
        print(f'\n{mutant} on {A.case_id(case)}: {ratio:.3g} bounds away')
        assert ratio >= WIDE, (mutant, A.case_id(case), ratio)
        shown += 1
    assert shown >= 3, 'the cases give this mutant room to show'


def test_the_neighbours_statistics_fall_outside_the_planes_bound(references):
    shown = 0
    for case in A.CASES:
        if case[0] < 5 or case[6] not in ('small', 'late_outlier', 'peaked'):
            continue
        inp = references[case][0]
        stats = A.emulate(inp)[2]
        calls = A.tap_calls(inp)
        with np.errstate(all='ignore'):
            ratio = A.worst(np.nan_to_num(A.emulate_text(inp, stats, mutant='neighbour_stats'), nan=np.inf), J.reference_sums(calls), J.sums_bound(calls))
        assert ratio >= WIDE, (A.case_id(case), ratio)
        shown += 1
    assert shown >= 3


def test_the_cases_cover_what_the_issue_lists():
    assert {c[0] for c in A.CASES} == set(A.PS) and {c[1] for c in A.CASES} == set(A.TS) and {c[2] for c in A.CASES} == {64, 128}
    assert {c[4][0] * c[4][1] for c in A.CASES} == {1, 3, 6} and {c[5] for c in A.CASES} == set(J.LAYOUTS)
    for dtype in ('f16', 'bf16'):
        assert {c[6] for c in A.CASES if c[3] == dtype} == set(A.LOGITS) and {c[7] for c in A.CASES if c[3] == dtype} == set(A.VALUES)


# ---- Python on stand-ins ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fakes(monkeypatch):
    return A.install(monkeypatch.setattr)


@pytest.mark.parametrize('batch', [2, 1])
def test_trace_joint_with_attend_calls_forward_once_with_the_whole_batch(fakes, batch):
    import daam_amd
    E, joint, aff, lib, loads = fakes
    pipe = M.make_pipe(dtype=torch.bfloat16, seed=1, batch=batch)
    recorded = M.record(pipe)
    cells, T, heads, first = 64, M.CLIP_ROWS + M.T5_ROWS, 2, batch // 2
    with daam_amd.trace_joint(pipe, self_affinity=True, attend=True) as tc:
        pipe(PROMPT, num_inference_steps=2)
        assert recorded == [] and joint.calls == [], 'neither the original processor nor the two-launch tap ran'
        assert len(lib.forwards) == len(lib.texts) == len(aff.calls) == 6 and tc.state.calls == 6 and tc.state.slices == 6 * (batch - first) * heads
        for f, t, a in zip(lib.forwards, lib.texts, aff.calls):
            assert (f['batch'], f['heads'], f['P'], f['T'], f['d']) == (batch, heads, cells, T, 64)
            assert (t['batch'], t['heads'], t['P'], t['T']) == (batch - first, heads, cells, T)
            assert f['strides'][0][:3] == [cells * 128, 64, 128] and f['strides'][2] == [cells * 128, 64, 128, T * 128, 64, 128]
            offset = 8 * first * heads * A.pad128(cells)
            assert t['stats'] == f['stats'] + offset == a[2] and t['stats_bytes'] == f['stats_bytes'] - offset
            assert t['q'] == f['ptrs'][0] + 2 * first * cells * 128 and t['kt'] == f['ptrs'][4] + 2 * first * T * 128
            assert a[0] == t['q'] and a[1] == f['ptrs'][1] + 2 * first * cells * 128
        assert [t['accumulate'] for t in lib.texts] == [0, 1, 1, 1, 1, 1]
        assert tc.state.stats.data_ptr() == lib.texts[-1]['stats']
        # the stand-in's statistics are those of a uniform softmax: every entry of the plane is calls * slices / (T + P)
        want = 6 * (batch - first) * heads / (T + cells)
        assert torch.allclose(tc.state.sums, torch.full_like(tc.state.sums, want), rtol=1e-5)
        assert all(o.shape == (batch, cells, 128) and torch.isfinite(o.float()).all() for o in pipe.outputs)
    assert all(b.attn.processor.__class__ is M.JointProcessor for b in pipe.transformer.transformer_blocks)


def test_calls_that_are_not_tappable_reach_the_original_processor(fakes):
    import daam_amd
    E, joint, aff, lib, loads = fakes
    pipe = M.make_pipe(dtype=torch.bfloat16, seed=1)
    plain = pipe(PROMPT, num_inference_steps=1) and [o.clone() for o in pipe.outputs]
    pipe.mask_fn = lambda n: torch.zeros(n, n, dtype=torch.bfloat16)
    masked = pipe(PROMPT, num_inference_steps=1) and [o.clone() for o in pipe.outputs]
    with daam_amd.trace_joint(pipe, attend=True):
        pipe(PROMPT, num_inference_steps=1)
        assert lib.forwards == [] and joint.calls == [] and all(torch.equal(a, b) for a, b in zip(masked, pipe.outputs)), 'a mask'
        pipe.mask_fn = None
        pipe(PROMPT, num_inference_steps=1, height=64, width=64)
        assert lib.forwards == [] and joint.calls == [], 'another length'
        attn = pipe.transformer.transformer_blocks[0].attn
        out = attn(torch.zeros(2, 64, 128, dtype=torch.bfloat16))
        assert isinstance(out, torch.Tensor) and lib.forwards == [], 'no context'
        for block in pipe.transformer.transformer_blocks:
            block.attn.add_v_proj_kept, block.attn.add_v_proj = block.attn.add_v_proj, None
        try:
            with pytest.raises(TypeError):            # the stand-in's own processor needs the projection: the call reached it
                pipe(PROMPT, num_inference_steps=1)
        finally:
            for block in pipe.transformer.transformer_blocks:
                block.attn.add_v_proj = block.attn.add_v_proj_kept
                del block.attn.add_v_proj_kept
        assert lib.forwards == [], 'a missing projection'
    assert plain is not None


def test_context_pre_only_returns_the_text_rows_as_they_are(fakes):
    import daam_amd
    E, joint, aff, lib, loads = fakes
    pipe = M.make_pipe(dtype=torch.float16, seed=2)
    last = pipe.transformer.transformer_blocks[-1].attn
    last.context_pre_only = True
    seen = []
    with daam_amd.trace_joint(pipe, attend=True):
        for attn in (pipe.transformer.transformer_blocks[0].attn, last):
            seen.append(attn(torch.zeros(2, 64, 128, dtype=torch.float16), encoder_hidden_states=torch.zeros(2, 96, 128, dtype=torch.float16)))
    (img0, txt0), (img1, txt1) = seen
    assert torch.equal(txt1, torch.full_like(txt1, 0.25)), 'out_txt as the library gave it'
    assert not torch.equal(txt0, torch.full_like(txt0, 0.25)) and img0.shape == img1.shape == (2, 64, 128) and txt0.shape == (2, 96, 128)
    last.to_add_out = None
    del last.context_pre_only
    with daam_amd.trace_joint(pipe, attend=True):
        _, txt = last(torch.zeros(2, 64, 128, dtype=torch.float16), encoder_hidden_states=torch.zeros(2, 96, 128, dtype=torch.float16))
    assert torch.equal(txt, torch.full_like(txt, 0.25))


def test_without_attend_nothing_is_loaded(fakes):
    import daam_amd
    E, joint, aff, lib, loads = fakes
    pipe = M.make_pipe(dtype=torch.bfloat16, seed=1)
    for kw in ({}, dict(attend=False)):
        with daam_amd.trace_joint(pipe, **kw) as tc:
            pipe(PROMPT, num_inference_steps=1)
            assert tc.attend is None and len(joint.calls) == 3
        joint.calls.clear()
    assert loads == [] and lib.forwards == [] and lib.texts == []
    with daam_amd.trace_joint(pipe, attend=True) as tc:
        assert loads == [], 'the library is loaded by the first forward'
        pipe(PROMPT, num_inference_steps=1)
    assert loads


def test_the_states_hold_their_limits(fakes):
    E, joint, aff, lib, loads = fakes
    mk = lambda rows, ch=128, dt=torch.float16, b=2: torch.zeros(b, rows, ch, dtype=dt)
    st = E.JointAttendState()
    good = [mk(64), mk(64), mk(64), mk(96), mk(96), mk(96)]
    out_i, out_t, stats = st.forward(*good, 2, 0.125)
    assert out_i.shape == (2, 64, 128) and out_t.shape == (2, 96, 128) and stats.numel() * 8 == 8 * 4 * 128 and st.calls == 1
    for i, bad in ((2, mk(63)), (4, mk(96, dt=torch.bfloat16)), (5, mk(96, b=1)), (0, mk(64, 120)), (3, mk(513))):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            st.forward(*args, 2, 0.125)
    with pytest.raises(ValueError, match='head dim'):
        st.forward(*[mk(r, 96) for r in (64, 64, 64, 96, 96, 96)], 2, 0.125)
    with pytest.raises(ValueError):
        st.forward(*[mk(r, dt=torch.float32) for r in (64, 64, 64, 96, 96, 96)], 2, 0.125)
    assert len(lib.forwards) == 1, 'every refusal came before the native call'
    tap = E.JointTapState(8, 8, 96)
    with pytest.raises(ValueError, match='statistics'):
        tap.tap_from_stats(mk(64), mk(96), 2, 0.125, stats[:100])
    with pytest.raises(ValueError):
        tap.tap_from_stats(mk(63), mk(96), 2, 0.125, stats)
    assert lib.texts == [] and tap.sums is None
    tap.tap_from_stats(mk(64), mk(96), 2, 0.125, stats, weight=0.5)
    tap.tap_from_stats(mk(64), mk(96), 2, 0.125, stats)
    assert [(t['accumulate'], t['weight']) for t in lib.texts] == [(0, 0.5), (1, 1.0)] and tap.calls == 2 and tap.slices == 8 and tap.stats is stats
    tap.reset()
    tap.tap_from_stats(mk(64), mk(96), 2, 0.125, stats)
    assert lib.texts[-1]['accumulate'] == 0
    # a plain tap on the same state writes a workspace of the state's own, never the view it was given
    assert tap._ws is None
    tap.tap(mk(64), mk(96), mk(64), 2, 0.125)
    assert tap._ws is not None and tap._ws.data_ptr() != stats.data_ptr() and tap.stats is tap._ws and joint.ptrs[-1][2] == tap._ws.data_ptr()
    with pytest.raises(RuntimeError, match='fp16 or bf16'):
        tap.tap_from_stats(mk(64, dt=torch.float32), mk(96, dt=torch.float32), 2, 0.125, stats)


def test_the_largest_v_is_the_dtypes_largest():
    assert A.HUGE16 == {'f16': float(torch.finfo(torch.float16).max), 'bf16': float(torch.finfo(torch.bfloat16).max)}
    for dtype in ('f16', 'bf16'):
        inp = A.inputs('small', 'huge', 1, 1, 65, 7, 64, dtype)
        big = np.abs(np.concatenate([inp['vt'], inp['vi']], axis=2))
        assert big.min() >= 0.24 * A.HUGE16[dtype] and 0.85 * A.HUGE16[dtype] <= big.max() <= 0.91 * A.HUGE16[dtype]


def test_a_stale_abi_is_refused(fakes, monkeypatch):
    E, joint, aff, lib, loads = fakes
    monkeypatch.setattr(lib, 'daam_joint_attend_abi_version', lambda: 2)
    with pytest.raises(RuntimeError, match='ABI 2'):
        E.JointAttendState().forward(*[torch.zeros(1, r, 64, dtype=torch.float16) for r in (8, 8, 8, 4, 4, 4)], 1, 0.125)
