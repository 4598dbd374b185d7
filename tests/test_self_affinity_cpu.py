"""The self-attention affinity (include/daam_self_affinity.h) without a GPU: ``libdaam_selfaff.so`` builds beside the other
libraries and exports what its header declares and the binding names; the header is C99; no kernel has scratch; every argument the
header rules out is refused before any HIP call; the float64 reference has the properties the contract states, the f32 emulation is
inside the bounds and the mutants are outside them; and the Python layer (``trace(pipe, self_affinity=True)``, ``SelfAffinity``,
``GlobalHeatMap.propagate``) on numpy stand-ins of the libraries.  The kernels run in ``test_gpu_self_affinity.py``."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import _fake_native as FN
import _libcheck as LC
import _self_affinity_domain as A
from oracle import fake_diffusers as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
N_KERNELS = 29                      # statistics and sums for 2 dtypes x 4 depths; propagate for 1 2 4 8 16 32 accumulators, first and later; copy


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.SELFAFF_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_self_affinity()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_selfaff.so' and not build.self_affinity_stale()
    assert build.SELFAFF_SOURCES == ['daam_self_affinity.hip']
    exported = LC.exported(built)
    assert exported == LC.declared('daam_self_affinity.h') == sorted(nat.SELFAFF_EXPORTS) and len(exported) == 6
    assert lib.daam_self_affinity_abi_version() == 1 == nat.SELFAFF_ABI_VERSION
    assert len(lib.daam_self_affinity_accumulate.argtypes) == 20 and len(lib.daam_self_affinity_propagate.argtypes) == 9
    names = list(build.kernel_shas(built))
    assert len(names) == N_KERNELS and sum('selfaff_stats_kernel' in n for n in names) == 8
    assert sum('selfaff_sums_kernel' in n for n in names) == 8 and sum('selfaff_propagate_kernel' in n for n in names) == 12


def test_self_affinity_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_self_affinity.h"\nint main(void) { return DAAM_SELF_AFFINITY_ABI_VERSION == 1 && '
                   'sizeof(&daam_self_affinity_accumulate) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)
    assert 'NOT rounded to the input dtype' in open(os.path.join(ROOT, 'include', 'daam_self_affinity.h')).read()


def test_no_kernel_has_scratch(built):
    """Private segment size 0 and the private-segment enable bit clear in every kernel descriptor; LDS only in the MFMA kernels."""
    from daam_amd import build
    kds = LC.kernel_descriptors(built)
    names = list(build.kernel_shas(built))
    assert len(names) == N_KERNELS and all(k in kds for k in names)
    for k in names:
        group, private = struct.unpack_from('<II', kds[k], 0)
        _, rsrc2 = struct.unpack_from('<II', kds[k], 48)
        assert private == 0 and not (rsrc2 & 1), (k, group, private)
        assert (group > 0) == ('selfaff_stats_kernel' in k or 'selfaff_sums_kernel' in k) and group <= 64 * 1024, (k, group)


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
def _accumulate(lib, **over):
    """A call that is in range but for ``over``; pointers are small fake addresses (nothing is dereferenced)."""
    a = dict(q=0x100000, k=0x200000, dtype=0, batch=2, heads=8, P=77, d=40, qs=(77 * 320, 40, 320), ks=(77 * 320, 40, 320), scale=0.158,
             weight=1.0, accumulate=0, sums=0x1000000, ws=0x2000000, ws_bytes=None, stream=None)
    a.update(over)
    if a['ws_bytes'] is None:
        a['ws_bytes'] = lib.daam_self_affinity_workspace(a['batch'], a['heads'], a['P']) or 1 << 20
    rc = lib.daam_self_affinity_accumulate(a['q'], a['k'], a['dtype'], a['batch'], a['heads'], a['P'], a['d'], *a['qs'], *a['ks'], a['scale'],
                                           a['weight'], a['accumulate'], a['sums'], a['ws'], a['ws_bytes'], a['stream'])
    return rc, lib.daam_self_affinity_last_error().decode()


def _propagate(lib, **over):
    a = dict(sums=0x1000000, P=77, maps=0x3000000, N=3, iterations=2, refined=0x4000000, ws=0x5000000, ws_bytes=None, stream=None)
    a.update(over)
    if a['ws_bytes'] is None:
        a['ws_bytes'] = lib.daam_self_affinity_propagate_workspace(a['N'], a['P']) or 1 << 20
    rc = lib.daam_self_affinity_propagate(a['sums'], a['P'], a['maps'], a['N'], a['iterations'], a['refined'], a['ws'], a['ws_bytes'], a['stream'])
    return rc, lib.daam_self_affinity_last_error().decode()


BAD_ACCUMULATE = {
    'f32 inputs': dict(dtype=1), 'dtype 3': dict(dtype=3), 'batch 0': dict(batch=0), 'heads 0': dict(heads=0), '4097 slices': dict(batch=4097, heads=1),
    '4160 slices': dict(batch=65, heads=64), 'P 0': dict(P=0), 'P 16385': dict(P=16385), 'd 32': dict(d=32), 'd 48': dict(d=48), 'd 168': dict(d=168),
    'd 0': dict(d=0), 'scale 0': dict(scale=0.0), 'scale -1': dict(scale=-1.0), 'scale inf': dict(scale=math.inf), 'scale nan': dict(scale=math.nan),
    'weight inf': dict(weight=math.inf), 'weight nan': dict(weight=math.nan), 'NULL q': dict(q=None), 'NULL k': dict(k=None),
    'NULL sums': dict(sums=None), 'NULL workspace': dict(ws=None), 'q off 16 bytes': dict(q=0x100008), 'k off 16 bytes': dict(k=0x200002),
    'sums off 4 bytes': dict(sums=0x1000002), 'workspace off 8 bytes': dict(ws=0x2000004), 'row stride not 8': dict(qs=(77 * 324, 40, 324)),
    'head stride not 8': dict(ks=(77 * 320, 36, 320)), 'batch stride not 8': dict(qs=(77 * 320 + 4, 40, 320)), 'negative stride': dict(ks=(-8, 40, 320)),
    'row stride below d': dict(qs=(77 * 32, 40, 32)), 'short workspace': dict(ws_bytes=8 * 16 * 128 - 8), 'sums in the workspace': dict(sums=0x2000000 + 64),
}
BAD_PROPAGATE = {
    'P 0': dict(P=0), 'P 16385': dict(P=16385), 'no maps': dict(N=0), '33 maps': dict(N=33), 'iterations -1': dict(iterations=-1),
    'iterations 17': dict(iterations=17), 'NULL sums': dict(sums=None), 'NULL maps': dict(maps=None), 'NULL refined': dict(refined=None),
    'NULL workspace': dict(ws=None), 'sums off 4 bytes': dict(sums=0x1000001), 'refined off 4 bytes': dict(refined=0x4000002),
    'short workspace': dict(ws_bytes=4 * 4 * 77 - 4), 'refined is maps': dict(refined=0x3000000),
    'refined inside maps': dict(refined=0x3000000 + 4 * 3 * 77 - 4), 'refined is the workspace': dict(refined=0x5000000),
    'refined ends in the workspace': dict(refined=0x5000000 - 4 * 3 * 77 + 4),
    'refined inside a larger workspace': dict(refined=0x5000000 + (1 << 20), ws_bytes=1 << 21),
    'maps are the workspace': dict(maps=0x5000000), 'maps end in the workspace': dict(maps=0x5000000 - 4 * 3 * 77 + 4),
    'maps inside a larger workspace': dict(maps=0x5000000 + (1 << 20), ws_bytes=1 << 21), 'sums are refined': dict(sums=0x4000000),
    'sums end in refined': dict(sums=0x4000000 - 4 * 77 * 77 + 4), 'sums are the workspace': dict(sums=0x5000000),
    'sums end in the workspace': dict(sums=0x5000000 - 4 * 77 * 77 + 4),
}
# The inside of every limit, through the entry points.  A call that passes the checks would launch, so each of these carries ONE fault
# that the LAST range check catches (a workspace eight bytes short): a message about the workspace shows that every check before it --
# the limit under test among them -- let the call through.
INSIDE_ACCUMULATE = {
    'P 1': dict(P=1), 'P 16384': dict(P=16384), '4096 slices': dict(batch=64, heads=64), '4096 x 1': dict(batch=4096, heads=1),
    'one slice': dict(batch=1, heads=1), 'bf16': dict(dtype=2), 'd 40': dict(d=40), 'd 64': dict(d=64, qs=(77 * 512, 64, 512), ks=(77 * 512, 64, 512)),
    'd 80': dict(d=80, qs=(77 * 640, 80, 640), ks=(77 * 640, 80, 640)), 'd 160': dict(d=160, qs=(77 * 1280, 160, 1280), ks=(77 * 1280, 160, 1280)),
    'packed layout': dict(qs=(8 * 77 * 40, 77 * 40, 40), ks=(8 * 77 * 40, 77 * 40, 40)), 'zero batch stride': dict(batch=1, qs=(0, 40, 320)),
    'tiny scale': dict(scale=1e-30), 'huge scale': dict(scale=1e30), 'weight 0': dict(weight=0.0), 'negative weight': dict(weight=-3.5),
    'accumulate 1': dict(accumulate=1),
}
INSIDE_PROPAGATE = {
    'P 1': dict(P=1), 'P 16384': dict(P=16384, sums=0x40000000, maps=0x10000000, refined=0x20000000, ws=0x30000000), 'one map': dict(N=1),
    '32 maps': dict(N=32), 'iterations 0': dict(iterations=0), 'iterations 16': dict(iterations=16),
}


@pytest.mark.parametrize('what', sorted(BAD_ACCUMULATE))
def test_accumulate_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _accumulate(lib, **BAD_ACCUMULATE[what])
    assert rc == E_INVALID and msg, (what, rc, msg)


@pytest.mark.parametrize('what', sorted(INSIDE_ACCUMULATE))
def test_accumulate_inside_every_limit_reaches_the_last_check(lib, what):
    over = dict(INSIDE_ACCUMULATE[what])
    shape = dict(batch=2, heads=8, P=77)
    shape.update({k: v for k, v in over.items() if k in shape})
    need = lib.daam_self_affinity_workspace(shape['batch'], shape['heads'], shape['P'])
    assert need > 0
    rc, msg = _accumulate(lib, **dict(over, ws_bytes=need - 8))
    assert rc == E_INVALID and msg.startswith('self_affinity_accumulate: workspace of'), (what, rc, msg)


@pytest.mark.parametrize('what', sorted(INSIDE_PROPAGATE))
def test_propagate_inside_every_limit_reaches_the_workspace_check(lib, what):
    over = dict(INSIDE_PROPAGATE[what])
    need = lib.daam_self_affinity_propagate_workspace(over.get('N', 3), over.get('P', 77))
    assert need > 0
    rc, msg = _propagate(lib, **dict(over, ws_bytes=need - 8))
    assert rc == E_INVALID and msg.startswith('self_affinity_propagate: workspace of'), (what, rc, msg)


@pytest.mark.parametrize('what', sorted(BAD_PROPAGATE))
def test_propagate_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _propagate(lib, **BAD_PROPAGATE[what])
    assert rc == E_INVALID and msg, (what, rc, msg)


def test_size_functions_agree_with_the_stand_in(lib):
    """The limits from inside: the largest sizes give a size, one past them gives 0 (a call at a limit cannot run here: past the checks
    it launches)."""
    fake = A.FakeSelfAffinityLib()
    for b, h, P in ((1, 1, 1), (2, 8, 77), (1, 10, 4096), (64, 64, 16384), (4096, 1, 128), (1, 4096, 129)):
        want = 8 * b * h * (-(-P // 128) * 128)
        assert lib.daam_self_affinity_workspace(b, h, P) == fake.daam_self_affinity_workspace(b, h, P) == want
    for bad in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (1, 1, 16385), (4097, 1, 4), (65, 64, 4), (-1, 4, 4)):
        assert lib.daam_self_affinity_workspace(*bad) == 0 == fake.daam_self_affinity_workspace(*bad), bad
    for n, P in ((1, 1), (3, 77), (32, 16384), (8, 4096), (2, 5)):
        got = lib.daam_self_affinity_propagate_workspace(n, P)
        assert got == fake.daam_self_affinity_propagate_workspace(n, P) == (4 * (n + 1) * P + 7) // 8 * 8 and got % 8 == 0
    for bad in ((0, 4), (33, 4), (1, 0), (1, 16385)):
        assert lib.daam_self_affinity_propagate_workspace(*bad) == 0 == fake.daam_self_affinity_propagate_workspace(*bad), bad


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_one_cell_and_equal_logits():
    q, k, scale = A.inputs('small', 2, 3, 1, 40, 'f16')
    for w in (1.0, -0.5):
        assert A.reference_sums([(q, k, scale, w)]).tolist() == [[6 * w]] and A.emulate_sums([(q, k, scale, w)]).tolist() == [[6 * w]]
    q, k, scale = A.inputs('zero_q', 1, 3, 65, 64, 'bf16')
    assert np.abs(A.reference_sums([(q, k, scale, 1.0)]) - 3 / 65).max() <= 2.0 ** -50
    assert np.abs(A.emulate_sums([(q, k, scale, 1.0)]) - np.float32(3 / 65)).max() <= 12 * A.U * 3 / 65


@pytest.mark.parametrize('regime', A.REGIMES)
@pytest.mark.parametrize('dtype', ['f16', 'bf16'])
def test_row_sums_and_the_emulation_inside_bound_a(regime, dtype):
    for P, d, slices in ((5, 40, (1, 1)), (65, 64, (1, 3)), (130, 80, (2, 3))):
        q, k, scale = A.inputs(regime, *slices, P, d, dtype, seed=3)
        q2, k2, _ = A.inputs('small', *slices, P, d, dtype, seed=4)
        s = slices[0] * slices[1]
        for calls in ([(q, k, scale, 1.0)], [(q, k, scale, 0.5), (q2, k2, scale, -0.25)]):
            ref, bound, emu = A.reference_sums(calls), A.sums_bound(calls), A.emulate_sums(calls)
            total = sum(c[3] for c in calls) * s
            assert np.abs(ref.sum(axis=1) - total).max() <= 2.0 ** -40
            assert np.abs(emu.astype(np.float64).sum(axis=1) - total).max() <= bound.sum(axis=1).max()
            err = np.abs(emu - ref)
            assert (err <= bound).all(), (regime, dtype, P, float((err / bound).max()))


MUTANTS = ('no_scale', 'padded_keys', 'neighbour_stats', 'packed_head_stride')


@pytest.mark.parametrize('mutant', MUTANTS)
def test_mutants_of_accumulate_fall_outside_bound_a(mutant):
    """The bound can fail: a dropped scale, padded keys counted in the row sum (P = 65 is no multiple of 32), the neighbour row's
    statistics, the packed layout's head stride on the interleaved layout."""
    q, k, scale = A.inputs('small', 1, 3, 65, 40, 'f16', seed=1)
    calls = [(q, k, scale, 1.0)]
    ref, bound = A.reference_sums(calls), A.sums_bound(calls)
    assert (np.abs(A.emulate_sums(calls) - ref) <= bound).all()
    assert (np.abs(A.emulate_sums(calls, mutant=mutant) - ref) > bound).any()
    if mutant == 'padded_keys':                       # at a multiple of the step there is nothing padded to count
        q, k, scale = A.inputs('small', 1, 1, 64, 40, 'f16', seed=1)
        assert np.array_equal(A.emulate_sums([(q, k, scale, 1.0)], mutant=mutant), A.emulate_sums([(q, k, scale, 1.0)]))


def test_propagation_properties_of_the_reference_and_the_emulation():
    rng = np.random.default_rng(0)
    for P in (1, 5, 65, 130):
        m = A.maps(3, P, seed=P, signed=True)
        eye = (4.0 * np.eye(P)).astype(np.float32)
        assert np.array_equal(A.reference_propagate(eye, m, 3), m.astype(np.float64)) and np.array_equal(A.emulate_propagate(eye, m, 3), m)
        flat = np.full((P, P), 0.75, np.float32)
        mean = m.astype(np.float64).mean(axis=1, keepdims=True)
        assert np.abs(A.reference_propagate(flat, m, 1) - mean).max() <= 2.0 ** -50
        assert np.abs(A.emulate_propagate(flat, m, 1) - mean).max() <= A.propagate_bound(P, m, 1)
        s = rng.uniform(0, 1, (P, P)).astype(np.float32)
        if P > 1:
            s[P // 2] = 0
        for T in (0, 1, 2, 16):
            ref, emu = A.reference_propagate(s, m, T), A.emulate_propagate(s, m, T)
            if T == 0:
                assert np.array_equal(ref, m.astype(np.float64)) and np.array_equal(emu.view(np.uint32), m.view(np.uint32))
            assert ref.min() >= m.min() - 1e-12 and ref.max() <= m.max() + 1e-12
            assert np.abs(emu - ref).max() <= A.propagate_bound(P, m, T)
            if P > 1:
                assert np.array_equal(ref[:, P // 2], m[:, P // 2].astype(np.float64)) and np.array_equal(emu[:, P // 2], m[:, P // 2])
        if P > 1:
            wrong = A.emulate_propagate(s, m, 1, mutant='no_normalisation')
            assert np.abs(wrong - A.reference_propagate(s, m, 1)).max() > A.propagate_bound(P, m, 1)


def test_end_to_end_bound_on_the_emulation():
    q, k, scale = A.inputs('small', 1, 3, 65, 40, 'f16', seed=5)
    calls = [(q, k, scale, 1.0)]
    exact, delta, sums = A.reference_sums(calls), A.sums_bound(calls), A.emulate_sums(calls)
    m = A.maps(3, 65, seed=2)
    for T in (1, 2, 16):
        got = A.emulate_propagate(sums, m, T)
        assert np.abs(got - A.reference_propagate(sums, m, T)).max() <= A.propagate_bound(65, m, T)
        assert np.abs(got - A.reference_propagate(exact, m, T)).max() <= A.combined_bound(delta, exact, m, T)


# ---- the Python layer on the numpy stand-ins -------------------------------------------------------------------------------------------
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def add_attn1(pipe, seed=0):
    """Give every transformer block of the stand-in UNet an ``attn1`` (a ``FakeAttention`` with identity projections, so Q = K = the
    hidden states) and let the UNet's forward call it before the block's ``attn2``: the outputs are ``[attn1, attn2, attn1, ...]``."""
    unet = pipe.unet
    owner = {}
    blocks = list(unet.down_blocks) + [unet.mid_block] + list(unet.up_blocks)
    for blk in blocks:
        for tr in getattr(blk, 'attentions', []):
            for tb in tr.transformer_blocks:
                a2 = tb.attn2
                inner = a2.heads * a2.dim_head
                tb.attn1 = fd.FakeAttention(inner, inner, a2.heads, a2.dim_head, identity_proj=True).to(device=pipe.device, dtype=pipe.dtype)
                owner[a2] = tb

    def forward(hidden_fn, context_fn, step, mask_fn=None):
        outs = []
        for i, spec in enumerate(unet.execution_order()):
            hs = hidden_fn(i, spec, step)
            outs.append(owner[spec.module].attn1(hs))
            outs.append(spec.module(hs, encoder_hidden_states=context_fn(i, spec)))
        return outs
    unet.forward = forward
    return owner


def self_attention_calls(pipe, steps, grid):
    """``[(q, k, scale, 1.0)]`` of every ``attn1`` call a traced generation taps: the layers (not the mid block) whose hidden states
    have ``grid`` positions, the second half of the batch, f32 [b, heads, P, d]."""
    calls = []
    for step in range(steps):
        for i, spec in enumerate(pipe.unet.execution_order()):
            if spec.res * spec.res != grid or spec.module in [tb.attn2 for tr in pipe.unet.mid_block.attentions for tb in tr.transformer_blocks]:
                continue
            hs = pipe.hidden_states(i, spec, step).float().cpu()
            kept = hs[hs.shape[0] // 2:]
            x = kept.reshape(kept.shape[0], kept.shape[1], spec.heads, spec.dim_head).permute(0, 2, 1, 3).contiguous().numpy()
            calls.append((x, x, float(np.float32(spec.module.scale)), 1.0))
    return calls


@pytest.fixture
def fakes(monkeypatch):
    E, hip = FN.install(monkeypatch.setattr)
    E._PARKED.clear()
    _, lib = A.install(monkeypatch.setattr)
    monkeypatch.setenv('DAAM_NO_FASTPATH', '1')
    yield E, hip, lib
    E._PARKED.clear()


def _pipe(batch=2):
    pipe = fd.make_pipe('sd15', dtype=torch.float16, batch=batch, seed=3, mini=True, identity_proj=True, dim_head=40, latent_size=8)
    add_attn1(pipe)
    pipe.keep_outputs = True
    return pipe


def _attn1s(pipe):
    return [tb.attn1 for blk in list(pipe.unet.up_blocks) + list(pipe.unet.down_blocks) + [pipe.unet.mid_block]
            for tr in getattr(blk, 'attentions', []) for tb in tr.transformer_blocks]


@pytest.mark.parametrize('batch', [2, 1])
def test_trace_taps_the_calls_of_the_grid_and_leaves_the_model_alone(fakes, batch):
    import daam_amd
    from daam_amd import SelfAffinity, UNetCrossAttentionLocator, UNetSelfAttentionLocator
    E, hip, lib = fakes
    pipe, steps = _pipe(batch), 2
    pipe(PROMPT, num_inference_steps=steps)
    plain = [o.clone() for o in pipe.last_outputs[0::2]]
    cross, selfs = UNetCrossAttentionLocator().locate(pipe.unet), UNetSelfAttentionLocator().locate(pipe.unet)
    assert len(cross) == len(selfs) == 15 and all(s is o.attn1 for s, o in zip(selfs, [add for add in _owners(pipe, cross)]))
    before = [a.processor for a in _attn1s(pipe)]
    with daam_amd.trace(pipe, height=64, width=64, self_affinity=True) as tc:
        hooked = [a for a in _attn1s(pipe) if type(a.processor).__name__ == 'UNetSelfAttentionHooker']
        assert hooked == selfs                                         # same blocks, same order, not the mid block
        pipe(PROMPT, num_inference_steps=steps)
        assert all(torch.equal(a, b) for a, b in zip(plain, pipe.last_outputs[0::2]))
        aff = tc.compute_self_affinity()
    assert [a.processor for a in _attn1s(pipe)] == before
    calls = self_attention_calls(pipe, steps, 64)
    kept = batch - batch // 2
    assert len(calls) == 5 * steps and isinstance(aff, SelfAffinity) and aff.grid == (8, 8)
    assert (aff.calls, aff.slices) == (len(calls), len(calls) * 8 * kept)
    rec = [c for c in lib.calls if c[0] == 'accumulate']
    assert len(rec) == len(calls) and [c[-1] for c in rec] == [0] + [1] * (len(calls) - 1)          # the first call overwrites
    assert all(c[1:7] == (A.DAAM_F16, kept, 8, 64, 40, (64 * 320, 40, 320, 64 * 320, 40, 320)) for c in rec)
    assert np.array_equal(aff.sums.numpy(), A.emulate_sums(calls))
    assert torch.allclose(aff.matrix().sum(dim=1), torch.ones(64), atol=1e-5) and aff.of(2, 3).shape == (8, 8)
    assert torch.equal(aff.of(2, 3).reshape(-1), aff.matrix()[2 * 8 + 3]) and torch.equal(aff.cpu().sums, aff.sums)
    with pytest.raises(ValueError):
        aff.of(8, 0)


def _owners(pipe, cross):
    table = {tb.attn2: tb for blk in list(pipe.unet.up_blocks) + list(pipe.unet.down_blocks) for tr in getattr(blk, 'attentions', [])
             for tb in tr.transformer_blocks}
    return [table[a] for a in cross]


def test_a_second_generation_starts_over_and_masked_calls_are_not_tapped(fakes):
    import daam_amd
    E, hip, lib = fakes
    pipe = _pipe()
    with daam_amd.trace(pipe, height=64, width=64, self_affinity=True) as tc:
        pipe(PROMPT, num_inference_steps=1)
        first = tc.compute_self_affinity()
        pipe(PROMPT, num_inference_steps=1)
        second = tc.compute_self_affinity()
        assert (second.calls, second.slices) == (first.calls, first.slices) == (5, 40) and torch.equal(first.sums, second.sums)
        n = len(lib.calls)
        attn = _attn1s(pipe)[0]
        hs = torch.zeros(2, 64, 320, dtype=torch.float16)
        attn(hs, attention_mask=torch.zeros(2, 1, 64, dtype=torch.float16))
        attn(hs, encoder_hidden_states=hs)
        attn(torch.zeros(2, 16, 320, dtype=torch.float16))
        assert len(lib.calls) == n
        attn(hs)
        assert len(lib.calls) == n + 1


def test_the_default_trace_installs_nothing_on_attn1_and_the_errors(fakes):
    import daam_amd
    E, hip, lib = fakes
    pipe = _pipe()
    before = [a.processor for a in _attn1s(pipe)]
    with daam_amd.trace(pipe, height=64, width=64) as tc:
        assert [a.processor for a in _attn1s(pipe)] == before and tc.engine.self_affinity is None
        pipe(PROMPT, num_inference_steps=1)
        assert not lib.calls
        with pytest.raises(ValueError, match='self_affinity=True'):
            tc.compute_self_affinity()
    with pytest.raises(ValueError, match='batch_prompts'):
        daam_amd.trace(pipe, self_affinity=True, batch_prompts=True)
    single = fd.make_pipe('sd15', dtype=torch.float32, mini=True, identity_proj=True, dim_head=40, latent_size=8)
    with pytest.raises(ValueError, match='fp16 or bf16.*float32'):
        daam_amd.trace(single, self_affinity=True)
    daam_amd.trace(single)                                             # the default trace of an fp32 pipeline is what it was
    with daam_amd.trace(pipe, self_affinity=True) as tc:               # the default 96 x 96 grid: no attn1 call of this UNet has 9216 positions
        pipe(PROMPT, num_inference_steps=1)
        assert not lib.calls and tc.engine.self_affinity.sums is None
        with pytest.raises(RuntimeError, match='No self-attention maps found'):
            tc.compute_self_affinity()
    with daam_amd.trace(pipe, height=64, width=64, self_affinity=True, probes=['a cat'], probe_embeds=torch.zeros(1, 77, 320)) as tc:
        pipe(PROMPT, num_inference_steps=1)
        assert tc.compute_self_affinity().calls == 5


@pytest.mark.parametrize('n', [1, 32, 33, 65])
def test_propagate_runs_in_blocks_of_32(fakes, n):
    from daam_amd import SelfAffinity
    E, hip, lib = fakes
    h, w = 5, 7
    rng = np.random.default_rng(n)
    sums = rng.uniform(0, 1, (h * w, h * w)).astype(np.float32)
    aff = SelfAffinity(torch.from_numpy(sums), (h, w), 3, 1)
    m = rng.uniform(0, 1, (n, h, w)).astype(np.float32)
    got = aff.propagate(torch.from_numpy(m), iterations=2)
    blocks = [32] * (n // 32) + ([n % 32] if n % 32 else [])
    assert lib.calls == [('propagate', h * w, b, 2) for b in blocks]
    assert got.dtype == torch.float32 and got.shape == (n, h, w)
    assert np.array_equal(got.numpy().reshape(n, -1), A.emulate_propagate(sums, m.reshape(n, -1), 2))
    assert np.array_equal(aff.propagate(torch.from_numpy(m), iterations=0).numpy(), m)
    for bad in (dict(iterations=17), dict(iterations=-1)):
        with pytest.raises(ValueError):
            aff.propagate(torch.from_numpy(m), **bad)
    with pytest.raises(ValueError, match='5 x 7.*5 x 6'):
        aff.propagate(torch.from_numpy(m[:, :, :6].copy()))
    with pytest.raises(ValueError):
        SelfAffinity(torch.from_numpy(sums), (5, 6), 3, 1)


def test_global_heat_map_propagate_is_the_propagated_word_map(fakes, monkeypatch):
    from daam_amd import GlobalHeatMap, SelfAffinity
    from daam_amd.utils import compute_token_merge_indices
    E, hip, lib = fakes
    monkeypatch.setattr(E, 'word_heat_map', lambda maps, idxs: maps[list(idxs)].mean(0))
    h, w = 9, 14
    rng = np.random.default_rng(1)
    sums = rng.uniform(0, 1, (h * w, h * w)).astype(np.float32)
    aff = SelfAffinity(torch.from_numpy(sums), (h, w), 3, 1)
    tok = fd.FakeTokenizer()
    planes = np.abs(rng.standard_normal((13, h, w))).astype(np.float32)
    ghm = GlobalHeatMap(tok, PROMPT, torch.from_numpy(planes))
    out = ghm.propagate(aff, iterations=2)
    assert isinstance(out, GlobalHeatMap) and out is not ghm and out.prompt == PROMPT and out.tokenizer is tok
    assert out.heat_maps.dtype == torch.float32 and np.array_equal(ghm.heat_maps.numpy(), planes)
    want = A.emulate_propagate(sums, planes.reshape(13, -1), 2).reshape(13, h, w)
    assert np.array_equal(out.heat_maps.numpy(), want)
    idxs = compute_token_merge_indices(tok, PROMPT, 'bicycle', None)[0]
    word = ghm.compute_word_heat_map('bicycle').heatmap.numpy()
    moved = A.reference_propagate(sums, word.reshape(1, -1), 2).reshape(h, w)
    assert len(idxs) == 2 and np.abs(out.compute_word_heat_map('bicycle').heatmap.numpy() - moved).max() <= 2 * A.propagate_bound(h * w, planes, 2)
    half = GlobalHeatMap(tok, PROMPT, torch.from_numpy(planes).half()).propagate(aff)
    assert half.heat_maps.dtype == torch.float16 and lib.calls[-1] == ('propagate', h * w, 13, 1)
    with pytest.raises(ValueError, match='9 x 14.*14 x 9'):
        GlobalHeatMap(tok, PROMPT, torch.zeros(13, 14, 9)).propagate(aff)
    with pytest.raises(TypeError):
        ghm.propagate(aff.sums)
