"""The rotary pass and ``trace_flux`` (include/daam_rope.h) without a GPU: ``libdaam_rope.so`` builds by the side
libraries' recipe beside their tables, exports what its header declares and the binding names; the header is C99; no kernel has
scratch or LDS; every argument the header rules out is refused before any HIP call; the numpy oracle equals the torch CPU expression
bit for bit on every case of the device test and every mutant differs from it; the T5 row lookup; what ``trace_flux`` refuses.  The
kernel runs in ``test_gpu_rope.py``, the hooker in ``test_gpu_flux.py``."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import _flux_standin as FS
import _libcheck as LC
import _rope_domain as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_KERNELS = 4                       # 2 dtypes x 2 head dims


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build_rope(verbose=False)
    return build.ROPE_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_rope()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_rope.so' and not build.rope_stale()
    assert build.ROPE_SOURCES == ['daam_rope.hip'] and build.ROPE.name == 'rope'
    exported = LC.exported(built)
    assert exported == LC.declared('daam_rope.h') == sorted(nat.ROPE_EXPORTS) and len(exported) == 3
    assert lib.daam_rope_abi_version() == 1 == nat.ROPE_ABI_VERSION and nat.ROPE_LIBRARY.env == 'DAAM_ROPE_LIB'
    assert len(lib.daam_rope_apply.argtypes) == 5 and ctypes.sizeof(nat.RopeJob) == 104
    assert nat.load_rope.__name__ == 'load_rope' and nat.check_rope.__name__ == 'check_rope'
    names = list(build.kernel_shas(built))
    assert len(names) == N_KERNELS and all('rope_kernel' in n for n in names)


def test_the_records_stand_outside_the_tables():
    from daam_amd import _native as nat, build
    assert [lib.name for lib in build.SIDE_LIBRARIES] == ['analysis', 'eval', 'locate', 'components', 'refine', 'selfaff']
    assert build.ROPE not in build.SIDE_LIBRARIES and build.ROPE != build.JOINT and isinstance(build.ROPE, build.SideLibrary)
    assert nat.ROPE_LIBRARY not in nat.LIBRARIES and len(nat.LIBRARIES) == 7 and isinstance(nat.ROPE_LIBRARY, nat.Library)
    assert build.JOINT_SOURCES == ['daam_joint_tap.hip'] and nat.JOINT_LIBRARY.file == 'libdaam_joint.so'
    assert 'daam_rope.hip' not in build.SOURCES and not any('rope' in h for h in build.HEADERS)
    assert build.rope_stale.func is build.side_stale and build.build_rope.func is build.build_side
    assert build.rope_stale.args == build.build_rope.args == (build.ROPE,)


def test_csrc_sha_does_not_see_the_rope_files(monkeypatch):
    from daam_amd import build
    before = build.csrc_sha()
    real_open = open
    seen = []

    def spy(path, *a, **k):
        seen.append(os.path.basename(str(path)))
        return real_open(path, *a, **k)
    monkeypatch.setattr('builtins.open', spy)
    assert build.csrc_sha() == before
    assert seen and not any('rope' in name for name in seen)


def test_build_rope_is_the_side_recipe(monkeypatch):
    from daam_amd import build
    ran = []
    monkeypatch.setattr(build.subprocess, 'run', lambda cmd, check: ran.append(cmd))
    assert build.build_rope(force=True, verbose=False) == build.ROPE_LIB
    src = os.path.join(build.HERE, 'csrc', 'daam_rope.hip')
    assert ran == [[build.hipcc(), *build.HIPCC_FLAGS, src, '-o', build.ROPE_LIB]]
    ran.clear()
    build.build(force=True, verbose=False)
    assert not any('rope' in ' '.join(cmd) for cmd in ran), 'build() makes the libraries of its tables alone'


def test_rope_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_rope.h"\nint main(void) { daam_rope_job j; j.rows = 1; return DAAM_ROPE_ABI_VERSION == 1 && j.rows && '
                   'sizeof(daam_rope_job) == 104 && sizeof(&daam_rope_apply) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)


def test_no_kernel_has_scratch_or_lds(built):
    from daam_amd import build
    names = list(build.kernel_shas(built))
    LC.assert_no_scratch(built, names)
    kds = LC.kernel_descriptors(built)
    for k in names:
        group, = struct.unpack_from('<I', kds[k], 0)
        assert group == 0, (k, group)


def test_the_source_fences_contraction():
    text = open(os.path.join(ROOT, 'daam_amd', 'csrc', 'daam_rope.hip')).read()
    assert '#pragma clang fp contract(off)' in text and 'fmaf' not in text
    includes = [line for line in text.splitlines() if line.startswith('#include "')]
    assert includes == ['#include "../../include/daam_rope.h"']
    header = open(os.path.join(ROOT, 'include', 'daam_rope.h')).read()
    assert [line for line in header.splitlines() if line.startswith('#include')] == ['#include "daam_hip.h"']
    assert 'UNDEFINED' in header, 'overlapping outputs of different jobs are documented as undefined'


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
def _job(**over):
    """A job that is in range but for ``over``; pointers are small fake addresses (nothing is dereferenced)."""
    from daam_amd import _native as nat
    a = dict(x=0x100000, out=0x900000, cos=0x2000000, sin=0x3000000, batch=2, heads=8, rows=96, xs=(96 * 512, 512, 64), os=(96 * 512, 512, 64),
             ts=64)
    a.update(over)
    return nat.RopeJob(a['x'], a['out'], a['cos'], a['sin'], a['batch'], a['heads'], a['rows'], *a['xs'], *a['os'], a['ts'])


def _apply(lib, jobs, n_jobs=None, dtype=0, d=64):
    from daam_amd import _native as nat
    table = (nat.RopeJob * max(len(jobs), 1))(*jobs)
    rc = lib.daam_rope_apply(table if jobs else None, len(jobs) if n_jobs is None else n_jobs, dtype, d, None)
    return rc, lib.daam_rope_last_error().decode()


BAD_JOB = {
    'rows 0': dict(rows=0), 'rows 16897': dict(rows=16897), 'batch 0': dict(batch=0), 'heads 0': dict(heads=0), '4097 slices': dict(batch=4097, heads=1),
    'NULL x': dict(x=None), 'NULL out': dict(out=None), 'NULL cos': dict(cos=None), 'NULL sin': dict(sin=None),
    'x off 16 bytes': dict(x=0x100008), 'out off 16 bytes': dict(out=0x900002), 'cos off 16 bytes': dict(cos=0x2000004), 'sin off 16 bytes': dict(sin=0x3000008),
    'x row stride not 8': dict(xs=(96 * 512, 516, 64)), 'x head stride not 8': dict(xs=(96 * 512, 512, 68)), 'x batch stride not 8': dict(xs=(96 * 512 + 4, 512, 64)),
    'out row stride not 8': dict(os=(96 * 512, 516, 64)), 'out head stride not 8': dict(os=(96 * 512, 512, 68)),
    'out batch stride not 8': dict(os=(96 * 512 + 4, 512, 64)), 'negative x stride': dict(xs=(-8, 512, 64)), 'negative out stride': dict(os=(96 * 512, 512, -64)),
    'x row stride below d': dict(xs=(96 * 512, 32, 64)), 'x head stride below d': dict(xs=(96 * 512, 512, 32)),
    'out row stride below d': dict(os=(96 * 512, 32, 64)), 'out head stride below d': dict(os=(96 * 512, 512, 56)),
    'table stride below d': dict(ts=60), 'table stride not 4': dict(ts=66), 'negative table stride': dict(ts=-64),
    'out on x': dict(out=0x100000), 'out inside x': dict(out=0x100000 + 2 * 96 * 512), 'out ends inside x': dict(out=0x100000 - 2 * 96 * 512),
    'out one row before the end of x': dict(out=0x100000 + 2 * (2 * 96 * 512 - 64)),
}
BAD_CALL = {
    'no jobs': dict(n_jobs=0), 'five jobs': dict(n_jobs=5), 'negative jobs': dict(n_jobs=-1), 'f32': dict(dtype=1), 'dtype 3': dict(dtype=3),
    'd 32': dict(d=32), 'd 96': dict(d=96), 'd 256': dict(d=256), 'd 0': dict(d=0),
}
# The inside of every limit.  A call that passes the checks would launch, so each of these carries ONE fault that the LAST check
# catches (out laid over x): a message about the overlap shows that the limit under test let the job through.
INSIDE = {
    'rows 1': dict(rows=1), 'rows 16896': dict(rows=16896, xs=(16896 * 512, 512, 64), os=(16896 * 512, 512, 64)), '4096 slices': dict(batch=64, heads=64,
                                                                                                                                     xs=(96 * 4096, 4096, 64), os=(96 * 4096, 4096, 64)),
    'one slice': dict(batch=1, heads=1), 'packed layout': dict(xs=(8 * 96 * 64, 64, 96 * 64), os=(8 * 96 * 64, 64, 96 * 64)),
    'zero batch stride': dict(batch=1, xs=(0, 512, 64)), 'wide table': dict(ts=4096), 'table stride 68': dict(ts=68), 'gapped strides': dict(xs=(96 * 600, 600, 72)),
}


@pytest.mark.parametrize('what', sorted(BAD_JOB))
def test_a_job_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _apply(lib, [_job(**BAD_JOB[what])])
    assert rc == R.E_INVALID and msg.startswith('rope_apply: job 0: '), (what, rc, msg)
    rc, msg = _apply(lib, [_job(out=0x5000000), _job(x=0x7000000, out=0x8000000), _job(**BAD_JOB[what])])
    assert rc == R.E_INVALID and msg.startswith('rope_apply: job 2: '), (what, rc, msg)


@pytest.mark.parametrize('what', sorted(BAD_CALL))
def test_a_call_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _apply(lib, [_job()] * 4, **BAD_CALL[what])
    assert rc == R.E_INVALID and msg.startswith('rope_apply: ') and 'job 0' not in msg, (what, rc, msg)


def test_null_jobs_and_d128_strides(lib):
    rc, msg = _apply(lib, [], n_jobs=1)
    assert rc == R.E_INVALID and 'NULL' in msg
    rc, msg = _apply(lib, [_job()], d=128)                                   # head stride 64 below d = 128
    assert rc == R.E_INVALID and 'below the head dim 128' in msg
    rc, msg = _apply(lib, [_job(xs=(96 * 1024, 1024, 128), os=(96 * 1024, 1024, 128), ts=64)], d=128)
    assert rc == R.E_INVALID and 'table_stride' in msg


@pytest.mark.parametrize('what', sorted(INSIDE))
def test_inside_every_limit_reaches_the_overlap_check(lib, what):
    over = dict(INSIDE[what])
    for dtype in (0, 2):
        rc, msg = _apply(lib, [_job(**dict(over, out=0x100000))], dtype=dtype)
        assert rc == R.E_INVALID and msg == 'rope_apply: job 0: out overlaps x', (what, rc, msg)


# ---- oracle and mutants ----------------------------------------------------------------------------------------------------------------
def test_the_tables_are_flux_tables():
    for d in R.HEAD_DIMS:
        cos, sin = R.case_table(d)
        rows = R.TEXT_ROWS + R.GRID[0] * R.GRID[1]
        assert cos.shape == sin.shape == (rows, d) and cos.dtype == sin.dtype == np.float32 and sum(R.AXES[d]) == d
        assert (cos[:R.TEXT_ROWS + 1] == 1).all() and (sin[:R.TEXT_ROWS + 1] == 0).all(), 'text rows and image cell (0, 0): the identity'
        assert np.array_equal(cos[:, 0::2], cos[:, 1::2]) and np.array_equal(sin[:, 0::2], sin[:, 1::2])
        y, x = 3, 7
        row = R.TEXT_ROWS + y * R.GRID[1] + x
        a1 = R.AXES[d][1]
        first = R.AXES[d][0]
        assert (cos[row, :first] == 1).all()
        assert cos[row, first] == np.float32(np.cos(float(y))) and sin[row, first + a1] == np.float32(np.sin(float(x)))
        assert abs(float(cos[row, first + 2]) - np.cos(y / 10000.0 ** (2 / a1))) < 1e-7


def test_the_case_table_meets_what_it_promises():
    assert len(R.CASES) == 60 == len(set(R.CASES))
    for col, values in ((0, R.ROWS), (1, R.HEADS), (2, R.BATCHES), (5, R.LAYOUTS), (6, R.LAYOUTS), (7, R.OFFSETS), (8, R.REGIMES)):
        for v in values:
            assert {(c[3], c[4]) for c in R.CASES if c[col] == v} == {(d, t) for d in R.HEAD_DIMS for t in ('f16', 'bf16')}, (col, v)
    assert {(c[5], c[6]) for c in R.CASES} == {(a, b) for a in R.LAYOUTS for b in R.LAYOUTS}


@pytest.mark.parametrize('case', R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_the_oracle_is_the_torch_expression_bit_for_bit(case):
    x, cos, sin = R.case_inputs(case)
    got, want = R.rotate(x, cos, sin, case[4], case[7]), R.torch_expression(x, cos, sin, case[4], case[7])
    assert got.dtype == want.dtype == np.uint16 and got.shape == want.shape == x.shape and np.array_equal(got, want)


def test_the_regimes_reach_what_they_are_for():
    inf = {'f16': 0x7C00, 'bf16': 0x7F80}
    seen = dict(inf=0, subnormal=0)
    for case in R.CASES:
        x, cos, sin = R.case_inputs(case)
        out = R.rotate(x, cos, sin, case[4], case[7])
        mag = out & 0x7FFF
        assert (mag <= inf[case[4]]).all(), 'no NaN: every input is finite'
        if case[8] == 'large' and case[0] >= 63:
            assert (mag == inf[case[4]]).any(), R.case_id(case)
            seen['inf'] += 1
        if case[8] == 'subnormal':
            assert (mag < (0x0400 if case[4] == 'f16' else 0x0080)).all() and (mag > 0).any()
            seen['subnormal'] += 1
    assert seen['inf'] >= 8 and seen['subnormal'] == 20


def _applies(mutant, case):
    rows, heads, batch, d, dtype, _, _, first_row, regime = case
    turned = first_row + rows > R.TEXT_ROWS + 1           # a row past the text rows and image cell (0, 0): a table that is not the identity
    if mutant == 'no_row_offset':
        return first_row != 0
    if mutant == 'head_as_row':
        return heads > 1
    return turned                                         # half_split, sin_sign, truncate: an identity row shows none of them


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_every_mutant_differs_in_at_least_one_bit(mutant):
    cases = [c for c in R.CASES if _applies(mutant, c)]
    assert len(cases) >= 20, mutant
    for case in cases:
        x, cos, sin = R.case_inputs(case)
        assert not np.array_equal(R.rotate(x, cos, sin, case[4], case[7], mutant=mutant), R.rotate(x, cos, sin, case[4], case[7])), (mutant, R.case_id(case))


def test_memory_images_round_trip():
    values = np.arange(2 * 5 * 3 * 64, dtype=np.uint16).reshape(2, 5, 3, 64)
    for layout in R.LAYOUTS + ('gapped',):
        strides = R.strides_of(layout, 5, 3, 64)
        flat = R.place(values, strides, fill=0xA5A5)
        assert np.array_equal(R.pick(flat, values.shape, strides), values)
        assert (flat == 0xA5A5).sum() == flat.size - values.size + (values == 0xA5A5).sum()
    assert R.strides_of('interleaved', 5, 3, 64) == (960, 192, 64) and R.strides_of('packed', 5, 3, 64) == (960, 64, 320)


# ---- the T5 row lookup -----------------------------------------------------------------------------------------------------------------
def test_t5_rows_of_words():
    from daam_amd import T5RowTokenizer
    from daam_amd.utils import compute_token_merge_indices
    tok = T5RowTokenizer(FS.FakeSentencePiece())
    prompt = 'a dog and a dogs bench'
    assert FS.FakeSentencePiece().tokenize(prompt) == ['▁a', '▁dog', '▁and', '▁a', '▁dog', 's', '▁bench']
    assert compute_token_merge_indices(tok, prompt, 'dog')[0] == [2]
    assert compute_token_merge_indices(tok, prompt, 'dogs')[0] == [5, 6]
    assert compute_token_merge_indices(tok, prompt, 'bench')[0] == [7]
    assert compute_token_merge_indices(tok, prompt, 'a')[0] == [1, 4]
    assert compute_token_merge_indices(tok, prompt, 'Dog')[0] == [2]
    with pytest.raises(ValueError, match='Search word cat not found in prompt!'):
        compute_token_merge_indices(tok, prompt, 'cat')
    # a marker that is a piece of its own keeps its row: the rows behind it do not move
    assert FS.FakeSentencePiece().tokenize('a dog, a bench') == ['▁a', '▁dog', '▁', ',', '▁a', '▁bench']
    assert len(tok.tokenize('a dog, a bench')) == 6
    assert compute_token_merge_indices(tok, 'a dog, a bench', 'bench')[0] == [6]
    assert compute_token_merge_indices(tok, 'a dog, a bench', 'dog')[0] == [2]


# ---- what trace_flux refuses -----------------------------------------------------------------------------------------------------------
def test_trace_flux_refuses_what_it_cannot_trace():
    import daam_amd
    import _mmdit_standin as M
    from oracle import fake_diffusers as fd
    assert hasattr(daam_amd, 'trace_flux') and daam_amd.trace_flux is daam_amd.FluxHeatMapHooker
    with pytest.raises(ValueError, match='single_transformer_blocks'):
        daam_amd.trace_flux(M.make_pipe())                                   # an SD3-class transformer
    with pytest.raises(ValueError, match='single_transformer_blocks'):
        daam_amd.trace_flux(fd.make_pipe('sd15', mini=True))
    with pytest.raises(ValueError, match='fp16 or bf16'):
        daam_amd.trace_flux(FS.make_pipe(dtype=torch.float32), height=128, width=128)
    with pytest.raises(ValueError, match='head dim 32'):
        daam_amd.trace_flux(FS.make_pipe(dim_head=32), height=128, width=128)
    for kw in (dict(height=100, width=128), dict(height=128, width=72), dict(height=128, width=128, cell=48)):
        with pytest.raises(ValueError, match='whole number of'):
            daam_amd.trace_flux(FS.make_pipe(), **kw)
    with pytest.raises(ValueError, match='cells'):
        daam_amd.trace_flux(FS.make_pipe(), height=2064, width=2048)         # 129 x 128 cells
    with pytest.raises(ValueError, match='blocks'):
        daam_amd.trace_flux(FS.make_pipe(), blocks='triple')
    tc = daam_amd.trace_flux(FS.make_pipe(dim_head=128, heads=1))
    assert tc.grid == (64, 64) and tc.cells == 4096 and tc.state is None and tc.calls_by_kind() == {'double': 0, 'single': 0}
    assert len(tc.module) == 1 + 2 + 2, 'the pipeline, two double-stream and two single-stream blocks'
    for blocks, kinds in (('double', ['double', 'double']), ('single', ['single', 'single'])):
        assert [h.kind for h in daam_amd.trace_flux(FS.make_pipe(), height=128, width=128, blocks=blocks).module[1:]] == kinds
    with pytest.raises(RuntimeError, match='No heat maps'):
        tc.raw_heat_maps()


def test_the_engine_launcher_checks_before_it_loads(monkeypatch):
    from daam_amd import engine as E
    assert E.MAX_ROPE_ROWS == 16896 and E.ROPE_HEAD_DIMS == (64, 128)
    monkeypatch.setattr(E.nat, 'load_rope', lambda: None)
    x = torch.zeros(1, 5, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='jobs'):
        E.rope_apply([], 64)
    with pytest.raises(ValueError, match='head dim'):
        E.rope_apply([(x, x, x, x, 2)], 32)
    with pytest.raises(RuntimeError, match='fp16 or bf16'):
        E.rope_apply([(x.float(), x.float(), x, x, 2)], 64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        E.rope_apply([(x, torch.zeros_like(x), torch.zeros(5, 64), torch.zeros(5, 64), 2)], 64)
    table = E.RopeTable()
    fit = torch.zeros(6, 64)
    assert table.get(fit) is fit and table.get(fit[2:]).data_ptr() == fit[2:].data_ptr() and len(table) == 0
    odd = torch.arange(6 * 64, dtype=torch.float64).view(64, 6).t()
    once = table.get(odd)
    assert once.dtype == torch.float32 and once.is_contiguous() and torch.equal(once, odd.float()) and table.get(odd) is once and len(table) == 1
    table.reset()
    assert len(table) == 0 and table.get(odd) is not once
