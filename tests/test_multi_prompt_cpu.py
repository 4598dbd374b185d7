"""Host-side pieces of batched-prompt tracing: the prompt -> key-group table, the argument checks, the C ABI declaration and
the machine code of the single-prompt finalize kernels."""
import json
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prompt_key_groups_hand_table():
    from daam_amd.engine import prompt_key_groups
    # two layers: layer 0 (factor 2) keeps 4 keys at offset 0, layer 3 (factor 4) keeps 8 keys at offset 4
    layout = [(0, 0, 2, 4), (3, 4, 4, 8)]
    assert prompt_key_groups(layout, 12, 1) == [0] * 12
    assert prompt_key_groups(layout, 12, 2) == [0, 0, 1, 1] + [0] * 4 + [1] * 4
    assert prompt_key_groups(layout, 12, 4) == [0, 1, 2, 3] + [0, 0, 1, 1, 2, 2, 3, 3]
    # head_idx counts inside a prompt's block (k = 2 images per prompt: block = 2 H)
    assert prompt_key_groups(layout, 12, 2, head_idx=1) == [-1, 0, -1, 1] + [-1, 0, -1, -1, -1, 1, -1, -1]
    assert prompt_key_groups(layout, 12, 2, layer_idx=3) == [-1] * 4 + [0] * 4 + [1] * 4
    assert prompt_key_groups(layout, 12, 2, factors=[2]) == [0, 0, 1, 1] + [-1] * 8
    assert prompt_key_groups(layout, 12, 4, factors=[4], head_idx=0) == [-1] * 4 + [0, -1, 1, -1, 2, -1, 3, -1]
    with pytest.raises(ValueError, match='not divisible'):
        prompt_key_groups(layout, 12, 3)


def _bare_trace(prompts, encode=None):
    from daam_amd.trace import DiffusionHeatMapHooker
    t = DiffusionHeatMapHooker.__new__(DiffusionHeatMapHooker)
    t.last_prompts, t.last_prompt = list(prompts), prompts[0]
    t._encode_args, t._batch_unchecked, t.batch_prompts = encode, True, True
    t.pipe = types.SimpleNamespace(tokenizer=None)
    return t


def test_batch_and_prompt_idx_errors():
    t = _bare_trace(['a', 'b'])
    t._check_batch(4)
    t._check_batch(8)                                           # k = 2
    with pytest.raises(ValueError, match='does not divide.*2 prompt'):
        t._check_batch(6)
    with pytest.raises(ValueError, match='without classifier-free guidance'):
        _bare_trace(['a', 'b'], encode=(1, False))._check_batch(4)
    with pytest.raises(ValueError, match='not 2 x 2 prompts x 2 images'):
        _bare_trace(['a', 'b'], encode=(2, True))._check_batch(4)
    with pytest.raises(ValueError, match='pass prompt_idx'):
        t.compute_global_heat_map()
    for bad in (2, -1, 'x'):
        with pytest.raises(ValueError, match='out of range'):
            t.compute_global_heat_map(prompt_idx=bad)


def test_single_prompt_batch_check_is_a_no_op():
    """One prompt under batch_prompts=True: any batch passes, with or without guidance (no-CFG batch 1, odd k)."""
    for batch in (1, 2, 3, 4):
        _bare_trace(['a dog'])._check_batch(batch)
        _bare_trace(['a dog'], encode=(3, False))._check_batch(batch)


def test_header_declares_finalize_groups():
    from daam_amd import _native
    src = open(os.path.join(ROOT, 'include', 'daam_hip.h')).read()
    assert 'daam_finalize_groups' in _native.EXPORTS
    assert 'DAAM_API int daam_finalize_groups(DaamCtx* ctx, const int32_t* key_group, int n_groups, const int32_t* n_rows,' in src
    assert '#define DAAM_ABI_VERSION 6' in src


def test_single_prompt_kernels_keep_their_machine_code():
    """Every kernel fingerprint of profiles/r06_counters.json is in a fresh build unchanged; the grouped finalize kernels are
    there under their own fingerprints."""
    from daam_amd import build
    build.build(verbose=False)
    have = build.kernel_shas()
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'r06_counters.json')))['kernel_shas']
    assert {k: have.get(k) for k in rec} == rec
    grouped = {k: v for k, v in have.items() if 'grouped_kernel' in k}
    for kind in ('finalize_grouped_kernel', 'finalize_same_grouped_kernel', 'finalize_up_grouped_kernel',
                 'finalize_down2_grouped_kernel', 'finalize_up32_pipe_grouped_kernel'):
        assert sum(kind in k for k in grouped) >= 3, kind
    assert not set(grouped.values()) & set(rec.values())


def test_c_program_links_finalize_groups(tmp_path):
    import subprocess
    from daam_amd import build
    lib = build.build(verbose=False)
    src = tmp_path / 'm.c'
    src.write_text('#include "daam_hip.h"\nint main(void) { int (*f)(DaamCtx*, const int32_t*, int, const int32_t*, float*, size_t, void*) = '
                   'daam_finalize_groups; return f(0, 0, 1, 0, 0, 0, 0) == DAAM_E_INVALID ? 0 : 1; }\n')
    exe = tmp_path / 'm'
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), str(src), lib,
                    '-Wl,-rpath,' + os.path.dirname(lib), '-o', str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
