"""The engine's conversation with ``libdaam_hip``, pinned: every scenario below drives ``HeatMapEngine`` on CPU tensors against
the recording stand-in (``tests/_fake_native.py``) and the calls it makes -- names, scalar arguments, decoded arrays and
descriptors, pointers as "which tensor + byte offset" -- must equal ``tests/golden/engine_calls.json`` in order and in arguments.
``daam_key_offset`` is left out: a host-side getter with no effect, which a table builder may ask as often as it likes.

The golden file is a record of the engine as it was BEFORE the host layer was reorganised (the commit that added this test); it is
the reference for every later change of ``daam_amd/engine.py`` that claims to change no behaviour.  ``python
tests/test_engine_calls_cpu.py --record`` rewrites it -- only for a change that means to alter what the library is asked for."""
import ctypes
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _fake_native import fake_engine, install  # noqa: E402,F401 -- fake_engine is the fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'engine_calls.json')
F16 = torch.float16


# ---- pointers -> stable labels -----------------------------------------------------------------------------------------
class Names:
    """Every tensor whose address may reach the library, by name.  The tensors are kept alive until the transcript is written, so
    no address is used twice."""

    def __init__(self):
        self.spans = []                                    # (first byte, end, name, tensor)

    def add(self, name, t):
        st = t.untyped_storage()
        if not any(s[0] == st.data_ptr() for s in self.spans):
            self.spans.append((st.data_ptr(), st.data_ptr() + max(st.nbytes(), 1), name, t))
        return t

    def engine(self, tag, eng):
        """The sum buffers ``eng`` holds now (``tag.acc<slot>``, a later buffer of the same slot ``tag.acc<slot>'``)."""
        for slot, buf in sorted(eng.acc.items()):
            name = f'{tag}.acc{slot}'
            while any(s[2] == name and s[0] != buf.untyped_storage().data_ptr() for s in self.spans):
                name += "'"
            self.add(name, buf)

    def label(self, addr):
        for a, b, name, _ in self.spans:
            if a <= addr < b:
                return name if addr == a else f'{name}+{addr - a}'
        raise AssertionError(f'pointer {addr:#x} belongs to no named tensor')


def _fields(s, names):
    return {f: _value(getattr(s, f), names, None) for f, _ in s._fields_}


def _value(a, names, lib):
    if a is None or isinstance(a, (bool, float, str)):
        return a
    if isinstance(a, int):
        return names.label(a) if a >= 1 << 32 else a       # heap addresses; every scalar of the ABI is far smaller
    if isinstance(a, ctypes.c_void_p):
        return f'ctx{lib.contexts.index(a.value)}'
    if isinstance(a, ctypes.Structure):
        return _fields(a, names)
    if isinstance(a, ctypes.Array):
        return list(a)
    if hasattr(a, '_obj'):                                 # byref(...)
        obj = a._obj
        return _fields(obj, names) if isinstance(obj, ctypes.Structure) else '&' + type(obj).__name__
    raise AssertionError(f'argument {a!r} of a type the transcript does not know')


def transcript(lib, names):
    from daam_amd import _native as nat
    out, many = [], iter(lib.enqueued)
    for name, args in lib.calls:
        if name == 'daam_key_offset':
            continue
        if name == 'daam_tap_qk_enqueue_many':
            rows = next(many)
            assert args[1] == len(rows)
            out.append([name, _value(args[0], names, lib), args[1],
                        [[layer, names.label(q), names.label(k), _fields(nat.QKDesc.from_buffer_copy(d), names)]
                         for layer, q, k, d in rows]])
        else:
            out.append([name] + [_value(a, names, lib) for a in args])
    return out


# ---- scenarios -----------------------------------------------------------------------------------------------------------
def _qk(names, tag, n_layers, batch=2, hw=64, channels=16):
    q = [names.add(f'{tag}.q{i}', torch.zeros(batch, hw, channels, dtype=F16)) for i in range(n_layers)]
    k = [names.add(f'{tag}.k{i}', torch.zeros(batch, 77, channels, dtype=F16)) for i in range(n_layers)]
    return q, k


def _steps(eng, q, k, steps, order=(2, 0, 1), heads=2, factors=(1, 1, 2)):
    for _ in range(steps):
        for layer in order:
            eng.tap_qk(layer, q[layer], k[layer], heads, 0.25, factors[layer])


def _lookup_error(fn, *a, **kw):
    with pytest.raises(LookupError, match='no heat maps'):
        fn(*a, **kw)


def deferred(E, names):
    """Five steps in execution order (2, 0, 1) at two steps per launch; the finalize on a cache miss (with the pending taps), on a
    hit, filtered, and on a selection that matches no key (flush, then LookupError)."""
    eng = E.HeatMapEngine(3, defer_steps=2)
    q, k = _qk(names, 'd', 3)
    _lookup_error(eng.global_heat_map)                                     # nothing tapped: no call at all
    _steps(eng, q, k, 5)
    names.engine('d', eng)
    out = [eng.global_heat_map(), eng.global_heat_map()]
    out += [eng.global_heat_map(factors=[1]), eng.global_heat_map(head_idx=1), eng.global_heat_map(layer_idx=2),
            eng.global_heat_map(n_rows=9), eng.global_heat_map(factors=[2, 1], head_idx=0, layer_idx=0, n_rows=200)]
    _steps(eng, q, k, 1)
    _lookup_error(eng.global_heat_map, factors=[2], layer_idx=1)           # the pending step is launched first
    _lookup_error(eng.global_heat_map, head_idx=5)
    assert eng.keys() == [(2, 2, 0), (2, 2, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
    for i, t in enumerate(out):
        names.add(f'd.out{i}', t)
    eng.close()


def batched(E, names):
    """Two prompts in one batch (B = 4: two kept batch entries of two heads per layer)."""
    eng = E.HeatMapEngine(3, defer_steps=2)
    q, k = _qk(names, 'b', 3, batch=4)
    _lookup_error(eng.global_heat_maps, 2, [5, 9])
    _steps(eng, q, k, 3)
    names.engine('b', eng)
    out = [eng.global_heat_maps(2, [5, 9]), eng.global_heat_maps(2, [5, 9]),
           eng.global_heat_maps(2, [5, 100], factors=[1], head_idx=1), eng.global_heat_maps(2, [0, 9], layer_idx=2)]
    _steps(eng, q, k, 1)
    _lookup_error(eng.global_heat_maps, 2, [5, 9], head_idx=2)
    with pytest.raises(ValueError, match='row counts'):
        eng.global_heat_maps(2, [5])
    assert eng.key_groups(2) == [0, 0, 1, 1] * 3
    for i, t in enumerate(out):
        names.add(f'b.out{i}', t)
    eng.close()


def windows(E, names):
    """``time_bins``: the binned redirects of ``global_heat_map`` / ``global_heat_maps``, 90 groups in two calls, the views."""
    eng = E.HeatMapEngine(3, defer_steps=4, time_bins=[0, 2, 4])
    q, k = _qk(names, 'w', 3, batch=4)
    _steps(eng, q, k, 5)
    names.engine('w', eng)
    out = [eng.global_heat_map(bins=(1, 3), n_rows=9), eng.global_heat_map(head_idx=0),
           eng.global_heat_maps(2, [5, 9], bins=(0, 2)), eng.global_heat_maps(2, [5, 9], factors=[2]),
           eng.time_heat_maps([(w, w + 1, 0) for w in range(3)] * 30, 1, [77]),
           eng.time_heat_maps([(0, 3, 1), (1, 2, 0)], 2, [7, 300], layer_idx=1)]
    _steps(eng, q, k, 1)
    _lookup_error(eng.time_heat_maps, [(0, 1, 0)], 1, [77], factors=[4])
    _steps(eng, q, k, 1)
    views = eng.window_items(1)
    assert list(views) == eng.keys() and views[(2, 2, 1)].data_ptr() == eng.acc[2][1][1].data_ptr()
    for i, t in enumerate(out):
        names.add(f'w.out{i}', t)
    eng.close()


def probes(E, names):
    """Two probes on a batch of two prompts: the deferred launch's probe chains, the grouped finalize, the views."""
    eng = E.HeatMapEngine(3, defer_steps=2, n_probes=2)
    q, k = _qk(names, 'p', 3, batch=4)
    for layer in range(3):
        eng.set_probe_keys(layer, names.add(f'p.probe_k{layer}', torch.zeros(2, 77, 16, dtype=F16)))
    _steps(eng, q, k, 3)
    names.engine('p', eng)
    out = [eng.probe_heat_maps([0, 1], 2, [4, 6]), eng.probe_heat_maps([0, 1], 2, [4, 6]), eng.probe_heat_maps([1], 2, [90], head_idx=0),
           eng.probe_heat_maps([1, 0], 2, [4, 6], factors=[1], layer_idx=1)]
    _steps(eng, q, k, 1)
    _lookup_error(eng.probe_heat_maps, [0], 2, [4], layer_idx=1, factors=[2])
    _steps(eng, q, k, 1)
    views = eng.probe_items(1)
    assert list(views) == eng.keys() and views[(1, 0, 3)].data_ptr() == eng.acc[eng.probe_slot(1, 0)][3].data_ptr()
    for i, t in enumerate(out):
        names.add(f'p.out{i}', t)
    eng.close()


def probes_72_groups(E, names):
    """8 probes x 9 prompts (one head, B = 18): 72 groups, two ``daam_finalize_groups`` calls."""
    eng = E.HeatMapEngine(1, defer_steps=2, n_probes=8)
    q, k = _qk(names, 'g', 1, batch=18, channels=8)
    eng.set_probe_keys(0, names.add('g.probe_k0', torch.zeros(8, 77, 8, dtype=F16)))
    _steps(eng, q, k, 1, order=(0,), heads=1)
    names.engine('g', eng)
    names.add('g.out0', eng.probe_heat_maps(list(range(8)), 9, [3, 4, 5, 6, 7, 8, 9, 10]))
    eng.close()


def probes_immediate(E, names):
    """``tap_probes`` on an immediate trace, and on a deferred one (which launches what is recorded first)."""
    eng = E.HeatMapEngine(3, defer_steps=0, n_probes=2)
    q, k = _qk(names, 'i', 3)
    for layer in (1, 2):
        eng.set_probe_keys(layer, names.add(f'i.probe_k{layer}', torch.zeros(2, 77, 16, dtype=F16)))
        eng.tap_qk(layer, q[layer], k[layer], 2, 0.25, 1)
        eng.tap_probes(layer, q[layer], 2, 0.25, 1)
        eng.tap_probes(layer, q[layer], 2, 0.5, 1, round_logits=False)
    names.engine('i', eng)
    eng.close()
    eng = E.HeatMapEngine(3, defer_steps=2, n_probes=2)
    eng.set_probe_keys(0, names.add('j.probe_k0', torch.zeros(2, 77, 16, dtype=F16)))
    eng.tap_qk(0, q[0], k[0], 2, 0.25, 1)
    eng.tap_probes(0, q[0], 2, 0.25, 1)
    names.engine('j', eng)
    eng.close()


def immediate(E, names):
    """``defer_steps=0``: ``tap_qk``, ``attend`` with the tap fused, ``attend`` declined, ``tap_probs`` and ``add_map``."""
    eng = E.HeatMapEngine(3, defer_steps=0)
    q, k = _qk(names, 'm', 3)
    v = names.add('m.v', torch.zeros(2, 77, 16, dtype=F16))
    eng.tap_qk(2, q[2], k[2], 2, 0.25, 1)
    eng.tap_qk(2, q[2], k[2], 2, 0.25, 1, round_logits=False)
    names.add('m.attend0', eng.attend(0, q[0], k[0], v, 2, 0.25, 1, True, True))          # head_dim 8: taken, tap fused
    names.add('m.attend1', eng.attend(0, q[0], k[0], v, 2, 0.25, 8, True, False))         # not tapped: attends only
    assert eng.attend(1, q[1], k[1], v, 4, 0.5, 1, True, True) is None                    # head_dim 4: declined, no call
    probs = names.add('m.probs', torch.zeros(4, 64, 77, dtype=F16))
    eng.tap_probs(1, probs, 1)
    eng.add_map(1, 1, 0, torch.zeros(77, 8, 8, dtype=F16))
    names.engine('m', eng)
    names.add('m.out0', eng.global_heat_map(n_rows=4))
    assert eng.touched == [2, 0, 1]
    eng.close()


def nonsquare(E, names):
    """An 8 x 12 map: the ``_rect`` entry points, no ``daam_finalize_prepare`` (flush, then ``daam_finalize``)."""
    eng = E.HeatMapEngine(3, defer_steps=2, out_hw=(8, 12))
    q = [names.add('r.q0', torch.zeros(2, 96, 16, dtype=F16)), names.add('r.q1', torch.zeros(2, 24, 16, dtype=F16))]
    k = [names.add(f'r.k{i}', torch.zeros(2, 77, 16, dtype=F16)) for i in range(2)]
    for _ in range(3):
        eng.tap_qk(1, q[1], k[1], 2, 0.25, 2)
        eng.tap_qk(0, q[0], k[0], 2, 0.25, 1)
    names.engine('r', eng)
    assert eng.layer_info[0] == (1, 2, (8, 12)) and eng.layer_info[1] == (2, 2, (4, 6))
    out = names.add('r.out0', eng.global_heat_map(n_rows=9))
    assert tuple(out.shape) == (9, 8, 12)
    eng.normalize_(out)
    names.add('r.out1', eng.global_heat_map(factors=[2]))
    names.add('r.out2', eng.global_heat_maps(1, [9]))
    eng.close()
    sq = E.HeatMapEngine(1, defer_steps=0, out_hw=(8, 8))                  # equal sides: the square names
    sq.tap_qk(0, names.add('r.q2', torch.zeros(2, 64, 16, dtype=F16)), k[0], 2, 0.25, 1)
    names.engine('s', sq)
    sq.normalize_(names.add('r.out3', sq.global_heat_map(n_rows=2)))
    sq.close()


def lifetime(E, names):
    """Views handed out, ``clear()`` (release), the next generation on new buffers; ``close()`` parks, a second engine adopts."""
    eng = E.HeatMapEngine(3, defer_steps=2, reuse_context=True)
    q, k = _qk(names, 'l', 3)
    _steps(eng, q, k, 3)
    names.engine('l', eng)
    views = list(eng.items())
    eng.clear()
    assert not eng.acc and not eng.layer_info
    _steps(eng, q, k, 1)
    names.engine('l', eng)
    eng.clear()                                                             # no views out: the buffers stay
    _steps(eng, q, k, 1)
    eng.close()                                                             # parked with one step recorded and dropped
    two = E.HeatMapEngine(3, defer_steps=2, reuse_context=True)
    _steps(two, q, k, 1)
    names.engine('l', two)
    names.add('l.out0', two.global_heat_map())
    two.close()
    E.release_parked_contexts()
    assert len(views) == 6


SCENARIOS = {'deferred[c++]': deferred, 'deferred[python]': deferred, 'batched': batched, 'windows': windows, 'probes[c++]': probes,
             'probes[python]': probes, 'probes_72_groups': probes_72_groups, 'probes_immediate': probes_immediate,
             'immediate': immediate, 'nonsquare': nonsquare, 'lifetime': lifetime}


def run(name, monkeypatch):
    E, lib = install(monkeypatch.setattr)
    E._PARKED.clear()
    if name.endswith('[python]'):
        monkeypatch.setenv('DAAM_NO_FASTPATH', '1')
    else:
        monkeypatch.delenv('DAAM_NO_FASTPATH', raising=False)
    monkeypatch.delenv('DAAM_CHECK_VERSIONS', raising=False)
    monkeypatch.delenv('DAAM_NO_CTX_POOL', raising=False)
    names = Names()
    SCENARIOS[name](E, names)
    E._PARKED.clear()
    return json.loads(json.dumps(transcript(lib, names)))


@pytest.mark.parametrize('name', list(SCENARIOS))
def test_engine_calls_match_the_recorded_transcript(name, monkeypatch):
    want = json.load(open(GOLDEN))['scenarios'][name]
    got = run(name, monkeypatch)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'{name}: call {i} differs'
    assert [c[0] for c in got] == [c[0] for c in want]


def test_both_recorders_ask_for_the_same_work():
    golden = json.load(open(GOLDEN))['scenarios']
    for name in ('deferred', 'probes'):
        assert golden[f'{name}[c++]'] == golden[f'{name}[python]']


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: python tests/test_engine_calls_cpu.py --record')
    scenarios = {}
    for scenario in SCENARIOS:
        with pytest.MonkeyPatch.context() as mp:
            scenarios[scenario] = run(scenario, mp)
    with open(GOLDEN, 'w') as f:
        f.write('{"what": "calls HeatMapEngine makes to libdaam_hip in the scenarios of tests/test_engine_calls_cpu.py '
                '(daam_key_offset left out)",\n "scenarios": {\n')
        f.write(',\n'.join(f'  {json.dumps(s)}: [\n' + ',\n'.join('   ' + json.dumps(c) for c in calls) + '\n  ]'
                           for s, calls in scenarios.items()))
        f.write('\n }\n}\n')
    print({s: len(c) for s, c in scenarios.items()})
