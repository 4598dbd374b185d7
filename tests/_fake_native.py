"""Shared by the CPU tests that drive ``HeatMapEngine`` without a GPU (``test_host_logic.py``, ``test_time_bins_cpu.py``,
``test_probes_cpu.py``, ``test_engine_calls_cpu.py``): one recording stand-in of ``libdaam_hip`` and the fixture that puts it,
a stream stub and a CPU "device" under the engine.  Test-only: the product has no fallback."""
import contextlib
import ctypes

import pytest
import torch


class FakeLib:
    """Records ``(name, args)`` of every ``daam_*`` call and returns 0.  It hands out contexts (``daam_ctx_create`` /
    ``daam_ctx_create_rect``), copies the arrays of ``daam_tap_qk_enqueue_many`` while they are alive (``enqueued``: one list of
    ``(layer, q, k, bytes of the DaamQKDesc)`` per call) and answers ``daam_key_offset`` as the C function does, from the slots
    that ``daam_layer_configure`` / ``_rect`` / ``daam_layer_release`` left configured, and ``daam_tap_steps`` from the taps it was
    handed since the last ``daam_reset`` (recorded ones count when they are enqueued, as in the library)."""

    def __init__(self):
        self.calls, self.enqueued = [], []
        self.contexts = []                                 # handle values, in creation order
        self.heads = {}                                    # handle -> {configured slot: heads}
        self.steps = {}                                    # handle -> {layer: taps since daam_reset}

    def _create(self, out):
        handle = 1234 + len(self.contexts)
        self.contexts.append(handle)
        self.heads[handle] = {}
        self.steps[handle] = {}
        out._obj.value = handle

    def _key_offset(self, ctx, layer, offset, total):
        heads = self.heads[ctx.value]
        if offset is not None:
            offset._obj.value = sum(h for slot, h in heads.items() if slot < layer)
        if total is not None:
            total._obj.value = sum(heads.values())

    def _count(self, ctx, layer):
        steps = self.steps[ctx.value]
        steps[layer] = steps.get(layer, 0) + 1

    def _enqueue_many(self, ctx, n, layers, q, k, desc):
        from daam_amd import _native as nat

        def arr(t, a):
            return list((t * n).from_address(a if isinstance(a, int) else ctypes.addressof(a)))
        u64 = ctypes.c_uint64
        for layer in arr(ctypes.c_int32, layers):
            self._count(ctx, layer)
        self.enqueued.append([(l, qq, kk, bytes(nat.QKDesc.from_address(dd)))
                              for l, qq, kk, dd in zip(arr(ctypes.c_int32, layers), arr(u64, q), arr(u64, k), arr(u64, desc))])

    def __getattr__(self, name):
        if not name.startswith('daam_'):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name in ('daam_ctx_create', 'daam_ctx_create_rect'):
                self._create(args[-1])
            elif name in ('daam_layer_configure', 'daam_layer_configure_rect'):
                self.heads[args[0].value][args[1]] = args[2]
            elif name == 'daam_layer_release':
                self.heads[args[0].value].pop(args[1], None)
            elif name == 'daam_key_offset':
                self._key_offset(*args)
            elif name == 'daam_tap_qk_enqueue_many':
                self._enqueue_many(*args)
            # include/daam_hip.h: daam_tap_qk(ctx, layer, ...), daam_tap_probs(ctx, layer, ...),
            # daam_attend(ctx, layer, q, k, v, out, desc, tap, stream): args[7] is ``tap`` (the call feeds the sums)
            elif name in ('daam_tap_qk', 'daam_tap_probs') or (name == 'daam_attend' and args[7]):
                self._count(args[0], args[1])
            elif name == 'daam_reset':
                self.steps[args[0].value] = {}
            elif name == 'daam_tap_steps':                 # daam_tap_steps(ctx, layer, int* steps)
                args[2]._obj.value = self.steps[args[0].value].get(args[1], 0)
            return 0
        return fn

    def names(self):
        return [c[0] for c in self.calls]


class FakeStream:
    cuda_stream = 0

    def wait_stream(self, other):
        pass

    def wait_event(self, ev):
        pass

    def record_event(self):
        return object()


def install(setattr_):
    """Put a ``FakeLib`` under ``daam_amd.engine`` through ``setattr_`` (``monkeypatch.setattr``): returns ``(engine module, lib)``."""
    from daam_amd import engine as E
    lib = FakeLib()
    one = FakeStream()
    setattr_(E.nat, 'load', lambda: lib)
    setattr_(E.HeatMapEngine, '_require_device', lambda self, t: setattr(self, 'device', torch.device('cpu')))
    setattr_(E.HeatMapEngine, '_current_stream', lambda self: one)
    setattr_(torch.cuda, 'device', lambda d: contextlib.nullcontext())
    return E, lib


@pytest.fixture
def fake_engine(monkeypatch):
    E, lib = install(monkeypatch.setattr)
    E._PARKED.clear()
    yield E, lib
    E._PARKED.clear()
