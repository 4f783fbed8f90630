"""The red-zone harness (tests/redzone.py) on CPU tensors: what the patched allocators hand out, what passes through, and
that damage to a band or to a `const` operand is reported by entry point, operand, side and offset."""
import ctypes
import types

import pytest
import torch

import redzone as RZ
from gemnet_pytorch_amd import _lib

BAND = RZ.BAND


@pytest.fixture
def rz():
    with RZ.guard("cpu") as g:
        yield g


def _arena_of(g, t):
    a = g.find(t.data_ptr())
    assert a is not None and a.lo == t.data_ptr() and a.n == t.numel() * t.element_size()
    return a


def test_band_is_as_the_harness_promises():
    assert BAND >= 128 * 1024 and BAND % 512 == 0 and BAND > 80 * 128 * 4


def test_patched_allocators_return_what_the_real_ones_would(rz):
    src = torch.zeros(3, 5, dtype=torch.float64)
    made = {
        "empty": (torch.empty(4, 3), (4, 3), torch.float32, None),
        "empty tuple": (torch.empty((2, 7), dtype=torch.int32), (2, 7), torch.int32, None),
        "empty size kw": (torch.empty(size=(2, 2), device="cpu"), (2, 2), torch.float32, None),
        "zeros": (torch.zeros(5, dtype=torch.int64), (5,), torch.int64, 0),
        "zeros grad": (torch.zeros(2, 3, requires_grad=True), (2, 3), torch.float32, 0),
        "ones": (torch.ones((3, 1, 2), dtype=torch.float64), (3, 1, 2), torch.float64, 1),
        "full float": (torch.full((3,), 2.5), (3,), torch.float32, 2.5),
        "full int": (torch.full((3, 2), 7), (3, 2), torch.int64, 7),
        "full bool": (torch.full((4,), True), (4,), torch.bool, True),
        "full dtype": (torch.full((4,), 3, dtype=torch.float32), (4,), torch.float32, 3),
        "full kw": (torch.full(size=(2,), fill_value=-1.5, dtype=torch.float64), (2,), torch.float64, -1.5),
        "empty_like": (torch.empty_like(src), (3, 5), torch.float64, None),
        "zeros_like grad": (torch.zeros_like(src, requires_grad=True), (3, 5), torch.float64, 0),
        "ones_like dtype": (torch.ones_like(src, dtype=torch.int32), (3, 5), torch.int32, 1),
        "full_like": (torch.full_like(src, 4.0), (3, 5), torch.float64, 4.0),
        "full_like kw": (torch.full_like(src, fill_value=2), (3, 5), torch.float64, 2),
        "new_empty": (src.new_empty((2, 2)), (2, 2), torch.float64, None),
        "new_empty ints": (src.new_empty(2, 3), (2, 3), torch.float64, None),
        "new_zeros": (src.new_zeros((6,), dtype=torch.int32), (6,), torch.int32, 0),
        "new_ones": (src.new_ones(2, 2), (2, 2), torch.float64, 1),
        "new_full": (src.new_full((3,), 9.0), (3,), torch.float64, 9.0),
        "scalar": (torch.zeros(()), (), torch.float32, 0),
    }
    for name, (t, shape, dtype, value) in made.items():
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cpu" and t.is_contiguous(), name
        assert t.requires_grad == ("grad" in name) and t.is_leaf and not t._is_view(), name
        assert t.data_ptr() % 64 == 0, name           # the arena is as aligned as the allocator makes it; the band adds a multiple of 512
        _arena_of(rz, t)
        if value is not None:
            assert bool((t == value).all()), name
    assert rz.n_guarded == len(made) + 1               # + src
    # a guarded tensor behaves: autograd through it, in-place writes, views
    w = torch.zeros(3, requires_grad=True)
    (w * torch.ones(3)).sum().backward()
    assert torch.equal(w.grad, torch.ones(3))


def test_empty_payloads_are_nan_or_minus_one(rz):
    assert torch.isnan(torch.empty(7, 3)).all() and torch.isnan(torch.empty(5, dtype=torch.float64)).all()
    assert bool((torch.empty(9, dtype=torch.int32) == -1).all()) and bool((torch.empty(9, dtype=torch.int64) == -1).all())
    assert torch.isnan(torch.empty_like(torch.zeros(4))).all() and torch.isnan(torch.zeros(2).new_empty(3)).all()
    for band in _arena_of(rz, torch.empty(3)).bands():
        assert band.numel() == BAND and bool((band == 0xFF).all())


def test_pass_through_cases_pass_through(rz):
    out, m = torch.zeros(4), torch.zeros(4, 6)
    n = rz.n_guarded
    outside = [torch.empty(3, device="meta"), torch.ones(4, out=out), torch.empty(0, 5), torch.zeros((2, 0)),
               torch.empty_like(m.t()), torch.zeros_like(m[:, ::2]),
               torch.empty(2, 3, 4, 5, memory_format=torch.channels_last), torch.zeros(3, dtype=torch.int8, device="meta"),
               out.new_empty((0,)), torch.empty_like(torch.zeros(0)), torch.full((2,), torch.tensor(3.0)),
               torch.zeros(2, 2, layout=torch.sparse_coo)]
    assert rz.n_guarded == n and all(rz.find(t.data_ptr()) is None for t in outside if t.layout == torch.strided and t.numel() and t is not out)
    assert outside[0].device.type == "meta" and outside[1] is out and tuple(outside[4].stride()) == (1, 6)
    assert float(outside[10][0]) == 3.0 and outside[11].layout == torch.sparse_coo
    with pytest.raises(TypeError):
        torch.empty(3, no_such_keyword=1)


def test_allocators_are_restored_and_arenas_released():
    before = (torch.empty, torch.full_like, torch.Tensor.new_zeros, "new_zeros" in torch.Tensor.__dict__)
    with RZ.guard("cpu") as g:
        assert torch.empty is not before[0] and _lib.TRACE is g
        t = torch.empty(3)
    assert (torch.empty, torch.full_like, torch.Tensor.new_zeros, "new_zeros" in torch.Tensor.__dict__) == before
    assert _lib.TRACE is None and not g.arenas and torch.isnan(t).all()
    assert not torch.isnan(torch.zeros(3)).any() and RZ.put(torch.ones(2), device="cpu").device.type == "cpu"


def test_put_copies_into_a_guarded_arena(rz):
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()          # a non-contiguous host tensor
    y = RZ.put(x)
    assert torch.equal(y, x) and y.is_contiguous() and _arena_of(rz, y).what == "put"
    assert RZ.put(torch.zeros(0, 3)).shape == (0, 3)
    assert RZ.put(torch.ones(2, requires_grad=True)).requires_grad


@pytest.mark.parametrize("side,elem,offset", [("after band", 6, 0), ("before band", -1, -4)])
def test_one_element_write_outside_a_payload_is_reported_at_exit(side, elem, offset):
    with pytest.raises(RZ.RedzoneError, match=rf"at exit.*{side} damaged, first byte at offset {offset}$"):
        with RZ.guard("cpu") as g:
            t = torch.zeros(2, 3)
            a = _arena_of(g, t)
            everything = a.buf.view(torch.float32)                       # the arena: band | payload | band
            torch.as_strided(everything, (1,), (1,), BAND // 4 + elem)[0] = 1.0


def _fake_lib(fn):
    """Stand-in for the loaded library: a Python function under a real entry point's name, so that _abi's kinds apply."""
    return types.SimpleNamespace(gn_gather_rows_f32=fn, gn_abi_version=lambda: 0)


def _gather(scribble=None):
    """gn_gather_rows_f32(const float* x, const int* idx, float* y, int T, int C, stream) on host memory."""
    def fn(x, idx, y, T, C, stream):
        f, i = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
        xs, ids, ys = ctypes.cast(x, f), ctypes.cast(idx, i), ctypes.cast(y, f)
        for t in range(T):
            for c in range(C):
                ys[t * C + c] = xs[ids[t] * C + c]
        if scribble == "x":
            xs[1] = 5.0
        return 0
    return fn


def _call(g, fn, x, idx, y, T):
    lib = g.proxy(_fake_lib(fn))
    assert lib.gn_abi_version() == 0                                     # not a launch: handed through
    return lib.gn_gather_rows_f32(_lib.ptr(x), _lib.ptr(idx), _lib.ptr(y), T, x.shape[1], None)


def test_a_clean_call_is_silent_and_counted(rz):
    x, idx, y = RZ.put(torch.randn(5, 3)), RZ.put(torch.tensor([4, 0, 2], dtype=torch.int32)), torch.empty(3, 3)
    assert _call(rz, _gather(), x, idx, y, 3) == 0
    assert torch.equal(y, x[[4, 0, 2]]) and rz.n_launches == 1 and rz.n_operands == 3
    plain = torch.from_numpy(torch.randn(5, 3).numpy().copy())           # an operand the harness does not own: ignored
    assert rz.find(plain.data_ptr()) is None and _call(rz, _gather(), plain, idx, y, 3) == 0 and rz.n_operands == 5


def test_a_launch_that_writes_past_its_output_is_reported_by_name(rz):
    x, idx, y = RZ.put(torch.randn(5, 3)), RZ.put(torch.tensor([4, 0, 2], dtype=torch.int32)), torch.empty(2, 3)
    with pytest.raises(RZ.RedzoneError, match=r"gn_gather_rows_f32: operand y \(torch.empty, 24 B payload\): after band "
                                              r"damaged, first byte at offset 0$"):
        _call(rz, _gather(), x, idx, y, 3)                                # T is one more than y has rows


def test_a_launch_that_writes_a_const_operand_is_reported_by_name(rz):
    x, idx, y = RZ.put(torch.randn(5, 3)), RZ.put(torch.tensor([4, 0, 2], dtype=torch.int32)), torch.empty(3, 3)
    with pytest.raises(RZ.RedzoneError, match=r"gn_gather_rows_f32: operand x .*const payload changed, first byte at offset [4-7]$"):
        _call(rz, _gather("x"), x, idx, y, 3)


def test_const_payloads_beyond_the_snapshot_limit_are_checksummed(rz, monkeypatch):
    monkeypatch.setattr(RZ, "SNAPSHOT", 16)
    x, idx, y = RZ.put(torch.randn(5, 3)), RZ.put(torch.tensor([4, 0, 2], dtype=torch.int32)), torch.empty(3, 3)
    assert _call(rz, _gather(), x, idx, y, 3) == 0
    with pytest.raises(RZ.RedzoneError, match=r"operand x .*const payload changed, first byte at offset None$"):
        _call(rz, _gather("x"), x, idx, y, 3)


def test_an_operand_also_passed_as_writable_counts_as_writable(rz):
    x, idx = RZ.put(torch.randn(5, 3)), RZ.put(torch.tensor([4, 0, 2], dtype=torch.int32))
    lib = rz.proxy(_fake_lib(_gather()))
    assert lib.gn_gather_rows_f32(_lib.ptr(x), _lib.ptr(idx), _lib.ptr(x[1:]), 3, 3, None) == 0     # y inside x's arena


def test_nesting_with_an_occupied_trace_slot_keeps_the_bands_and_restores_the_slot(monkeypatch):
    other = object()
    monkeypatch.setattr(_lib, "TRACE", other)
    with pytest.raises(RZ.RedzoneError, match="at exit.*after band"):
        with RZ.guard("cpu") as g:
            assert _lib.TRACE is other and not g.tracing
            t = torch.empty(4)
            _arena_of(g, t).buf[BAND + 16] = 0
    assert _lib.TRACE is other
    monkeypatch.setattr(_lib, "TRACE", None)
    with RZ.guard("cpu") as outer:
        with RZ.guard("cpu") as inner:
            assert _lib.TRACE is outer and not inner.tracing and inner.find(torch.empty(2).data_ptr()) is not None
            with outer.untraced():
                assert _lib.TRACE is None
        assert _lib.TRACE is outer and outer.find(torch.empty(2).data_ptr()) is not None
    assert _lib.TRACE is None


def test_the_first_load_of_the_library_under_a_tracer_is_proxied_too(monkeypatch, rz):
    """_lib.load() used to hand out the bare library on the call that loads it: the first launch of a process went untraced."""
    class FakeLibrary:
        def __getattr__(self, name):
            fn = types.SimpleNamespace()
            self.__dict__[name] = fn
            return fn
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", __file__)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: FakeLibrary())
    first = _lib.load()
    assert first is rz.proxy(_lib._lib) and _lib.load() is first and isinstance(_lib._lib, FakeLibrary)
