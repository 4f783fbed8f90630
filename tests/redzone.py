"""Red-zone harness for the kernel-level GPU tests: guard bands around every tensor a test or a launcher allocates, checked
around every C-ABI launch.  A helper module (no conftest, no plugin), pure Python and device-agnostic.

    from redzone import put, redzone        # noqa: F401  -- `redzone` is an autouse fixture of the importing module
                                            #               (`redzone_on_request`: only tests that name `redzone`)

Inside `guard(device)` (the fixture is `guard("cuda")` around one test)

  * torch.empty / zeros / ones / full, their *_like forms and Tensor.new_empty / new_zeros / new_ones / new_full hand out, for
    a strided contiguous request on `device`, the payload of one uint8 arena  [band | payload | band].  Bands are BAND bytes
    of 0xFF (a quiet NaN as float32, -1 as int32 / int64); the payload of `empty` is 0xFF too, so an element nobody wrote
    is NaN.  Every other request (another device, out=, pin_memory, a layout, a non-contiguous *_like source, 0 elements)
    goes to the real function untouched.  `put(t)` copies a test input into such an arena.
  * a tracer in `_lib.TRACE` (the slot of hbcheck.Recorder; left alone, with tracing off, when it is taken) resolves every
    pointer operand of a gn_* launch (arguments, struct fields, host arrays of pointers, note()d table operands) to its
    arena by address range and, after the launch, compares both bands of each bit for bit and the payload of every
    operand the header declares `const` (and the same call does not also receive as writable) with its state before.
  * at exit every band is compared once more.

While the current stream is capturing the harness allocates nothing and checks nothing (its checks synchronise).  A
failure raises RedzoneError naming the entry point, the parameter or struct field, the band ("before band", "after band")
or "const payload", and the byte offset of the first damaged byte: for the after band counted from the payload's end
(0 = the first byte past it), for the before band from its start (-1 = the last byte in front of it), for a const payload
from its start (None when the payload is larger than SNAPSHOT bytes and only its checksum was kept)."""
import bisect
import contextlib

import pytest
import torch

BAND = 128 * 1024          # > the largest tile footprint in the tree (80 rows x 128 floats x 4 B = 40 KiB); a multiple of 512
SNAPSHOT = 1 << 20         # const payloads up to this size are kept as a copy (exact offset), larger ones as a checksum
_FACTORIES = ("empty", "zeros", "ones", "full")
_KW = {"dtype", "device", "requires_grad", "layout", "memory_format", "pin_memory"}
_ACTIVE = []


class RedzoneError(AssertionError):
    pass


class _Arena:
    __slots__ = ("buf", "lo", "n", "what", "dead")

    def __init__(self, buf, n, what):
        self.buf, self.n, self.what, self.dead = buf, n, what, False
        self.lo = buf.data_ptr() + BAND          # address of the payload

    def bands(self):
        return self.buf[:BAND], self.buf[BAND + self.n:]

    def payload(self):
        return self.buf[BAND:BAND + self.n]


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def _size(size):
    """(2, 3) / ((2, 3),) / ([2, 3],) / (torch.Size,) -> (2, 3); None when it is not a plain list of ints."""
    if size is not None and len(size) == 1 and isinstance(size[0], (tuple, list)):
        size = size[0]
    if size is None or not all(isinstance(s, int) and not isinstance(s, bool) for s in size):
        return None
    return tuple(int(s) for s in size)


def _parse(name, args, kw, value):
    """Arguments after the source tensor, if any -> (size | None, fill, the other keywords).  `full` takes (size, fill_value)."""
    kw = dict(kw)
    if name != "full":
        return _size(args if args else (kw.pop("size"),) if "size" in kw else None), value, kw
    pos = dict(zip(("size", "fill_value"), args))
    size = pos["size"] if "size" in pos else kw.pop("size", None)
    fill = pos["fill_value"] if "fill_value" in pos else kw.pop("fill_value", None)
    ok = len(args) <= 2 and type(fill) in (bool, int, float) and isinstance(size, (tuple, list))
    return (_size((size,)) if ok else None), fill, kw


def _fill_dtype(fill):
    """dtype `full` infers from a Python scalar (None: the default dtype)."""
    return torch.bool if type(fill) is bool else torch.int64 if type(fill) is int else None


class Guard:
    def __init__(self, device):
        self.device = torch.device(device)
        self.arenas, self.los = [], []           # sorted by payload address
        self.real = {}
        self.n_guarded = self.n_launches = self.n_operands = 0
        self.tracing = False

    # ------------------------------------------------------------------------------------------------ allocation
    def _mine(self, device):
        d = torch.device(device) if device is not None else torch.get_default_device()
        return d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)

    def alloc(self, size, dtype, fill, what, requires_grad=False):
        """The payload view of a fresh arena; fill None = 0xFF bytes."""
        n = dtype.itemsize
        for s in size:
            n *= s
        buf = self.real["full"]((2 * BAND + n,), 0xFF, dtype=torch.uint8, device=self.device)
        arena = _Arena(buf, n, what)
        i = bisect.bisect_left(self.los, arena.lo)
        self.los.insert(i, arena.lo)
        self.arenas.insert(i, arena)
        self.n_guarded += 1
        stride, acc = [], 1
        for s in reversed(size):
            stride.append(acc)
            acc *= max(s, 1)
        t = self.real["empty"]((0,), dtype=dtype, device=self.device)
        t.set_(buf.untyped_storage(), (buf.storage_offset() + BAND) // dtype.itemsize, size, tuple(reversed(stride)))   # no view: a plain tensor
        if fill is not None:
            t.fill_(fill)
        return t.requires_grad_(True) if requires_grad else t

    def _request(self, kw, dtype, device, contiguous=True):
        """Common pass-through rules; -> (dtype, requires_grad) or None (not ours)."""
        if not set(kw) <= _KW or kw.get("pin_memory") or kw.get("layout", torch.strided) not in (None, torch.strided):
            return None
        mf = kw.get("memory_format")
        if mf not in (None, torch.contiguous_format) and not (mf == torch.preserve_format and contiguous):
            return None
        device = kw.get("device") if kw.get("device") is not None else device
        if not contiguous or not self._mine(device) or _capturing(self.device):
            return None
        dtype = kw.get("dtype") or dtype or torch.get_default_dtype()
        return dtype, bool(kw.get("requires_grad", False))

    def _factory(self, name, value):
        real = self.real[name]

        def f(*args, **kw):
            size, fill, rest = _parse(name, args, kw, value)
            req = None if size is None or 0 in size else self._request(rest, _fill_dtype(fill) if name == "full" else None, None)
            if req is None:
                return real(*args, **kw)
            return self.alloc(size, req[0], fill, "torch." + name, req[1])
        return f

    def _like(self, name, value):
        real = self.real[name + "_like"]

        def f(src, *args, **kw):
            fill, rest = value, dict(kw)
            if name == "full":
                fill = args[0] if args else rest.pop("fill_value", None)
            ok = (torch.is_tensor(src) and len(args) == (name == "full" and "fill_value" not in kw) and src.numel() > 0
                  and src.layout == torch.strided and (name != "full" or type(fill) in (bool, int, float)))
            req = self._request(rest, src.dtype, src.device, src.is_contiguous()) if ok else None
            if req is None:
                return real(src, *args, **kw)
            return self.alloc(tuple(src.shape), req[0], fill, f"torch.{name}_like", req[1])
        return f

    def _new(self, name, value):
        real = self.real["new_" + name]

        def f(src, *args, **kw):
            size, fill, rest = _parse(name, args, kw, value)
            req = None if size is None or 0 in size else self._request(rest, src.dtype, src.device)
            if req is None:
                return real(src, *args, **kw)
            return self.alloc(size, req[0], fill, "Tensor.new_" + name, req[1])
        return f

    def put(self, t):
        """A copy of a host or device tensor inside a guarded arena on the guarded device (0 elements: a plain copy)."""
        if t.numel() == 0 or t.layout != torch.strided or _capturing(self.device):
            return t.to(self.device)
        out = self.alloc(tuple(t.shape), t.dtype, None, "put")
        out.copy_(t.detach())
        return out.requires_grad_(True) if t.requires_grad else out

    # ------------------------------------------------------------------------------------------------ checks
    def find(self, addr):
        i = bisect.bisect_right(self.los, addr) - 1
        if i >= 0 and addr < self.los[i] + max(self.arenas[i].n, 1):
            return self.arenas[i]
        return None

    @staticmethod
    def _checksum(p):
        k = p.numel() // 8 * 8
        return p[:k].view(torch.int64).sum() + p[k:].sum(dtype=torch.int64)

    def check_bands(self, items, where):
        """items: [(arena, operand name)].  One synchronisation for all of them."""
        items = [(a, w) for a, w in items if not a.dead]
        if not items:
            return
        flags = [b.amin() for a, _ in items for b in a.bands()]
        flags = torch.stack(flags).tolist()
        for k, (a, w) in enumerate(items):
            for side, name in ((0, "before band"), (1, "after band")):
                if flags[2 * k + side] != 0xFF:
                    a.dead = True
                    first = int((a.bands()[side] != 0xFF).nonzero()[0])
                    raise RedzoneError(f"redzone: {where}: operand {w} ({a.what}, {a.n} B payload): {name} damaged, first "
                                       f"byte at offset {first - BAND if side == 0 else first}")

    def check_all(self):
        for i in range(0, len(self.arenas), 256):
            self.check_bands([(a, "-") for a in self.arenas[i:i + 256]], "at exit (no launch named it)")

    # ------------------------------------------------------------------------------------------------ tracer (_lib.TRACE)
    @contextlib.contextmanager
    def untraced(self):
        """Free the `_lib.TRACE` slot for the block (a test that installs hbcheck's recorder itself); the bands stay."""
        from gemnet_pytorch_amd import _lib
        mine = _lib.TRACE is self
        if mine:
            _lib.TRACE = None
        try:
            yield
        finally:
            if mine:
                _lib.TRACE = self

    def touch(self, t):
        pass

    def note(self, reads=(), writes=()):
        self._notes.append((list(reads), list(writes)))

    def proxy(self, lib):
        if self._proxy is None or self._proxy._lib is not lib:
            self._proxy = _Proxy(lib, self)
        return self._proxy

    def operands(self, name, args):
        """[(address, 'r' | 'w', operand name)] of one call, from the header's kinds."""
        from gemnet_pytorch_amd import _lib
        out = []

        def val(x):
            return x if isinstance(x, int) else int(getattr(x, "value", None) or 0) if x is not None else 0

        def fields(obj, sname, prefix):
            out.extend((val(getattr(obj, f)), k, prefix + f) for f, k in self.structs[sname] if k in ("r", "w"))

        for (pname, kind), arg in zip(self.funcs[name], args):
            if kind in ("r", "w"):
                out.append((val(arg), kind, pname))
            elif kind in ("ra", "wa"):
                out.extend((val(arg[i]), kind[0], f"{pname}[{i}]") for i in range(len(arg)))
            elif kind == "struct:gn_gemm_args":
                fields(arg._obj, "gn_gemm_args", pname + ".")
            elif kind == "struct:gn_chain_args":
                ca = _lib.ChainArgs.from_address(val(arg))
                for i in range(ca.n_ops):
                    fields(ca.ops[i], "gn_chain_op", f"{pname}.ops[{i}].")
        for reads, writes in self._notes:
            for lst, kind in ((reads, "r"), (writes, "w")):
                out.extend((x.data_ptr() if torch.is_tensor(x) else x[0], kind, "table operand") for x in lst)
        self._notes = []
        return [o for o in out if o[0]]

    def call(self, name, fn, args):
        if _capturing(self.device):
            self._notes = []
            return fn(*args)
        seen = {}                                    # arena -> [kind, operand name]
        for addr, kind, what in self.operands(name, args):
            a = self.find(addr)
            if a is not None and not a.dead:
                e = seen.setdefault(id(a), [a, kind, what])
                if kind == "w" and e[1] == "r":
                    e[1], e[2] = "w", what
        before = {k: (a.payload().clone() if a.n <= SNAPSHOT else self._checksum(a.payload()))
                  for k, (a, kind, _) in seen.items() if kind == "r"}
        rc = fn(*args)
        self.n_launches += 1
        self.n_operands += len(seen)
        self.check_bands([(a, w) for a, _, w in seen.values()], name)
        for k, old in before.items():
            a, _, w = seen[k]
            if a.n <= SNAPSHOT:
                diff = (a.payload() != old).nonzero()
                first = int(diff[0]) if diff.numel() else None
                changed = first is not None
            else:
                first, changed = None, int(self._checksum(a.payload())) != int(old)
            if changed:
                raise RedzoneError(f"redzone: {name}: operand {w} ({a.what}, {a.n} B payload) is const in the header but its "
                                   f"const payload changed, first byte at offset {first}")
        return rc


class _Proxy:
    def __init__(self, lib, guard_):
        self._lib, self._guard = lib, guard_

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        g = self._guard
        sig = g.funcs.get(name)
        if sig is None or not any(k == "stream" for _, k in sig):
            return fn                                # queries: no launch
        call = lambda *args: g.call(name, fn, args)  # noqa: E731
        self.__dict__[name] = call
        return call


@contextlib.contextmanager
def guard(device="cuda"):
    """Guarded allocation and per-launch checks on `device` for the duration of the block; yields the Guard (counters
    n_guarded / n_launches / n_operands, `put`)."""
    from gemnet_pytorch_amd import _abi, _lib
    g = Guard(device)
    g.funcs, g.structs = _abi.parse_header()
    g._notes, g._proxy = [], None
    missing = object()
    saved = [(torch, n, torch.__dict__.get(n, missing)) for n in _FACTORIES + tuple(n + "_like" for n in _FACTORIES)]
    saved += [(torch.Tensor, "new_" + n, torch.Tensor.__dict__.get("new_" + n, missing)) for n in _FACTORIES]
    for n, v in zip(_FACTORIES, (None, 0, 1, None)):
        g.real[n], g.real[n + "_like"], g.real["new_" + n] = getattr(torch, n), getattr(torch, n + "_like"), getattr(torch.Tensor, "new_" + n)
    for n, v in zip(_FACTORIES, (None, 0, 1, None)):
        setattr(torch, n, g._factory(n, v))
        setattr(torch, n + "_like", g._like(n, v))
        setattr(torch.Tensor, "new_" + n, g._new(n, v))
    g.tracing = _lib.TRACE is None
    if g.tracing:
        _lib.TRACE = g
    _ACTIVE.append(g)
    try:
        yield g
        if not _capturing(g.device):
            g.check_all()
    finally:
        _ACTIVE.pop()
        if g.tracing:
            _lib.TRACE = None
        for owner, n, old in saved:
            if old is missing:
                delattr(owner, n)
            else:
                setattr(owner, n, old)
        g.arenas, g.los = [], []


def put(t, device="cuda"):
    """Test input -> guarded copy on the guarded device (outside a guard: a plain copy to `device`)."""
    return _ACTIVE[-1].put(t) if _ACTIVE else t.to(device)


TOTALS = {"tests": 0, "guarded": 0, "launches": 0, "operands": 0}      # over the session, for whoever wants to print them
LARGEST = {"test": None, "guarded": 0, "launches": 0}


def _around_one_test(request):
    with guard("cuda") as g:
        yield g
    for k, v in (("tests", 1), ("guarded", g.n_guarded), ("launches", g.n_launches), ("operands", g.n_operands)):
        TOTALS[k] += v
    if g.n_launches > LARGEST["launches"]:
        LARGEST.update(test=request.node.nodeid, guarded=g.n_guarded, launches=g.n_launches)


@pytest.fixture(autouse=True)
def redzone(request):
    """Importing this name into a test module runs every test of that module under guard("cuda"); the value is the Guard."""
    yield from _around_one_test(request)


@pytest.fixture(name="redzone")
def redzone_on_request(request):
    """Imported instead of `redzone` by a module whose kernel-level tests alone ask for it (argument `redzone`)."""
    yield from _around_one_test(request)
