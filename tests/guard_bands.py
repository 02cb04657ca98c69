"""Guard bands: every buffer the library sizes itself sits between two poisoned bands, and every pointer it hands to a kernel is looked up.

The suite compares every VALUE the library returns; this helper looks at what a kernel does OUTSIDE the buffers it was given.

    with Guard(monkeypatch) as guard:
        X = guard.home(X)                     # tensors the test makes itself
        ... build graph and plans, run the layer ...
        problems = guard.check()              # damaged bands, as strings that name the allocation's call site
        calls, guarded, total, loose = guard.ledger()

While a Guard is active torch.empty / zeros / full / empty_like / zeros_like / full_like and Tensor.new_empty / new_zeros / new_full are
replaced (for tensors on the guarded device type; pin_memory=, out=, other devices and layouts pass straight through); so are the
host-to-device copies Tensor.to / Tensor.cuda and torch.tensor / torch.as_tensor with a device, whose results move into guarded
allocations (the plan arrays the library builds on the host).  An allocation of n
bytes becomes one uint8 arena of the ORIGINAL torch.empty:

    | GUARD bytes of 0xFF | n bytes: the tensor, 16-byte aligned | GUARD bytes of 0xFF |

The upper band starts at the first byte past the tensor (not rounded up: a 2-byte overrun of an odd bf16 row lands in it).  The tensor
handed back owns a storage of exactly n bytes at offset 0 with no base, as one from the allocator does (functional._rows16,
_zero_padded_rows and dist._dense look at these properties, and a view into the arena would move layers to another route); the storage is
a DLPack import of arena[GUARD : GUARD + n], which keeps the arena alive.  Arenas stay alive until the Guard exits, so no guarded address is
reused and a late store into a band of a buffer that was already dropped is still seen.

0xFF..FF is NaN as fp32 / bf16 / fp16 / fp64, -1 as int32 / int64, 255 as uint8:
  * a stray floating-point LOAD meets NaN instead of the zero of fresh device memory, and the value checks of the test see it;
  * a stray STORE changes a band byte and check() reports it (a store of the very pattern 0xFF.. -- a NaN with all bits set, -1 -- is not
    seen);
  * a stray INTEGER load yields -1, which the kernels treat as a pad destination and which as a source index points back into the lower
    band: stray integer reads are made harmless, NOT detected.
Floating-point interiors of empty / empty_like are NaN (0xFF) too; integer interiors of empty are left as they come; zeros / full get
their value.

The pointer ledger: include/rgcn_hip.h is parsed with the regular expression of _native._bind; while the Guard is active _native._lib is a
proxy that forwards every call and notes for every integer-valued pointer argument whether it points into a guarded interior (the parameter
`stream`, entry points named *_host, None and ctypes.byref objects are skipped).  ledger() names the non-const pointers that did not: a
buffer a kernel writes that no band protects.

Not seen: buffers ATen allocates in C++ (the results of .contiguous(), .clone(), torch.cat, autograd's gradient buffers) and anything
inside a captured graph."""
import bisect
import os
import re
import sys
import threading

import torch

GUARD = 16 * 1024
_HERE = os.path.abspath(__file__)
HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "rgcn_hip.h")

_FACTORIES = ("empty", "zeros", "full", "empty_like", "zeros_like", "full_like")
_METHODS = ("new_empty", "new_zeros", "new_full")
_UPLOADS = ("to", "cuda")                      # Tensor methods that copy host arrays (units, work items, owner tables) to the device
_FROM_DATA = ("tensor", "as_tensor")           # torch functions that build a device tensor from host data


def parse_header(path=HEADER):
    """-> {entry point: [(parameter name, is a pointer, is const), ...]}, read with the regular expression of _native._bind"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", "", open(path).read(), flags=re.S | re.M)
    protos = re.findall(r"\bRGCN_API\s+([^;()]+?)\b(rgcn_\w+)\s*\(([^;()]*)\)\s*;", text)
    table = {}
    for _, name, params in protos:
        table[name] = []
        if params.strip() in ("", "void"):
            continue
        for p in params.split(","):
            p = p.strip()
            table[name].append((re.search(r"(\w+)\s*$", p).group(1), "*" in p, bool(re.match(r"const\b", p))))
    return table


class _Record:
    __slots__ = ("arena", "lo", "nbytes", "site", "shape", "dtype", "kind", "start")

    def describe(self):
        return f"{self.kind} {tuple(self.shape)} {str(self.dtype).replace('torch.', '')} allocated at {self.site}"


class _LibProxy:
    """forwards every attribute to the loaded library; rgcn_* entry points are wrapped so that their pointer arguments reach the ledger"""

    def __init__(self, real, guard):
        self.__dict__["_real"], self.__dict__["_guard"], self.__dict__["_wrapped"] = real, guard, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        params = self._guard.protos.get(name)
        if params is None or name.endswith("_host") or not any(ptr for _, ptr, _ in params):
            return fn
        w = self._wrapped.get(name)
        if w is None:
            guard = self._guard

            def w(*args, _fn=fn, _name=name, _params=params):
                guard._note_call(_name, _params, args)
                return _fn(*args)
            self._wrapped[name] = w
        return w

    def __setattr__(self, name, value):
        setattr(self._real, name, value)


class Guard:
    """see the module docstring.  device: the device TYPE whose allocations are guarded ("cuda"; "cpu" runs the same code in the CPU
    self-tests).  native: also empty the library's workspace caches and put the ledger proxy in place of _native._lib."""

    def __init__(self, monkeypatch, device="cuda", native=True, allow=()):
        self.monkeypatch = monkeypatch
        self.allow = {(fn, par) for fn, par, *_ in allow}        # non-const pointers that may stay outside: (function, parameter, reason)
        self.allow_used = set()
        self.device_type = torch.device(device).type
        self.native = native
        self.records = []
        self._starts = []                 # sorted interior start addresses / their records, for the ledger's lookup
        self._by_start = []
        self._lock = threading.Lock()
        self.protos = parse_header() if native else {}
        self.calls = self.guarded = self.total = 0
        self.loose = {}                   # (function, parameter) of non-const pointers outside every guarded interior -> count
        self.loose_const = {}             # the same for const pointers (inputs ATen made: reported, never a problem)
        self.layout_problems = []         # rows wider than GUARD / 2
        self._orig = {}
        self._active = False

    # ------------------------------------------------------------------ context
    def __enter__(self):
        for n in _FACTORIES:
            self._orig[n] = getattr(torch, n)
            self.monkeypatch.setattr(torch, n, self._factory(n, self._orig[n], method=False))
        for n in _METHODS:
            self._orig[n] = getattr(torch.Tensor, n)
            self.monkeypatch.setattr(torch.Tensor, n, self._factory(n, self._orig[n], method=True))
        for n in _UPLOADS:
            self._orig[n] = getattr(torch.Tensor, n)
            self.monkeypatch.setattr(torch.Tensor, n, self._adopting(n, self._orig[n], method=True))
        for n in _FROM_DATA:
            self._orig[n] = getattr(torch, n)
            self.monkeypatch.setattr(torch, n, self._adopting(n, self._orig[n], method=False))
        if self.native:
            from torch_rgcn import _native
            real = _native.lib()
            for mod, name in ((_native, "_TABLE_WS"), (_native, "_BCE_WS"), (_native, "_WS_KEEP")):
                cache = getattr(mod, name, None)
                if isinstance(cache, dict):                       # reallocated under guard; the old ones come back on exit
                    self.monkeypatch.setattr(mod, name, {})
                elif isinstance(cache, list):
                    self.monkeypatch.setattr(mod, name, [])
            self.monkeypatch.setattr(_native, "_lib", _LibProxy(real, self))
        self._active = True
        return self

    def __exit__(self, *exc):
        self._active = False
        for n in _FACTORIES:           # (monkeypatch undoes everything at the end of the test; the code between here and there is unguarded too)
            self.monkeypatch.setattr(torch, n, self._orig[n])
        for n in _METHODS + _UPLOADS:
            self.monkeypatch.setattr(torch.Tensor, n, self._orig[n])
        for n in _FROM_DATA:
            self.monkeypatch.setattr(torch, n, self._orig[n])
        if self.native:
            from torch_rgcn import _native
            if isinstance(_native._lib, _LibProxy):
                self.monkeypatch.setattr(_native, "_lib", _native._lib._real)
        return False

    # ------------------------------------------------------------------ allocation
    def _site(self):
        f = sys._getframe(1)
        while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
            f = f.f_back
        if f is None:
            return "?"
        name = f.f_code.co_filename
        for marker in ("torch_rgcn" + os.sep, "tests" + os.sep):
            if marker in name:
                name = name[name.rindex(marker):]
                break
        return f"{name}:{f.f_lineno}"

    def _factory(self, name, orig, method):
        guard = self
        kind = name.replace("new_", "").replace("_like", "")

        def patched(*args, **kwargs):
            if not guard._active or kwargs.get("pin_memory") or kwargs.get("out") is not None:
                return orig(*args, **kwargs)
            if kwargs.get("layout", torch.strided) is not torch.strided or "names" in kwargs:
                return orig(*args, **kwargs)
            dev = kwargs.get("device")
            if dev is None and (method or name.endswith("_like")):
                dev = args[0].device if args else None
            if dev is None:
                return orig(*args, **kwargs)
            dev = torch.device(dev)
            if dev.type != guard.device_type:
                return orig(*args, **kwargs)
            # shape, dtype and strides as the constructor itself works them out
            meta = orig(*args, **dict(kwargs, device="meta"))
            if not meta.is_contiguous():
                return orig(*args, **kwargs)
            if kind == "full":
                value = kwargs["fill_value"] if "fill_value" in kwargs else args[2 if method else 1]
            else:
                value = 0 if kind == "zeros" else None
            t = guard._alloc(meta.shape, meta.dtype, dev, kind, value, guard._site())
            if kwargs.get("requires_grad"):
                t.requires_grad_(True)
            return t
        patched.__name__ = name
        return patched

    def _adopting(self, name, orig, method):
        """host data that becomes a device tensor (x.to(dev), x.cuda(), torch.tensor(data, device=dev)): ATen allocates the result, so it
        is copied into a guarded allocation -- the plan arrays the library builds on the host (units, work items, owner tables) are read
        by kernels through const pointers, and a read past their end should meet a band too.  Tensors in an autograd graph pass through."""
        guard = self

        def patched(*args, **kwargs):
            out = orig(*args, **kwargs)
            if not guard._active or not isinstance(out, torch.Tensor) or out.device.type != guard.device_type or out.requires_grad:
                return out
            if args and isinstance(args[0], torch.Tensor) and (out is args[0] or args[0].device.type == guard.device_type):
                return out                                        # a dtype change on the device, or nothing at all: ATen's business
            if out.layout is not torch.strided or not out.is_contiguous() or type(out) is not torch.Tensor:
                return out
            home = guard._alloc(out.shape, out.dtype, out.device, "upload", None, guard._site())
            home.copy_(out)
            return home
        patched.__name__ = name
        return patched

    def _alloc(self, shape, dtype, dev, kind, value, site):
        empty = self._orig["empty"]
        item = empty(0, dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= int(s)
        n = numel * item
        if len(shape) >= 2 and int(shape[-1]) * item * 2 > GUARD:          # (reported by check(): an exception here would surface inside autograd)
            self.layout_problems.append(f"{kind} {tuple(shape)} {dtype} allocated at {site}: a row of {int(shape[-1]) * item} bytes, GUARD must "
                                        f"be at least two rows or an access at row -1 or N jumps the band")
        arena = empty(GUARD + 16 + n + GUARD, dtype=torch.uint8, device=dev)
        lo = GUARD + (-(arena.data_ptr() + GUARD)) % 16
        floating = dtype.is_floating_point or dtype.is_complex
        if kind == "empty" and floating:
            arena.fill_(0xFF)                                  # bands and interior in one launch: 0xFF.. is NaN in every floating type
        else:
            arena[:lo].fill_(0xFF)
            arena[lo + n:].fill_(0xFF)
        body = torch.utils.dlpack.from_dlpack(torch.utils.dlpack.to_dlpack(arena[lo:lo + n]))     # a storage of its own: n bytes, offset 0
        stride, acc = [], 1
        for s in reversed(shape):
            stride.append(acc)
            acc *= max(int(s), 1)
        t = empty(0, dtype=dtype, device=dev).set_(body.untyped_storage(), 0, tuple(shape), tuple(reversed(stride)))
        if value is not None:
            t.fill_(value)
        rec = _Record()
        rec.arena, rec.lo, rec.nbytes, rec.site, rec.shape, rec.dtype, rec.kind = arena, lo, n, site, tuple(shape), dtype, kind
        rec.start = arena.data_ptr() + lo
        assert rec.start % 16 == 0 and (n == 0 or t.data_ptr() == rec.start), (rec.start, t.data_ptr())
        with self._lock:
            self.records.append(rec)
            i = bisect.bisect_left(self._starts, rec.start)
            self._starts.insert(i, rec.start)
            self._by_start.insert(i, rec)
        return t

    def home(self, t):
        """a copy of t (values, dtype, requires_grad) inside a guarded allocation"""
        out = self._alloc(t.shape, t.dtype, t.device, "home", None, self._site())
        out.copy_(t.detach())
        return out.requires_grad_(t.requires_grad)

    # ------------------------------------------------------------------ the check
    def check(self):
        """-> one string per damaged band (empty: every band intact).  One synchronisation; one reduction per band on the device, the
        bytes of a damaged band are fetched for the report only."""
        recs = list(self.records)
        if not recs:
            return list(self.layout_problems)
        mins = []
        for r in recs:
            mins.append(r.arena[:r.lo].min())
            mins.append(r.arena[r.lo + r.nbytes:].min())
        host = torch.stack(mins).cpu().tolist()                  # the one synchronisation
        problems = list(self.layout_problems)
        for i, m in enumerate(host):
            if m == 0xFF:
                continue
            r, upper = recs[i // 2], bool(i % 2)
            band = r.arena[r.lo + r.nbytes:] if upper else r.arena[:r.lo]
            bad = (band != 0xFF).nonzero().flatten()
            first, last, count = int(bad[0]), int(bad[-1]), int(bad.numel())
            found = bytes(band[first:first + 16].cpu().tolist()).hex(" ")
            if upper:
                where = f"upper band damaged: first byte at offset {first} past the tensor's end"
            else:
                where = f"lower band damaged: first byte at offset {first - r.lo} from the tensor's start (last at {last - r.lo})"
            problems.append(f"{r.describe()}: {where}, {count} bytes differ from 0xFF in all, 16 bytes from the first: {found}")
        return problems

    # ------------------------------------------------------------------ the ledger
    def _inside(self, ptr):
        i = bisect.bisect_right(self._starts, ptr) - 1
        if i < 0:
            return False
        r = self._by_start[i]
        return ptr < r.start + r.nbytes or (r.nbytes == 0 and ptr == r.start)

    def _note_call(self, name, params, args):
        if not self._active:
            return
        self.calls += 1
        for (pname, is_ptr, is_const), a in zip(params, args):
            if not is_ptr or pname == "stream" or a is None or isinstance(a, bool) or not isinstance(a, int) or a == 0:
                continue                                          # (ctypes.byref objects and bytes are not integers; 0 is NULL)
            self.total += 1
            if self._inside(a):
                self.guarded += 1
            else:
                book = self.loose_const if is_const else self.loose
                book[(name, pname)] = book.get((name, pname), 0) + 1

    def ledger(self):
        """-> (native calls, pointers inside a guarded interior, pointers in all, sorted [(function, parameter)] of the non-const pointers
        that were not)"""
        return self.calls, self.guarded, self.total, sorted(self.loose)


    def problems(self, label=""):
        """what a guarded case asserts to be empty: check(), the non-const pointers outside every guarded allocation that are not on the
        allow-list, and a case that made no native call.  Prints the ledger's totals and adds them to TOTALS."""
        out = self.check()
        calls, guarded, total, loose = self.ledger()
        for fn, par in loose:
            if (fn, par) in self.allow:
                self.allow_used.add((fn, par))
            else:
                out.append(f"{fn}: `{par}` is written by the kernel and pointed outside every guarded allocation in {self.loose[(fn, par)]} "
                           f"calls (an ATen-made buffer?): no band protects it")
        if self.native and not calls:
            out.append("no native call was made under the guard")
        print(f"[guard] {label}{' ' if label else ''}calls {calls} / guarded pointers {guarded} / total pointers {total} "
              f"({len(self.records)} guarded allocations)")
        for k, v in (("cases", 1), ("calls", calls), ("guarded", guarded), ("total", total), ("allocations", len(self.records))):
            TOTALS[k] = TOTALS.get(k, 0) + v
        for k, v in self.loose_const.items():
            UNSEEN_INPUTS[k] = UNSEEN_INPUTS.get(k, 0) + v
        return out


UNSEEN_INPUTS = {}        # (function, const parameter) -> calls in which it pointed outside the guarded allocations, over the session
TOTALS = {}               # summed over the guarded cases of a session: cases, calls, guarded pointers, total pointers, allocations


def assert_allocator_like(t, shape, dtype):
    """what the patched constructors promise about the tensor they hand back"""
    assert tuple(t.shape) == tuple(shape) and t.dtype == dtype, (t.shape, t.dtype)
    assert t.storage_offset() == 0 and t._base is None and t.is_contiguous(), (t.storage_offset(), t._base is None, t.stride())
    assert t.untyped_storage().nbytes() == t.numel() * t.element_size(), (t.untyped_storage().nbytes(), t.numel() * t.element_size())
    assert t.numel() == 0 or t.data_ptr() % 16 == 0
