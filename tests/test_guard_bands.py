"""The guard-band helper (tests/guard_bands.py) on CPU tensors: the same constructors, arena layout, check and header parse that the GPU
module uses, with the device filter set to "cpu".  The overruns are written by the test itself, through torch.as_strided, into the helper's
own bands."""
import re

import pytest
import torch

import guard_bands as gb

BF = torch.bfloat16


def _line_of(marker):
    """the line of this file that holds `marker` (the expected call site of an allocation)"""
    hits = [i + 1 for i, l in enumerate(open(__file__.replace(".pyc", ".py"))) if marker in l and "_line_of" not in l]
    assert len(hits) == 1, (marker, hits)
    return hits[0]


def _beyond(t, first, n=1):
    """a view of n elements of t's dtype that starts `first` elements from t's first element (outside t: what a stray kernel would touch);
    built on the arena, since t's own storage ends where t ends"""
    g = t._guard_record
    raw = g.arena[g.lo + first * t.element_size(): g.lo + (first + n) * t.element_size()]
    return raw.view(t.dtype)


@pytest.fixture
def guard(monkeypatch):
    with gb.Guard(monkeypatch, device="cpu", native=False) as g:
        yield g


def _alloc(guard, *a, **k):
    t = torch.empty(*a, device="cpu", **k)                                  # ALLOC-SITE
    t._guard_record = guard.records[-1]
    return t


@pytest.mark.parametrize("shape,dtype", [((3, 5), BF), ((4,), torch.float32), ((7,), torch.uint8), ((2, 3), torch.int32)], ids=str)
def test_store_one_element_past_the_end_is_reported(guard, shape, dtype):
    t = _alloc(guard, shape, dtype=dtype)
    assert guard.check() == []
    # through as_strided on the arena-backed storage: element numel() of the tensor, i.e. the first byte of the upper band
    _beyond(t, t.numel()).fill_(1)
    problems = guard.check()
    assert len(problems) == 1, problems
    p = problems[0]
    assert "upper band damaged" in p and "offset 0 past the tensor's end" in p, p
    assert f"test_guard_bands.py:{_line_of('ALLOC-SITE')}" in p and str(tuple(shape)) in p and str(dtype).replace("torch.", "") in p, p
    assert f"{t.element_size()} bytes differ" in p, p


def test_as_strided_store_past_the_end_is_reported(guard):
    """the issue's form: a view made by torch.as_strided whose one element lies past the end (of a guarded tensor that is itself a slice
    of a guarded tensor's storage cannot exist -- the storage ends with the tensor -- so the stride trick runs on the arena's storage)"""
    t = _alloc(guard, (3, 5), dtype=BF)
    g = t._guard_record
    whole = g.arena.view(BF)
    torch.as_strided(whole, (1,), (1,), g.lo // 2 + t.numel()).fill_(2.0)
    problems = guard.check()
    assert len(problems) == 1 and "upper band damaged" in problems[0] and "offset 0 past" in problems[0], problems
    assert "00 40" in problems[0], problems[0]                               # bf16 2.0 = 0x4000, little endian


def test_store_one_element_before_the_start_is_reported(guard):
    t = _alloc(guard, (3, 5), dtype=BF)
    _beyond(t, -1).fill_(1)
    problems = guard.check()
    assert len(problems) == 1, problems
    assert "lower band damaged" in problems[0] and "offset -2 from the tensor's start" in problems[0], problems[0]
    assert f"test_guard_bands.py:{_line_of('ALLOC-SITE')}" in problems[0]


def test_store_of_the_last_element_is_not_reported(guard):
    t = _alloc(guard, (3, 5), dtype=BF)
    t.view(-1)[-1] = 1
    t.view(-1)[0] = 1
    _beyond(t, t.numel() - 1).fill_(3)
    assert guard.check() == []
    assert float(t[2, 4]) == 3.0


@pytest.mark.parametrize("dtype", [BF, torch.int32, torch.uint8, torch.float32, torch.int64], ids=str)
@pytest.mark.parametrize("shape", [(0,), (1,), (5, 7)], ids=str)
@pytest.mark.parametrize("ctor", ["empty", "zeros", "full", "empty_like", "zeros_like", "full_like", "new_empty", "new_zeros", "new_full"])
def test_tensors_look_like_the_allocator_s(guard, ctor, shape, dtype):
    like = torch.ones(shape, dtype=dtype)
    t = {"empty": lambda: torch.empty(shape, dtype=dtype, device="cpu"),
         "zeros": lambda: torch.zeros(*shape, dtype=dtype, device="cpu"),
         "full": lambda: torch.full(shape, 3, dtype=dtype, device="cpu"),
         "empty_like": lambda: torch.empty_like(like),
         "zeros_like": lambda: torch.zeros_like(like),
         "full_like": lambda: torch.full_like(like, 3),
         "new_empty": lambda: like.new_empty(shape),
         "new_zeros": lambda: like.new_zeros(*shape),
         "new_full": lambda: like.new_full(shape, 3)}[ctor]()
    assert len(guard.records) == 1, "the constructor was not intercepted"
    gb.assert_allocator_like(t, shape, dtype)
    rec = guard.records[0]
    assert rec.nbytes == t.numel() * t.element_size() and rec.start % 16 == 0
    assert rec.lo >= gb.GUARD and rec.arena.numel() - rec.lo - rec.nbytes >= gb.GUARD
    if "zeros" in ctor:
        assert bool((t == 0).all())
    if "full" in ctor:
        assert bool((t == 3).all())
    if "empty" in ctor and dtype.is_floating_point:
        assert bool(t.isnan().all())
    assert guard.check() == []
    t.fill_(1)                                                              # the whole interior can be written
    assert guard.check() == []


def test_floating_point_interiors_of_empty_are_nan(guard):
    for dtype in (torch.float32, BF, torch.float16, torch.float64):
        t = torch.empty((9, 3), dtype=dtype, device="cpu")
        assert bool(t.isnan().all()), dtype
        assert bool(torch.empty_like(t).isnan().all()), dtype
    assert bool((torch.zeros(4, device="cpu") == 0).all()) and bool((torch.full((4,), 2.5, device="cpu") == 2.5).all())


def test_what_passes_straight_through(guard):
    # no device, a meta device: not the guarded type
    torch.empty(3)
    torch.zeros(3, device="meta")
    # out=
    buf = torch.ones(3)
    torch.zeros(3, out=buf)
    assert len(guard.records) == 0
    try:
        pinned = torch.empty(1, dtype=torch.int32, pin_memory=True, device="cpu")
    except RuntimeError:                                                    # no accelerator to pin for: the call still reached torch's own
        pinned = None
    assert len(guard.records) == 0
    assert pinned is None or pinned.is_pinned()


def test_requires_grad_and_home(guard):
    t = torch.zeros((2, 3), device="cpu", requires_grad=True)
    assert t.requires_grad and t.is_leaf
    src = torch.arange(12, dtype=torch.float32).view(3, 4)[:, :3].requires_grad_(True)      # not contiguous
    h = guard.home(src)
    gb.assert_allocator_like(h, (3, 3), torch.float32)
    assert h.requires_grad and h.is_leaf and torch.equal(h.detach(), src.detach())
    assert "home (3, 3) float32" in guard.records[-1].describe()
    assert guard.check() == []


def test_device_tensors_made_from_host_data_are_adopted(guard):
    """torch.tensor / torch.as_tensor with host data (Tensor.to and Tensor.cuda take the same path for a host tensor on its way to the
    guarded device: only the GPU self-test can run that)"""
    import numpy as np
    t = torch.tensor([[1, 2], [3, 4]], dtype=torch.int32, device="cpu")
    assert len(guard.records) == 1 and guard.records[0].kind == "upload" and guard.records[0].start == t.data_ptr()
    gb.assert_allocator_like(t, (2, 2), torch.int32)
    assert t.tolist() == [[1, 2], [3, 4]]
    u = torch.as_tensor(np.arange(5, dtype=np.float32), device="cpu")
    assert len(guard.records) == 2 and u.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert torch.as_tensor(u) is u and u.to(torch.float64).dtype == torch.float64 and len(guard.records) == 2      # already there: ATen's
    w = torch.tensor([1.0], requires_grad=True, device="cpu")
    assert w.requires_grad and len(guard.records) == 2
    assert guard.check() == []


def test_rows_wider_than_half_the_band_are_reported(guard):
    torch.empty((2, gb.GUARD // 8 + 1), dtype=torch.float32, device="cpu")
    problems = guard.check()
    assert len(problems) == 1 and "GUARD must be at least two rows" in problems[0], problems
    assert gb.GUARD >= 2 * 3 * 500 * 4                                      # the widest row of the GPU cases


def test_the_guard_ends_with_its_block(monkeypatch):
    with gb.Guard(monkeypatch, device="cpu", native=False) as g:
        torch.empty(3, device="cpu")
    t = torch.empty(3, device="cpu")
    assert len(g.records) == 1 and not hasattr(t, "_guard_record")
    assert torch.empty.__module__ != gb.__name__


def test_header_parse_matches_the_binding():
    from torch_rgcn import _native
    protos = gb.parse_header()
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", "", open(_native._HEADER_PATH).read(), flags=re.S | re.M)
    assert len(protos) == len(re.findall(r"\bRGCN_API\b", text)) > 100

    class Anything:                                                         # _bind declares argtypes on whatever it is given
        _name = "stub"

        def __getattr__(self, name):
            fn = type("F", (), {})()
            self.__dict__[name] = fn
            return fn
    assert _native._bind(Anything(), _native._HEADER_PATH) == len(protos)
    spmm = {n: (ptr, const) for n, ptr, const in protos["rgcn_spmm_f32"]}
    assert spmm["X"] == (True, True) and spmm["out"] == (True, False) and spmm["stream"] == (True, False)
    assert spmm["n_dst"] == (False, False) if "n_dst" in spmm else True
    assert all(not ptr for _, ptr, _ in protos["rgcn_gemm_scratch_floats"])


def test_ledger_counts_guarded_and_loose_pointers(monkeypatch):
    g = gb.Guard(monkeypatch, device="cpu", native=False)
    g.protos = gb.parse_header()
    with g:
        a = torch.empty(8, device="cpu")
        b = torch.empty(0, device="cpu")
        outside = torch.ones(8)
        params = g.protos["rgcn_colsum_f32"]                               # (const float *G, float *db, float *scratch, ..., void *stream)
        names = [n for n, _, _ in params]
        args = {"G": outside.data_ptr(), "db": a.data_ptr() + 28, "scratch": outside.data_ptr(), "stream": 1234}
        g._note_call("rgcn_colsum_f32", params, [args.get(n, 5) for n in names])
        assert g.ledger() == (1, 1, 3, [("rgcn_colsum_f32", "scratch")])
        args.update(db=a.data_ptr() + 32, scratch=None, G=g.records[1].start)        # one past the end; NULL; an empty allocation's address
        g._note_call("rgcn_colsum_f32", params, [args.get(n, 5) for n in names])
        assert g.ledger() == (2, 2, 5, [("rgcn_colsum_f32", "db"), ("rgcn_colsum_f32", "scratch")])
        del b
