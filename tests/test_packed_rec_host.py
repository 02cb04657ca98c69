"""The packed chunk records (96 bytes per chunk) on the CPU, through the torch twin of the native packer
(_native.pack_rec_torch / pack_rec_fields_torch, the bytes of rgcn_bwd_blk_prepare_packed_f32; tests/test_gpu_packed_rec.py compares the
two): everything the kernels decode from a packed record equals the wide record's field bit for bit, and the packer refuses what does not
fit -- a source of 2^24, a 257th val."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-rgcn_amd"))

from torch_rgcn import _native  # noqa: E402

N, R, ROWS = 4003, 11, 40                     # 101 tiles of 40 rows, the last one of 3


def small_plan(seed=5, own=True):
    """soft-window owner plan (torch form) of 30 000 messages on N nodes: 1111 buckets of ~27 messages, most of them padded; vals 1 / k"""
    rng = np.random.default_rng(seed)
    M = 30_000
    dst = torch.from_numpy(rng.integers(0, N, M).astype(np.int32))
    src = torch.from_numpy(rng.integers(0, N, M).astype(np.int32))
    rel = torch.from_numpy(rng.integers(0, R, M).astype(np.int32))
    val = torch.from_numpy((1.0 / rng.integers(1, 9, M)).astype(np.float32))
    kw = dict(own_waves=16, own_per_wave=8, own_shared=True) if own else {}
    p = _native.build_softwin_plan(dst, src, rel, val, None, N, N, R, ROWS, **kw)
    assert p is not None and p.n_chunks > 0
    return p


def same_fields(got, want):
    for name, g, w in zip(("src", "row", "val bits", "rel", "unit"), got, want):
        assert g.dtype == torch.int32 and w.dtype == torch.int32, name
        assert torch.equal(g, w), f"{name}: {int((g != w).sum())} of {g.numel()} differ"


def test_round_trip_of_a_small_plan():
    p = small_plan()
    want = _native.rec_fields_torch(p.src, p.dst, p.val, p.chunk_rel, ROWS)
    src, row, bits, rel, unit = want
    pad = (p.dst[:p.m_pad] < 0)
    assert pad.any() and (~pad).any() and int(unit.max()) > 0 and (N % ROWS) != 0
    # the wide record's description itself: pads are +0.0f on the source and row of their chunk's first slot (never a pad: a chunk starts with a message)
    first = torch.arange(p.m_pad) // 16 * 16
    assert not pad[first].any()
    assert (bits[pad] == 0).all() and torch.equal(src[pad], p.src[first][pad]) and torch.equal(row[pad], (p.dst[first] % ROWS)[pad])
    assert torch.equal(bits[~pad], p.val[:p.m_pad].view(torch.int32)[~pad]) and torch.equal(row[~pad], (p.dst[:p.m_pad] % ROWS)[~pad])
    rec = _native.pack_rec_torch(p.src, p.dst, p.val, p.chunk_rel, ROWS, N)
    assert rec.dtype == torch.uint8 and rec.numel() == 1024 + 96 * p.n_chunks == int(_native.lib().rgcn_bwd_blk_packed_rec_bytes(p.n_chunks))
    same_fields(_native.unpack_rec_torch(rec, p.n_chunks), want)
    # pads decode to +0.0f (the sign bit too)
    assert (_native.unpack_rec_torch(rec, p.n_chunks)[2][pad] == 0).all()


def test_header_bits_and_row_bits_do_not_mix():
    """row 1023 (all ten bits) in every slot, relation 0xFFFE, unit 8 -- and the complement: row 0, header 0 next to a full one"""
    p = small_plan(own=False)
    src, row, bits, rel, unit = _native.rec_fields_torch(p.src, p.dst, p.val, p.chunk_rel, ROWS)
    d = _native.packed_rec_dictionary(p.dst[:p.m_pad], p.val[:p.m_pad])
    for row_v, rel_v, unit_v in ((1023, 0xFFFE, 8), (0, 0xFFFE, 8), (1023, 0, 0), (1023, 0xFFFF, 15), (682, 0x5555, 5)):
        want = (src, torch.full_like(row, row_v), bits, torch.full_like(rel, rel_v), torch.full_like(unit, unit_v))
        rec = _native.pack_rec_fields_torch(*want, d)
        same_fields(_native.unpack_rec_torch(rec, p.n_chunks), want)
        rows16 = rec[1024:].view(p.n_chunks, 96)[:, 64:].contiguous().view(torch.int16).long() & 0xFFFF
        assert ((rows16[:, 4:] & 63) == 0).all(), "header bits outside rows 0 .. 3"
        assert ((rows16 >> 6) == row_v).all()
    # one chunk differs from its neighbours in every field
    rel2, unit2, row2 = rel.clone(), unit.clone(), row.clone()
    rel2[1], unit2[1], row2[16:32] = 0xFFFE, 8, 1023
    want = (src, row2, bits, rel2, unit2)
    same_fields(_native.unpack_rec_torch(_native.pack_rec_fields_torch(*want, d), p.n_chunks), want)


def synthetic(n_chunks, src_value=7, bits=None):
    n = 16 * n_chunks
    i32 = lambda v: torch.full((n,), v, dtype=torch.int32)      # noqa: E731
    bits = torch.zeros(n, dtype=torch.int32) if bits is None else bits
    return [i32(src_value), torch.arange(n, dtype=torch.int32) % 1000, bits, torch.arange(n_chunks, dtype=torch.int32) % 65536, torch.arange(n_chunks, dtype=torch.int32) % 16]


def dictionary_of(bits):
    return _native.packed_rec_dictionary(torch.zeros_like(bits), bits.view(torch.float32))


def test_limits_source():
    f = synthetic(3, (1 << 24) - 1)
    same_fields(_native.unpack_rec_torch(_native.pack_rec_fields_torch(*f, dictionary_of(f[2])), 3), f)
    f = synthetic(3, 1 << 24)
    with pytest.raises(ValueError):
        _native.pack_rec_fields_torch(*f, dictionary_of(f[2]))
    plan_args = (torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.int32), torch.ones(16), torch.zeros(1, dtype=torch.int32))
    _native.pack_rec_torch(*plan_args, 40, 1 << 24)
    with pytest.raises(ValueError):
        _native.pack_rec_torch(*plan_args, 40, (1 << 24) + 1)
    with pytest.raises(ValueError):
        _native.pack_rec_torch(*plan_args, 1024, 100)


def test_limits_dictionary_size():
    n = 16 * 17                                                   # 272 slots
    vals = (torch.arange(n, dtype=torch.float32) % 256 + 1.0)
    f = synthetic(17, bits=vals.view(torch.int32))
    d = dictionary_of(f[2])
    assert d.numel() == 256
    same_fields(_native.unpack_rec_torch(_native.pack_rec_fields_torch(*f, d), 17), f)
    vals = (torch.arange(n, dtype=torch.float32) % 257 + 1.0)
    f = synthetic(17, bits=vals.view(torch.int32))
    assert dictionary_of(f[2]) is None
    with pytest.raises(ValueError):
        _native.pack_rec_fields_torch(*f, None)
    with pytest.raises(ValueError):
        _native.pack_rec_fields_torch(*f, torch.unique(f[2]))      # 257 entries
    with pytest.raises(ValueError):
        _native.pack_rec_fields_torch(*f, torch.unique(f[2])[:256])      # a val that is not in the dictionary


def test_bit_patterns_stay_apart():
    """-0.0f, +0.0f, a denormal and two NaN payloads: five int32 patterns, none merged by a float comparison"""
    special = torch.tensor([-0x80000000, 0, 0x00000001, 0x7FC00000, 0x7FC00001, 0x3F800000], dtype=torch.int64)
    special = torch.where(special >= (1 << 31), special - (1 << 32), special).to(torch.int32)
    bits = special[torch.arange(32) % 6]
    f = synthetic(2, bits=bits)
    d = dictionary_of(bits)
    assert d.numel() == 6 and set(d.tolist()) == set(special.tolist())
    got = _native.unpack_rec_torch(_native.pack_rec_fields_torch(*f, d), 2)
    same_fields(got, f)
    # through the plan-level packer: the pads' +0.0f joins the dictionary, -0.0f of a message stays -0.0f
    val = bits[:16].clone().view(torch.float32)
    dst = torch.arange(16, dtype=torch.int32)
    dst[12:] = -1
    rec = _native.pack_rec_torch(torch.arange(16, dtype=torch.int32), dst, val, torch.zeros(1, dtype=torch.int32), 40, 100)
    got = _native.unpack_rec_torch(rec, 1)[2]
    assert torch.equal(got[:12], bits[:12]) and (got[12:] == 0).all()


def test_dictionary_is_sorted_and_codes_are_in_range():
    p = small_plan()
    d = _native.packed_rec_dictionary(p.dst[:p.m_pad], p.val[:p.m_pad])
    assert d.dtype == torch.int32 and d.numel() == 9               # 1 / 1 .. 1 / 8 and the pads' +0.0f
    assert (d[1:] > d[:-1]).all(), "ascending int32 bit patterns, no duplicates"
    assert 0 in d.tolist()
    rec = _native.pack_rec_torch(p.src, p.dst, p.val, p.chunk_rel, ROWS, N)
    head = rec[:1024].view(torch.int32)
    assert torch.equal(head[:9], d) and (head[9:] == 0).all()
    codes = rec[1024:].view(p.n_chunks, 96)[:, :64].contiguous().view(torch.int32) & 0xFF
    assert int(codes.max()) < d.numel()
    # a plan without pads has no +0.0f entry
    d2 = _native.packed_rec_dictionary(torch.zeros(32, dtype=torch.int32), torch.full((32,), 0.5))
    assert d2.tolist() == [0x3F000000]
