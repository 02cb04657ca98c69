"""How level the 16 owner waves of the relation-owner backward are, tile by tile, from the plan itself (CPU, the torch-op builder).

A workgroup's tile ends at a barrier, so it takes as long as its busiest wave.  The figure here is, per tile,
(chunks of the busiest wave) / (chunks of the tile / 16), averaged over the tiles.  own_relations' own balance figure is the static one on
the relations' message counts; it misses the rounding of every (tile, relation) bucket to whole chunks (a quarter of a 9-chunk bucket is
3, 2, 2, 2) and the spread of the six or seven buckets a wave holds from tile to tile (+-3 % per wave, the maximum of 16 waves ~6 % above
the mean), which no static assignment removes.  The shared form deals the chunks of the largest relation at run time; with the other
relations in the level layout (own_level=True) the figure falls from 1.11 to 1.02.

What the figure is NOT is a model of the kernel's time (profiles/own_shared_*.txt): on the MI355X the level layouts ran
slower than today's packing -- every part of a cut relation adds a set of atomics per workgroup on that relation's dW -- and the form
graph.win_plan asks for (own_shared=True alone: the other relations whole, figure 1.11) is the fastest of the four.  The bounds below
hold the plan builders to what they promise; they say nothing about speed.

The graph is S1 at the scale where a tile's statistics are S1's: 652-row tiles, 101 relations, ~130 messages per (tile, relation) bucket,
8 tiles -- N = 5216, 1043 triples per relation and direction, plus self loops."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-rgcn_amd"))

N, R0, PER_REL, ROWS, NW, K, U = 5216, 50, 1043, 652, 16, 8, 2
R = 2 * R0 + 1


def s1_messages(seed=1):
    rng = np.random.default_rng(seed)
    s, o = rng.integers(0, N, R0 * PER_REL), rng.integers(0, N, R0 * PER_REL)
    p = np.repeat(np.arange(R0), PER_REL)
    loops = np.arange(N)
    dst, src, rel = np.concatenate([s, o, loops]), np.concatenate([o, s, loops]), np.concatenate([p, p + R0, np.full(N, 2 * R0)])
    t32 = lambda a: torch.from_numpy(a.astype(np.int32))                                          # noqa: E731
    return t32(dst), t32(src), t32(rel), torch.ones(len(dst)), None


def dealt(own, shared):
    """the busiest wave after the shared chunks went, U at a time, to whichever wave had the least work"""
    own = own.astype(np.int64).copy()
    while shared > 0:
        w = int(own.argmin())
        own[w] += min(U, shared)
        shared -= U
    return int(own.max())


def busiest_over_mean(plan):
    if getattr(plan, "group_ptr", None) is not None:
        chunks = np.diff(plan.group_ptr.numpy().astype(np.int64)).reshape(plan.n_tiles, NW + 1)
        return float(np.mean([dealt(c[:NW], int(c[NW])) / (c.sum() / NW) for c in chunks]))
    chunks = np.diff(plan.own_ptr.numpy().astype(np.int64)).reshape(plan.n_tiles, NW)
    return float(np.mean(chunks.max(1) / (chunks.sum(1) / NW)))


def test_shared_plan_levels_the_waves_of_every_tile():
    from torch_rgcn import _native
    g = s1_messages()
    today = _native.build_softwin_plan(*g, N, N, R, ROWS, own_waves=NW, own_per_wave=K)
    level = _native.build_softwin_plan(*g, N, N, R, ROWS, own_waves=NW, own_per_wave=K, own_level=True)
    shared = _native.build_softwin_plan(*g, N, N, R, ROWS, own_waves=NW, own_per_wave=K, own_level=True, own_shared=True)
    shipped = _native.build_softwin_plan(*g, N, N, R, ROWS, own_waves=NW, own_per_wave=K, own_shared=True)
    f_today, f_level, f_shared, f_shipped = (busiest_over_mean(p) for p in (today, level, shared, shipped))
    print(f"busiest / mean chunks per tile: today {f_today:.4f}, level packing {f_level:.4f}, shared queue on the level packing {f_shared:.4f}, "
          f"shared queue beside whole relations (graph.win_plan) {f_shipped:.4f}")
    assert f_today > 1.08, f_today                 # (else the bounds below say nothing)
    assert f_level < f_today - 0.03, (f_level, f_today)
    assert f_shared <= 1.04, f_shared
    assert f_shipped <= f_today, (f_shipped, f_today)


def test_level_packing_of_s1():
    """96 relations whole, 6 per wave; the 4 largest of the rest in 4 parts, the self loops in 16: 8 units on every wave, all 128 slots"""
    from torch_rgcn import _native
    counts = np.bincount(s1_messages()[2].numpy(), minlength=R)
    parts, base, owner, local, unit_rel, balance = _native.own_relations(counts, NW, K, level=True)
    assert parts[2 * R0] == NW and sorted(parts[:2 * R0].tolist()) == [1] * 96 + [4] * 4 and (unit_rel >= 0).all()
    for w in range(NW):
        mine = unit_rel[w * K:(w + 1) * K]
        assert len(set(mine.tolist())) == K and sum(parts[r] == 1 for r in mine) == 6 and 2 * R0 in mine
    assert balance < 1.01 < _native.own_relations(counts, NW, K)[5]
    # where the level layout does not fit the slots: today's packing, value for value
    for c, nw, k in (([1000] + [200] * 100, 12, 9), ([1000] + [200] * 120, 16, 8)):
        a, b = _native.own_relations(c, nw, k), _native.own_relations(c, nw, k, level=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("level", [False, True], ids=["whole", "level"])
def test_shared_plan_invariants(level):
    from torch_rgcn import _native
    dst, src, rel, val, _ = g = s1_messages()
    p = _native.build_softwin_plan(*g, N, N, R, ROWS, own_waves=NW, own_per_wave=K, own_level=level, own_shared=True)
    assert p.shared_rel == 2 * R0 and p.shared_local == K - 1
    D, S, V = (t.numpy()[:p.m_pad] for t in (p.dst, p.src, p.val))
    packed = p.chunk_rel.numpy()[:p.n_chunks]
    crel, cloc = packed & 0xFFFF, packed >> 16
    real = D >= 0
    got = sorted(zip(D[real].tolist(), S[real].tolist(), np.repeat(crel, 16)[real].tolist(), V[real].tolist()))
    assert got == sorted(zip(dst.tolist(), src.tolist(), rel.tolist(), val.tolist()))          # every message in exactly one slot
    unit_rel = p.unit_rel.numpy().reshape(NW, K)
    assert (unit_rel[:, K - 1] == p.shared_rel).all() and (unit_rel[:, :K - 1] != p.shared_rel).all()
    gp, op, sp, tp = p.group_ptr.numpy(), p.own_ptr.numpy(), p.shared_ptr.numpy(), p.tile_ptr.numpy()
    assert gp.shape[0] == p.n_tiles * (NW + 1) + 1 and op.shape[0] == p.n_tiles * NW + 1 and sp.shape == (p.n_tiles, 2)
    assert gp[0] == 0 and gp[-1] == p.n_chunks and np.all(np.diff(gp) >= 0) and op[-1] == p.n_chunks
    for t in range(p.n_tiles):
        g0 = t * (NW + 1)
        assert gp[g0] == tp[t] and gp[g0 + NW + 1] == tp[t + 1] and tuple(sp[t]) == (gp[g0 + NW], gp[g0 + NW + 1]) and sp[t, 1] > sp[t, 0]
        for w in range(NW + 1):
            firsts = []
            for c in range(gp[g0 + w], gp[g0 + w + 1]):
                assert D[16 * c] >= 0 and D[16 * c] // ROWS == t
                firsts.append(int(S[16 * c]))
                if w == NW:
                    assert crel[c] == p.shared_rel and cloc[c] == p.shared_local               # shared chunks: the shared relation only
                else:
                    assert crel[c] != p.shared_rel and unit_rel[w, cloc[c]] == crel[c] and op[t * NW + w] == gp[g0 + w]
            assert firsts == sorted(firsts)                                                     # every range: by first source


def test_own_relations_unchanged_without_the_new_arguments():
    """the inputs of test_softwin_plan.test_own_relations_lpt_packing: the values the function returned before it had the new arguments
    (parts of relation 0, units, units per wave, balance, and a digest of the five arrays, recorded on the commit before)"""
    import hashlib
    from torch_rgcn import _native
    was = {(101, 12, 9): (2, 102, [7, 7, 9, 9, 9, 9, 9, 9, 9, 9, 8, 8], 1.0285714285714285, "c498b692ee85f131"),
           (4, 12, 9): (24, 27, [3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2], 1.0017989206476114, "e6377a7101ed1f59"),
           (1, 12, 9): (24, 24, [2] * 12, 1.0, "e23fc86cc2e2f7bc")}
    for counts in ([1000] + [200] * 100, [5000, 1, 1, 1], [4096]):
        got = _native.own_relations(counts, 12, 9)
        assert len(got) == 6
        digest = hashlib.sha1(b"".join(np.ascontiguousarray(a, dtype=np.int64).tobytes() for a in got[:5])).hexdigest()[:16]
        assert (int(got[0][0]), int(got[0].sum()), np.bincount(got[2], minlength=12).tolist(), float(got[5]), digest) == was[(len(counts), 12, 9)]
    assert _native.own_relations([1] * 109, 12, 9) is None
