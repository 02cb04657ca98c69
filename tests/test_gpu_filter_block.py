"""The filter block of the twelve filtered all-candidate entry points on the device: the lists and the index together, a negative K and
a K without its keys are RGCN_EINVAL under the entry's own name with nothing launched, and the index alone is taken.  (That the index
gives the bits of the lists is tests/test_gpu_filter_index.py's subject.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, D, Q, TOPK = 10, 8, 2, 3
ROLES = ["rank_fused", "topk", "lse", "lse_smooth", "softmax_grad", "softmax_grad_smooth"]


def p(x):
    return None if x is None else x.data_ptr()


@pytest.fixture(scope="module")
def world():
    from torch_rgcn import _native
    w = {"f32": torch.randn(N, D, device=DEV), "rel": torch.randn(3, D, device=DEV),
         "batch": torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV),
         # one list entry and one key: the known head 5 of (?, 1, 2), key = p * N + o = 12
         "fq": torch.tensor([0], device=DEV, dtype=torch.int32), "fn": torch.tensor([5], device=DEV, dtype=torch.int32),
         "keys": torch.tensor([12], device=DEV), "ptr": torch.tensor([0, 1], device=DEV), "vals": torch.tensor([5], device=DEV, dtype=torch.int32),
         "lse": torch.zeros(Q, device=DEV), "g": torch.ones(1, device=DEV),
         "keep": torch.full((1,), 0.75, device=DEV), "uni": torch.full((Q,), 0.025, device=DEV)}
    w["bf16"] = w["f32"].to(torch.bfloat16)
    sizes = [_native.rank_fused_workspace_bytes(Q, N, D, 0, True), _native.topk_workspace_bytes(Q, N, D, TOPK, 0, True),
             _native.lse_smooth_workspace_bytes(Q, N, D, 0, True), _native.softmax_grad_workspace_bytes(Q, N, D, True),
             _native.lse_smooth_workspace_bytes(Q, N, D, 0, False), _native.softmax_grad_workspace_bytes(Q, N, D, False)]
    w["ws"] = torch.empty(max(sizes) + 16, device=DEV, dtype=torch.uint8)
    assert p(w["ws"]) % 16 == 0
    return w


def entry(world, role, storage):
    """-> (call(filt_q, filt_n, F, fkeys, fptr, fvals, K), its pre-filled outputs): the raw entry point on N = 10, d = 8, Q = 2"""
    from torch_rgcn import _native
    L, st = _native.lib(), _native._stream(torch.device(DEV))
    b, nd, rl, ws = p(world["batch"]), p(world[storage]), p(world["rel"]), p(world["ws"])
    lse, g, keep, uni = p(world["lse"]), p(world["g"]), p(world["keep"]), p(world["uni"])
    i64 = lambda *shape: torch.full(shape, -7, device=DEV, dtype=torch.int64)  # noqa: E731
    i32 = lambda *shape: torch.full(shape, -7, device=DEV, dtype=torch.int32)  # noqa: E731
    f32 = lambda *shape: torch.full(shape, -7.0, device=DEV)  # noqa: E731
    bf16 = storage == "bf16"
    if role == "rank_fused":
        out = [i64(Q), i64(Q), f32(Q)]
        o = [p(t) for t in out]
        if bf16:
            return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_rank_fused_bf16(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K,
                                                                                    0, ws, o[0], o[1], o[2], N, 3, D, st), out
        return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_rank_fused_f32(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K,
                                                                               0, ws, o[0], o[1], o[2], N, 3, D, st), out
    if role == "topk":
        out = [i64(Q, TOPK), f32(Q, TOPK)]
        o = [p(t) for t in out]
        if bf16:
            return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_topk_bf16(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K, TOPK,
                                                                              0, ws, o[0], o[1], N, 3, D, st), out
        return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_topk_f32(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K, TOPK,
                                                                         0, ws, o[0], o[1], N, 3, D, st), out
    if role == "lse":
        out = [f32(Q), f32(Q)]
        o = [p(t) for t in out]
        if bf16:
            return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_lse_bf16(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K, 0, ws,
                                                                             o[0], o[1], N, 3, D, st), out
        return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_lse_f32(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K, 0, ws,
                                                                        o[0], o[1], N, 3, D, st), out
    if role == "lse_smooth":
        out = [f32(Q), f32(Q), f32(Q), i32(Q)]
        o = [p(t) for t in out]
        if bf16:
            return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_lse_smooth_bf16(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K,
                                                                                    0, ws, o[0], o[1], o[2], o[3], N, 3, D, st), out
        return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_lse_smooth_f32(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K,
                                                                               0, ws, o[0], o[1], o[2], o[3], N, 3, D, st), out
    out = [f32(Q, N)]
    dS = p(out[0])
    if role == "softmax_grad":
        if bf16:
            return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_softmax_grad_bf16(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K,
                                                                                      lse, g, 0, 2, 0, N, ws, dS, N, 3, D, st), out
        return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_softmax_grad_f32(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv, K,
                                                                                 lse, g, 0, 2, 0, N, ws, dS, N, 3, D, st), out
    assert role == "softmax_grad_smooth"
    if bf16:
        return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_softmax_grad_smooth_bf16(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv,
                                                                                         K, lse, g, keep, uni, 0, 2, 0, N, ws, dS, N, 3, D, st), out
    return lambda fq, fn, F, fk, fp, fv, K: L.rgcn_distmult_softmax_grad_smooth_f32(b, Q, 1, nd, rl, None, None, None, fq, fn, F, fk, fp, fv,
                                                                                    K, lse, g, keep, uni, 0, 2, 0, N, ws, dS, N, 3, D, st), out


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("role", ROLES)
def test_the_filter_block_of_every_folded_entry_point(world, role, storage):
    from torch_rgcn import _native
    L = _native.lib()
    call, out = entry(world, role, storage)
    name = ("distmult_" + role + ("_bf16" if storage == "bf16" else "")).encode()
    fq, fn, keys, ptr, vals = (p(world[k]) for k in ("fq", "fn", "keys", "ptr", "vals"))
    refused = {"lists and index together": (fq, fn, 1, keys, ptr, vals, 1),
               "K = -1": (None, None, 0, keys, ptr, vals, -1),
               "K = 1 without keys": (None, None, 0, None, ptr, vals, 1)}
    for what, block in refused.items():
        assert call(*block) == _native.EINVAL, what
        assert L.rgcn_last_error().startswith(name + b":"), (what, L.rgcn_last_error())
    torch.cuda.synchronize()
    for t in out:
        assert (t == -7).all()                                                  # nothing was launched
    assert call(None, None, 0, keys, ptr, vals, 1) == _native.OK
    torch.cuda.synchronize()
    for t in out:
        assert (t != -7).all()
