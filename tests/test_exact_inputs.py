"""Self-test of the exact-arithmetic method (tests/exact_inputs.py), on the CPU: the power of tests/test_gpu_exact.py is itself tested.

A float32 evaluation in any message order must equal the float64 oracle in every element, and each one-message mutant must not."""
import numpy as np
import pytest

import exact_inputs as ex
from oracle import oracle

N, R0, D = 2048, 3, 16
R = 2 * R0 + 1


def rel_err(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def hub():
    """the hub fixture: a 2^15 hub (and 2^12, 2^10, 2^10) in relation 0, groups of 1 .. 16 elsewhere; 109 k messages"""
    T = ex.pow2_triples(N, R0, 1200, hub_log2=15, seed=1)
    tp = oracle.add_inverse_and_self(T, N, R0)
    rng = np.random.default_rng(2)
    X = ex.ints((N, D), -2, 2, 0.5, rng)
    g = ex.ints((N, D), -2, 2, 0.5, rng)
    W = ex.ints((R, D, D), -2, 2, 1.0, rng)
    bias = ex.ints((D,), -2, 2, 1.0, rng)
    val = oracle.nc_edge_norm(tp, N, R, False)
    ref = oracle.layer(tp, val, N, R, X, {"weights": W}, "none", bias, g)
    ref = {"out": ref["out"], "dX": ref["dX"], "weights": ref["grads"]["weights"]}
    return dict(T=T, tp=tp, val=val, X=X, g=g, W=W, bias=bias, ref=ref)


@pytest.mark.parametrize("vertical", [False, True])
def test_generator_gives_powers_of_two_under_both_stackings(vertical):
    for hub_log2, seed in ((None, 3), (15, 4), (6, 5)):
        T = ex.pow2_triples(777, 5, 300, hub_log2=hub_log2, seed=seed)
        tp = oracle.add_inverse_and_self(T, 777, 5)
        val = oracle.nc_edge_norm(tp, 777, 11, vertical)
        assert ex.is_pow2(val) and val.max() == 1.0
        if hub_log2:
            assert val.min() == 2.0 ** -hub_log2
    # duplicates and s == o are kept (the kernels meet both)
    T = ex.pow2_triples(50, 2, 40, seed=6)
    assert len(np.unique(T, axis=0)) < len(T) and (T[:, 0] == T[:, 2]).any()
    # uniform random triples are NOT powers of two: the property is the generator's
    tp = oracle.add_inverse_and_self(oracle.synthetic_triples(777, 5, 6000, seed=1), 777, 5)
    assert not ex.is_pow2(oracle.nc_edge_norm(tp, 777, 11, vertical))


@pytest.mark.parametrize("hub_log2", [None, 10, 15], ids=["plain", "hub10", "hub15"])
def test_generator_gives_powers_of_two_under_the_lp_formula(hub_log2):
    """the LP layer's message list is [T | inverses | T | self loops] with the count formula of layers.py:498-510 (oracle.lp_layer's val, no
    dropout: every self loop kept), under which the base triples are counted twice -- 2 x 2^k is still a power of two.  And the method
    holds there: a float32 evaluation in shuffled message orders equals the oracle."""
    n, r0, d = 777, 3, 8
    r = 2 * r0 + 1
    T = ex.pow2_triples(n, r0, 300, hub_log2=hub_log2, seed=8)
    tp, n_self = oracle.lp_augment(T, n, r0, None)
    assert len(tp) == 3 * len(T) + n and n_self == len(T) + n
    for vertical in (False, True):
        assert ex.is_pow2(oracle.edge_norm(tp, n, r, vertical, len(T), n_self))
    val = oracle.edge_norm(tp, n, r, False, len(T), n_self)
    if hub_log2:
        assert val.min() <= 2.0 ** -hub_log2
    rng = np.random.default_rng(9)
    X, g = ex.ints((n, d), -2, 2, 0.5, rng), ex.ints((n, d), -2, 2, 0.5, rng)
    W, bias = ex.ints((r, d, d), -2, 2, 1.0, rng), ex.ints((d,), -2, 2, 1.0, rng)
    ex.assert_provably_exact(tp, val, n, r, X, {"weights": W}, "none", bias, g)
    ref = oracle.lp_layer(T, n, r, X, {"weights": W}, "none", bias, False, None, g)
    for _ in range(2):
        got = ex.eval_f32(tp, val, n, r, X, W, bias, g, rng.permutation(len(tp)))
        ex.assert_equal_exact(got["out"], ref["out"], "out")
        ex.assert_equal_exact(got["dX"], ref["dX"], "dX")
        ex.assert_equal_exact(got["weights"], ref["grads"]["weights"], "dW")
    # uniform random triples are not powers of two under this formula either
    Tu = oracle.synthetic_triples(n, r0, 6000, seed=1)
    tpu, nsu = oracle.lp_augment(Tu, n, r0, None)
    assert not ex.is_pow2(oracle.edge_norm(tpu, n, r, False, len(Tu), nsu))


def test_values_are_small_integers_exact_in_bf16():
    import torch
    a = ex.ints((1000, 7), -2, 2, 0.5, 0)
    assert a.dtype == np.float32 and set(np.unique(a)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and 0.3 < (a != 0).mean() < 0.5
    assert np.array_equal(torch.from_numpy(a).to(torch.bfloat16).float().numpy(), a)
    assert np.array_equal(ex.ints((5, 5), -2, 2, 0.5, 7), ex.ints((5, 5), -2, 2, 0.5, 7))


def test_hub_fixture_is_provably_exact(hub):
    bits = ex.assert_provably_exact(hub["tp"], hub["val"], N, R, hub["X"], {"weights": hub["W"]}, "none", hub["bias"], hub["g"])
    print("proof bound, bits:", {k: round(v, 1) for k, v in bits.items()})
    assert set(bits) == {"out", "dX", "db", "weights"} and max(bits.values()) <= ex.MAX_BITS


def test_float32_evaluation_in_any_order_equals_the_oracle(hub):
    rng = np.random.default_rng(11)
    for _ in range(3):
        got = ex.eval_f32(hub["tp"], hub["val"], N, R, hub["X"], hub["W"], hub["bias"], hub["g"], rng.permutation(len(hub["tp"])))
        for k in ("out", "dX", "weights"):
            ex.assert_equal_exact(got[k], hub["ref"][k], k)


MUTANTS = ("dropped", "duplicated", "moved to another relation", "val halved")


def _mutate(hub, kind):
    tp, val = hub["tp"].copy(), hub["val"].copy()
    e = int(np.nonzero(val == val.min())[0][7])          # one message of the 2^15 hub row
    if kind == "dropped":
        keep = np.arange(len(tp)) != e
        return tp[keep], val[keep]
    if kind == "duplicated":
        return np.concatenate([tp, tp[e:e + 1]]), np.concatenate([val, val[e:e + 1]])
    if kind == "moved to another relation":
        tp[e, 1] = (tp[e, 1] + 1) % (2 * R0)
        return tp, val
    val[e] *= np.float32(0.5)
    return tp, val


@pytest.mark.parametrize("kind", MUTANTS)
def test_one_message_mutants_are_caught(hub, kind):
    """One message of the hub row (32 768 messages, val = 2^-15) dropped / duplicated / moved to the next relation / its val halved.
    Under the suite's former metric max|a - b| / max|b| every mutant passes 1e-4 by more than an order of magnitude:

        mutant                      out       dX        dW
        dropped                     1.0e-5    7.3e-6    9.9e-7
        duplicated                  1.0e-5    7.3e-6    9.9e-7
        moved to another relation   1.4e-5    1.1e-5    9.9e-7
        val halved                  5.1e-6    3.7e-6    5.0e-7

    under assert_equal_exact each fails in at least one of out / dX / dW (most in all three)."""
    tp, val = _mutate(hub, kind)
    got = ex.eval_f32(tp, val, N, R, hub["X"], hub["W"], hub["bias"], hub["g"], np.random.default_rng(12).permutation(len(tp)))
    caught = []
    for k in ("out", "dX", "weights"):
        err = rel_err(got[k], hub["ref"][k])
        print(f"{kind}: rel_err {k} = {err:.2e}")
        assert err < 1e-4, "the mutant is meant to be one the max-norm metric lets through"
        try:
            ex.assert_equal_exact(got[k], hub["ref"][k], k)
        except AssertionError:
            caught.append(k)
    assert caught, f"mutant '{kind}' equals the exact result in out, dX and dW"


def test_comparison_reports_and_ignores_the_sign_of_zero():
    import torch
    ref = np.array([[0.0, 1.5], [2.0, -3.0]], np.float32)
    ex.assert_equal_exact(np.array([[-0.0, 1.5], [2.0, -3.0]], np.float32), ref, "x")
    ex.assert_equal_exact(torch.tensor([[0.0, 1.5], [2.0, -3.0]]).to(torch.bfloat16), ref, "x")
    # bf16: against the reference rounded once (257 -> 256 to nearest even)
    ex.assert_equal_exact(torch.tensor([256.0]).to(torch.bfloat16), np.array([257.0], np.float32), "x")
    with pytest.raises(AssertionError, match=r"1 of 4 elements.*\n.*\(1, 0\).*degree 9"):
        ex.assert_equal_exact(np.array([[0.0, 1.5], [2.0000002, -3.0]], np.float32), ref, "x", degree=np.array([4, 9]))
    with pytest.raises(AssertionError, match="NaN"):
        ex.assert_equal_exact(np.array([[np.nan, 1.5], [2.0, -3.0]], np.float32), ref, "x")


def test_gaussian_inputs_are_rejected(hub):
    rng = np.random.default_rng(0)
    Xg = rng.standard_normal((N, D)).astype(np.float32)
    with pytest.raises(AssertionError, match="not provably exact"):
        ex.assert_provably_exact(hub["tp"], hub["val"], N, R, Xg, {"weights": hub["W"]}, "none", hub["bias"], hub["g"])
    # and a graph whose counts are not powers of two
    tp = oracle.add_inverse_and_self(oracle.synthetic_triples(N, R0, 20_000, seed=1), N, R0)
    with pytest.raises(AssertionError, match="power of two"):
        ex.assert_provably_exact(tp, oracle.nc_edge_norm(tp, N, R, False), N, R, hub["X"], {"weights": hub["W"]}, "none", hub["bias"], hub["g"])
