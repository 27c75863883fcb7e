"""The judges of tests/abi_mab.py held to the arithmetic they judge, on the CPU.

Positive controls: a correct fp32 accumulation (the same sum reassociated) and a correct bf16 one (torch's
own round-to-nearest-even: bf16(P + s) against P + bf16(s)) pass ``accumulated_ok``.  Negative controls:
each wrong result a write / accumulate contract can hide behind - an overwrite, a double add, P dropped, a
sign flip, half of the rows accumulated, a NaN left in a written output, one nonzero padding row - is
rejected by the judge that guards it."""
import pytest
import torch

import abi_mab as am
import grad_bars as gb


def _fresh(shape, seed, scale=1e-3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale * torch.rand(shape, generator=g)


SHAPES = [(128, 128), (3, 200, 128), (128,), (1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_fp32_accumulation_accepted(shape):
    fresh = _fresh(shape, 1)
    P = am.prefill_like(fresh, 2)
    # the kernel adds its partial sums onto P in another order than it forms fresh: two halves
    half = _fresh(shape, 3)
    acc = (P + half) + (fresh - half)
    assert am.accumulated_ok(acc, P, fresh, torch.float32) == []
    assert am.accumulated_ok((P.double() + fresh.double()).float(), P, fresh) == []


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bf16_accumulation_accepted(shape):
    s = _fresh(shape, 4)                         # the kernel's fp32 result
    fresh = s.to(torch.bfloat16)                 # what a written bf16 output holds
    P = am.prefill_like(fresh.float(), 5, dtype=torch.bfloat16)
    acc = (P.float() + s).to(torch.bfloat16)     # bf16(P + s): one rounding of the fp32 sum
    assert am.accumulated_ok(acc, P, fresh, torch.bfloat16) == []
    # and an s that differs in its last fp32 bits between the two calls
    s2 = s * (1 + 2.0 ** -22)
    assert am.accumulated_ok((P.float() + s2).to(torch.bfloat16), P, fresh, torch.bfloat16) == []
    # a P much smaller than fresh, and the reverse
    for sc in (1e-3, 1e3):
        Pk = (P.float() * sc).to(torch.bfloat16)
        assert am.accumulated_ok((Pk.float() + s).to(torch.bfloat16), Pk, fresh, torch.bfloat16) == []


def _mutations(P, fresh, dtype):
    n0 = fresh.shape[0]
    half = (P.float() + fresh.float()).clone()
    half[n0 // 2:] = fresh.float()[n0 // 2:]
    return {
        "overwrite": fresh.float(),
        "double add": P.float() + 2 * fresh.float(),
        "P subtracted": fresh.float() - P.float(),
        "P doubled": 2 * P.float() + fresh.float(),
        "sign flip": P.float() - fresh.float(),
        "half of the rows accumulated": half,
    }


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(128, 128), (3, 200, 128), (64,), (2, 1)], ids=str)
def test_wrong_accumulations_rejected(dtype, shape):
    fresh = _fresh(shape, 6).to(dtype)
    P = am.prefill_like(fresh.float(), 7, dtype=dtype)
    for what, acc in _mutations(P, fresh, dtype).items():
        if what == "half of the rows accumulated" and shape[0] < 2:
            continue
        bad = am.accumulated_ok(acc.to(dtype), P, fresh, dtype, what)
        assert bad, f"{what} accepted ({dtype})"


def test_fresh_scale_prefill_makes_errors_order_one():
    """With P drawn on the output's own scale, an overwrite is an O(1) error of the bound, not a rounding."""
    fresh = _fresh((64, 64), 8)
    P = am.prefill_like(fresh, 9)
    assert am.acc_ratio(fresh, P, fresh) > 1e4
    assert am.acc_ratio(P + fresh, P, fresh) < 1e-2      # one fp32 rounding of the sum


def test_written_judge():
    a = _fresh((5, 7), 10)
    assert am.written_ok(a, a.clone()) == []
    b = a.clone()
    b[3, 2] = float("nan")                      # an element never written with the NaN prefill
    assert am.written_ok(b, a)
    c = a.clone()
    c[0, 0] = 0.0                               # took the zero prefill instead of being written
    assert am.written_ok(a, c)
    assert am.written_ok(a, a * (1 + 1e-7), exact=False, bar=gb.F32) == []
    assert am.written_ok(a, a * 1.5, exact=False, bar=gb.F32)
    # bitwise: -0 and +0 are different writes of an exact output
    z = torch.zeros(4)
    assert am.written_ok(z, -z)
    bf = a.to(torch.bfloat16)
    assert am.written_ok(bf, bf.clone()) == []


def test_padding_rows_judge():
    B, nk, dk = 3, 10, 4
    lengths = [10, 1, 7]
    g = _fresh((B, nk, dk), 11)
    for b, n in enumerate(lengths):
        g[b, n:] = 0
    assert am.padding_rows_ok(g, lengths) == []
    bad = g.clone()
    bad[2, 8, 1] = 1e-30                         # one nonzero padding row
    assert am.padding_rows_ok(bad, lengths)
    P = am.prefill_like(g, 12)
    acc = P + g
    for b, n in enumerate(lengths):
        acc[b, n:] = P[b, n:]
    assert am.padding_rows_ok(acc, lengths, P) == []
    acc2 = acc.clone()
    acc2[1, 5] = 0.0                             # an accumulated padding row overwritten
    assert am.padding_rows_ok(acc2, lengths, P)
    acc3 = acc.clone()
    acc3[1, 5, 0] = torch.nextafter(acc3[1, 5, 0], torch.tensor(float("inf")))
    assert am.padding_rows_ok(acc3, lengths, P)
    gb16 = g.to(torch.bfloat16)
    assert am.padding_rows_ok(gb16, lengths) == []


def test_same_or_bar():
    a = _fresh((32, 32), 13)
    assert am.same_or_bar(a, a.clone(), True, gb.F32) == []
    b = a.clone()
    b[1, 1] = torch.nextafter(b[1, 1], torch.tensor(1.0))
    assert am.same_or_bar(b, a, True, gb.F32)          # one ulp is a difference when reproducible
    assert am.same_or_bar(b, a, False, gb.F32) == []   # and none under the bar otherwise
    assert am.same_or_bar(a * 0, a, False, gb.BF16_VS_ORACLE)


def test_oracle_lengths_and_shared_query():
    """The float64 oracle: a padded set equals its truncation, padding key rows get zero gradient, and a
    shared query's gradient is the sum over the sets."""
    p = am.mab_params(8, 6, 8, seed=1)
    g = torch.Generator().manual_seed(2)
    Q, K, dY = torch.randn(5, 8, generator=g), torch.randn(3, 9, 6, generator=g), torch.randn(3, 5, 8, generator=g)
    r = am.oracle(Q, K, p, 2, dY, True, lengths=[9, 2, 5])
    for b, n in enumerate([9, 2, 5]):
        assert bool((r["dK"][b, n:] == 0).all())
        rb = am.oracle(Q, K[b:b + 1, :n], p, 2, dY[b:b + 1], True)
        assert torch.allclose(r["Y"][b], rb["Y"][0], atol=1e-12)
        assert torch.allclose(r["dK"][b, :n], rb["dK"][0], atol=1e-12)
    dense = am.oracle(Q, K, p, 2, dY, True)
    per = sum(am.oracle(Q, K[b:b + 1], p, 2, dY[b:b + 1], True)["dQ"] for b in range(3))
    assert torch.allclose(dense["dQ"], per, atol=1e-12)


@pytest.mark.parametrize("shape,dtype", [((3, 37, 5), torch.float32), ((7,), torch.bfloat16), ((1,), torch.float32)],
                         ids=str)
def test_arena_guard_follows_the_last_element(shape, dtype):
    """The guard starts right after a tensor's last byte, whatever its size: one element written past the end
    is reported."""
    ar = am.Arena("cpu")
    t = ar.tensor(shape, dtype, 0.0)
    assert ar.check() == []
    es = t.element_size()
    ar.guards[-1][:es] = am.POISON            # what a store of one element past the end leaves there
    assert ar.check()
