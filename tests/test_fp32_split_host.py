"""The power of the per-product probes (tests/test_gpu_fp32_product_probes.py), proven without a GPU: on the operand generator the GPU probe
imports, a torch restatement of the kernels' split product (tests/fp32_split.py) stays within the bound the probe asserts, and the same
product with ANY single term left out -- six for bf16x6, three for bf16x3 -- exceeds that bound at least four times over.  This is the
condition that makes the GPU assertion meaningful: a kernel that pairs the wrong planes or skips a term cannot pass it."""
import math

import pytest
import torch

from tests.fp32_split import BOUND, MIN_PRODUCTS, PARTS, operands, rel_err, split_bf16, split_product, terms


@pytest.fixture(scope="module")
def pairs():
    # as many pairs as the smallest probed launch yields single products; the probe draws its dense and one-hot operands with other seeds of
    # the same generator
    return operands(MIN_PRODUCTS, seed=101), operands(MIN_PRODUCTS, seed=202)


def test_operands_are_full_mantissa_fp32_in_a_quarter_to_four():
    v = operands(64, 64, seed=7)
    assert v.dtype == torch.float32 and v.shape == (64, 64)
    assert float(v.abs().min()) >= 0.25 and float(v.abs().max()) < 4.0
    assert torch.equal(v, operands(64, 64, seed=7)) and not torch.equal(v, operands(64, 64, seed=8))
    bits = v.view(torch.int32).flatten()
    for k in range(23):                                  # every mantissa bit is set in about half of the values
        frac = float(((bits >> k) & 1).float().mean())
        assert 0.45 < frac < 0.55, f"mantissa bit {k}: set in {frac:.3f}"
    assert 0.45 < float((v < 0).float().mean()) < 0.55
    assert sorted(set(torch.frexp(v.abs())[1].flatten().tolist())) == [-1, 0, 1, 2]     # four binades: [0.25, 0.5) .. [2, 4)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x6"])
def test_split_is_exact_to_the_claimed_bits(mode, pairs):
    a, _ = pairs
    parts = split_bf16(a, PARTS[mode])
    for p in parts:
        assert torch.equal(p, p.bfloat16().float())
    left = (a.double() - sum(p.double() for p in parts)).abs() / a.double().abs()
    # what is left after k bf16 parts: <= 2^-(8 k) of the value (8 significant bits, half an ulp per rounding) -- 2^-24 for hi + mid + lo
    assert float(left.max()) <= 2.0 ** (-8 * PARTS[mode])


def test_term_order_is_the_kernels():
    assert terms(2) == [(0, 1), (1, 0), (0, 0)]
    assert terms(3) == [(0, 2), (1, 1), (0, 1), (2, 0), (1, 0), (0, 0)]
    assert all(ka + kb < 3 for ka, kb in terms(3)) and len(set(terms(3))) == 6


def test_exact_product_is_within_its_bound(pairs):
    a, b = pairs
    e = rel_err(a * b, a, b)
    assert float(e.max()) <= 2.0 ** -24 <= BOUND["exact"] / 2


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x6"])
def test_full_split_product_is_within_the_probe_bound(mode, pairs):
    a, b = pairs
    worst = float(rel_err(split_product(a, b, PARTS[mode]), a, b).max())
    print(f"{mode}: full product worst 2^{math.log2(worst):.2f}")
    assert worst <= BOUND[mode], f"{mode}: full product errs by 2^{math.log2(worst):.2f}"
    # ... and within what include/biu.h states (half the probe's bound) on these operands
    assert worst <= BOUND[mode] / 2


@pytest.mark.parametrize("mode,drop", [(m, t) for m in ("bf16x3", "bf16x6") for t in terms(PARTS[m])])
def test_every_single_term_omission_exceeds_the_bound_four_times(mode, drop, pairs):
    a, b = pairs
    e = rel_err(split_product(a, b, PARTS[mode], drop=drop), a, b)
    worst, median = float(e.max()), float(e.median())
    print(f"{mode} without part {drop[0]} x part {drop[1]}: worst 2^{math.log2(worst):.2f} median 2^{math.log2(median):.2f}")
    assert worst >= 4 * BOUND[mode], f"{mode} without term {drop}: worst error 2^{math.log2(worst):.2f} is under 4 x the bound"
    # not only the worst pair: most single products give the omission away, so one that hits a single tap or chunk position is caught too
    assert median > BOUND[mode], f"{mode} without term {drop}: median error 2^{math.log2(median):.2f}"
