"""The device's deterministic math against the oracle, bit for bit, over the default input sets of tests/math_sweep.py: every 61st f32 bit pattern plus every
pattern within 2^16 of each boundary for the unary functions, crossed edge sets, random and denormal-landing pairs for the binary ones.  One test per function,
so a failure names it.  (`python tests/math_sweep.py full` is the exhaustive form: all 2^32 patterns per unary function.)"""
import pytest

from tests import math_sweep

pytestmark = pytest.mark.gpu


def _device_equals_oracle(name):
    res = math_sweep.run(name, "default", arm="device", against="oracle")
    print(f"{name}: {res.inputs} inputs, {res.mismatches} mismatches, {res.seconds:.1f} s")
    assert res.inputs > 0
    assert res.mismatches == 0, res.message()


@pytest.mark.parametrize("name", ["sinf", "cosf", "expf", "logf", "acosf", "asinf", "sqrt_rn", "powf", "atan2f"])
def test_device_function_equals_oracle(built, name):
    _device_equals_oracle(name)


def test_device_div_rn_is_the_ieee_quotient(built):
    """1 / x, x / c, c / x over the unary set and a / b over pairs.  Before the device is asked: the pairs must be able to tell a divide from a multiplication by
    the rounded reciprocal, or a cheaper div_rn would pass unseen."""
    assert math_sweep.discriminating_pairs("div_rn") >= 100_000
    _device_equals_oracle("div_rn")


def test_device_mul_add_is_not_contracted(built):
    """a * b + a in two roundings.  Before the device is asked: the pairs must be able to tell a fused multiply-add from that."""
    assert math_sweep.discriminating_pairs("mul_add") >= 100_000
    _device_equals_oracle("mul_add")
