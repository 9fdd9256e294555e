#!/usr/bin/env python3
"""The constants of the Gaussian rule in include/mxv_policy.h, generated: every one is an exact fraction — or pi/2,
ln(2 pi), ln 2, 1/ln 2, sqrt(1/2) from arithmetic of 250 decimal digits (more than 800 bits) — rounded once, to nearest even, to
double.  ln2_hi / ln2_lo / inv_ln2 / sqrt_half and the EXP / LOG coefficients are those of tools/policy_coefficients.py.  Prints the
C++ block that gym_amd/csrc/mxv_policy_rule.hpp carries verbatim, once, for every kernel of the policy heads (tests/test_gaussian_host.py
compares the two and the NumPy twin against this module).

    python tools/gaussian_coefficients.py          # the block
"""
import os
import sys
from decimal import Decimal, localcontext
from fractions import Fraction
from math import factorial

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
try:
    import policy_coefficients
finally:
    sys.path.pop(0)

SIN_TERMS = 9        # sin r = r + r z P(z),  P(z) = sum_{j=1}^{9}  (-1)^j z^(j-1) / (2j+1)!   on |r| < pi/4, z = r r
COS_TERMS = 10       # cos r = 1 + z Q(z),    Q(z) = sum_{j=1}^{10} (-1)^j z^(j-1) / (2j)!
PIO2_HI_BITS = 19    # pio2_hi = floor(pi/2 * 2^19) / 2^19: 20 significant bits, so f * pio2_hi is exact for the 33-bit f of SINCOS2PI

_DIGITS = 250


def _atan_inv(n: int) -> Fraction:
    """atan(1/n) = sum (-1)^j / ((2j+1) n^(2j+1)), to better than 10^-250."""
    total, j = Fraction(0), 0
    while True:
        term = Fraction(1, (2 * j + 1) * n ** (2 * j + 1))
        if term * 10 ** (_DIGITS + 3) < 1:
            break
        total += -term if j & 1 else term
        j += 1
    return total


def _pi() -> Fraction:
    return 16 * _atan_inv(5) - 4 * _atan_inv(239)        # Machin


def _log_2pi() -> Fraction:
    with localcontext() as ctx:
        ctx.prec = _DIGITS
        two_pi = 2 * _pi()
        return Fraction((Decimal(two_pi.numerator) / Decimal(two_pi.denominator)).ln())


def constants() -> dict:
    """name -> float (float(Fraction) rounds correctly); the keys of policy_coefficients.constants() and the Gaussian rule's own."""
    c = dict(policy_coefficients.constants())
    pio2 = _pi() / 2
    hi = Fraction(int(pio2 * 2 ** PIO2_HI_BITS), 2 ** PIO2_HI_BITS)
    half_log_2pi = _log_2pi() / 2
    c.update({
        "pio2_hi": float(hi),
        "pio2_lo": float(pio2 - hi),
        "half_log_2pi": float(half_log_2pi),
        "ent_c": float(Fraction(1, 2) + half_log_2pi),
        "sin_c": [float(Fraction((-1) ** j, factorial(2 * j + 1))) for j in range(1, SIN_TERMS + 1)],     # index j-1: (-1)^j / (2j+1)!
        "cos_c": [float(Fraction((-1) ** j, factorial(2 * j))) for j in range(1, COS_TERMS + 1)],         # index j-1: (-1)^j / (2j)!
    })
    return c


def block() -> str:
    c = constants()
    lines = [policy_coefficients.block(),
             f"constexpr double kPio2Hi = {c['pio2_hi'].hex()};",
             f"constexpr double kPio2Lo = {c['pio2_lo'].hex()};",
             f"constexpr double kHalfLog2Pi = {c['half_log_2pi'].hex()};",
             f"constexpr double kEntC = {c['ent_c'].hex()};",
             f"constexpr double kSinC[{SIN_TERMS}] = {{" + ", ".join(x.hex() for x in c["sin_c"]) + "};",
             f"constexpr double kCosC[{COS_TERMS}] = {{" + ", ".join(x.hex() for x in c["cos_c"]) + "};"]
    return "\n".join(lines)


if __name__ == "__main__":
    print(block())
