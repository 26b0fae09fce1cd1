"""Coefficients of the res_2s second-order exponential integrator (reference components/res2s.py): the phi functions and the
two-stage Runge-Kutta weights for one step of size h = log(sigma / sigma_next).  Plain Python doubles; the engine
(csrc/dit_engine.hip, res2s_plan) computes the same numbers in C."""
import math
from typing import Dict, Tuple


def phi(j: int, neg_h: float) -> float:
    """phi_j(z) = (e^z - sum_{k<j} z^k / k!) / z^j at z = neg_h; phi_j(0) = 1 / j!, used for |z| < 1e-10."""
    if abs(neg_h) < 1e-10:
        return 1.0 / math.factorial(j)
    head = sum(neg_h**k / math.factorial(k) for k in range(j))
    return (math.exp(neg_h) - head) / (neg_h**j)


def get_res2s_coefficients(h: float, phi_cache: Dict, c2: float = 0.5) -> Tuple[float, float, float]:
    """(a21, b1, b2) for step size h with the intermediate point at c2: a21 = c2 * phi_1(-h*c2) places the midpoint,
    b2 = phi_2(-h) / c2 and b1 = phi_1(-h) - b2 weigh the two evaluations.  phi_cache maps (j, z) to phi_j(z) across steps."""
    def cached(j: int, z: float) -> float:
        if (j, z) not in phi_cache:
            phi_cache[(j, z)] = phi(j, z)
        return phi_cache[(j, z)]

    a21 = c2 * cached(1, -h * c2)
    b2 = cached(2, -h) / c2
    b1 = cached(1, -h) - b2
    return a21, b1, b2
