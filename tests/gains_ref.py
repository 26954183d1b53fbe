"""The gain system of exposure_gains (tscm_calib.hpp, tscm_calib_amd/panorama.py) solved exactly: the n x n system of
   sum_ij N_ij [(g_i I_ij - g_j I_ji)^2 / sigma_n^2 + (1 - g_i)^2 / sigma_g^2],  N = count, I = sum / count
in rational arithmetic from the same integer count and sum, for the tests of the two fp64 routes (numpy's solve with rint,
the header's Gaussian elimination with floor(x + 0.5))."""
from fractions import Fraction

HALF = Fraction(1, 2)
# a camera whose exact 256 g lies this close to a half-integer is left out of a comparison: the two rounding rules, and an
# fp64 solve that is a few ulp off, may differ there
NEAR_HALF = Fraction(1, 10 ** 6)


def exact_q8(count, total, sigma_n="10", sigma_g="0.1"):
    """count, total: [n][n] integers -> the exact values 256 g_i as Fractions (before rounding and the clip)."""
    n = len(count)
    alpha, beta = 1 / Fraction(sigma_n) ** 2, 1 / Fraction(sigma_g) ** 2
    N = [[Fraction(int(count[i][j])) for j in range(n)] for i in range(n)]
    I = [[Fraction(int(total[i][j])) / N[i][j] if N[i][j] > 0 else Fraction(0) for j in range(n)] for i in range(n)]
    A = [[Fraction(0)] * n for _ in range(n)]
    b = [Fraction(0)] * n
    for i in range(n):
        for j in range(n):
            b[i] += beta * N[i][j]
            A[i][i] += beta * N[i][j]
            if j != i:
                A[i][i] += 2 * alpha * I[i][j] * I[i][j] * N[i][j]
                A[i][j] -= 2 * alpha * I[i][j] * I[j][i] * N[i][j]
    for i in range(n):                       # a camera that covers nothing keeps gain 1
        if A[i][i] == 0:
            A[i][i], b[i] = Fraction(1), Fraction(1)
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c] != 0)          # StopIteration: the system is singular
        A[c], A[piv], b[c], b[piv] = A[piv], A[c], b[piv], b[c]
        for r in range(c + 1, n):
            f = A[r][c] / A[c][c]
            if f:
                A[r] = [x - f * y for x, y in zip(A[r], A[c])]
                b[r] -= f * b[c]
    g = [Fraction(0)] * n
    for r in range(n - 1, -1, -1):
        g[r] = (b[r] - sum(A[r][k] * g[k] for k in range(r + 1, n))) / A[r][r]
    return [256 * x for x in g]


def half_distance(x: Fraction) -> Fraction:
    """The distance of x to the nearest half-integer."""
    y = x - HALF
    return abs(y - round(y))


def rounded_q8(x: Fraction) -> int:
    """round(x) clipped to 64..1024 (for an x that is not NEAR_HALF of a half-integer the rounding rule does not matter)."""
    return min(max((x + HALF).__floor__(), 64), 1024)
