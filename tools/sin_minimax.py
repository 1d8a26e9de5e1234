"""Derives the fast sine's polynomial (vcrt_math.h sin_fast_try, kSinC): the odd polynomial
s(r) = r + r^3 P(r^2), P of degree 6 (s of degree 15), that minimises the relative error
|s(r) - sin r| / |sin r| on |r| <= pi/2 + 2^-20 (the reduced argument's range: r = x - k pi with
k = rint(x / pi), a hair over pi/2 by the rounding of x / pi).

Weighted Remez exchange in u = r^2 with mpmath at 80 digits: P approximates
f(u) = (sin(sqrt u) / sqrt u - 1) / u under the weight w(u) = u sqrt(u) / sin(sqrt u), which is
the relative error of s. The coefficients are then rounded to double and the error of the
rounded polynomial is measured on a dense grid; the script prints the C literals (highest degree
first, the order of kSinC[4..10]) and log2 of that error.

  python tools/sin_minimax.py [--degree 6]
"""
import argparse

import mpmath as mp

mp.mp.dps = 80


def f(u):
    if u == 0:
        return -mp.mpf(1) / 6
    r = mp.sqrt(u)
    if r < mp.mpf(2) ** -40:  # the series, where the difference cancels
        return -mp.mpf(1) / 6 + u / 120 - u * u / 5040
    return (mp.sin(r) / r - 1) / u


def weight(u):
    if u == 0:
        return mp.mpf(0)
    r = mp.sqrt(u)
    return u * r / mp.sin(r)


def polyval(c, u):  # c: lowest degree first
    acc = mp.mpf(0)
    for a in reversed(c):
        acc = acc * u + a
    return acc


def remez(n, umax, iters=40):
    """Coefficients (lowest first) of the degree-n weighted minimax P and its levelled error."""
    m = n + 2
    # Chebyshev nodes of [0, umax], kept off u = 0 where the weight vanishes
    pts = [umax * (1 - mp.cos(mp.pi * (i + mp.mpf(1) / 2) / m)) / 2 for i in range(m)]
    grid = [umax * mp.mpf(i) / 4000 for i in range(1, 4001)]
    c, e = None, None
    for _ in range(iters):
        a = mp.matrix(m, m)
        b = mp.matrix(m, 1)
        for i, u in enumerate(pts):
            for j in range(n + 1):
                a[i, j] = u ** j
            a[i, n + 1] = (-1) ** i / weight(u)
            b[i] = f(u)
        sol = mp.lu_solve(a, b)
        c, e = [sol[j] for j in range(n + 1)], sol[n + 1]
        err = lambda u: (polyval(c, u) - f(u)) * weight(u)  # noqa: E731
        # the extrema of the error: per sign run of the grid, the point of largest |error|,
        # refined by golden-section search between its neighbours
        vals = [err(u) for u in grid]
        runs, cur = [], [0]
        for i in range(1, len(grid)):
            if (vals[i] > 0) == (vals[cur[-1]] > 0):
                cur.append(i)
            else:
                runs.append(cur)
                cur = [i]
        runs.append(cur)
        new = []
        for run in runs:
            k = max(run, key=lambda i: abs(vals[i]))
            lo, hi = grid[max(k - 1, 0)], grid[min(k + 1, len(grid) - 1)]
            s = 1 if vals[k] > 0 else -1
            g = (mp.sqrt(5) - 1) / 2
            x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
            for _ in range(60):
                if s * err(x1) < s * err(x2):
                    lo, x1 = x1, x2
                    x2 = lo + g * (hi - lo)
                else:
                    hi, x2 = x2, x1
                    x1 = hi - g * (hi - lo)
            new.append((lo + hi) / 2)
        if len(new) != m:
            raise RuntimeError(f"{len(new)} extrema for {m} points")
        spread = max(abs(err(u)) for u in new) / min(abs(err(u)) for u in new)
        pts = new
        if spread < 1 + mp.mpf(10) ** -12:
            break
    return c, abs(e)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--degree", type=int, default=6, help="degree of P in r^2 (6: s of degree 15)")
    a = p.parse_args()
    rmax = mp.pi / 2 + mp.mpf(2) ** -20
    c, e = remez(a.degree, rmax * rmax)
    print(f"levelled relative error of the exact minimax: 2^{float(mp.log(e, 2)):.2f}")
    cd = [float(x) for x in c]  # rounded to nearest double
    worst = mp.mpf(0)
    for i in range(1, 20001):
        r = rmax * i / 20000
        s = r + r ** 3 * polyval([mp.mpf(x) for x in cd], r * r)
        worst = max(worst, abs(s - mp.sin(r)) / mp.sin(r))
    print(f"relative error with the coefficients rounded to double: 2^{float(mp.log(worst, 2)):.2f}")
    print("coefficients of r^15 .. r^3 (kSinC[4..10]):")
    for x in reversed(cd):
        print(f"    {x.hex()},")


if __name__ == "__main__":
    main()
